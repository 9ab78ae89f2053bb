"""The yardstick of tests/test_gif_dither.py and tests/test_gif_dither_gpu.py, in plain loops: the Floyd-Steinberg rule of the device GIF writer
(DESIGN.md 4d), its frame differencing, and what a decoder shows for a differenced clip.  Nothing here comes from mmgt_amd.

The rule, per frame, raster order (y outer, x inner), integers, per channel; d is 0 outside the frame:
    E(x, y) = 7 d(x-1, y) + 3 d(x+1, y-1) + 5 d(x, y-1) + d(x-1, y-1)
    v       = clamp(p(x, y) + floor((E + 8) / 16), 0, 255)
    idx     = lut[(v_r >> 3) << 10 | (v_g >> 3) << 5 | (v_b >> 3)]
    d(x, y) = v - palette[idx]"""
import numpy as np


def dither_frame(frame, lut, palette):
    """(H, W, 3) uint8, lut (32768,), palette (256, 3) -> (H, W) uint8."""
    H, W, _ = frame.shape
    pix = frame.tolist()
    lut = [int(v) for v in lut]
    pal = [[int(c) for c in row] for row in palette]
    zero = (0, 0, 0)
    above = [zero] * (W + 2)                                        # d of the row above, at x + 1; zero left and right of the frame
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        here = [zero] * (W + 2)
        for x in range(W):
            v = []
            for ch in range(3):
                E = 7 * here[x][ch] + 3 * above[x + 2][ch] + 5 * above[x + 1][ch] + above[x][ch]
                v.append(min(255, max(0, pix[y][x][ch] + ((E + 8) >> 4))))                   # Python's >> is the floor
            k = lut[(v[0] >> 3) << 10 | (v[1] >> 3) << 5 | (v[2] >> 3)]
            out[y, x] = k
            here[x + 1] = (v[0] - pal[k][0], v[1] - pal[k][1], v[2] - pal[k][2])
        above = here
    return out


def dither(frames, lut, palette):
    """(n, H, W, 3) uint8 -> (n, H, W) uint8: every frame on its own."""
    return np.stack([dither_frame(f, lut, palette) for f in frames])


def undithered(frames, lut):
    f = frames.astype(np.int64)
    return np.asarray(lut)[(f[..., 0] >> 3) << 10 | (f[..., 1] >> 3) << 5 | (f[..., 2] >> 3)].astype(np.uint8)


def delta(idx):
    """(n, H, W) index maps -> the same with 255 where a pixel equals the frame before; frame 0 as it is."""
    n, H, W = idx.shape
    out = np.zeros_like(idx)
    for f in range(n):
        for y in range(H):
            for x in range(W):
                same = f > 0 and idx[f, y, x] == idx[f - 1, y, x]
                out[f, y, x] = 255 if same else idx[f, y, x]
    return out


def compose(coded, palette, transparent=255):
    """What a decoder shows for index maps written with write_gif(..., transparent=255): frame 0 drawn in full, every frame left in place, later
    frames drawn except where they hold the transparent index.  -> (n, H, W, 3) uint8."""
    palette = np.asarray(palette)
    canvas = palette[coded[0]].copy()
    frames = [canvas.copy()]
    for f in range(1, coded.shape[0]):
        for y in range(coded.shape[1]):
            for x in range(coded.shape[2]):
                if coded[f, y, x] != transparent:
                    canvas[y, x] = palette[coded[f, y, x]]
        frames.append(canvas.copy())
    return np.stack(frames)


def ramp(H=96, W=128):
    """R = x 255 // 127, G = y 255 // 95, B = (x + y) 255 // 222 on 128 x 96, cropped to H x W (larger sizes repeat it)."""
    y, x = np.mgrid[0:H, 0:W]
    y, x = y % 96, x % 128
    return np.stack([x * 255 // 127, y * 255 // 95, (x + y) * 255 // 222], axis=-1).astype(np.uint8)
