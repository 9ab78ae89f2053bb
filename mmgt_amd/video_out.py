"""Output path of the sampler: the counterpart of `save_videos_grid` / `save_videos_from_pil`
(src/utils/util.py:76-107,148-165).  The uint8 conversion runs on the device (AutoencoderKL.decode_video_uint8,
csrc/conditioning.hip: mmgt_frames_to_u8); this module only lays frames out and writes them.  The reference's .mp4 branch
encodes with PyAV / libx264, which is not part of this build: .gif goes through PIL exactly as the reference's .gif branch does,
.npy stores the raw uint8 frames, .mp4 raises.  .avi is this build's video file: baseline JPEG frames encoded on the device
(csrc/mjpeg.hip; encode_jpeg_frames) in a RIFF AVI 1.0 container with an optional PCM sound track (write_avi).  gif_encoder="device" is a second,
opt-in .gif writer: one palette for the clip (gif_palette, gif_lut), index map, LZW and sub-block packing on the device (csrc/gif.hip;
encode_gif_frames) and the GIF89a container here (write_gif); gif_dither="fs" adds Floyd-Steinberg dithering against that palette and
gif_delta=True frame differencing through a transparent index, both on the device too.  .apng / .png are the lossless output: scanline filters and deflate on the device
(csrc/png.hip; encode_png_frames), Huffman code lengths, block headers and the PNG / APNG chunks here (write_png, write_png_sequence, write_apng).
.webp is the second lossless output, WebP lossless / animated WebP: subtract green, predictor choice and prefix coding on the device (csrc/webp.hip;
encode_webp_frames), the five codes of a frame, its header and the RIFF chunks here (webp_prefix_code, webp_frame_header, write_webp).
webp_quality=Q makes the .webp lossy instead: every frame a VP8 key frame, colour conversion, intra prediction with its reconstruction loop,
transforms, quantisers, the boolean coder and the packing on the device (csrc/vp8.hip; encode_vp8_frames), the same container with 'VP8 ' chunks."""
import os
import struct
from pathlib import Path

import numpy as np
import torch


def frames_uint8(videos, n_rows=6) -> np.ndarray:
    """(b, c, t, h, w) float in [0, 1] (Pose2VideoPipelineOutput.videos) or (b, t, h, w, 3) uint8 (output_type="uint8") ->
    (t, H, W, 3) uint8 grid frames laid out as torchvision.utils.make_grid(x, nrow=n_rows) does it (util.py:148-160): one clip is
    returned as it is; b > 1 clips sit in rows of min(n_rows, b) cells of (h + 2) x (w + 2) with a 2-pixel zero border."""
    v = torch.as_tensor(videos)
    if v.dtype != torch.uint8:
        v = (v.permute(0, 2, 3, 4, 1) * 255).numpy().astype(np.uint8)           # (x * 255).numpy().astype(np.uint8)
        v = torch.from_numpy(v)
    v = v.numpy()
    b, t, h, w, c = v.shape
    if b == 1:
        return v[0]
    pad = 2
    xmaps = min(int(n_rows), b)
    ymaps = -(-b // xmaps)
    ch, cw = h + pad, w + pad
    grid = np.zeros((t, ch * ymaps + pad, cw * xmaps + pad, c), dtype=np.uint8)
    for k in range(b):
        y, x = divmod(k, xmaps)
        grid[:, y * ch + pad:y * ch + pad + h, x * cw + pad:x * cw + pad + w] = v[k]
    return grid


def _clip(frames, who, empty=True, max_side=None, a_frame="a frame", strip_rows=False, default_rows=None):
    """The common opening of the encode_*_frames functions, in `who`'s name: frames must be uint8 (n, H, W, 3); unless empty=False an empty clip is
    refused; max_side limits H and W; strip_rows (False: the function has none) defaults to default_rows, must be at least 1 and is clamped to H.
    -> (the frames as a tensor, where they were; n, H, W, strip_rows).  _on_device uploads them: whatever else a function checks stands between the
    two, so that every bad argument is refused on a host without a GPU."""
    x = torch.as_tensor(frames)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError(f"{who}: expected uint8 (n, H, W, 3), got {x.dtype} {tuple(x.shape)}")
    n, H, W, _ = x.shape
    if empty and (n == 0 or H == 0 or W == 0):
        raise ValueError(f"{who}: empty clip {tuple(x.shape)}")
    if max_side is not None and (H > max_side or W > max_side):
        raise ValueError(f"{who}: {a_frame} is at most {max_side} x {max_side}, got {W} x {H}")
    if strip_rows is not False:
        strip_rows = int(default_rows if strip_rows is None else strip_rows)
        if strip_rows < 1:
            raise ValueError(f"{who}: strip_rows must be at least 1, got {strip_rows}")
        strip_rows = min(strip_rows, H)
    return x, n, H, W, strip_rows


def _on_device(x):
    return (x if x.is_cuda else x.cuda()).contiguous()


def _batches(x, scratch_bytes, per_frame):
    """The clip in the parts that one set of launches takes: as many frames as scratch_bytes hold at per_frame bytes each, one at least."""
    per_call = max(1, scratch_bytes // per_frame)
    for f0 in range(0, x.shape[0], per_call):
        yield x[f0:f0 + per_call]


# ---- JFIF headers: everything of a frame's file that does not depend on its pixels (T.81 Annex B, JFIF 1.01) ----------------------------------
# T.81 Annex K.3 BITS / HUFFVAL of the four standard Huffman tables (the same tables csrc/mjpeg.hip codes with)
_DC_BITS = (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]))
_AC_BITS = (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]), bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]))
_AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7"
    "b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5"
    "b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def _seg(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def jfif_headers(width, height, quality=90, subsampling="4:2:0") -> bytes:
    """SOI .. SOS of a frame: APP0 (JFIF 1.01, 1:1 aspect), two DQT, SOF0 with the TRUE size, the four Annex K DHT, DRI (one MCU row) and the
    scan header.  What follows in the file is the entropy-coded data with its RSTm markers and EOI, as the device lays it out."""
    from . import hip
    ql, qc = hip.jpeg_qtables(quality)
    _, mcu_cols, bpm = hip.jpeg_geometry(height, width, subsampling)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0]) + struct.pack(">HH", 1, 1) + b"\0\0")
    out += _seg(0xDB, b"\x00" + ql) + _seg(0xDB, b"\x01" + qc)
    y_hv = 0x22 if bpm == 6 else 0x11
    out += _seg(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, y_hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_id, bits, vals in ((0x00, _DC_BITS[0], bytes(range(12))), (0x10, _AC_BITS[0], _AC_VALS[0]),
                               (0x01, _DC_BITS[1], bytes(range(12))), (0x11, _AC_BITS[1], _AC_VALS[1])):
        out += _seg(0xC4, bytes([cls_id]) + bits + vals)
    out += _seg(0xDD, struct.pack(">H", mcu_cols))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


JPEG_SCRATCH_BYTES = 256 << 20      # encode_jpeg_frames codes at most this much worst-case segment space per set of launches


def encode_jpeg_frames(frames, quality=90, subsampling="4:2:0") -> list:
    """(n, H, W, 3) uint8 RGB frames (a CUDA tensor, or host data that is uploaded) -> n byte strings, each a complete baseline JFIF file.
    Colour transform, DCT, quantiser, Huffman coding, byte stuffing and compaction run on the device (csrc/mjpeg.hip); the host receives the
    offsets and ONE buffer of scan data and prepends the fixed headers.  The bytes are the same on every call."""
    from . import hip
    x, n, H, W, _ = _clip(frames, "encode_jpeg_frames", empty=False)
    x = _on_device(x)
    if n == 0:
        return []
    head = jfif_headers(W, H, quality, subsampling)                          # also the argument check: the library refuses bad ones
    rows = hip.jpeg_geometry(H, W, subsampling)[0]
    out = []
    for part in _batches(x, JPEG_SCRATCH_BYTES, rows * hip.jpeg_segment_stride(W, subsampling)):
        segs, sizes = hip.jpeg_entropy(hip.jpeg_dct_quant(part, quality, subsampling), H, W, subsampling)
        data, off = hip.jpeg_compact(segs, sizes, rows)
        data = data.cpu().numpy().tobytes()
        off = off.tolist()
        out += [head + data[off[k * rows]:off[(k + 1) * rows]] for k in range(part.shape[0])]
    return out


# ---- RIFF AVI 1.0 ------------------------------------------------------------------------------------------------------------------------------
AVI_MAX_BYTES = 1 << 30             # one RIFF chunk; larger files need OpenDML (AVIX), which is not written


def _chunk(fourcc: bytes, body: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def write_avi(path, jpeg_frames, width, height, fps, audio=None):
    """Motion-JPEG AVI: RIFF 'AVI ' { LIST 'hdrl' { avih, LIST 'strl' { strh vids/MJPG, strf BITMAPINFOHEADER } [, LIST 'strl' { strh auds,
    strf WAVEFORMATEX PCM }] }, LIST 'movi' { 00dc [01wb] ... }, idx1 }.  `jpeg_frames`: one complete JPEG file per frame;
    `audio` = (int16 samples (n, channels) or (n,), sample rate): interleaved as one 01wb chunk of a video frame's duration after each 00dc
    chunk (any remainder after the last frame).  Chunks are padded to even length; idx1 offsets count from the 'movi' fourcc.  DESIGN.md lists
    the fields."""
    frames = [bytes(f) for f in jpeg_frames]
    if not frames:
        raise ValueError("write_avi: no frames")
    fps = float(fps)
    usec = int(round(1e6 / fps))
    rate, scale = (int(fps), 1) if fps == int(fps) else (int(round(fps * 1000)), 1000)
    pcm, channels, srate, block = None, 0, 0, 0
    if audio is not None:
        samples, srate = audio
        samples = np.ascontiguousarray(np.asarray(samples))
        if samples.dtype != np.int16 or samples.ndim not in (1, 2):
            raise ValueError(f"write_avi: audio must be int16 samples (n, channels), got {samples.dtype} {samples.shape}")
        samples = samples.reshape(samples.shape[0], -1)
        channels, srate = samples.shape[1], int(srate)
        block = 2 * channels
        pcm = samples.astype("<i2").tobytes()
    est = sum(len(f) + 50 for f in frames) + (len(pcm) if pcm else 0) + 4096      # chunk headers, padding, index entries: an upper estimate
    if est > AVI_MAX_BYTES:
        raise ValueError(f"write_avi: {path} would pass 1 GiB (about {est} bytes); AVI 1.0 holds one RIFF chunk and OpenDML is not written")

    movi, index = [b"movi"], []
    pos = 4                                                                  # offset of the next chunk from the 'movi' fourcc

    def add(fourcc, body, flags):
        nonlocal pos
        index.append(fourcc + struct.pack("<III", flags, pos, len(body)))
        c = _chunk(fourcc, body)
        movi.append(c)
        pos += len(c)

    n = len(frames)
    total_samples = len(pcm) // block if pcm else 0
    for k, f in enumerate(frames):
        add(b"00dc", f, 0x10)                                                # AVIIF_KEYFRAME: every JPEG frame is one
        if pcm:
            a = min(total_samples, int(round(k * srate / fps)))
            b = total_samples if k == n - 1 else min(total_samples, int(round((k + 1) * srate / fps)))
            if b > a:
                add(b"01wb", pcm[a * block:b * block], 0x10)
    movi = b"".join(movi)
    streams = 2 if pcm else 1
    big = max(len(f) for f in frames)
    avih = struct.pack("<14I", usec, int(big * fps) + (srate * block), 0, 0x10 | (0x100 if pcm else 0),       # AVIF_HASINDEX | AVIF_ISINTERLEAVED
                       n, 0, streams, big, width, height, 0, 0, 0, 0)
    strh_v = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, n, big, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf_v = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", b"strl" + _chunk(b"strh", strh_v) + _chunk(b"strf", strf_v))
    if pcm:
        strh_a = b"auds" + b"\0\0\0\0" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, block, srate * block, 0, total_samples, srate * block // 2,
                                                      0xFFFFFFFF, block, 0, 0, 0, 0)
        strf_a = struct.pack("<HHIIHHH", 1, channels, srate, srate * block, block, 16, 0)                     # WAVE_FORMAT_PCM
        hdrl += _chunk(b"LIST", b"strl" + _chunk(b"strh", strh_a) + _chunk(b"strf", strf_a))
    body = b"AVI " + _chunk(b"LIST", hdrl) + _chunk(b"LIST", movi) + _chunk(b"idx1", b"".join(index))
    if len(body) + 8 > AVI_MAX_BYTES:
        raise ValueError(f"write_avi: {path} would pass 1 GiB ({len(body) + 8} bytes); AVI 1.0 holds one RIFF chunk and OpenDML is not written")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return len(body) + 8


# ---- GIF89a with one palette for the clip ----------------------------------------------------------------------------------------
GIF_BINS = 32768                    # 5 bits per channel: bin = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3)
GIF_STRIP_ROWS = 16                 # image rows per LZW strip of encode_gif_frames: 768 workgroups for 24 frames of 512 rows
GIF_SCRATCH_BYTES = 256 << 20       # encode_gif_frames holds at most this much index map, strip slots and packed frames per set of launches


def _gif_hist(hist):
    h = np.asarray(hist)
    if h.shape != (GIF_BINS,) or h.dtype.kind not in "iu":
        raise ValueError(f"expected an integer histogram of shape ({GIF_BINS},), got {h.dtype} {h.shape}")
    h = h.astype(np.int64)
    if (h < 0).any():
        raise ValueError("histogram counts must not be negative")
    return h


def gif_palette(hist, colors=256) -> np.ndarray:
    """(32768,) pixel counts per bin -> (256, 3) uint8 palette by median cut over the occupied bins, in integer arithmetic only (the same table on
    every call and every host).  A bin has the coordinates (r, g, b) = (bin >> 10, bin >> 5 & 31, bin & 31) and the centre 8 i + 4 per channel.

    Up to 256 occupied bins: entry k is the centre of the k-th occupied bin in ascending bin order, the rest is zero.  Otherwise box 0 holds every
    occupied bin and, until there are 256 boxes: a box's side along an axis is max - min + 1 of its bins' coordinates; among the boxes of two or more
    bins the one with the largest (pixel count x longest side) is split, the lowest box index winning a tie; the axis is the longest side, R before G
    before B on a tie; with c(v) the box's pixels at coordinate v of that axis and T their sum, the cut m is the smallest v with
    2 (c(min) + ... + c(v)) >= T, lowered to max - 1 if it is max; bins with coordinate <= m keep the box's index, the others become the box with the
    next free index.  Entry k is, per channel, the count-weighted mean of the centres of box k's bins, rounded half up:
    floor((2 sum(c (8 i + 4)) + sum c) / (2 sum c)).

    colors=255 keeps entry 255 out of it (zero), for the transparent index of frame differencing: "up to 255 occupied bins", "until there are 255
    boxes"."""
    colors = _gif_colors(colors)
    h = _gif_hist(hist)
    occ = np.flatnonzero(h)
    pal = np.zeros((256, 3), np.uint8)
    if occ.size == 0:
        raise ValueError("gif_palette: the histogram is empty")
    coord = np.stack([occ >> 10, (occ >> 5) & 31, occ & 31], axis=1).astype(np.int64)       # (bins, 3)
    cnt = h[occ]
    if occ.size <= colors:
        pal[:occ.size] = 8 * coord + 4
        return pal

    def score(members):                                                                       # (count x longest side, axis), or None: not splittable
        if members.size < 2:
            return None
        c = coord[members]
        side = c.max(0) - c.min(0) + 1
        axis = int(np.argmax(side))                                                           # first maximum: R, G, B
        return int(cnt[members].sum()) * int(side[axis]), axis

    boxes = [np.arange(occ.size)]
    scores = [score(boxes[0])]
    while len(boxes) < colors:
        best = max((k for k in range(len(boxes)) if scores[k] is not None), key=lambda k: (scores[k][0], -k))
        members, axis = boxes[best], scores[best][1]
        v = coord[members, axis]
        lo, hi = int(v.min()), int(v.max())
        per = np.zeros(hi - lo + 1, np.int64)
        np.add.at(per, v - lo, cnt[members])                                                  # int64 sums (bincount's weights are floats)
        cum = np.cumsum(per)
        m = lo + int(np.argmax(2 * cum >= cum[-1]))
        m = min(m, hi - 1)
        lower, upper = members[v <= m], members[v > m]
        boxes[best] = lower
        scores[best] = score(lower)
        boxes.append(upper)
        scores.append(score(upper))
    for k, members in enumerate(boxes):
        c = cnt[members]
        tot = int(c.sum())
        for ch in range(3):
            pal[k, ch] = (2 * int((c * (8 * coord[members, ch] + 4)).sum()) + tot) // (2 * tot)
    return pal


def _gif_colors(colors):
    if colors not in (255, 256):
        raise ValueError(f"colors must be 256, or 255 to keep index 255 free, got {colors!r}")
    return int(colors)


def _gif_check_palette(palette):
    pal = np.asarray(palette)
    if pal.shape != (256, 3) or pal.dtype != np.uint8:
        raise ValueError(f"palette must be uint8 (256, 3), got {pal.dtype} {pal.shape}")
    return pal


def gif_lut(palette, colors=256) -> np.ndarray:
    """(256, 3) uint8 palette -> (32768,) uint8: for every bin the palette entry nearest to the bin's centre (8 r + 4, 8 g + 4, 8 b + 4) by squared
    RGB distance, the lowest index on a tie.  colors=255 looks among entries 0 .. 254 only: no bin maps to index 255."""
    colors = _gif_colors(colors)
    pal = _gif_check_palette(palette).astype(np.int32)[:colors]
    centre = 8 * np.arange(32, dtype=np.int32) + 4
    d = [(centre[:, None] - pal[None, :, ch]) ** 2 for ch in range(3)]                       # (32, 256) each
    dist = d[0][:, None, None, :] + d[1][None, :, None, :] + d[2][None, None, :, :]          # (32, 32, 32, colors)
    return np.argmin(dist.reshape(GIF_BINS, colors), axis=1).astype(np.uint8)                   # argmin returns the first minimum


def encode_gif_frames(frames_u8, palette=None, strip_rows=None, dither=None, delta=False):
    """(n, H, W, 3) uint8 RGB frames (a CUDA tensor, or host data that is uploaded) -> (palette (256, 3) uint8, n byte strings): each string is
    one frame's GIF image data as write_gif takes it, LZW-coded against `palette` and cut into data sub-blocks with the 0x00 terminator.  Colour
    histogram, index map, LZW and packing run on the device (csrc/gif.hip); the host builds palette and lookup table from the 128 KB histogram
    (gif_palette / gif_lut, skipped for the histogram if `palette` is given) and receives the sizes and ONE buffer of finished bytes per set of
    launches.  The bytes are the same on every call.

    dither=None: a pixel takes the palette entry of its 5-bit bin.  dither="fs": Floyd-Steinberg error diffusion against the palette, per frame
    (mmgt_gif_dither; DESIGN.md 4d states the rule).  delta=True: frame differencing; the palette has 255 colours (entry 255 zero; one you supply
    must have it so), and from the second frame on a pixel whose index equals the frame before's is written as 255, which write_gif(...,
    transparent=255) declares transparent.  The comparison runs across the whole clip, also where it is split into sets of launches."""
    from . import hip
    x, n, H, W, strip_rows = _clip(frames_u8, "encode_gif_frames", max_side=65535, a_frame="a GIF frame", strip_rows=strip_rows,
                                   default_rows=GIF_STRIP_ROWS)
    if dither not in (None, "fs"):
        raise ValueError(f"encode_gif_frames: dither must be None or 'fs', got {dither!r}")
    colors = 255 if delta else 256
    if palette is not None:
        palette = _gif_check_palette(palette).copy()
        if delta and palette[255].any():
            raise ValueError("encode_gif_frames: with delta=True index 255 is the transparent one: row 255 of the palette must be zero")
    x = _on_device(x)
    if palette is None:
        palette = gif_palette(hip.gif_histogram(x).cpu().numpy().view(np.uint32), colors)
    lut = torch.from_numpy(gif_lut(palette, colors)).to(x.device)
    pal_d = torch.from_numpy(palette).to(x.device) if dither else None
    strips = -(-H // strip_rows)
    stride = hip.gif_strip_stride(W, strip_rows)
    blobs = []
    last = None                                                    # the index map of the frame before this set of launches
    per_frame = H * W * (2 if delta else 1) + (4 * W if dither else 0) + strips * stride + hip.gif_packed_stride(strips, stride)
    for part in _batches(x, GIF_SCRATCH_BYTES, per_frame):
        if part.data_ptr() % 4:                                    # a later part of a clip whose frames are no multiple of 4 bytes
            part = part.clone()
        idx = hip.gif_dither(part, lut, pal_d) if dither else hip.gif_index(part, lut)
        if delta:
            idx, last = hip.gif_delta(idx, last), idx[-1]
        packed, sizes = hip.gif_pack(*hip.gif_lzw(idx, strip_rows))
        sizes = sizes.tolist()
        if min(sizes) < 1:
            raise RuntimeError("encode_gif_frames: the packed frame did not fit its slot (mmgt_gif_pack)")
        data = packed[:, :max(sizes)].cpu().numpy()
        blobs += [data[k, :sizes[k]].tobytes() for k in range(len(sizes))]
    return palette, blobs


def write_gif(path, palette, frame_blobs, W, H, fps, loop=0, transparent=None):
    """GIF89a: header, logical screen descriptor with a 256-entry global colour table, the NETSCAPE2.0 loop extension (`loop` repetitions, 0 = for
    ever), per frame a graphic control extension (delay, no disposal, no transparency) and an image descriptor covering the screen with no local
    table, the LZW minimum code size 8 and the frame's data sub-blocks as encode_gif_frames returns them; then the trailer.  Returns the bytes
    written.  A GIF delay is a whole number of centiseconds, round(100 / fps): 25 fps is 4 cs exactly, but most rates are not expressible
    (8 fps -> 12 cs = 8.33 fps, 30 fps -> 3 cs = 33.3 fps).  DESIGN.md 4d lists the fields.

    transparent = an index (255 for encode_gif_frames(..., delta=True)) writes the clip for frame differencing: every frame is left in place
    (disposal 1), and from the second frame on that index is declared transparent, so a pixel coded with it keeps what the frames before drew."""
    pal = _gif_check_palette(palette)
    if transparent is not None and not 0 <= int(transparent) <= 255:
        raise ValueError(f"write_gif: transparent must be None or an index 0 .. 255, got {transparent!r}")
    blobs = [bytes(b) for b in frame_blobs]
    if not blobs:
        raise ValueError("write_gif: no frames")
    if not (1 <= int(W) <= 65535 and 1 <= int(H) <= 65535):
        raise ValueError(f"write_gif: a GIF screen is 1 .. 65535 pixels a side, got {W} x {H}")
    if not float(fps) > 0:
        raise ValueError(f"write_gif: fps must be positive, got {fps}")
    delay = min(65535, int(round(100.0 / float(fps))))
    loop = int(loop)
    if not 0 <= loop <= 65535:
        raise ValueError(f"write_gif: loop must be 0 .. 65535, got {loop}")
    out = [b"GIF89a", struct.pack("<HHBBB", int(W), int(H), 0xF7, 0, 0), pal.tobytes(),
           b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"]
    gce = b"\x21\xf9\x04" + struct.pack("<BHB", 0, delay, 0) + b"\x00"
    gce_later = gce
    if transparent is not None:                                    # packed: disposal 1 << 2, transparency flag 1
        gce = b"\x21\xf9\x04" + struct.pack("<BHB", 0x04, delay, 0) + b"\x00"
        gce_later = b"\x21\xf9\x04" + struct.pack("<BHB", 0x05, delay, int(transparent)) + b"\x00"
    desc = b"\x2c" + struct.pack("<HHHHB", 0, 0, int(W), int(H), 0) + b"\x08"
    for k, b in enumerate(blobs):
        if not b or b[-1] != 0:
            raise ValueError("write_gif: a frame's data must be sub-blocks ending with the 0x00 terminator")
        out += [gce if k == 0 else gce_later, desc, b]
    out.append(b"\x3b")
    body = b"".join(out)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(body)
    return len(body)


# ---- PNG / APNG: lossless frames, filtered and deflated on the device ---------------------------------------------------------------
PNG_STRIP_ROWS = 64                 # scanlines per deflate block of encode_png_frames: the strip_rows sweep of tools/bench_png.py
PNG_SCRATCH_BYTES = 256 << 20       # encode_png_frames holds at most this much filtered rows, strip slots and tables per set of launches
PNG_MAX_SIDE = 16384
_ADLER = 65521
_CL_ORDER = np.array([16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15])
# extra bits of the literal/length symbols 0 .. 285 (RFC 1951 3.2.5)
_LEN_EXTRA = np.zeros(286, np.int64)
_LEN_EXTRA[265:285] = np.repeat(np.arange(1, 6), 4)


def deflate_code_lengths(hist, max_bits) -> np.ndarray:
    """Counts per symbol -> optimal code lengths of at most max_bits, by package-merge.  The used symbols are the leaves, sorted by (count, symbol).
    List 1 is the leaves; list k + 1 merges the leaves with the packages of list k (its items paired in order, an odd last one dropped) by weight,
    at equal weight every leaf before every package.  The first 2 m - 2 items of list max_bits (m = used symbols) are taken; a symbol's length is
    the number of lists in which its leaf is among the items taken, where taking a package takes the two items it was made of.  Only the weights
    and which item is a leaf are kept: the leaves taken from a list are always its first ones.  One used symbol gets length 1."""
    h = np.asarray(hist).astype(np.int64).reshape(-1)
    max_bits = int(max_bits)
    if (h < 0).any():
        raise ValueError("deflate_code_lengths: counts must not be negative")
    order = np.flatnonzero(h)
    order = order[np.argsort(h[order], kind="stable")]                    # (count, symbol)
    m = order.size
    lengths = np.zeros(h.size, np.int64)
    if m == 1:
        lengths[order[0]] = 1
    if m < 2:
        return lengths
    if max_bits < 1 or m > (1 << max_bits):
        raise ValueError(f"deflate_code_lengths: {m} symbols do not fit codes of {max_bits} bits")
    w = h[order]
    leaf_flags = [np.ones(m, bool)]                                          # per list: which of its items are leaves
    cur = w
    for _ in range(max_bits - 1):
        pk = cur[0:cur.size - 1:2] + cur[1:cur.size:2]
        pos = np.searchsorted(w, pk, side="right") + np.arange(pk.size)      # a package stands after the leaves of its weight
        flags = np.ones(m + pk.size, bool)
        flags[pos] = False
        nxt = np.empty(m + pk.size, np.int64)
        nxt[pos] = pk
        nxt[flags] = w
        leaf_flags.append(flags)
        cur = nxt
    take = 2 * m - 2
    depth = np.zeros(m + 1, np.int64)
    for flags in reversed(leaf_flags):
        leaves = int(np.count_nonzero(flags[:take]))
        depth[0] += 1
        depth[leaves] -= 1
        take = 2 * (take - leaves)
        if take == 0:
            break
    lengths[order] = np.cumsum(depth)[:m]
    return lengths


_REV16 = np.zeros(1 << 16, np.int64)
for _b in range(16):
    _REV16 |= ((np.arange(1 << 16) >> _b) & 1) << (15 - _b)


def _canonical_codes(lengths):
    """RFC 1951 3.2.2 -> the codes, already bit-reversed for an LSB-first writer."""
    lengths = np.asarray(lengths, np.int64)
    count = np.bincount(lengths, minlength=17)
    first = np.concatenate([[0], np.cumsum(count)])                          # where each length starts among the symbols sorted by (length, symbol)
    count[0] = 0
    nxt = np.zeros(17, np.int64)
    for b in range(1, 17):
        nxt[b] = (nxt[b - 1] + count[b - 1]) << 1
    idx = np.argsort(lengths, kind="stable")
    ls = lengths[idx]
    code = np.zeros(lengths.size, np.int64)
    code[idx] = nxt[ls] + np.arange(lengths.size) - first[ls]
    return np.where(lengths > 0, _REV16[code & 0xFFFF] >> (16 - lengths), 0)


def _rle_code_lengths(seq, prev=None):
    """The code lengths as (symbol, extra bits, extra value) of the code-length alphabet.  Zeros: 18 for min(run, 138) while 11 or more are left,
    then 17 for 3 .. 10, then single zeros.  A non-zero length equal to the one that 16 repeats, with 3 or more equal lengths from here on, is 16
    for min(run, 6) of them; otherwise the length itself.  prev=None is RFC 1951's rule: 16 repeats the length written just before it, so a
    non-zero length is written once and then repeated.  An integer is VP8L's rule: 16 repeats `prev`, which starts at that value (the format says
    8) and which only a non-zero length written as itself changes."""
    seq = np.asarray(seq)
    cut = np.flatnonzero(np.diff(seq)) + 1
    starts = np.concatenate([[0], cut])
    runs = np.diff(np.concatenate([starts, [seq.size]]))
    out, last = [], prev
    for v, run in zip(seq[starts].tolist(), runs.tolist()):
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, 7, k - 11))
                run -= k
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
            out += [(0, 0, 0)] * run
            continue
        if prev is None:
            last = None
        while run:
            if v == last and run >= 3:
                k = min(run, 6)
                out.append((16, 2, k - 3))
                run -= k
            else:
                out.append((v, 0, 0))
                last = v
                run -= 1
    return out


def _put_code_lengths(acc, nb, syms, order, vp8l):
    """Appends to the LSB-first bit string (acc, nb) what describes a prefix code in deflate and in VP8L alike, given its code lengths as `syms`
    (_rle_code_lengths): the code-length code's lengths by package-merge at limit 7 and its canonical codes; in 4 bits the count - 4 of those lengths
    that are written, in the format's `order` with the trailing zeros trimmed, at least 4; those lengths at 3 bits each; then `syms` coded with that
    code, each with its extra bits.  vp8l: a zero bit stands before the symbols (max_symbol is not used), and a code-length code with ONE used
    symbol is read with zero bits per token, whatever length it states: then only the extra bits are written.  -> (acc, nb)."""
    cl = deflate_code_lengths(np.bincount([s for s, _, _ in syms], minlength=19), 7)
    codes = _canonical_codes(cl)
    ncl = max(4, int(np.flatnonzero(cl[order])[-1]) + 1)
    acc |= (ncl - 4) << nb
    nb += 4
    for k in range(ncl):
        acc |= int(cl[order[k]]) << nb
        nb += 3
    if vp8l:
        nb += 1
    free = vp8l and int(np.count_nonzero(cl)) == 1
    cl, codes = ([0] * 19, [0] * 19) if free else (cl.tolist(), codes.tolist())
    for s, eb, ev in syms:
        acc |= (codes[s] | ev << cl[s]) << nb
        nb += cl[s] + eb
    return acc, nb


def deflate_block_header(litlen_lengths, dist_lengths, final):
    """The head of a dynamic-Huffman block (RFC 1951 3.2.7) as an LSB-first bit string: BFINAL, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length
    code's lengths in the permuted order, then the literal/length and distance code lengths coded with it (runs as 16 / 17 / 18, which may cross
    from one alphabet into the other).  -> (bytes, bit count); the bits past the count are zero."""
    ll = np.asarray(litlen_lengths, np.int64)
    dl = np.asarray(dist_lengths, np.int64)
    if ll.size != 286 or not 1 <= dl.size <= 30 or ll[256] == 0:
        raise ValueError("deflate_block_header: 286 literal/length code lengths with symbol 256 used, and 1 .. 30 distance code lengths")
    nll = max(257, int(np.flatnonzero(ll)[-1]) + 1)
    acc, nb = (1 if final else 0) | 2 << 1 | (nll - 257) << 3 | (dl.size - 1) << 8, 13          # HCLEN and what follows it: _put_code_lengths
    acc, nb = _put_code_lengths(acc, nb, _rle_code_lengths(np.concatenate([ll[:nll], dl])), _CL_ORDER, False)
    return acc.to_bytes((nb + 7) // 8, "little"), nb


def adler32_combine(adler1, adler2, len2) -> int:
    """Adler-32 of A + B from those of A and B and len(B), as zlib's adler32_combine."""
    a1, b1, a2, b2 = adler1 & 0xFFFF, adler1 >> 16 & 0xFFFF, adler2 & 0xFFFF, adler2 >> 16 & 0xFFFF
    if len2 < 0:
        raise ValueError("adler32_combine: negative length")
    return ((b1 + b2 + (len2 % _ADLER) * (a1 + _ADLER - 1)) % _ADLER) << 16 | (a1 + a2 + _ADLER - 1) % _ADLER


def png_strip_tables(hist, final):
    """One strip's histogram of the 286 literal/length symbols -> (codes u32[286] = bit-reversed code | length << 16, header bytes, header bits,
    bits of the whole block)."""
    ll = deflate_code_lengths(hist, 15)
    matches = int(hist[257:].sum())
    head, hbits = deflate_block_header(ll, [1 if matches else 0], final)
    table = (_canonical_codes(ll) | ll << 16).astype(np.uint32)
    return table, head, hbits, hbits + int((hist * (ll + _LEN_EXTRA)).sum()) + matches


def encode_png_frames(frames_u8, strip_rows=None) -> list:
    """(n, H, W, 3) uint8 RGB frames (a CUDA tensor, or host data that is uploaded) -> n byte strings, each the zlib stream of one frame's PNG image
    data (write_png / write_apng put the chunks around it).  Filter choice, tokens, Huffman coding and bit packing run on the device
    (csrc/png.hip); the host builds each strip's codes and block header from the device's symbol histograms, knows every strip's bit count from
    them, and receives the Adler-32 sums of the rows and ONE buffer of finished bytes per set of launches.  The bytes are the same on every call;
    DESIGN.md 4g defines them."""
    from . import hip
    x, n, H, W, strip_rows = _clip(frames_u8, "encode_png_frames", max_side=PNG_MAX_SIDE, strip_rows=strip_rows, default_rows=PNG_STRIP_ROWS)
    x = _on_device(x)
    rowlen = 1 + 3 * W
    strips = -(-H // strip_rows)
    # filtered rows; slots and output, each at most 15 bits a byte and a header per strip; histograms, code tables, headers and offsets
    per_frame = 5 * H * rowlen + strips * (2 * 286 * 4 + 3 * hip.PNG_HEADER_BYTES + 64)
    blobs = []
    for part in _batches(x, PNG_SCRATCH_BYTES, per_frame):
        filt, sums = hip.png_filter(part)
        raw = deflate_strips_device(filt.view(filt.shape[0], H * rowlen), strip_rows * rowlen)
        for body, rows in zip(raw, sums.cpu().numpy().tolist()):
            adler = 1
            for s1, s2 in rows:                                                  # a row's sum of d[i] and of (rowlen - i) d[i]
                adler = adler32_combine(adler, ((rowlen + s2) % _ADLER) << 16 | (1 + s1) % _ADLER, rowlen)
            blobs.append(b"\x78\x01" + body + struct.pack(">I", adler))
    return blobs


def deflate_strips_device(data, strip_bytes) -> list:
    """(k, frame_bytes) uint8 on the device, any bytes -> k raw deflate streams (no zlib wrapper): every row cut into strips of strip_bytes (the
    last may be shorter), each strip one dynamic-Huffman block of distance-1 matches and literals.  Two passes over the bytes: symbol histograms
    per strip (down), codes and block headers (host, up), then coding into exactly sized slots and joining them at bit offsets."""
    from . import hip
    k, strips = data.shape[0], -(-data.shape[1] // int(strip_bytes))
    hist = hip.png_histogram(data, strip_bytes).cpu().numpy().view(np.uint32).astype(np.int64)                   # (k, strips, 286)
    codes = np.empty((k, strips, 286), np.uint32)
    heads, hbits = np.zeros((k, strips, hip.PNG_HEADER_BYTES), np.uint8), np.empty((k, strips), np.int32)
    want = np.empty((k, strips), np.int64)
    seen = {}                                                                # flat and pose-like clips repeat a few histograms many times
    for f in range(k):
        for s in range(strips):
            key = (hist[f, s].tobytes(), s == strips - 1)
            if key not in seen:
                seen[key] = png_strip_tables(hist[f, s], s == strips - 1)
            codes[f, s], head, hbits[f, s], want[f, s] = seen[key]
            heads[f, s, :len(head)] = np.frombuffer(head, np.uint8)
    slots, bits = hip.png_deflate(data, strip_bytes, codes, heads, hbits, want)
    packed, out_off = hip.png_pack(slots, want)
    bits = bits.cpu().numpy()
    if not np.array_equal(bits, want):
        bad = tuple(np.argwhere(bits != want)[0])
        raise RuntimeError(f"deflate_strips_device: strip {bad} took {bits[bad]} bits on the device, its histogram gives {want[bad]} "
                           "(mmgt_png_deflate)")
    packed = packed.cpu().numpy()
    return [packed[out_off[f]:out_off[f + 1]].tobytes() for f in range(k)]


def _png_chunk(kind: bytes, body: bytes) -> bytes:
    import zlib
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _png_ihdr(W, H, what):
    W, H = int(W), int(H)
    if not (1 <= W <= PNG_MAX_SIDE and 1 <= H <= PNG_MAX_SIDE):
        raise ValueError(f"{what}: a frame is 1 .. {PNG_MAX_SIDE} pixels a side, got {W} x {H}")
    return _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))      # 8 bit, truecolour, deflate, adaptive filtering, no interlace


def _write(path, body):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(body)
    return len(body)


def write_png(path, blob, W, H):
    """One frame of encode_png_frames -> a PNG file: signature, IHDR, one IDAT, IEND.  Returns the bytes written."""
    return _write(path, _PNG_SIG + _png_ihdr(W, H, "write_png") + _png_chunk(b"IDAT", bytes(blob)) + _png_chunk(b"IEND", b""))


def write_png_sequence(directory, blobs, W, H):
    """0000.png, 0001.png, ... in `directory` (what `ffmpeg -i %04d.png` reads).  Returns the paths."""
    blobs = [bytes(b) for b in blobs]
    if not blobs:
        raise ValueError("write_png_sequence: no frames")
    paths = [os.path.join(str(directory), f"{k:04d}.png") for k in range(len(blobs))]
    for p, b in zip(paths, blobs):
        write_png(p, b, W, H)
    return paths


def write_apng(path, blobs, W, H, fps, loop=0):
    """APNG 1.0: IHDR, acTL (frames, `loop` plays, 0 = for ever), then per frame one fcTL covering the whole frame at offset 0 with the delay
    Fraction(1 / fps).limit_denominator(65535) seconds, dispose and blend 0; frame 0's data in IDAT, every later frame's in fdAT; fcTL and fdAT
    carry consecutive sequence numbers from 0.  With one frame no animation chunks are written: the file is an ordinary PNG.  Returns the bytes
    written."""
    from fractions import Fraction
    blobs = [bytes(b) for b in blobs]
    if not blobs:
        raise ValueError("write_apng: no frames")
    if not float(fps) > 0:
        raise ValueError(f"write_apng: fps must be positive, got {fps}")
    loop = int(loop)
    if not 0 <= loop < 1 << 31:
        raise ValueError(f"write_apng: loop must be 0 .. 2^31 - 1, got {loop}")
    ihdr = _png_ihdr(W, H, "write_apng")
    if len(blobs) == 1:
        return write_png(path, blobs[0], W, H)
    delay = Fraction(1 / float(fps)).limit_denominator(65535)
    if delay.numerator > 65535:
        raise ValueError(f"write_apng: a frame's delay is at most 65535 s, got fps = {fps}")
    out, seq = [_PNG_SIG, ihdr, _png_chunk(b"acTL", struct.pack(">II", len(blobs), loop))], 0
    for k, b in enumerate(blobs):
        out.append(_png_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, int(W), int(H), 0, 0, delay.numerator, delay.denominator, 0, 0)))
        seq += 1
        if k == 0:
            out.append(_png_chunk(b"IDAT", b))
        else:
            out.append(_png_chunk(b"fdAT", struct.pack(">I", seq) + b))
            seq += 1
    out.append(_png_chunk(b"IEND", b""))
    return _write(path, b"".join(out))


# ---- WebP lossless / animated WebP: VP8L frames, predicted and coded on the device ----------------------------------------------------
WEBP_STRIP_ROWS = 64                # rows per strip of encode_webp_frames: the strip_rows sweep of tools/bench_webp.py
WEBP_SCRATCH_BYTES = 256 << 20      # encode_webp_frames holds at most this much residuals, strip slots, packed frames and tables per set of launches
WEBP_MAX_SIDE = 16384               # VP8L's 14-bit sizes
WEBP_PREDICTOR_BITS = 4             # blocks of 16 x 16 pixels choose a predictor mode (csrc/webp_core.h: WP_PREDICTOR_BITS)
WEBP_MAX_BYTES = (1 << 32) - 1      # a RIFF size is 32 bits
_WEBP_CL_ORDER = np.array([17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])
# bits that follow each symbol of the green + length alphabet: a length prefix 2 hb + sb from 4 on takes hb - 1 extra bits
_WEBP_GREEN_EXTRA = np.zeros(280, np.int64)
_WEBP_GREEN_EXTRA[260:] = np.arange(4, 24) // 2 - 1


def webp_prefix_code(counts):
    """Counts per symbol of one alphabet -> (lengths as the pixels are coded with them, the code's description as an LSB-first bit string, its bit
    count).  One used symbol (below 256), or none (then symbol 0): a simple code, bits 1 0 and 0 + 1 bit or 1 + 8 bits of symbol, and the symbol
    costs NO bits, so the lengths are all zero.  Otherwise a normal code: bit 0, the count of code-length-code lengths - 4 (trailing zeros in
    VP8L's order trimmed, at least 4), those lengths at 3 bits each, bit 0 (max_symbol is not used), then the alphabet's lengths
    (deflate_code_lengths, limit 15) run-length coded (_rle_code_lengths with prev = 8) with the code-length code (limit 7): _put_code_lengths.  A
    code-length code with ONE used symbol is read with zero bits per token, whatever length it states: then only the extra bits are written."""
    h = np.asarray(counts).astype(np.int64).reshape(-1)
    used = np.flatnonzero(h)
    if used.size <= 1:
        s = int(used[0]) if used.size else 0
        if s >= 256:
            raise ValueError(f"webp_prefix_code: the only used symbol is {s}; a simple code names symbols below 256")
        acc, nb = (0b01 | 0 << 2 | s << 3, 4) if s < 2 else (0b01 | 1 << 2 | s << 3, 11)
        return np.zeros(h.size, np.int64), acc, nb
    lengths = deflate_code_lengths(h, 15)
    acc, nb = _put_code_lengths(0, 1, _rle_code_lengths(lengths, prev=8), _WEBP_CL_ORDER, True)   # bit 0: a normal code
    return lengths, acc, nb


def _webp_code_bits(symbols, lengths):
    """Symbols coded one after the other with the canonical code of `lengths` -> (LSB-first bit string, bit count)."""
    lengths = np.asarray(lengths, np.int64)
    ln = lengths[symbols]
    codes = _canonical_codes(lengths)[symbols]
    bits = (codes[:, None] >> np.arange(15)) & 1
    flat = bits[np.arange(15) < ln[:, None]].astype(np.uint8)
    return int.from_bytes(np.packbits(flat, bitorder="little").tobytes(), "little"), int(ln.sum())


def webp_frame_tables(hist):
    """A frame's histogram u32[793] (the sum of its strips': green + length [280], red [256], blue [256], matches) -> (code tables u32[792] =
    bit-reversed code | length << 16 as csrc/webp.hip reads them, bits that one occurrence of each of the 793 entries takes, the five codes'
    description as (bit string, bit count)).  Alpha is 0 in every literal and the distance is prefix symbol 1 (the left pixel) in every match."""
    h = np.asarray(hist).astype(np.int64).reshape(-1)
    if h.size != 793:
        raise ValueError(f"webp_frame_tables: expected 793 counts, got {h.size}")
    alpha, dist = np.zeros(256, np.int64), np.zeros(40, np.int64)
    alpha[0], dist[1] = h[:256].sum(), h[792]
    acc, nb, lens = 0, 0, []
    for counts in (h[:280], h[280:536], h[536:792], alpha, dist):
        ln, a, k = webp_prefix_code(counts)
        acc |= a << nb
        nb += k
        lens.append(ln)
    table = np.concatenate([_canonical_codes(ln) | ln << 16 for ln in lens[:3]]).astype(np.uint32)
    cost = np.concatenate([lens[0] + _WEBP_GREEN_EXTRA, lens[1], lens[2], [0]])
    return table, cost, (acc, nb)


def webp_frame_header(W, H, modes, codes):
    """Everything of a VP8L bitstream that stands before the pixels, as (bytes, bit count), the bits past the count zero: signature 0x2f, W - 1 and
    H - 1 in 14 bits each, alpha-is-used 0, version 0; the subtract-green transform (1, type 2); the predictor transform (1, type 0, block bits - 2
    in 3 bits) with its sub-image of `modes` (bh, bw): no colour cache, five codes, the pixels (255, 0, mode, 0) as literals, of which only the
    mode takes bits; then 0 0 0 (no further transform, no colour cache, no meta prefix codes) and `codes`, the five codes of the frame as
    webp_frame_tables describes them."""
    W, H = int(W), int(H)
    if not (1 <= W <= WEBP_MAX_SIDE and 1 <= H <= WEBP_MAX_SIDE):
        raise ValueError(f"webp_frame_header: a frame is 1 .. {WEBP_MAX_SIDE} pixels a side, got {W} x {H}")
    m = np.asarray(modes).astype(np.int64)
    B = 1 << WEBP_PREDICTOR_BITS
    if m.shape != (-(-H // B), -(-W // B)) or m.min() < 0 or m.max() > 13:
        raise ValueError(f"webp_frame_header: modes must be ({-(-H // B)}, {-(-W // B)}) values 0 .. 13")
    m = m.reshape(-1)
    acc = 0x2F | (W - 1) << 8 | (H - 1) << 22                                   # alpha-is-used and the version: four zero bits
    nb = 40
    acc |= (1 | 2 << 1) << nb                                                    # subtract green
    nb += 3
    acc |= (1 | 0 << 1 | (WEBP_PREDICTOR_BITS - 2) << 3) << nb                   # predictor; then its sub-image's colour-cache bit 0
    nb += 7
    zero, a255 = np.zeros(256, np.int64), np.zeros(256, np.int64)
    zero[0] = a255[255] = m.size
    ml = None
    for counts in (np.bincount(m, minlength=280), zero, zero, a255, np.zeros(40, np.int64)):
        ln, a, k = webp_prefix_code(counts)
        ml = ln if ml is None else ml
        acc |= a << nb
        nb += k
    a, k = _webp_code_bits(m, ml)
    acc |= a << nb
    nb += k + 3                                                                  # 0 0 0
    acc |= codes[0] << nb
    nb += codes[1]
    return acc.to_bytes((nb + 7) // 8, "little"), nb


def encode_webp_frames(frames_u8, strip_rows=None) -> list:
    """(n, H, W, 3) uint8 RGB frames (a CUDA tensor, or host data that is uploaded) -> n byte strings, each one frame's VP8L bitstream (write_webp
    puts the chunks around it).  Subtract green, predictor choice, tokens, prefix coding and bit packing run on the device (csrc/webp.hip); the host
    builds each frame's five codes and its header from the device's block modes and symbol histograms, knows every strip's bit count from them,
    and receives ONE buffer of finished bytes per set of launches.  The bytes are the same on every call; DESIGN.md 4j defines them."""
    from . import hip
    x, n, H, W, strip_rows = _clip(frames_u8, "encode_webp_frames", max_side=WEBP_MAX_SIDE, strip_rows=strip_rows, default_rows=WEBP_STRIP_ROWS)
    x = _on_device(x)
    strips = -(-H // strip_rows)
    blocks = -(-H >> WEBP_PREDICTOR_BITS) * -(-W >> WEBP_PREDICTOR_BITS)
    # residual words; slots and output, each at most 45 bits a pixel; the header with its modes; histograms and offsets
    per_frame = 4 * H * W + 2 * 6 * H * W + 3 * (blocks + 2048) + strips * (793 * 4 + 64) + 792 * 4
    blobs = []
    for part in _batches(x, WEBP_SCRATCH_BYTES, per_frame):
        modes, res = hip.webp_predict(part)
        k = res.shape[0]
        data = res.view(k, H * W)
        hist = hip.webp_histogram(data, strip_rows * W).cpu().numpy().view(np.uint32).astype(np.int64)          # (k, strips, 793)
        modes = modes.cpu().numpy()
        codes, heads, want = np.empty((k, 792), np.uint32), [], np.empty((k, 1 + strips), np.int64)
        for f in range(k):
            codes[f], cost, described = webp_frame_tables(hist[f].sum(0))
            head, want[f, 0] = webp_frame_header(W, H, modes[f], described)
            heads.append(head)
            want[f, 1:] = hist[f] @ cost
        slots, bits = hip.webp_code(data, strip_rows * W, codes, heads, want)
        packed, out_off = hip.webp_pack(slots, want)
        bits = bits.cpu().numpy()
        if not np.array_equal(bits, want[:, 1:]):
            bad = tuple(np.argwhere(bits != want[:, 1:])[0])
            raise RuntimeError(f"encode_webp_frames: strip {bad} took {bits[bad]} bits on the device, its histogram gives {want[:, 1:][bad]} "
                               "(mmgt_webp_code)")
        packed = packed.cpu().numpy()
        blobs += [packed[out_off[f]:out_off[f + 1]].tobytes() for f in range(k)]
    return blobs


VP8_SCRATCH_BYTES = 256 << 20       # encode_vp8_frames holds at most this much planes, levels, worst-case slots and packed frames per set of launches
VP8_MAX_SIDE = 16383                # VP8's 14-bit sizes


def vp8_default_partitions(H) -> int:
    """8 token partitions when the frame has at least 8 macroblock rows, otherwise the largest of 1 / 2 / 4 that does not exceed the row count."""
    rows = -(-int(H) // 16)
    return 8 if rows >= 8 else 4 if rows >= 4 else 2 if rows >= 2 else 1


def encode_vp8_frames(frames_u8, quality=75, partitions=None, filter_level=None) -> list:
    """(n, H, W, 3) uint8 RGB frames (a CUDA tensor, or host data that is uploaded) -> n byte strings, each one frame's VP8 key frame, the payload
    of a 'VP8 ' chunk (write_webp(..., lossy=True) puts the chunks around it).  Colour conversion, prediction, transforms, quantisation,
    reconstruction, the boolean coder of every partition and the packing run on the device (csrc/vp8.hip); the host reads the partitions' byte counts
    to place the frames and receives ONE buffer of finished bytes per set of launches.  quality 0 .. 100 picks the quantiser index; partitions is 1,
    2, 4 or 8 (None: vp8_default_partitions); filter_level 0 .. 63 is the loop filter level the decoder applies (None: the default of the quantiser
    index; 0 makes the decode equal the encoder's reconstruction).  The bytes are the same on every call; DESIGN.md 4l defines them."""
    from . import hip
    x, n, H, W, _ = _clip(frames_u8, "encode_vp8_frames", max_side=VP8_MAX_SIDE)
    quality = int(quality)
    if not 0 <= quality <= 100:
        raise ValueError(f"encode_vp8_frames: quality must be 0 .. 100, got {quality}")
    partitions = vp8_default_partitions(H) if partitions is None else int(partitions)
    if partitions not in (1, 2, 4, 8):
        raise ValueError(f"encode_vp8_frames: partitions must be 1, 2, 4 or 8, got {partitions}")
    q, level = hip.vp8_quantiser(quality)
    filter_level = level if filter_level is None else int(filter_level)
    if not 0 <= filter_level <= 63:
        raise ValueError(f"encode_vp8_frames: filter_level must be 0 .. 63, got {filter_level}")
    x = _on_device(x)
    mbs = -(-H // 16) * -(-W // 16)
    first, token = hip.vp8_slot_bytes(H, W, partitions)
    # source and reconstructed planes, levels, modes and masks; the worst-case slots; the packed frames are never longer than the slots
    per_frame = 2 * 384 * mbs + (800 + 6) * mbs + 2 * (first + partitions * token) + 64
    blobs = []
    for part in _batches(x, VP8_SCRATCH_BYTES, per_frame):
        _, levels, modes, nz, skipped = hip.vp8_analyse(hip.vp8_convert(part), H, W, q)
        slots, counts = hip.vp8_code(levels, nz, modes, skipped, H, W, q, partitions, filter_level)
        packed, out_off = hip.vp8_pack(slots, counts, H, W, partitions)
        packed = packed.cpu().numpy()
        blobs += [packed[out_off[f]:out_off[f + 1]].tobytes() for f in range(part.shape[0])]
    return blobs


def _u24(v):
    return struct.pack("<I", v)[:3]


def webp_duration_ms(fps) -> int:
    """A frame's duration in whole milliseconds, at least 1: 25 fps -> 40, 8 -> 125, 29.97 -> 33."""
    return max(1, int(1000 / float(fps) + 0.5))


def write_webp(path, blobs, W, H, fps, loop=0, lossy=False):
    """VP8L payloads of encode_webp_frames -> a WebP file.  One frame: RIFF 'WEBP' { VP8L }.  Several: RIFF 'WEBP' { VP8X (flags 0x02 = animation,
    canvas W - 1 and H - 1 in 24 bits), ANIM (background 0, `loop` plays, 0 = for ever), per frame ANMF (offset 0 0, W - 1, H - 1, the duration in ms
    in 24 bits, flags 0x02 = do not blend, do not dispose) wrapping one VP8L chunk }.  Chunks are padded to even length.  lossy=True takes VP8
    payloads of encode_vp8_frames instead and writes 'VP8 ' where VP8L stands above; nothing else changes.  Returns the bytes written."""
    blobs = [bytes(b) for b in blobs]
    W, H = int(W), int(H)
    if not blobs:
        raise ValueError("write_webp: no frames")
    if not (1 <= W <= WEBP_MAX_SIDE and 1 <= H <= WEBP_MAX_SIDE):
        raise ValueError(f"write_webp: a frame is 1 .. {WEBP_MAX_SIDE} pixels a side, got {W} x {H}")
    if not float(fps) > 0:
        raise ValueError(f"write_webp: fps must be positive, got {fps}")
    loop = int(loop)
    if not 0 <= loop <= 65535:
        raise ValueError(f"write_webp: loop must be 0 .. 65535, got {loop}")
    duration = webp_duration_ms(fps)
    if duration > (1 << 24) - 1:
        raise ValueError(f"write_webp: a frame's duration is at most 2^24 - 1 ms, got fps = {fps}")
    total = 12 + sum(8 + len(b) + (len(b) & 1) for b in blobs) + (0 if len(blobs) == 1 else 18 + 14 + 24 * len(blobs))
    if total > WEBP_MAX_BYTES:
        raise ValueError(f"write_webp: {path} would pass 4 GiB - 1 ({total} bytes); a RIFF size is 32 bits")
    kind = b"VP8 " if lossy else b"VP8L"
    if len(blobs) == 1:
        body = b"WEBP" + _chunk(kind, blobs[0])
    else:
        size = _u24(W - 1) + _u24(H - 1)
        out = [b"WEBP", _chunk(b"VP8X", b"\x02\0\0\0" + size), _chunk(b"ANIM", struct.pack("<IH", 0, loop))]
        out += [_chunk(b"ANMF", _u24(0) + _u24(0) + size + _u24(duration) + b"\x02" + _chunk(kind, b)) for b in blobs]
        body = b"".join(out)
    assert len(body) + 8 == total
    return _write(path, b"RIFF" + struct.pack("<I", len(body)) + body)


def save_videos_grid(videos, path: str, rescale=False, n_rows=6, fps=8, quality=90, gif_encoder="pil", webp_quality=None, gif_dither=None,
                     gif_delta=False):
    """`quality` is the Motion-JPEG quality of .avi.  `webp_quality` = None writes .webp lossless; 0 .. 100 writes it lossy (VP8 key frames).
    `gif_dither` ("fs": Floyd-Steinberg) and `gif_delta` (frame differencing through a transparent index) are options of gif_encoder="device"."""
    if gif_encoder not in ("pil", "device"):
        raise ValueError(f"gif_encoder must be 'pil' or 'device', got {gif_encoder!r}")
    if gif_dither not in (None, "fs"):
        raise ValueError(f"gif_dither must be None or 'fs', got {gif_dither!r}")
    if gif_encoder == "pil" and (gif_dither is not None or gif_delta):
        raise ValueError("gif_dither and gif_delta are options of gif_encoder='device'; gif_encoder='pil' writes what PIL writes")
    if webp_quality is not None and not 0 <= int(webp_quality) <= 100:
        raise ValueError(f"webp_quality must be None or 0 .. 100, got {webp_quality!r}")
    if rescale:
        if torch.as_tensor(videos).dtype == torch.uint8:
            raise ValueError("rescale=True maps [-1, 1] floats to [0, 1]; uint8 frames are already in their final range")
        if torch.as_tensor(videos).shape[0] != 1:
            raise NotImplementedError("rescale with more than one clip also rescales make_grid's zero padding (to 127) in the "
                                      "reference; not reproduced: rescale each clip before calling")
        videos = (torch.as_tensor(videos).float() + 1.0) / 2.0
    frames = frames_uint8(videos, n_rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fmt = Path(path).suffix
    if fmt == ".gif" and gif_encoder == "device":
        palette, blobs = encode_gif_frames(frames, dither=gif_dither, delta=bool(gif_delta))
        write_gif(path, palette, blobs, frames.shape[2], frames.shape[1], fps, transparent=255 if gif_delta else None)
    elif fmt == ".gif":
        from PIL import Image
        pil = [Image.fromarray(f) for f in frames]
        pil[0].save(fp=path, format="GIF", append_images=pil[1:], save_all=True, duration=(1 / fps * 1000), loop=0)
    elif fmt == ".npy":
        np.save(path, frames)
    elif fmt == ".avi":
        write_avi(path, encode_jpeg_frames(frames, quality), frames.shape[2], frames.shape[1], fps)
    elif fmt in (".apng", ".png"):                                          # lossless; one frame gives an ordinary PNG
        write_apng(path, encode_png_frames(frames), frames.shape[2], frames.shape[1], fps)
    elif fmt == ".webp" and webp_quality is not None:                       # lossy; one frame gives a plain VP8 file
        write_webp(path, encode_vp8_frames(frames, int(webp_quality)), frames.shape[2], frames.shape[1], fps, lossy=True)
    elif fmt == ".webp":                                                    # lossless; one frame gives a plain VP8L file
        write_webp(path, encode_webp_frames(frames), frames.shape[2], frames.shape[1], fps)
    elif fmt == ".mp4":
        raise RuntimeError("mp4 output needs PyAV / libx264 (src/utils/util.py:83-97), which this build does not include: "
                           "write .gif or .npy, or hand frames_uint8() to your encoder")
    else:
        raise ValueError("Unsupported file type. Use .mp4 or .gif.")
