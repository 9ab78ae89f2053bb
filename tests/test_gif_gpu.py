"""The device side of the opt-in GIF writer (csrc/gif.hip) through the C ABI: histogram and index map against numpy, LZW + pack against PIL's
decoder and the yardstick coder of tests/test_gif.py, slot bounds with guard regions, then save_videos_grid(gif_encoder="device") and the script.

Size gate (test_stream_is_no_longer_than_the_yardsticks): the device coder follows the yardstick's rule (Clear as soon as code 4095 is defined),
so with one strip per frame its stream has the yardstick's length: expected ratio 1.000 (a host-thread emulation of the kernels gave equal byte
counts on the gated inputs; the test prints the ratio it finds on the GPU).  The gate is that ratio plus 1 % for inputs not tried."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from tests.test_gif import distinct_palette, lzw_decode, lzw_encode, read_gif_indices, unblock

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                                                       # bytes of 0xA5-style filler after every slot
SIZE_RATIO_GATE = 1.0 * 1.01


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bins(frames):
    f = frames.astype(np.int64)
    return (f[..., 0] >> 3) << 10 | (f[..., 1] >> 3) << 5 | (f[..., 2] >> 3)


def _rgb_cases():
    rng = np.random.default_rng(21)
    return {"random_3x40x56": rng.integers(0, 256, (3, 40, 56, 3), dtype=np.uint8),
            "one_colour_8x8": np.broadcast_to(np.array([200, 17, 99], np.uint8), (1, 8, 8, 3)).copy(),
            "odd_33x17": rng.integers(0, 256, (1, 17, 33, 3), dtype=np.uint8)}


@pytest.mark.parametrize("case", ["random_3x40x56", "one_colour_8x8"])
def test_histogram_equals_bincount(case):
    from mmgt_amd import hip
    frames = _rgb_cases()[case]
    got = hip.gif_histogram(_dev(frames)).cpu().numpy().view(np.uint32)
    want = np.bincount(_bins(frames).reshape(-1), minlength=32768)
    assert got.shape == (32768,) and np.array_equal(got.astype(np.int64), want)
    assert int(got.sum()) == frames.size // 3


@pytest.mark.parametrize("case", ["random_3x40x56", "one_colour_8x8", "odd_33x17"])
def test_index_map_equals_lut_of_bin(case):
    from mmgt_amd import hip
    frames = _rgb_cases()[case]
    lut = np.random.default_rng(4).integers(0, 256, 32768, dtype=np.uint8)               # any table: the kernel only looks up
    got = hip.gif_index(_dev(frames), _dev(lut)).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, lut[_bins(frames)])


# ---- LZW + pack ----------------------------------------------------------------------------------------------------------------------------------
def _bars():
    f0 = np.broadcast_to(((np.arange(64) // 8) % 2).astype(np.uint8), (48, 64))          # two colours, vertical bars of 8 pixels
    return np.stack([np.roll(f0, k, axis=1) for k in (0, 3, 5)])


def _lzw_cases():
    rng = np.random.default_rng(5)
    rnd = rng.integers(0, 256, (1, 96, 128), dtype=np.uint8)
    return {"one_index_8x8": (np.full((1, 8, 8), 7, np.uint8), 16),                      # strip_rows > H: a frame shorter than one strip
            "random_33x17": (rng.integers(0, 256, (1, 17, 33), dtype=np.uint8), 4),     # odd sizes, last strip of one row
            "random_128x96_one_strip": (rnd, 96),                                        # the dictionary fills and Clears mid-strip
            "random_128x96_strips_of_8": (rnd, 8),                                       # twelve strips joined at arbitrary bit offsets
            "bars_64x48x3": (_bars(), 48),                                               # long matches
            "random_128x24_one_strip": (rnd[:, :24], 24)}                                # the width grows 9 -> 12 and the dictionary does not fill


def _encode(idx, strip_rows, fill):
    """(n, H, W) indices -> (blobs, bits (n, strips), the bound of a strip in bytes), through buffers whose every slot is followed by GUARD bytes
    of `fill`; asserts that the filler is intact.  The ABI takes ONE stride per buffer (slot size = slot spacing), so the guard lies inside the
    stride that is passed; the strip's own bound, mmgt_gif_strip_stride, is what `bits` is held to."""
    from mmgt_amd import hip
    n, H, W = idx.shape
    strips = -(-H // strip_rows)
    bound = hip.gif_strip_stride(W, strip_rows)
    slots = torch.full((n * strips, bound + GUARD), fill, device="cuda", dtype=torch.uint8)
    bits = torch.full((n, strips), -3, device="cuda", dtype=torch.int64)
    hip.gif_lzw(_dev(idx), strip_rows, out=(slots, bits))
    pbound = hip.gif_packed_stride(strips, bound + GUARD)
    packed = torch.full((n, pbound + GUARD), fill, device="cuda", dtype=torch.uint8)
    sizes = torch.full((n,), -9, device="cuda", dtype=torch.int32)
    hip.gif_pack(slots, bits, out=(packed, sizes))
    slots_h, bits_h, packed_h, sizes_h = slots.cpu().numpy(), bits.cpu().numpy(), packed.cpu().numpy(), sizes.cpu().numpy()
    assert (bits_h >= 9).all() and (bits_h <= 8 * bound).all(), (bits_h.max(), 8 * bound)
    for s, b in enumerate(bits_h.reshape(-1)):
        written = 4 * -(-int(b) // 32)                                                   # the coder stores whole words
        assert written <= bound and (slots_h[s, written:] == fill).all(), f"slot {s}: bytes after word {written // 4} were touched"
    assert (slots_h[:, bound:] == fill).all()
    for f in range(n):
        total = int(bits_h[f].sum())
        nbytes = -(-total // 8)
        assert sizes_h[f] == nbytes + -(-nbytes // 255) + 1 <= pbound
        assert (packed_h[f, sizes_h[f]:] == fill).all(), f"frame {f}: bytes after its {sizes_h[f]} were touched"
    return [packed_h[f, :sizes_h[f]].tobytes() for f in range(n)], bits_h, bound


@pytest.mark.parametrize("case", sorted(_lzw_cases()))
def test_lzw_and_pack_decode_to_the_input_indices(case, tmp_path):
    from mmgt_amd.video_out import write_gif
    idx, strip_rows = _lzw_cases()[case]
    n, H, W = idx.shape
    blobs, bits, bound = _encode(idx, strip_rows, 0xA5)
    blobs2, bits2, _ = _encode(idx, strip_rows, 0x3C)                                    # other filler in every buffer: the same bytes
    assert blobs == blobs2 and np.array_equal(bits, bits2)
    print(f"{case}: strips {bits.shape[1]}, bits {bits.sum(1).tolist()}, largest strip {int(bits.max())} of {8 * bound} bits")
    pal = distinct_palette(2)
    path = tmp_path / "d.gif"
    write_gif(str(path), pal, blobs, W, H, 25)
    back, img = read_gif_indices(path, pal)
    assert img.n_frames == n and img.size == (W, H)
    assert np.array_equal(back, idx)
    for f, blob in enumerate(blobs):
        stream = unblock(blob)
        assert len(stream) == -(-int(bits[f].sum()) // 8)
        assert all(blob[p] == 255 for p in range(0, len(blob) - 256, 256))              # full sub-blocks but the last
        assert np.array_equal(lzw_decode(stream, H * W).reshape(H, W), idx[f])           # one strip or joined strips: one stream for the yardstick


@pytest.mark.parametrize("case", ["random_128x96_one_strip", "bars_64x48x3", "random_128x24_one_strip"])
def test_stream_is_no_longer_than_the_yardsticks(case):
    idx, strip_rows = _lzw_cases()[case]
    assert strip_rows == idx.shape[1]
    _, bits, _ = _encode(idx, strip_rows, 0xA5)
    for f in range(idx.shape[0]):
        ref, full_clears = lzw_encode(idx[f])
        got = -(-int(bits[f, 0]) // 8)
        print(f"{case} frame {f}: device {got} B ({int(bits[f, 0])} bits), yardstick {len(ref)} B, ratio {got / len(ref):.6f}, "
              f"yardstick dictionary-full Clears {full_clears}")
        assert (full_clears >= 1) == (case == "random_128x96_one_strip")
        assert got <= SIZE_RATIO_GATE * len(ref)


def test_bad_arguments_are_refused_before_any_launch():
    from mmgt_amd import hip
    L = hip.lib()
    x = _dev(np.zeros((1, 8, 8, 3), np.uint8))
    idx = _dev(np.zeros((1, 8, 8), np.uint8))
    buf = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    bits = torch.zeros(8, device="cuda", dtype=torch.int64)
    sizes = torch.zeros(8, device="cuda", dtype=torch.int32)
    hist = torch.zeros(32768, device="cuda", dtype=torch.int32)
    p = lambda t: t.data_ptr()
    assert L.mmgt_gif_histogram(p(x), p(hist), 0, 8, 8, None) != 0 and b"range" in L.mmgt_last_error()
    assert L.mmgt_gif_histogram(None, p(hist), 1, 8, 8, None) != 0
    assert L.mmgt_gif_index(p(x), p(hist), p(idx), 1, 70000, 8, None) != 0
    assert L.mmgt_gif_index(p(x) + 1, p(hist), p(idx), 1, 8, 8, None) != 0 and b"aligned" in L.mmgt_last_error()
    assert L.mmgt_gif_lzw(p(idx), p(buf), p(bits), 1, 8, 8, 8, 64, None) != 0 and b"worst case" in L.mmgt_last_error()
    assert L.mmgt_gif_lzw(p(idx), p(buf), p(bits), 1, 8, 8, 0, 4096, None) != 0
    assert L.mmgt_gif_pack(p(buf), p(bits), p(buf), p(sizes), 1, 1, 128, 128, None) != 0 and b"worst case" in L.mmgt_last_error()
    assert L.mmgt_gif_pack(p(buf), p(bits), p(buf), p(sizes), 1, 5000, 128, 1 << 20, None) != 0
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0 and int(buf.sum()) == 0
    assert hip.gif_strip_stride(128, 8) == (12 * (1024 + 2) // 8 + 15) // 16 * 16
    assert hip.gif_strip_stride(512, 16) == ((12 * (8192 + 8192 // 3838 + 2) + 7) // 8 + 15) // 16 * 16


# ---- the layers above ----------------------------------------------------------------------------------------------------------------------------
def _gradient_clip():
    yy, xx = np.mgrid[0:48, 0:64]
    clip = np.zeros((1, 3, 48, 64, 3), np.uint8)
    for k in range(3):
        clip[0, k, ..., 0] = 4 * xx
        clip[0, k, ..., 1] = 5 * yy
        clip[0, k, ..., 2] = 2 * xx + 2 * yy
        clip[0, k, 10 + 6 * k:22 + 6 * k, 8 + 9 * k:20 + 9 * k] = (250, 30, 30)           # the moving square
    return clip


def test_save_videos_grid_device_gif_is_the_palette_lookup_of_every_pixel(tmp_path):
    from mmgt_amd import video_out
    clip = _gradient_clip()
    path = tmp_path / "t.gif"
    video_out.save_videos_grid(torch.from_numpy(clip), str(path), fps=25, gif_encoder="device")
    img = Image.open(path)
    assert img.n_frames == 3 and img.size == (64, 48) and img.info["duration"] == 40 and img.info["loop"] == 0
    palette = np.array(img.getpalette()[:768], np.uint8).reshape(256, 3)
    hist = np.bincount(_bins(clip[0]).reshape(-1), minlength=32768)
    assert hist[hist > 0].size > 256, "the clip must need the median cut"
    assert np.array_equal(palette, video_out.gif_palette(hist))
    pal2, blobs = video_out.encode_gif_frames(clip[0])
    assert np.array_equal(pal2, palette) and len(blobs) == 3
    want = palette[video_out.gif_lut(palette)[_bins(clip[0])]]                            # (3, 48, 64, 3)
    for k in range(3):
        img.seek(k)
        assert np.array_equal(np.asarray(img.convert("RGB")), want[k]), f"frame {k}"
    # a palette handed in is used as it is; chunking by the scratch budget gives the same frames
    pal3, blobs3 = video_out.encode_gif_frames(_dev(clip[0]), palette=palette)
    assert np.array_equal(pal3, palette) and blobs3 == blobs
    old = video_out.GIF_SCRATCH_BYTES
    try:
        video_out.GIF_SCRATCH_BYTES = 1
        assert video_out.encode_gif_frames(clip[0])[1] == blobs
    finally:
        video_out.GIF_SCRATCH_BYTES = old


def test_save_videos_grid_pil_gif_is_unchanged(tmp_path):
    from mmgt_amd import video_out
    clip = _gradient_clip()
    for kw in ({}, {"gif_encoder": "pil"}):
        path = tmp_path / "p.gif"
        video_out.save_videos_grid(torch.from_numpy(clip), str(path), fps=25, **kw)
        pil = [Image.fromarray(f) for f in clip[0]]
        ref = io.BytesIO()
        pil[0].save(fp=ref, format="GIF", append_images=pil[1:], save_all=True, duration=(1 / 25 * 1000), loop=0)
        assert path.read_bytes() == ref.getvalue()


def test_pose2vid_synthetic_gif_encoder_device(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pose2vid.py"), "--synthetic", "-W", "64", "-H", "64", "-L", "8", "--steps", "2",
                        "--format", "gif", "--gif_encoder", "device", "--out_dir", str(tmp_path)], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["gif"].endswith(".gif") and rec["gif_bytes"] == os.path.getsize(rec["gif"])
    img = Image.open(rec["gif"])
    assert img.n_frames == 8 and img.size == (64, 64) and img.info["duration"] == 40
    img.seek(7)
    assert np.asarray(img.convert("RGB")).std() > 0
