"""The device side of the PNG / APNG writer (csrc/png.hip) against the CPU yardstick of tests/png_ref.py, byte for byte: filtered rows and whole zlib
streams of frames, crafted byte buffers through the low-level wrappers, scratch independence, then PIL reading what save_videos_grid and the script
write."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP_ROWS = (1, 5, 16, 37, 1000)
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frames(kind):
    """The inputs, made once: the (3, 37, 29) contents and the degenerate shapes."""
    if not _cache:
        rng = np.random.default_rng(17)
        noise = rng.integers(0, 256, (3, 37, 29, 3), dtype=np.uint8)
        noise[0].reshape(-1)[:256] = np.arange(256)                                      # every literal occurs
        _cache.update({"noise": noise, "flat": np.full((3, 37, 29, 3), 143, np.uint8), "smooth": R.smooth_frames(3, 37, 29),
                       "pose": R.pose_frames(3, 37, 29), "1x1": np.array([[[[9, 0, 200]]], [[[0, 0, 0]]]], np.uint8),
                       "300x1": R.smooth_frames(1, 1, 300), "1x300": rng.integers(0, 4, (1, 300, 1, 3), dtype=np.uint8) * 60})
    return _cache[kind]


def _reference(kind, strip_rows):
    key = ("ref", kind, strip_rows)
    if key not in _cache:
        _cache[key] = R.encode_frames(_frames(kind), strip_rows)
    return _cache[key]


@pytest.mark.parametrize("kind", ["noise", "flat", "smooth", "pose", "1x1", "300x1", "1x300"])
def test_filter_equals_the_yardstick(kind):
    from mmgt_amd import hip
    frames = _frames(kind)
    want = R.filter_frames(frames)
    filt, sums = hip.png_filter(_dev(frames))
    assert np.array_equal(filt.cpu().numpy(), want)
    L = want.shape[2]
    w = want.astype(np.int64)
    assert np.array_equal(sums.cpu().numpy(), np.stack([w.sum(2), (w * (L - np.arange(L))).sum(2)], axis=2))


@pytest.mark.parametrize("strip_rows", STRIP_ROWS)
@pytest.mark.parametrize("kind", ["noise", "flat", "smooth", "pose", "1x1", "300x1", "1x300"])
def test_streams_equal_the_yardstick(kind, strip_rows):
    from mmgt_amd.video_out import encode_png_frames
    frames = _frames(kind)
    got = encode_png_frames(_dev(frames), strip_rows=strip_rows)
    want = _reference(kind, strip_rows)
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"frame {f}: {len(g)} bytes against {len(w)}, first difference at {next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), None)}"


def _runs(lengths, values=(7, 7, 200, 0)):
    """Runs of the given lengths; neighbours differ, so each is a maximal run."""
    out, k = [], 0
    for n in lengths:
        v = values[k % len(values)] + (k % 2)
        out.append(bytes([v]) * n)
        k += 1
    return b"".join(out)


def _crafted():
    edge = list(range(1, 6)) + list(range(258, 264)) + list(range(516, 522))            # remainders 0, 1, 2, 3 after a 258-match, and two of them
    rng = np.random.default_rng(23)
    return {"runs_one_strip": (_runs(edge), 1 << 20),
            "runs_reversed": (_runs(edge[::-1]), 1 << 20),
            "run_cut_by_strips": (b"ab" + b"\x05" * 700 + b"c", 300),                    # the run crosses two strip boundaries and restarts at each
            "strip_of_one_byte": (_runs([4, 9, 260]) + b"z", 273),                       # 274 bytes: the last strip is the single byte z
            "strips_of_one_byte": (b"\x00\x00\x00\x01\x01", 1),
            "chunk_edges": (_runs([255, 1, 2, 254, 3, 509, 258, 259]), 1 << 20),         # runs that start and end around the 256-position rounds
            "two_rows": (rng.integers(0, 3, 2 * 1500, dtype=np.uint8).tobytes(), 700)}   # two buffers in one call (see the test)


@pytest.mark.parametrize("case", sorted(_crafted()))
def test_crafted_buffers_through_the_low_level_wrapper(case):
    from mmgt_amd.video_out import deflate_strips_device
    data, strip_bytes = _crafted()[case]
    rows = 2 if case == "two_rows" else 1
    buf = np.frombuffer(data, np.uint8).reshape(rows, -1).copy()
    got = deflate_strips_device(_dev(buf), strip_bytes)
    assert len(got) == rows
    for r in range(rows):
        assert got[r] == R.deflate_strips(buf[r].tobytes(), strip_bytes)
        assert zlib.decompress(got[r], -15) == buf[r].tobytes()


def test_repeatable_and_independent_of_what_the_buffers_held():
    from mmgt_amd import hip
    from mmgt_amd import video_out as V
    frames = _frames("smooth")
    x = _dev(frames)
    first = V.encode_png_frames(x, strip_rows=5)
    assert V.encode_png_frames(x, strip_rows=5) == first == _reference("smooth", 5)
    # the same launches by hand, every output and scratch tensor filled with 0xFF beforehand
    n, H, W, _ = frames.shape
    L, sb, strips = 1 + 3 * W, 5 * (1 + 3 * W), -(-H // 5)
    ff = lambda shape, dt: torch.full(shape, -1, device="cuda", dtype=dt) if dt != torch.uint8 else torch.full(shape, 255, device="cuda", dtype=dt)
    filt, sums = hip.png_filter(x, out=(ff((n, H, L), torch.uint8), ff((n, H, 2), torch.int64)))
    data = filt.view(n, H * L)
    hist = hip.png_histogram(data, sb, out=ff((n, strips, 286), torch.int32)).cpu().numpy().view(np.uint32).astype(np.int64)
    tables = [[V.png_strip_tables(hist[f, s], s == strips - 1) for s in range(strips)] for f in range(n)]
    codes = np.array([[t[0] for t in row] for row in tables], np.uint32)
    heads = np.zeros((n, strips, hip.PNG_HEADER_BYTES), np.uint8)
    for f in range(n):
        for s in range(strips):
            heads[f, s, :len(tables[f][s][1])] = np.frombuffer(tables[f][s][1], np.uint8)
    hbits = np.array([[t[2] for t in row] for row in tables], np.int32)
    want = np.array([[t[3] for t in row] for row in tables], np.int64)
    words = int(hip.png_slot_offsets(want)[-1])
    guard = 16
    slots, bits = hip.png_deflate(data, sb, codes, heads, hbits, want, out=(ff((words + guard,), torch.int32), ff((n, strips), torch.int64)))
    assert np.array_equal(bits.cpu().numpy(), want)
    assert (slots[words:] == -1).all()                                                    # nothing past the last slot
    total = int(((want.sum(1) + 7) // 8).sum())
    packed, off = hip.png_pack(slots, want, out=ff((total + guard,), torch.uint8))
    assert int(off[-1]) == total and (packed[total:] == 255).all()
    packed, sums = packed.cpu().numpy(), sums.cpu().numpy()
    for f in range(n):
        adler = 1
        for s1, s2 in sums[f].tolist():
            adler = V.adler32_combine(adler, ((L + s2) % 65521) << 16 | (1 + s1) % 65521, L)
        assert b"\x78\x01" + packed[off[f]:off[f + 1]].tobytes() + adler.to_bytes(4, "big") == first[f]
    # one frame per set of launches
    old = V.PNG_SCRATCH_BYTES
    try:
        V.PNG_SCRATCH_BYTES = 1
        assert V.encode_png_frames(frames, strip_rows=5) == first                         # host data: uploaded
    finally:
        V.PNG_SCRATCH_BYTES = old


def test_a_wrong_bit_count_raises():
    from mmgt_amd import hip
    from mmgt_amd import video_out as V
    buf = _dev(np.frombuffer(b"abcabcabc" * 20, np.uint8).reshape(1, -1).copy())
    real = V.png_strip_tables

    def one_bit_more(hist, final):
        table, head, hbits, want = real(hist, final)
        return table, head, hbits, want + 1
    V.png_strip_tables = one_bit_more
    try:
        with pytest.raises(RuntimeError, match="bits on the device"):
            V.deflate_strips_device(buf, 64)
    finally:
        V.png_strip_tables = real
    assert zlib.decompress(V.deflate_strips_device(buf, 64)[0], -15) == b"abcabcabc" * 20
    L = hip.lib()
    assert L.mmgt_png_filter(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1, 16385, 1, None) != 0 and b"range" in L.mmgt_last_error()
    assert L.mmgt_png_histogram(buf.data_ptr(), buf.data_ptr(), 1, 180, 0, None) != 0 and b"range" in L.mmgt_last_error()
    assert L.mmgt_png_histogram(None, buf.data_ptr(), 1, 180, 10, None) != 0


def test_pil_reads_the_apng_and_the_sequence(tmp_path):
    from mmgt_amd import video_out as V
    frames = _frames("smooth")
    n, H, W, _ = frames.shape
    blobs = V.encode_png_frames(_dev(frames))
    V.write_apng(str(tmp_path / "c.apng"), blobs, W, H, 25)
    img = Image.open(tmp_path / "c.apng")
    assert img.n_frames == n and img.size == (W, H)
    for k in range(n):
        img.seek(k)
        assert np.array_equal(np.asarray(img.convert("RGB")), frames[k])
    for k, p in enumerate(V.write_png_sequence(tmp_path / "seq", blobs, W, H)):
        one = Image.open(p)
        assert one.mode == "RGB" and np.array_equal(np.asarray(one), frames[k])


def test_save_videos_grid_apng_and_png(tmp_path):
    from mmgt_amd import video_out as V
    g = torch.Generator().manual_seed(3)
    videos = torch.rand((1, 3, 4, 40, 24), generator=g)
    want = V.frames_uint8(videos)
    for name in ("clip.apng", "clip.png"):
        path = tmp_path / name
        V.save_videos_grid(videos, str(path), fps=8)
        img = Image.open(path)
        assert img.n_frames == 4 and img.size == (24, 40) and img.info["duration"] == 125.0
        for k in range(4):
            img.seek(k)
            assert np.array_equal(np.asarray(img.convert("RGB")), want[k]), (name, k)
    V.save_videos_grid(videos[:, :, :1], str(tmp_path / "still.png"))
    still = Image.open(tmp_path / "still.png")
    assert getattr(still, "n_frames", 1) == 1 and np.array_equal(np.asarray(still), want[0])
    with pytest.raises(RuntimeError, match="mp4 output needs PyAV / libx264"):
        V.save_videos_grid(videos, str(tmp_path / "clip.mp4"))
    with pytest.raises(ValueError, match=r"Unsupported file type. Use .mp4 or .gif."):
        V.save_videos_grid(videos, str(tmp_path / "clip.webm"))


def test_pose2vid_synthetic_apng(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pose2vid.py"), "--synthetic", "-W", "64", "-H", "64", "-L", "8", "--steps", "2",
                        "--format", "apng", "--out_dir", str(tmp_path)], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["apng"].endswith(".apng") and rec["apng_bytes"] == os.path.getsize(rec["apng"])
    img = Image.open(rec["apng"])
    assert img.n_frames == 8 and img.size == (64, 64) and img.info["duration"] == 40.0
    img.seek(7)
    assert np.asarray(img.convert("RGB")).std() > 0
