"""The device side of the lossy WebP writer (csrc/vp8.hip) against the CPU yardstick of tests/vp8_ref.py, byte for byte: planes, modes, levels,
masks, reconstruction and whole VP8 payloads; poisoned outputs with guard regions; scratch independence; range errors; then PIL reading what
encode_vp8_frames, save_videos_grid and the script write."""
import functools
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from tests import vp8_ref as R
from tests import webp_ref as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("noise", "flat", "black", "mask", "smooth", "photo")
SIZES = ((16, 16), (17, 33), (48, 40), (144, 136))              # (W, H), as in tests/test_vp8.py
QUALITIES = (10, 75, 100)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def analysed(kind, W, H, quality):
    return R.analyse(R.case_image(kind, W, H), R.quality_to_q(quality))


@functools.lru_cache(maxsize=None)
def reference(kind, W, H, quality, partitions, filter_level):
    """The yardstick's frame, its analysis shared between the partition counts."""
    recon, modes, levels, nz = analysed(kind, W, H, quality)
    q = R.quality_to_q(quality)
    level = R.default_filter_level(q) if filter_level is None else filter_level
    parts = [R.first_partition(q, partitions, level, modes, nz)] + [R.token_partition(levels, nz, p, partitions) for p in range(partitions)]
    return dict(payload=R.assemble(W, H, parts), parts=parts, recon=recon, modes=modes, levels=levels, nz=nz, skipped=int((nz == 0).sum()))


def clip_of(kind, W, H):
    """Two frames: the kind's and the next kind's, so a frame's index matters."""
    other = KINDS[(KINDS.index(kind) + 1) % len(KINDS)]
    return (kind, other), np.stack([R.case_image(kind, W, H), R.case_image(other, W, H)])


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("kind", KINDS)
def test_stages_and_payloads_equal_the_yardstick(kind, quality):
    """Every size x every partition count; the yardstick's analysis of a (kind, size, quality) is made once and shared."""
    from mmgt_amd import hip
    from mmgt_amd import video_out as V
    for W, H in SIZES:
        kinds, frames = clip_of(kind, W, H)
        x = _dev(frames)
        q, _ = hip.vp8_quantiser(quality)
        assert q == R.quality_to_q(quality)
        planes = hip.vp8_convert(x)
        for f in range(2):
            for got, want in zip(planes, R.rgb_to_yuv420(frames[f])):
                assert np.array_equal(got[f].cpu().numpy(), want)
        recon, levels, modes, nz, skipped = hip.vp8_analyse(planes, H, W, q)
        for f, k in enumerate(kinds):
            ref = reference(k, W, H, quality, 1, 0)
            assert np.array_equal(modes[f].cpu().numpy(), ref["modes"]), (W, H, f)
            assert np.array_equal(levels[f].cpu().numpy(), ref["levels"]), (W, H, f)
            assert np.array_equal(nz[f].cpu().numpy().view(np.uint32), ref["nz"]) and int(skipped[f]) == ref["skipped"]
            for got, want in zip(recon, ref["recon"]):
                assert np.array_equal(got[f].cpu().numpy(), want), (W, H, f)
        for partitions in (1, 2, 8):
            got = V.encode_vp8_frames(x, quality, partitions, 0)
            assert len(got) == 2
            for f, k in enumerate(kinds):
                w = reference(k, W, H, quality, partitions, 0)["payload"]
                assert got[f] == w, (f"{W}x{H} P={partitions} frame {f}: {len(got[f])} bytes against {len(w)}, first difference at "
                                     f"{next((i for i, (a, b) in enumerate(zip(got[f], w)) if a != b), None)}")


def test_defaults_four_partitions_and_pil_reads_the_file(tmp_path):
    from mmgt_amd import video_out as V
    W, H = 144, 136
    kinds, frames = clip_of("photo", W, H)
    # filter_level = 0: PIL's decode is the yardstick's reconstruction through libwebp's output path
    blobs = V.encode_vp8_frames(_dev(frames), 75, 4, 0)
    assert blobs == [reference(k, W, H, 75, 4, 0)["payload"] for k in kinds]
    V.write_webp(str(tmp_path / "exact.webp"), blobs, W, H, 25, lossy=True)
    img = Image.open(tmp_path / "exact.webp")
    assert img.n_frames == 2 and img.size == (W, H)
    for f, k in enumerate(kinds):
        img.seek(f)
        assert np.array_equal(np.asarray(img.convert("RGB")), R.decoded_rgb(reference(k, W, H, 75, 4, 0)["recon"], H, W)) and img.info["duration"] == 40
    # the defaults: 8 partitions at nine macroblock rows, the filter level of the quantiser index
    blobs = V.encode_vp8_frames(_dev(frames))
    assert blobs == [reference(k, W, H, 75, 8, None)["payload"] for k in kinds]
    V.write_webp(str(tmp_path / "default.webp"), blobs, W, H, 8, lossy=True)
    img = Image.open(tmp_path / "default.webp")
    assert img.n_frames == 2 and img.size == (W, H) and img.info["loop"] == 0
    for f in range(2):
        img.seek(f)
        assert np.asarray(img.convert("RGB")).shape == (H, W, 3) and img.info["duration"] == 125
    V.write_webp(str(tmp_path / "still.webp"), blobs[:1], W, H, 8, lossy=True)
    assert [k for k, _ in L.parse_chunks((tmp_path / "still.webp").read_bytes())] == [b"VP8 "]
    assert Image.open(tmp_path / "still.webp").size == (W, H)


def test_poisoned_outputs_guards_scratch_and_repeatability():
    from mmgt_amd import hip
    from mmgt_amd import video_out as V
    W, H, quality, partitions = 48, 40, 75, 2
    kinds, frames = clip_of("mask", W, H)
    x = _dev(frames)
    first = V.encode_vp8_frames(x, quality, partitions, 0)
    assert V.encode_vp8_frames(x, quality, partitions, 0) == first == [reference(k, W, H, quality, partitions, 0)["payload"] for k in kinds]
    assert V.encode_vp8_frames(frames, quality, partitions, 0) == first                    # host data: uploaded
    # the same launches by hand, every output filled with 0xFF beforehand and longer than needed
    n, guard, mbh, mbw = 2, 64, 3, 3
    mbs = mbh * mbw
    q, _ = hip.vp8_quantiser(quality)
    ff = lambda count, dt: torch.full((count + guard,), 255 if dt == torch.uint8 else -1, device="cuda", dtype=dt)

    def planes_in(bufs):
        return tuple(b[:n * s * s * mbs].view(n, s * mbh, s * mbw) for b, s in zip(bufs, (16, 8, 8)))

    def guards_ok(bufs, counts):
        return all(bool((b[c:] == (255 if b.dtype == torch.uint8 else -1)).all()) for b, c in zip(bufs, counts))
    p_bufs = [ff(n * s * s * mbs, torch.uint8) for s in (16, 8, 8)]
    planes = hip.vp8_convert(x, out=planes_in(p_bufs))
    assert guards_ok(p_bufs, [n * s * s * mbs for s in (16, 8, 8)])
    r_bufs = [ff(n * s * s * mbs, torch.uint8) for s in (16, 8, 8)]
    l_buf, m_buf, z_buf, s_buf = ff(n * mbs * 400, torch.int16), ff(n * mbs * 2, torch.uint8), ff(n * mbs, torch.int32), ff(n, torch.int32)
    recon, levels, modes, nz, skipped = hip.vp8_analyse(planes, H, W, q, out=(
        planes_in(r_bufs), l_buf[:n * mbs * 400].view(n, mbh, mbw, 25, 16), m_buf[:n * mbs * 2].view(n, mbh, mbw, 2), z_buf[:n * mbs].view(n, mbh, mbw),
        s_buf[:n]))
    assert guards_ok(r_bufs + [l_buf, m_buf, z_buf, s_buf], [n * s * s * mbs for s in (16, 8, 8)] + [n * mbs * 400, n * mbs * 2, n * mbs, n])
    for f, k in enumerate(kinds):
        ref = reference(k, W, H, quality, partitions, 0)
        assert np.array_equal(levels[f].cpu().numpy(), ref["levels"]) and np.array_equal(recon[0][f].cpu().numpy(), ref["recon"][0])
    fb, tb = hip.vp8_slot_bytes(H, W, partitions)
    assert (fb, tb) == (R.HEADER_SYMBOLS + R.MB_MODE_SYMBOLS * mbs + R.FLUSH_BYTES, R.MB_TOKEN_SYMBOLS * 2 * mbw + R.FLUSH_BYTES)
    total = n * (fb + partitions * tb)
    slot_buf, c_buf = ff(total, torch.uint8), ff(n * (1 + partitions), torch.int64)
    slots, counts = hip.vp8_code(levels, nz, modes, skipped, H, W, q, partitions, 0, out=(slot_buf[:total], c_buf[:n * (1 + partitions)].view(n, 1 + partitions)))
    assert guards_ok([slot_buf, c_buf], [total, n * (1 + partitions)])
    want_counts = [[len(p) for p in reference(k, W, H, quality, partitions, 0)["parts"]] for k in kinds]
    assert counts.cpu().numpy().tolist() == want_counts
    for f in range(n):                                                                   # nothing written past a partition's bytes inside its slot
        base = f * (fb + partitions * tb)
        assert bool((slots[base + want_counts[f][0]:base + fb] == 255).all())
    size = sum(10 + 3 * (partitions - 1) + sum(c) for c in want_counts)
    out_buf = ff(size, torch.uint8)
    packed, off = hip.vp8_pack(slots, counts, H, W, partitions, out=out_buf)
    assert int(off[-1]) == size and guards_ok([out_buf], [size])
    packed = packed.cpu().numpy()
    assert [packed[off[f]:off[f + 1]].tobytes() for f in range(n)] == first
    # one frame per set of launches
    old = V.VP8_SCRATCH_BYTES
    try:
        V.VP8_SCRATCH_BYTES = 1
        calls = [hip.call_count(w) for w in ("mmgt_vp8_convert", "mmgt_vp8_analyse", "mmgt_vp8_code", "mmgt_vp8_pack")]
        assert V.encode_vp8_frames(x, quality, partitions, 0) == first
        assert [hip.call_count(w) for w in ("mmgt_vp8_convert", "mmgt_vp8_analyse", "mmgt_vp8_code", "mmgt_vp8_pack")] == [c + n for c in calls]
    finally:
        V.VP8_SCRATCH_BYTES = old


def test_range_errors():
    from mmgt_amd import hip
    from mmgt_amd import video_out as V
    import ctypes
    Lb = hip.lib()
    x = _dev(np.zeros((1, 16, 16, 3), np.uint8))
    p = x.data_ptr()
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    la, lb = ctypes.c_longlong(0), ctypes.c_longlong(0)
    assert Lb.mmgt_vp8_quantiser(101, ctypes.byref(a), ctypes.byref(b)) != 0 and b"0 .. 100" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_quantiser(-1, ctypes.byref(a), ctypes.byref(b)) != 0
    assert Lb.mmgt_vp8_slot_bytes(16, 16384, 1, ctypes.byref(la), ctypes.byref(lb)) != 0 and b"range" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_slot_bytes(16, 16, 3, ctypes.byref(la), ctypes.byref(lb)) != 0 and b"1, 2, 4 or 8" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_convert(p, p, p, p, 1, 16384, 16, None) != 0 and b"range" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_convert(p, p, p, p, 0, 16, 16, None) != 0 and b"range" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_convert(None, p, p, p, 1, 16, 16, None) != 0
    assert Lb.mmgt_vp8_analyse(p, p, p, p, p, p, p, p, p, p, 1, 16, 16384, 0, None) != 0 and b"range" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_analyse(p, p, p, p, p, p, p, p, p, p, 1, 16, 16, 128, None) != 0 and b"0 .. 127" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_code(p, p, p, p, p, 1 << 30, p, 1, 16, 16, 0, 3, 0, None) != 0 and b"1, 2, 4 or 8" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_code(p, p, p, p, p, 1 << 30, p, 1, 16, 16, 0, 1, 64, None) != 0 and b"0 .. 63" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_code(p, p, p, p, p, 1 << 30, p, 0, 16, 16, 0, 1, 0, None) != 0 and b"range" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_code(p, p, p, p, p, 100, p, 1, 16, 16, 0, 1, 0, None) != 0 and b"slots_bytes" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_pack(p, 1 << 30, p, p, p, 100, 1, 16, 16, 5, None) != 0 and b"1, 2, 4 or 8" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_pack(p, 1 << 30, p, p, p, 100, 1, 16385, 16, 1, None) != 0 and b"range" in Lb.mmgt_last_error()
    assert Lb.mmgt_vp8_pack(p, 10, p, p, p, 100, 1, 16, 16, 1, None) != 0 and b"slots_bytes" in Lb.mmgt_last_error()
    with pytest.raises(ValueError, match="at most 16383"):
        V.encode_vp8_frames(np.zeros((1, 1, 16384, 3), np.uint8))
    with pytest.raises(ValueError, match="empty clip"):
        V.encode_vp8_frames(np.zeros((0, 16, 16, 3), np.uint8))
    for quality in (-1, 101):
        with pytest.raises(ValueError, match="quality"):
            V.encode_vp8_frames(np.zeros((1, 16, 16, 3), np.uint8), quality)
    for partitions in (0, 3, 16):
        with pytest.raises(ValueError, match="partitions"):
            V.encode_vp8_frames(np.zeros((1, 16, 16, 3), np.uint8), 75, partitions)
    for level in (-1, 64):
        with pytest.raises(ValueError, match="filter_level"):
            V.encode_vp8_frames(np.zeros((1, 16, 16, 3), np.uint8), 75, 1, level)
    assert V.encode_vp8_frames(np.zeros((1, 16, 16, 3), np.uint8), 75, 1, 0) == [R.encode_frame(np.zeros((16, 16, 3), np.uint8), 75, 1, 0)["payload"]]


def test_save_videos_grid_lossy_webp(tmp_path):
    from mmgt_amd import video_out as V
    g = torch.Generator().manual_seed(3)
    videos = torch.rand((1, 3, 4, 40, 24), generator=g)
    want = V.frames_uint8(videos)
    path = tmp_path / "clip.webp"
    V.save_videos_grid(videos, str(path), fps=8, webp_quality=75)
    data = path.read_bytes()
    chunks = L.parse_chunks(data)
    assert [k for k, _ in chunks] == [b"VP8X", b"ANIM"] + [b"ANMF"] * 4 and all(body[16:20] == b"VP8 " for k, body in chunks if k == b"ANMF")
    assert data == R.webp_file([R.encode_frame(f, 75)["payload"] for f in want], 24, 40, 125, 0)
    img = Image.open(path)
    assert img.n_frames == 4 and img.size == (24, 40) and img.info["loop"] == 0
    for k in range(4):
        img.seek(k)
        assert np.asarray(img.convert("RGB")).shape == (40, 24, 3) and img.info["duration"] == 125
    V.save_videos_grid(videos, str(tmp_path / "lossless.webp"), fps=8)                     # without the argument: the lossless bytes
    assert (tmp_path / "lossless.webp").read_bytes() == L.webp_file(V.encode_webp_frames(want), 24, 40, 8, 0)
    assert len(data) < os.path.getsize(tmp_path / "lossless.webp")
    with pytest.raises(ValueError, match=r"Unsupported file type. Use .mp4 or .gif."):
        V.save_videos_grid(videos, str(tmp_path / "clip.webm"), webp_quality=75)


def test_pose2vid_synthetic_lossy_webp(tmp_path):
    from mmgt_amd import video_out as V
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pose2vid.py"), "--synthetic", "-W", "64", "-H", "64", "-L", "8", "--steps", "2",
                        "--format", "webp", "--webp_quality", "60", "--out_dir", str(tmp_path)], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lossy = json.loads(r.stdout.strip().splitlines()[-1])
    assert lossy["webp_quality"] == 60
    assert lossy["webp"].endswith(".webp") and lossy["webp_bytes"] == os.path.getsize(lossy["webp"])
    # what the same command writes without the flag: the lossless file of the clip the script saved
    V.save_videos_grid(torch.load(lossy["saved"]), str(tmp_path / "lossless.webp"), n_rows=1, fps=25)
    lossless = {"webp_bytes": os.path.getsize(tmp_path / "lossless.webp")}
    chunks = L.parse_chunks(open(lossy["webp"], "rb").read())
    assert chunks[0][0] == b"VP8X" and sum(1 for k, body in chunks if k == b"ANMF" and body[16:20] == b"VP8 ") == 8
    img = Image.open(lossy["webp"])
    assert img.n_frames == 8 and img.size == (64, 64)
    img.seek(7)
    assert np.asarray(img.convert("RGB")).std() > 0 and img.info["duration"] == 40
    assert lossy["webp_bytes"] < lossless["webp_bytes"]
