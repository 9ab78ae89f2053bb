"""The device side of the WebP lossless writer (csrc/webp.hip) against the CPU yardstick of tests/webp_ref.py, byte for byte: block modes, residual
words, strip histograms, bit counts and whole VP8L payloads of frames, crafted residual buffers through the low-level wrappers, scratch
independence, then PIL reading what save_videos_grid and the script write."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_ref as P
from tests import webp_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIP_ROWS = (1, 5, 16, 37, 1000)
KINDS = ["noise", "flat", "black", "mask", "smooth", "gradient", "1x1", "300x1", "1x300", "16x17", "17x16", "33x47"]
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frames(kind):
    """The inputs, made once: three frames of each content at 37 x 29 (W x H) and the other sizes."""
    if not _cache:
        rng = np.random.default_rng(17)
        noise = rng.integers(0, 256, (3, 29, 37, 3), dtype=np.uint8)
        noise[0].reshape(-1)[:256] = np.arange(256)                                      # every literal occurs
        _cache.update({"noise": noise, "flat": np.full((3, 29, 37, 3), 143, np.uint8), "black": np.zeros((3, 29, 37, 3), np.uint8),
                       "mask": R.mask_frames(3, 29, 37), "smooth": P.smooth_frames(3, 29, 37), "gradient": R.gradient_frames(3),
                       "1x1": np.array([[[[9, 0, 200]]], [[[0, 0, 0]]], [[[255, 255, 255]]]], np.uint8), "300x1": P.smooth_frames(3, 1, 300),
                       "1x300": rng.integers(0, 4, (3, 300, 1, 3), dtype=np.uint8) * 60, "16x17": P.smooth_frames(3, 17, 16),
                       "17x16": rng.integers(0, 2, (3, 16, 17, 3), dtype=np.uint8) * 255, "33x47": P.smooth_frames(3, 47, 33)})
    return _cache[kind]


def _reference(kind, strip_rows):
    key = ("ref", kind, min(strip_rows, _frames(kind).shape[1]))
    if key not in _cache:
        _cache[key] = [R.frame_parts(f, key[2]) for f in _frames(kind)]
    return _cache[key]


def _hist_rows(parts):
    return np.array([h[0] + h[1] + h[2] + [h[3]] for h in parts["hist"]], np.int64)


@pytest.mark.parametrize("kind", KINDS)
def test_modes_and_residuals_equal_the_yardstick(kind):
    from mmgt_amd import hip
    frames = _frames(kind)
    modes, res = hip.webp_predict(_dev(frames))
    ref = _reference(kind, 1000)
    assert np.array_equal(modes.cpu().numpy(), np.stack([p["modes"] for p in ref]))
    assert np.array_equal(res.cpu().numpy().view(np.uint32), np.stack([p["words"] for p in ref]))


@pytest.mark.parametrize("strip_rows", STRIP_ROWS)
@pytest.mark.parametrize("kind", KINDS)
def test_histograms_bit_counts_and_payloads_equal_the_yardstick(kind, strip_rows):
    from mmgt_amd import hip
    from mmgt_amd import video_out as V
    frames = _frames(kind)
    n, H, W, _ = frames.shape
    ref = _reference(kind, strip_rows)
    x = _dev(frames)
    rows = min(strip_rows, H)
    modes, res = hip.webp_predict(x)
    data = res.view(n, H * W)
    hist = hip.webp_histogram(data, rows * W).cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(hist, np.stack([_hist_rows(p) for p in ref]))
    tabs = [V.webp_frame_tables(hist[f].sum(0)) for f in range(n)]
    heads = [V.webp_frame_header(W, H, modes[f].cpu().numpy(), tabs[f][2]) for f in range(n)]
    want = np.array([[heads[f][1]] + (hist[f] @ tabs[f][1]).tolist() for f in range(n)], np.int64)
    slots, bits = hip.webp_code(data, rows * W, np.stack([t[0] for t in tabs]), [h[0] for h in heads], want)
    assert bits.cpu().numpy().tolist() == [p["strip_bits"] for p in ref]
    got = V.encode_webp_frames(x, strip_rows=strip_rows)
    assert len(got) == n
    for f, (g, p) in enumerate(zip(got, ref)):
        w = p["payload"]
        assert g == w, f"frame {f}: {len(g)} bytes against {len(w)}, first difference at {next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), None)}"


def _runs(lengths, values=(0x00070707, 0x00070707, 0x00C80000, 0)):
    """Runs of the given lengths; neighbours differ, so each is a maximal run."""
    out = []
    for k, n in enumerate(lengths):
        out += [values[k % len(values)] + (k % 2)] * n
    return out


def _crafted():
    edge = list(range(1, 6)) + list(range(4095, 4100)) + list(range(8191, 8196))        # remainders 0 .. 3 after one and after two matches of 4096
    rng = np.random.default_rng(23)
    return {"runs_one_strip": (_runs(edge), 1 << 20),
            "runs_reversed": (_runs(edge[::-1]), 1 << 20),
            "run_cut_by_strips": ([1, 2] + [5] * 700 + [3], 300),                        # the run crosses two strip boundaries and restarts at each
            "run_cut_by_every_boundary": ([4] * 9001, 1000),                             # every strip is one literal and one match
            "strip_of_one_pixel": (_runs([4, 9, 260]) + [77], 273),                      # 274 words: the last strip is the single word 77
            "strips_of_one_pixel": ([0, 0, 0, 1, 1], 1),
            "chunk_edges": (_runs([255, 1, 2, 254, 3, 509, 258, 259, 256, 256, 257, 511, 2, 2, 512]), 1 << 20),   # around the 256-position rounds
            "two_rows": (rng.integers(0, 3, 2 * 1500).tolist(), 700)}                    # two buffers in one call (see the test)


def _stream_of(words_row, strip_px, table_lengths):
    """The yardstick's bits of one row's strips under the given (green, red, blue) lengths: (bit string, bits per strip)."""
    (gl, rl, bl), bw, per = table_lengths, P.BitWriter(), []
    gc, rc, bc = (R.canonical_codes(ln) for ln in (gl, rl, bl))
    for s in range(0, len(words_row), strip_px):
        n0 = bw.n
        for kind, v in R.tokens(words_row[s:s + strip_px]):
            if kind == "lit":
                for c, ln, sym in ((gc, gl, v >> 8 & 255), (rc, rl, v >> 16 & 255), (bc, bl, v & 255)):
                    bw.huff(c[sym], ln[sym])
            else:
                sym, eb, ev = R.prefix_value(v)
                bw.huff(gc[256 + sym], gl[256 + sym])
                bw.put(ev, eb)
        per.append(bw.n - n0)
    return bw.bytes(), per


@pytest.mark.parametrize("case", sorted(_crafted()))
def test_crafted_residuals_through_the_low_level_wrappers(case):
    """Any words are residuals to the coder.  The header here is 13 marker bits, so that the strips start off a word boundary."""
    from mmgt_amd import hip
    from mmgt_amd import video_out as V
    words, strip_px = _crafted()[case]
    rows = 2 if case == "two_rows" else 1
    buf = np.array(words, np.int64).reshape(rows, -1)
    data = _dev(buf.astype(np.uint32).view(np.int32))
    strip_px = min(strip_px, buf.shape[1])
    strips = -(-buf.shape[1] // strip_px)
    hist = hip.webp_histogram(data, strip_px).cpu().numpy().view(np.uint32).astype(np.int64)
    want_hist = np.array([[(lambda h: h[0] + h[1] + h[2] + [h[3]])(R.strip_histograms(buf[r, s:s + strip_px])) for s in range(0, buf.shape[1], strip_px)]
                          for r in range(rows)], np.int64)
    assert np.array_equal(hist, want_hist)
    tabs = [V.webp_frame_tables(hist[r].sum(0)) for r in range(rows)]
    marker = (0x1555).to_bytes(2, "little")
    want = np.array([[13] + (hist[r] @ tabs[r][1]).tolist() for r in range(rows)], np.int64)
    slots, bits = hip.webp_code(data, strip_px, np.stack([t[0] for t in tabs]), [marker] * rows, want)
    assert np.array_equal(bits.cpu().numpy(), want[:, 1:])
    packed, off = hip.webp_pack(slots, want)
    packed = packed.cpu().numpy()
    for r in range(rows):
        lens = [R.code_lengths(c, 15) if np.count_nonzero(c) > 1 else [0] * len(c) for c in (hist[r].sum(0)[:280], hist[r].sum(0)[280:536], hist[r].sum(0)[536:792])]
        body, per = _stream_of(buf[r].tolist(), strip_px, lens)
        assert per == want[r, 1:].tolist() and len(per) == strips
        whole = 0x1555 | int.from_bytes(body, "little") << 13
        nbits = 13 + sum(per)
        assert packed[off[r]:off[r + 1]].tobytes() == whole.to_bytes((nbits + 7) // 8, "little")


def test_the_run_frame_through_the_whole_encoder():
    """Runs of 1 .. 6, 4095 .. 4100 and 8191 .. 8197 equal residuals, whole and cut by the strips' ends (62 000 pixels)."""
    from mmgt_amd.video_out import encode_webp_frames
    frame, _ = R.run_frame(list(range(1, 7)) + list(range(4095, 4101)) + list(range(8191, 8198)), 251)
    x = _dev(frame[None])
    for strip_rows in (7, 1000):
        (got,) = encode_webp_frames(x, strip_rows=strip_rows)
        assert got == R.frame_parts(frame, strip_rows)["payload"]


def test_repeatable_and_independent_of_what_the_buffers_held():
    from mmgt_amd import hip
    from mmgt_amd import video_out as V
    frames = _frames("smooth")
    x = _dev(frames)
    first = V.encode_webp_frames(x, strip_rows=5)
    assert V.encode_webp_frames(x, strip_rows=5) == first == [p["payload"] for p in _reference("smooth", 5)]
    # the same launches by hand, every output and scratch tensor filled with 0xFF beforehand and longer than needed
    n, H, W, _ = frames.shape
    strips, guard = -(-H // 5), 16
    ff = lambda shape, dt: torch.full(shape, -1, device="cuda", dtype=dt) if dt != torch.uint8 else torch.full(shape, 255, device="cuda", dtype=dt)
    bh, bw = -(-H // 16), -(-W // 16)
    m_buf, r_buf = ff((n * bh * bw + guard,), torch.uint8), ff((n * H * W + guard,), torch.int32)
    modes, res = hip.webp_predict(x, out=(m_buf[:n * bh * bw].view(n, bh, bw), r_buf[:n * H * W].view(n, H, W)))
    assert (m_buf[n * bh * bw:] == 255).all() and (r_buf[n * H * W:] == -1).all()
    data = res.view(n, H * W)
    h_buf = ff((n * strips * 793 + guard,), torch.int32)
    hist = hip.webp_histogram(data, 5 * W, out=h_buf[:n * strips * 793].view(n, strips, 793))
    assert (h_buf[n * strips * 793:] == -1).all()
    hist = hist.cpu().numpy().view(np.uint32).astype(np.int64)
    tabs = [V.webp_frame_tables(hist[f].sum(0)) for f in range(n)]
    heads = [V.webp_frame_header(W, H, modes[f].cpu().numpy(), tabs[f][2]) for f in range(n)]
    want = np.array([[heads[f][1]] + (hist[f] @ tabs[f][1]).tolist() for f in range(n)], np.int64)
    words = int(hip.webp_slot_offsets(want)[-1])
    b_buf = ff((n * strips + guard,), torch.int64)
    slots, bits = hip.webp_code(data, 5 * W, np.stack([t[0] for t in tabs]), [h[0] for h in heads], want,
                                out=(ff((words + guard,), torch.int32), b_buf[:n * strips].view(n, strips)))
    assert np.array_equal(bits.cpu().numpy(), want[:, 1:]) and (b_buf[n * strips:] == -1).all()
    assert (slots[words:] == -1).all()                                                    # nothing past the last slot
    total = int(((want.sum(1) + 7) // 8).sum())
    packed, off = hip.webp_pack(slots, want, out=ff((total + guard,), torch.uint8))
    assert int(off[-1]) == total and (packed[total:] == 255).all()
    packed = packed.cpu().numpy()
    assert [packed[off[f]:off[f + 1]].tobytes() for f in range(n)] == first
    # one frame per set of launches
    old = V.WEBP_SCRATCH_BYTES
    try:
        V.WEBP_SCRATCH_BYTES = 1
        calls = hip.call_count("mmgt_webp_predict")
        assert V.encode_webp_frames(frames, strip_rows=5) == first                        # host data: uploaded
        assert hip.call_count("mmgt_webp_predict") == calls + n
    finally:
        V.WEBP_SCRATCH_BYTES = old


def test_a_wrong_bit_count_raises():
    from mmgt_amd import hip
    from mmgt_amd import video_out as V
    x = _dev(_frames("smooth"))
    real = V.webp_frame_tables

    def one_bit_more(hist):
        table, cost, described = real(hist)
        cost = cost.copy()
        cost[np.flatnonzero(np.asarray(hist)[:256])[0]] += 1
        return table, cost, described
    V.webp_frame_tables = one_bit_more
    try:
        with pytest.raises(RuntimeError, match="bits on the device"):
            V.encode_webp_frames(x, strip_rows=16)
    finally:
        V.webp_frame_tables = real
    assert V.encode_webp_frames(x, strip_rows=16) == [p["payload"] for p in _reference("smooth", 16)]
    L = hip.lib()
    p = x.data_ptr()
    assert L.mmgt_webp_predict(p, p, p, 1, 16385, 1, None) != 0 and b"range" in L.mmgt_last_error()
    assert L.mmgt_webp_histogram(p, p, 1, 180, 0, None) != 0 and b"range" in L.mmgt_last_error()
    assert L.mmgt_webp_histogram(None, p, 1, 180, 10, None) != 0
    assert L.mmgt_webp_code(p, p, p, p, 1, p, p, 1, p, 1, (1 << 28) + 1, 10, None) != 0 and b"range" in L.mmgt_last_error()
    with pytest.raises(ValueError, match="at most 16384"):
        V.encode_webp_frames(np.zeros((1, 1, 16385, 3), np.uint8))
    with pytest.raises(ValueError, match="strip_rows"):
        V.encode_webp_frames(np.zeros((1, 4, 4, 3), np.uint8), strip_rows=0)


def test_save_videos_grid_webp(tmp_path):
    from mmgt_amd import video_out as V
    g = torch.Generator().manual_seed(3)
    videos = torch.rand((1, 3, 4, 40, 24), generator=g)
    want = V.frames_uint8(videos)
    path = tmp_path / "clip.webp"
    V.save_videos_grid(videos, str(path), fps=8)
    img = Image.open(path)
    assert img.n_frames == 4 and img.size == (24, 40) and img.info["loop"] == 0
    for k in range(4):
        img.seek(k)
        assert np.array_equal(np.asarray(img.convert("RGB")), want[k]) and img.info["duration"] == 125, k
    V.save_videos_grid(videos[:, :, :1], str(tmp_path / "still.webp"))
    data = (tmp_path / "still.webp").read_bytes()
    assert [k for k, _ in R.parse_chunks(data)] == [b"VP8L"]
    still = Image.open(io.BytesIO(data))
    assert getattr(still, "n_frames", 1) == 1 and np.array_equal(np.asarray(still.convert("RGB")), want[0])
    with pytest.raises(ValueError, match=r"Unsupported file type. Use .mp4 or .gif."):
        V.save_videos_grid(videos, str(tmp_path / "clip.webm"))


def test_pose2vid_synthetic_webp(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pose2vid.py"), "--synthetic", "-W", "64", "-H", "64", "-L", "8", "--steps", "2",
                        "--format", "webp", "--out_dir", str(tmp_path)], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["webp"].endswith(".webp") and rec["webp_bytes"] == os.path.getsize(rec["webp"])
    img = Image.open(rec["webp"])
    assert img.n_frames == 8 and img.size == (64, 64)
    img.seek(7)
    assert np.asarray(img.convert("RGB")).std() > 0 and img.info["duration"] == 40
