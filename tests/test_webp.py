"""WebP lossless output without a GPU.  The stream definition is restated in tests/webp_ref.py and held to PIL's decoder (libwebp) on
every input kind, size and strip height: what PIL reads back equals the input exactly.  The product's host functions (codes, header, container)
are held to the yardstick's bits, and the product's per-pixel arithmetic -- csrc/webp_core.h, the code the kernels call -- runs in a stand-alone
host program built with AddressSanitizer and UBSan, where its modes, residuals and tokens must equal the yardstick's.  Nothing is compared with a
tolerance except the stream-size ratios, which are held to what was measured."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import png_ref as P
from tests import webp_ref as R
from tests.host_check import host_check  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((37, 29), (1, 1), (300, 1), (1, 300), (16, 17), (17, 16), (33, 47))              # W x H
STRIP_ROWS = (1, 5, 16, 1000)
_cache = {}


def inputs():
    """The input kinds at 37 x 29 (W x H; the gradient is one row of 256), two frames each, made once."""
    if not _cache:
        rng = np.random.default_rng(17)
        noise = rng.integers(0, 256, (2, 29, 37, 3), dtype=np.uint8)
        noise[0].reshape(-1)[:256] = np.arange(256)                                      # every literal occurs
        _cache.update({"noise": noise, "flat": np.full((2, 29, 37, 3), 143, np.uint8), "black": np.zeros((2, 29, 37, 3), np.uint8),
                       "mask": R.mask_frames(2, 29, 37), "smooth": P.smooth_frames(2, 29, 37), "gradient": R.gradient_frames(2)})
    return _cache


def pil_frames(data):
    img = Image.open(io.BytesIO(data))
    out = []
    for k in range(getattr(img, "n_frames", 1)):
        img.seek(k)
        out.append(np.asarray(img.convert("RGB")))
    return np.stack(out)


def round_trip(frames, strip_rows):
    frames = np.asarray(frames)
    blobs = R.encode_frames(frames, strip_rows)
    assert np.array_equal(pil_frames(R.webp_file(blobs, frames.shape[2], frames.shape[1], 25)), frames)
    return blobs


# ---- the yardstick against PIL ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strip_rows", STRIP_ROWS)
@pytest.mark.parametrize("kind", ["noise", "flat", "black", "mask", "smooth", "gradient"])
def test_pil_decodes_the_yardstick_exactly(kind, strip_rows):
    round_trip(inputs()[kind], strip_rows)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pil_decodes_the_yardstick_at_every_size(size):
    W, H = size
    rng = np.random.default_rng(W * 1000 + H)
    for strip_rows in (1, 5, 1000):
        round_trip(P.smooth_frames(2, H, W), strip_rows)
        round_trip(rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8), strip_rows)
        round_trip(rng.integers(0, 2, (1, H, W, 3), dtype=np.uint8) * 255, strip_rows)


def test_the_gradient_has_a_one_symbol_code_length_code():
    """All used lengths equal: the lengths are then coded with ONE code-length symbol, which libwebp reads with zero bits.  The input must hit that
    case for the round trip above to cover it."""
    frame = inputs()["gradient"][0]
    parts = R.frame_parts(frame, 16)
    hit = 0
    g = [sum(h[0][k] for h in parts["hist"]) for k in range(280)]
    r = [sum(h[1][k] for h in parts["hist"]) for k in range(256)]
    b = [sum(h[2][k] for h in parts["hist"]) for k in range(256)]
    for counts in (g, r, b):
        syms = R.rle_code_lengths(R.code_lengths(counts, 15))
        hit += len({s for s, _, _ in syms}) == 1
    assert hit == 2 and not parts["modes"].any()


def test_a_one_row_frame_is_mode_0_throughout():
    parts = R.frame_parts(P.smooth_frames(1, 1, 300)[0], 1)
    assert not parts["modes"].any() and parts["costs"].min(-1).tolist() == parts["costs"].max(-1).tolist()


def test_the_vectorised_predictors_equal_the_pixel_ones():
    rng = np.random.default_rng(5)
    px = R.subtract_green(rng.integers(0, 256, (9, 11, 3), dtype=np.uint8))
    pred = R.predictions(px)
    for m in range(14):
        for y in range(1, 9):
            for x in range(1, 11):
                tr = px[y - 1, x + 1] if x + 1 < 11 else px[y, 0]
                t = lambda v: tuple(int(c) for c in v)
                assert tuple(pred[m, y, x]) == R.predict_pixel(m, t(px[y, x - 1]), t(px[y - 1, x]), t(px[y - 1, x - 1]), t(tr)), (m, y, x)


@pytest.mark.parametrize("mode", range(14))
def test_a_frame_made_for_one_mode_costs_nothing_there(mode):
    """Zero residuals under `mode` behind a random top row and left column: every block must find a mode of cost 0 and the frame must decode."""
    rng = np.random.default_rng(100 + mode)
    H, W = 21, 37
    res = np.zeros((H, W, 4), np.int64)
    res[0, :, 1:] = rng.integers(0, 256, (W, 3))
    res[:, 0, 1:] = rng.integers(0, 256, (H, 3))
    modes = np.full((2, 3), mode)
    px = R.inverse_predictor(modes, res)
    assert (px[..., 0] == 255).all()
    frame = R.add_green(px)
    assert np.array_equal(R.subtract_green(frame), px)
    parts = R.frame_parts(frame, 5)
    assert (parts["costs"][..., mode] == parts["costs"].min(-1)).all()
    inner = parts["costs"][1, 1]                                                          # a block without forced pixels
    assert inner[mode] == 0 and parts["costs"][np.arange(2)[:, None], np.arange(3)[None], parts["modes"]].tolist() == parts["costs"].min(-1).tolist()
    assert np.array_equal(R.words(R.inverse_predictor(parts["modes"], np.stack([(parts["words"] >> s) & 255 for s in (24, 16, 8, 0)], -1))),
                          R.words(px))
    round_trip(frame[None], 5)


# ---- runs -------------------------------------------------------------------------------------------------------------------------------------------
RUNS = list(range(1, 7)) + list(range(4095, 4101)) + list(range(8191, 8198))


def run_frame():
    if "runs" not in _cache:
        _cache["runs"] = R.run_frame(RUNS, 251)
    return _cache["runs"]


def test_tokens_of_runs_around_4096():
    for k in RUNS + [12289]:
        toks = R.tokens([7] * k + [9])
        rest, want = k - 1, [("lit", 7)]
        while rest:
            blk = min(rest, 4096)
            want += [("len", blk)] if blk >= 3 else [("lit", 7)] * blk
            rest -= blk
        assert toks == want + [("lit", 9)], k
    assert [R.prefix_value(v) for v in (1, 2, 3, 4, 5, 6, 7, 9, 4096)] == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 1, 0), (4, 1, 1), (5, 1, 0),
                                                                            (6, 2, 0), (23, 10, 1023)]


@pytest.mark.parametrize("strip_rows", (1, 7, 16, 1000))
def test_runs_whole_and_cut_by_strip_ends(strip_rows):
    frame, runs = run_frame()
    H, W, _ = frame.shape
    parts = R.frame_parts(frame, strip_rows)
    assert not parts["modes"].any()
    w = parts["words"].reshape(-1)
    cut = np.flatnonzero(np.diff(w)) + 1
    zero_runs = [int(b - a) for a, b in zip(np.concatenate([[0], cut]), np.concatenate([cut, [w.size]])) if w[a] == 0]
    assert zero_runs == runs
    if strip_rows == 1000:
        want = []
        for k in runs:                                                                    # the first of a run is a literal, the rest blocks of 4096
            want += [4096] * ((k - 1) // 4096) + [(k - 1) % 4096] * ((k - 1) % 4096 >= 3)
        assert [v for kind, v in parts["tokens"][0] if kind == "len"] == want and {3, 4, 5, 4094, 4095, 4096} <= set(want)
    else:
        assert max(v for t in parts["tokens"] for kind, v in t if kind == "len") <= min(4096, strip_rows * W - 1)
    assert np.array_equal(pil_frames(R.webp_file([parts["payload"]], W, H, 25))[0], frame)


# ---- container --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fps, ms", [(25, 40), (8, 125), (29.97, 33)])
def test_container_chunk_by_chunk_and_through_pil(tmp_path, fps, ms):
    from mmgt_amd import video_out as V
    frames = inputs()["smooth"]
    n, H, W, _ = frames.shape
    blobs = R.encode_frames(frames, 16)
    path = tmp_path / "clip.webp"
    size = V.write_webp(str(path), blobs, W, H, fps, loop=3)
    data = path.read_bytes()
    assert size == len(data) and data == R.webp_file(blobs, W, H, fps, loop=3) and V.webp_duration_ms(fps) == ms == R.duration_ms(fps)
    chunks = R.parse_chunks(data)
    assert [k for k, _ in chunks] == [b"VP8X", b"ANIM"] + [b"ANMF"] * n
    assert chunks[0][1] == b"\x02\0\0\0" + struct.pack("<I", W - 1)[:3] + struct.pack("<I", H - 1)[:3]
    assert chunks[1][1] == struct.pack("<IH", 0, 3)
    for (_, body), blob in zip(chunks[2:], blobs):
        assert body[:6] == bytes(6) and body[6:12] == chunks[0][1][4:] and body[12:15] == struct.pack("<I", ms)[:3] and body[15] == 2
        assert body[16:20] == b"VP8L" and struct.unpack("<I", body[20:24])[0] == len(blob) and body[24:24 + len(blob)] == blob
        assert len(body) == 24 + len(blob) + (len(blob) & 1)
    img = Image.open(path)
    assert img.n_frames == n and img.size == (W, H) and img.info["loop"] == 3
    for k in range(n):
        img.seek(k)
        assert np.array_equal(np.asarray(img.convert("RGB")), frames[k]) and img.info["duration"] == ms      # PIL knows it once the frame is loaded


def test_one_frame_gives_a_plain_vp8l_file(tmp_path):
    from mmgt_amd import video_out as V
    frames = inputs()["mask"][:1]
    blobs = R.encode_frames(frames, 16)
    for k, blob in enumerate((blobs[0], blobs[0] + b"\0")):                               # an even and an odd payload
        V.write_webp(str(tmp_path / f"{k}.webp"), [blob], 37, 29, 8)
        data = (tmp_path / f"{k}.webp").read_bytes()
        assert R.parse_chunks(data) == [(b"VP8L", blob)] and len(data) % 2 == 0
        img = Image.open(io.BytesIO(data))
        assert getattr(img, "n_frames", 1) == 1 and np.array_equal(np.asarray(img.convert("RGB")), frames[0])


def test_write_webp_refuses_what_the_container_cannot_hold(tmp_path):
    from mmgt_amd import video_out as V
    p = str(tmp_path / "x.webp")
    for kw, text in ((dict(blobs=[]), "no frames"), (dict(fps=0), "fps must be positive"), (dict(fps=-1), "fps must be positive"),
                     (dict(loop=65536), "loop must be"), (dict(loop=-1), "loop must be"), (dict(fps=1e-5), "duration"), (dict(W=16385), "pixels a side")):
        args = dict(blobs=[b"ab"], W=4, H=4, fps=25, loop=0)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            V.write_webp(p, **args)
    old = V.WEBP_MAX_BYTES
    try:
        V.WEBP_MAX_BYTES = 100
        with pytest.raises(ValueError, match="4 GiB"):
            V.write_webp(p, [bytes(200)], 4, 4, 25)
    finally:
        V.WEBP_MAX_BYTES = old
    assert not os.path.exists(p)


# ---- the product's host functions against the yardstick ------------------------------------------------------------------------------------------------
def product_payload(frame, strip_rows):
    """The product's header and code functions fed with the yardstick's modes and histograms, the yardstick's own token bits behind them."""
    from mmgt_amd import video_out as V
    parts = R.frame_parts(frame, strip_rows)
    hist = np.array([h[0] + h[1] + h[2] + [h[3]] for h in parts["hist"]], np.int64)
    table, cost, described = V.webp_frame_tables(hist.sum(0))
    head, hbits = V.webp_frame_header(frame.shape[1], frame.shape[0], parts["modes"], described)
    return parts, hist, table, cost, head, hbits


@pytest.mark.parametrize("kind", ["noise", "flat", "black", "mask", "smooth", "gradient"])
def test_product_header_and_codes_equal_the_yardsticks(kind):
    for strip_rows in (5, 1000):
        for frame in inputs()[kind]:
            parts, hist, table, cost, head, hbits = product_payload(frame, strip_rows)
            assert hbits == parts["header_bits"]
            want = int.from_bytes(parts["payload"], "little")
            assert int.from_bytes(head, "little") == want & ((1 << hbits) - 1)
            assert (hist @ cost).tolist() == parts["strip_bits"]
            # the code table: every used symbol's bits, as the yardstick writes them
            lens = [R.code_lengths(c, 15) if sum(1 for v in c if v) > 1 else [0] * len(c) for c in (hist.sum(0)[:280], hist.sum(0)[280:536], hist.sum(0)[536:792])]
            for ln, lo in zip(lens, (0, 280, 536)):
                codes = R.canonical_codes(ln)
                for s, l in enumerate(ln):
                    assert table[lo + s] >> 16 == l
                    if l:
                        assert int(table[lo + s] & 0xFFFF) == int(format(codes[s], f"0{l}b")[::-1], 2)


def test_product_rle_equals_the_yardsticks():
    from mmgt_amd import video_out as V
    rng = np.random.default_rng(9)
    seqs = [[8] * 20, [8, 8], [8, 8, 8], [7] * 9 + [8] * 4, [0] * 150 + [3, 3, 3, 3, 0, 0, 0, 5], [0] * 10 + [1] + [0] * 11 + [1] * 7 + [0, 0], [5]]
    seqs += [rng.choice([0, 0, 0, 4, 8, 8, 9], 280).tolist() for _ in range(20)]
    for seq in seqs:
        assert V._rle_code_lengths(seq, prev=8) == R.rle_code_lengths(seq), seq
    with pytest.raises(ValueError, match="simple code"):
        V.webp_prefix_code([0] * 256 + [4] + [0] * 23)


# ---- stream size: measured, then held -----------------------------------------------------------------------------------------------------------------
def vp8l_bytes_of_pil(frame, method):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="WEBP", lossless=True, method=method)
    (kind, body), = [c for c in R.parse_chunks(buf.getvalue()) if c[0] == b"VP8L"]
    return len(body)


SIZE_CASES = {"smooth": lambda: P.smooth_frames(2, 96, 128), "mask": lambda: R.mask_frames(2, 96, 128)}
# measured on this code (yardstick bytes / the other writer's bytes, 2 frames of 128 x 96, strips of 64 rows; PIL 12.2 with libwebp 1.6.0); the bound is
# the measurement x 1.02, room for a later change of tie order.  The five-filter input is made of bands of 6 rows that each favour one PNG filter: a
# filter per row follows them, a mode per 16 x 16 block cannot, hence more than twice PNG's bytes there (DESIGN 4j says so)
MEASURED = {("smooth", "pil"): 23923 / 23879, ("smooth", "png"): 23923 / 11229, ("mask", "pil"): 240 / 366, ("mask", "png"): 240 / 586}


@pytest.mark.parametrize("kind", sorted(SIZE_CASES))
def test_stream_size_against_pil_and_png(kind):
    frames = SIZE_CASES[kind]()
    ours = sum(len(b) for b in round_trip(frames, 64))
    pil = sum(vp8l_bytes_of_pil(f, 0) for f in frames)
    png = sum(len(b) for b in P.encode_frames(frames, 64))
    print(f"{kind}: webp {ours} bytes, PIL lossless WebP method 0 {pil} ({ours / pil:.4f}), PNG yardstick {png} ({ours / png:.4f})")
    assert ours / pil <= MEASURED[kind, "pil"] * 1.02
    assert ours / png <= MEASURED[kind, "png"] * 1.02


# ---- the product's arithmetic in a host program under ASan + UBSan ------------------------------------------------------------------------------------
def host_run(exe, tmp_path, frames, strip_rows):
    frames = np.ascontiguousarray(frames)
    n, H, W, _ = frames.shape
    job, out = tmp_path / "job.bin", tmp_path / "out.bin"
    job.write_bytes(struct.pack("<4i", n, H, W, strip_rows) + frames.tobytes())
    r = subprocess.run([exe, str(job), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-3000:]}"
    raw = out.read_bytes()
    bh, bw = -(-H // 16), -(-W // 16)
    modes = np.frombuffer(raw, np.uint8, n * bh * bw).reshape(n, bh, bw)
    res = np.frombuffer(raw, np.uint32, n * H * W, n * bh * bw).reshape(n, H, W)
    rest = np.frombuffer(raw, np.uint32, -1, n * bh * bw + 4 * n * H * W).tolist()
    toks, p = [], 0
    for _ in range(n * -(-H // min(strip_rows, H))):
        k = rest[p]
        toks.append([(rest[p + 1 + 2 * i], rest[p + 2 + 2 * i]) for i in range(k)])
        p += 1 + 2 * k
    assert p == len(rest)
    return modes, res, toks


def host_equals_yardstick(exe, tmp_path, frames, strip_rows):
    modes, res, toks = host_run(exe, tmp_path, frames, strip_rows)
    at = 0
    for f, frame in enumerate(np.asarray(frames)):
        parts = R.frame_parts(frame, strip_rows)
        assert np.array_equal(modes[f], parts["modes"]) and np.array_equal(res[f], parts["words"])
        for want in parts["tokens"]:
            flat = []
            for kind, v in want:
                if kind == "lit":
                    flat.append((0, v))
                else:
                    sym, eb, ev = R.prefix_value(v)
                    flat.append((v, sym | eb << 8 | ev << 16))
            assert toks[at] == flat
            at += 1
    assert at == len(toks)


@pytest.mark.parametrize("kind", ["noise", "flat", "black", "mask", "smooth", "gradient"])
def test_host_program_equals_the_yardstick(host_check, tmp_path, kind):
    for strip_rows in (1, 5, 1000):
        host_equals_yardstick(host_check, tmp_path, inputs()[kind], strip_rows)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_program_at_every_size(host_check, tmp_path, size):
    W, H = size
    rng = np.random.default_rng(W * 1000 + H)
    host_equals_yardstick(host_check, tmp_path, P.smooth_frames(2, H, W), 5)
    host_equals_yardstick(host_check, tmp_path, rng.integers(0, 2, (1, H, W, 3), dtype=np.uint8) * 255, 16)


def test_host_program_on_the_runs_and_the_per_mode_frames(host_check, tmp_path):
    frame, _ = run_frame()
    for strip_rows in (7, 1000):
        host_equals_yardstick(host_check, tmp_path, frame[None], strip_rows)
    rng = np.random.default_rng(3)
    frames = []
    for mode in range(14):
        res = np.zeros((21, 37, 4), np.int64)
        res[0, :, 1:] = rng.integers(0, 256, (37, 3))
        res[:, 0, 1:] = rng.integers(0, 256, (21, 3))
        frames.append(R.add_green(R.inverse_predictor(np.full((2, 3), mode), res)))
    host_equals_yardstick(host_check, tmp_path, np.stack(frames), 16)
