"""The host side of the PNG / APNG writer (mmgt_amd/video_out.py) and its CPU yardstick (tests/png_ref.py), without a GPU: the yardstick's
streams against zlib and PIL, the product's package-merge, Adler-32 combination and containers against independent restatements.

Stream size (test_yardstick_stream_size_against_zlib_rle): for the smooth input at 96 x 64 and the default 64 rows per strip the yardstick's deflate
stream is 3011 bytes against 2948 of zlib's Z_RLE strategy (level 6, memLevel 9) on the same filtered bytes, ratio 1.0214; the gate is that ratio
rounded up to the next whole percent.  The bytes are deterministic: this guards against regressions, it is no tolerance."""
import io
import itertools
import struct
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_ref as R
from tests.host_check import host_check  # noqa: F401  (the fixture)
from tests.test_png_gpu import _crafted

SIZE_RATIO_GATE = 1.03


def _blobs(frames, strip_rows=16):
    return R.encode_frames(frames, strip_rows)


# ---- the yardstick itself ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strip_rows", [1, 5, 1000])
@pytest.mark.parametrize("kind", ["smooth", "noise", "pose", "flat"])
def test_yardstick_streams_inflate_and_open_in_pil(kind, strip_rows):
    n, H, W = 2, 37, 29
    frames = {"smooth": R.smooth_frames(n, H, W), "noise": np.random.default_rng(3).integers(0, 256, (n, H, W, 3), dtype=np.uint8),
              "pose": R.pose_frames(n, H, W), "flat": np.full((n, H, W, 3), 77, np.uint8)}[kind]
    filt = R.filter_frames(frames)
    for f, blob in enumerate(_blobs(frames, strip_rows)):
        assert zlib.decompress(blob) == filt[f].tobytes()
        assert struct.unpack(">I", blob[-4:])[0] == R.adler32(filt[f].tobytes())
        img = Image.open(io.BytesIO(R.png_file(blob, W, H)))
        assert img.mode == "RGB" and img.size == (W, H) and np.array_equal(np.asarray(img), frames[f])


def test_smooth_input_makes_the_yardstick_pick_every_filter_type():
    for shape in ((3, 37, 29), (1, 96, 64)):
        types = R.filter_frames(R.smooth_frames(*shape))[:, :, 0]
        assert set(np.unique(types).tolist()) == {0, 1, 2, 3, 4}, np.bincount(types.reshape(-1), minlength=5)


def test_filter_ties_go_to_the_lowest_type():
    assert (R.filter_frames(np.zeros((1, 6, 9, 3), np.uint8))[0, :, 0] == 0).all()
    types = R.filter_frames(np.full((1, 6, 9, 3), 200, np.uint8))[0, :, 0]
    assert types[0] == 1 and (types[1:] == 2).all()                              # Up and Paeth both give zeros below row 0: Up has the lower number


def test_yardstick_tokens_cut_runs_as_the_definition_says():
    assert R.tokens(b"\x05" * 3) == [("lit", 5), ("lit", 5), ("lit", 5)]
    assert R.tokens(b"\x05" * 4) == [("lit", 5), ("len", 3)]
    assert R.tokens(b"\x05" * 260) == [("lit", 5), ("len", 258), ("lit", 5)]
    assert R.tokens(b"\x05" * 262) == [("lit", 5), ("len", 258), ("len", 3)]
    assert R.tokens(b"ab" + b"\x05" * 5 + b"c") == [("lit", 97), ("lit", 98), ("lit", 5), ("len", 4), ("lit", 99)]


def test_yardstick_stream_size_against_zlib_rle():
    frames = R.smooth_frames(1, 96, 64)
    from mmgt_amd.video_out import PNG_STRIP_ROWS
    filt = R.filter_frames(frames)[0].tobytes()
    ours = len(_blobs(frames, PNG_STRIP_ROWS)[0]) - 6                             # without the zlib header and the Adler-32
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
    rle = len(c.compress(filt) + c.flush())
    print(f"yardstick {ours} B, zlib Z_RLE {rle} B, ratio {ours / rle:.4f}")
    assert ours <= SIZE_RATIO_GATE * rle


# ---- deflate_code_lengths ------------------------------------------------------------------------------------------------------------------------------
def _cost(hist, lengths):
    return int(sum(int(h) * int(ln) for h, ln in zip(hist, lengths)))


def _kraft(lengths):
    return sum(Fraction(1, 1 << int(ln)) for ln in lengths if ln)


def _histograms():
    rng = np.random.default_rng(11)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    out = {"random_286": rng.integers(0, 500, 286), "sparse_286": rng.integers(0, 40, 286) * (rng.random(286) < 0.3),
           "geometric_286": (2.0 ** rng.uniform(0, 30, 286)).astype(np.int64), "fibonacci_40": np.array(fib),
           "fibonacci_19": np.array(fib[:19]), "random_19": rng.integers(0, 60, 19), "equal_19": np.full(19, 5)}
    out["sparse_286"][256] = 1
    return out


@pytest.mark.parametrize("name", sorted(_histograms()))
def test_code_lengths_equal_the_yardsticks_package_merge(name):
    from mmgt_amd.video_out import deflate_code_lengths
    hist = _histograms()[name]
    for limit in ((7, 15) if hist.size <= 19 else (15,)):
        got = deflate_code_lengths(hist, limit)
        ref = R.code_lengths(hist, limit)
        assert got.max() <= limit and ((got > 0) == (hist > 0)).all()
        assert _kraft(got) == 1
        assert _cost(hist, got) == _cost(hist, ref)
        assert got.tolist() == ref                                               # the tie rule is part of the stream definition: the same lengths
    if name.startswith(("fibonacci", "geometric")):                             # the limit binds: an unlimited Huffman code would be deeper
        limit = 7 if hist.size <= 19 else 15
        assert deflate_code_lengths(hist, limit).max() == limit
        assert _cost(hist, deflate_code_lengths(hist, limit)) > _cost(hist, deflate_code_lengths(hist, 40))


def test_code_lengths_are_optimal_by_exhaustive_search():
    from mmgt_amd.video_out import deflate_code_lengths
    rng = np.random.default_rng(5)
    for m in range(2, 7):
        for _ in range(12):
            hist = rng.integers(1, 30, m)
            best = min(_cost(hist, ls) for ls in itertools.product((1, 2, 3), repeat=m) if _kraft(ls) <= 1)
            got = deflate_code_lengths(hist, 3)
            assert _kraft(got) == 1 and _cost(hist, got) == best, (hist, got)


def test_code_lengths_small_cases():
    from mmgt_amd.video_out import deflate_code_lengths
    assert deflate_code_lengths([0, 9, 0, 1], 15).tolist() == [0, 1, 0, 1]       # two symbols: a bit each
    assert deflate_code_lengths([0, 0, 4], 15).tolist() == [0, 0, 1]
    assert deflate_code_lengths([0, 0, 0], 15).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        deflate_code_lengths([1] * 9, 3)
    with pytest.raises(ValueError):
        deflate_code_lengths([1, -1], 3)


def test_block_header_equals_the_yardsticks():
    from mmgt_amd.video_out import deflate_block_header, deflate_code_lengths
    rng = np.random.default_rng(8)
    for trial in range(6):
        hist = rng.integers(0, 50, 286) * (rng.random(286) < (0.1, 0.5, 1.0)[trial % 3])
        hist[256] = 1
        hist[0] += 1
        if trial % 2:
            hist[257:] = 0
        ll = deflate_code_lengths(hist, 15)
        dl = [1] if hist[257:].sum() else [0]
        head, nbits = deflate_block_header(ll, dl, trial == 0)
        # the yardstick writes the same header in front of a block with these lengths: rebuild it from its parts
        bw = R.BitWriter()
        nll = max(257, max(s for s in range(286) if ll[s]) + 1)
        syms = R.rle_code_lengths(ll[:nll].tolist() + dl)
        cl = R.code_lengths(np.bincount([s for s, _, _ in syms], minlength=19), 7)
        ncl = max(4, max(k for k in range(19) if cl[R.CL_ORDER[k]]) + 1)
        codes = R.canonical_codes(cl)
        for v, b in ((1 if trial == 0 else 0, 1), (2, 2), (nll - 257, 5), (0, 5), (ncl - 4, 4)):
            bw.put(v, b)
        for k in range(ncl):
            bw.put(cl[R.CL_ORDER[k]], 3)
        for s, eb, ev in syms:
            bw.huff(codes[s], cl[s])
            bw.put(ev, eb)
        assert nbits == bw.n and head == bw.bytes()
        assert nbits <= 8 * 576


# ---- Adler-32 ------------------------------------------------------------------------------------------------------------------------------------------
def test_adler32_combine_equals_zlib():
    from mmgt_amd.video_out import adler32_combine
    rng = np.random.default_rng(2)
    parts = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (0, 1, 5, 5552, 5553, 70000)] + [b"\xff" * (1 + 3 * 16384)] * 3
    for a, b in itertools.product(parts, repeat=2):
        assert adler32_combine(zlib.adler32(a), zlib.adler32(b), len(b)) == zlib.adler32(a + b)
    row = b"\xff" * 16384                                                        # 1 x 16384 of 255: the sums are at their largest per byte
    acc = 1
    for _ in range(7):
        acc = adler32_combine(acc, zlib.adler32(row), len(row))
    assert acc == zlib.adler32(row * 7)
    # a row's Adler-32 from the two sums the device returns: s1 = sum d[i], s2 = sum (L - i) d[i]
    d = np.frombuffer(parts[5], np.uint8).astype(np.int64)
    L = d.size
    s1, s2 = int(d.sum()), int(((L - np.arange(L)) * d).sum())
    assert ((L + s2) % 65521) << 16 | (1 + s1) % 65521 == zlib.adler32(parts[5])
    with pytest.raises(ValueError):
        adler32_combine(1, 1, -1)


# ---- containers ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fps,loop", [(25, 0), (8, 3), (29.97, 0)])
def test_apng_structure(tmp_path, fps, loop):
    from mmgt_amd.video_out import write_apng
    n, H, W = 4, 12, 10
    frames = R.smooth_frames(n, H, W)
    blobs = _blobs(frames, 5)
    path = tmp_path / "a.apng"
    size = write_apng(str(path), blobs, W, H, fps, loop=loop)
    data = path.read_bytes()
    assert size == len(data)
    chunks = R.parse_chunks(data)                                                # checks every CRC
    kinds = [k for k, _ in chunks]
    assert kinds == [b"IHDR", b"acTL"] + [b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n - 1) + [b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    assert struct.unpack(">II", chunks[1][1]) == (n, loop)
    num, den = R.delay_fraction(fps)
    assert Fraction(num, den) == Fraction(1 / fps).limit_denominator(65535) and 0 < num <= 65535 and 0 < den <= 65535
    seq, frame = [], 0
    for kind, body in chunks:
        if kind == b"fcTL":
            s, w, h, x0, y0, dn, dd, dispose, blend = struct.unpack(">IIIIIHHBB", body)
            assert (w, h, x0, y0, dn, dd, dispose, blend) == (W, H, 0, 0, num, den, 0, 0)
            seq.append(s)
        elif kind == b"fdAT":
            seq.append(struct.unpack(">I", body[:4])[0])
            frame += 1
            assert body[4:] == blobs[frame]
        elif kind == b"IDAT":
            assert body == blobs[0]
    assert seq == list(range(2 * n - 1))
    img = Image.open(path)
    assert img.n_frames == n and img.size == (W, H) and img.info["loop"] == loop
    for k in range(n):
        img.seek(k)
        assert img.info["duration"] == pytest.approx(1000.0 * num / den)
        assert np.array_equal(np.asarray(img.convert("RGB")), frames[k])


def test_one_frame_apng_is_a_png_and_the_sequence_is_numbered(tmp_path):
    from mmgt_amd.video_out import write_apng, write_png, write_png_sequence
    frames = R.smooth_frames(3, 12, 10)
    blobs = _blobs(frames, 16)
    write_apng(str(tmp_path / "one.png"), blobs[:1], 10, 12, 25)
    assert (tmp_path / "one.png").read_bytes() == R.png_file(blobs[0], 10, 12)
    assert write_png(str(tmp_path / "two.png"), blobs[1], 10, 12) == len(R.png_file(blobs[1], 10, 12))
    paths = write_png_sequence(tmp_path / "seq", blobs, 10, 12)
    assert [p.split("/")[-1] for p in paths] == ["0000.png", "0001.png", "0002.png"]
    for k, p in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(p)), frames[k])


def test_bad_arguments_raise(tmp_path):
    from mmgt_amd import video_out as V
    blob = _blobs(R.smooth_frames(1, 4, 4), 16)
    for bad in (np.zeros((1, 4, 4, 3), np.float32), np.zeros((4, 4, 3), np.uint8), np.zeros((1, 4, 4, 4), np.uint8), np.zeros((0, 4, 4, 3), np.uint8),
                np.zeros((1, 0, 4, 3), np.uint8), np.zeros((1, 16385, 1, 3), np.uint8), np.zeros((1, 1, 16385, 3), np.uint8)):
        with pytest.raises(ValueError):
            V.encode_png_frames(torch.from_numpy(bad))
    for strip_rows in (0, -4):
        with pytest.raises(ValueError):
            V.encode_png_frames(np.zeros((1, 4, 4, 3), np.uint8), strip_rows=strip_rows)
    p = str(tmp_path / "x.apng")
    for kw in ({"fps": 0}, {"fps": -2.0}, {"fps": 25, "loop": -1}, {"fps": 25, "loop": 1 << 31}):
        with pytest.raises(ValueError):
            V.write_apng(p, blob * 2, 4, 4, **kw)
    with pytest.raises(ValueError):
        V.write_apng(p, [], 4, 4, 25)
    with pytest.raises(ValueError):
        V.write_png(p, blob[0], 0, 4)
    with pytest.raises(ValueError):
        V.write_png(p, blob[0], 4, 16385)
    with pytest.raises(ValueError):
        V.write_png_sequence(str(tmp_path / "d"), [], 4, 4)


# ---- the product's tokens in a host program under ASan + UBSan -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(_crafted()))
def test_host_program_tokens_equal_the_yardstick(host_check, tmp_path, case):
    """csrc/strip_coder.h's closed form at 258, the tokens of csrc/png.hip, on the device tests' crafted buffers: every strip's tokens are the
    yardstick's greedy parse."""
    data, strip_bytes = _crafted()[case]
    rows = 2 if case == "two_rows" else 1
    for row in np.frombuffer(data, np.uint8).reshape(rows, -1):
        row = row.tobytes()
        job, out = tmp_path / "job.bin", tmp_path / "out.bin"
        job.write_bytes(struct.pack("<2i", len(row), strip_bytes) + row)
        r = subprocess.run([host_check, "--png-tokens", str(job), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-3000:]}"
        got, at = np.frombuffer(out.read_bytes(), np.uint32).tolist(), 0
        for first in range(0, len(row), strip_bytes):
            want = [v if kind == "lit" else v | 0x1000 for kind, v in R.tokens(row[first:first + strip_bytes])]
            assert got[at] == len(want) and got[at + 1:at + 1 + got[at]] == want, (case, first)
            at += 1 + got[at]
        assert at == len(got)
