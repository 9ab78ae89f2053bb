"""PNG / APNG decode without a GPU: the host parser mmgt_amd.video_in.parse_png is held to its scope and its refusals, and the product's
own arithmetic -- csrc/pngdec_core.h, the code the kernels call -- runs in a stand-alone host program built with AddressSanitizer and UBSan: on
well-formed files against PIL's Image.open(f).convert("RGB") on every byte, and over seeded corruptions, where it must end clean with pixels or a
status.  The yardsticks are zlib and PIL; nothing is compared with a tolerance."""
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_ref as P
from tests import pngdec_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pil_save(mode, W=37, H=29, **kw):
    rng = np.random.default_rng(3)
    if mode == "1":
        im = Image.fromarray(rng.integers(0, 2, (H, W)).astype(bool))
    elif mode == "P":
        im = Image.fromarray(rng.integers(0, 1 << kw.get("bits", 8), (H, W)).astype(np.uint8), "P")
        im.putpalette(rng.integers(0, 256, 3 << kw.get("bits", 8)).astype(np.uint8).tobytes())
    else:
        ch = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4}[mode]
        im = Image.fromarray(rng.integers(0, 256, (H, W, ch) if ch > 1 else (H, W)).astype(np.uint8), mode)
    b = io.BytesIO()
    im.save(b, format="PNG", **kw)
    return b.getvalue()


PIL_FILES = {"1": (0, 1), "L": (0, 8), "LA": (4, 8), "RGB": (2, 8), "RGBA": (6, 8), "P1": (3, 1), "P2": (3, 2), "P4": (3, 4), "P8": (3, 8)}


# ---- the host parser ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PIL_FILES))
def test_parse_png_reads_pil_files_of_every_colour_type(name):
    from mmgt_amd import video_in
    data = _pil_save("P", bits=int(name[1])) if name[0] == "P" else _pil_save(name)
    h = video_in.parse_png(data)
    assert (h.width, h.height, h.colour_type, h.bit_depth) == (37, 29) + PIL_FILES[name] and len(h.streams) == 1 and not h.animated
    raw = zlib.decompressobj(-15).decompress(h.streams[0])
    assert len(raw) == 29 * h.stride and zlib.adler32(raw) == h.adlers[0]
    assert (h.palette is not None) == (h.colour_type == 3)


@pytest.mark.parametrize("ct,depth", C.DEPTHS)
def test_parse_png_accepts_every_depth_and_joins_idat_chunks(ct, depth):
    from mmgt_amd import video_in
    one, split = C.case_png(37, 29, ct, depth, seed=1), C.case_png(37, 29, ct, depth, seed=1, idat_split=7)
    a, b = video_in.parse_png(one), video_in.parse_png(split)
    assert split.count(b"IDAT") > 5 and a.streams == b.streams and a.adlers == b.adlers and a.geometry == (29, 37, ct, depth)
    assert a.stride == 1 + C.rowbytes(37, ct, depth)
    if ct == 3:
        assert np.array_equal(a.palette, C.palette_for(depth, 1))


def test_parse_png_reads_the_projects_own_files(tmp_path):
    from mmgt_amd import video_in, video_out
    frames = P.smooth_frames(3, 29, 37, seed=4)
    blobs = P.encode_frames(frames, 5)
    video_out.write_apng(str(tmp_path / "clip.apng"), blobs, 37, 29, 8)
    h = video_in.parse_png((tmp_path / "clip.apng").read_bytes())
    assert h.animated and h.geometry == (29, 37, 2, 8) and [b[2:-4] for b in blobs] == h.streams
    assert h.adlers == [int.from_bytes(b[-4:], "big") for b in blobs]
    for k, path in enumerate(video_out.write_png_sequence(tmp_path / "seq", blobs, 37, 29)):
        g = video_in.parse_png(open(path, "rb").read())
        assert not g.animated and g.streams == [blobs[k][2:-4]]


def _chunks(data):
    return P.parse_chunks(data)


def _join(chunks):
    return C.SIG + b"".join(P.chunk(k, b) for k, b in chunks)


def _refused():
    good = C.case_png(21, 37, 2, 8, seed=1)
    pal = C.case_png(21, 37, 3, 4, seed=1)
    ch = _chunks(good)
    ihdr = lambda **kw: struct.pack(">IIBBBBB", kw.get("W", 21), kw.get("H", 37), kw.get("depth", 8), kw.get("ct", 2), 0, 0, kw.get("lace", 0))
    with_ihdr = lambda **kw: _join([(b"IHDR", ihdr(**kw))] + ch[1:])
    blob = ch[1][1]
    crc = bytearray(good)
    crc[good.index(b"IDAT") + 10] ^= 1
    frames = [C.zcompress(C.filter_rows(C.raw_rows(21, 37, 6, 8, k), 4, [0] * 37).tobytes()) for k in range(2)]
    small = C.zcompress(C.filter_rows(C.raw_rows(5, 5, 6, 8, 1), 4, [0] * 5).tobytes())
    return {
        "bit depth 16": (with_ihdr(depth=16), "bit depth 16"),
        "interlace": (with_ihdr(lace=1), "Adam7 interlace"),
        "sub-rectangle": (C.make_apng([frames[0], small], 21, 37, 6, 8, rect=(5, 5, 2, 3)), "sub-rectangle"),
        "blend over with alpha": (C.make_apng(frames, 21, 37, 6, 8, blend=1), "blend OVER"),
        "missing IHDR": (_join(ch[1:]), "missing IHDR"),
        "missing IDAT": (_join([ch[0], ch[-1]]), "missing IDAT"),
        "missing IEND": (_join(ch[:-1]), "missing IEND"),
        "truncated": (good[:len(good) - 20], "missing IEND"),
        "palette without PLTE": (_join([c for c in _chunks(pal) if c[0] != b"PLTE"]), "without PLTE"),
        "bad CRC": (bytes(crc), "bad CRC"),
        "zlib CM": (_join([ch[0], (b"IDAT", bytes([blob[0] ^ 1]) + blob[1:]), ch[-1]]), "bad zlib header"),
        "zlib FDICT": (_join([ch[0], (b"IDAT", bytes([0x78, 0x20 | 0x1b]) + blob[2:]), ch[-1]]), "bad zlib header"),
        "zlib FCHECK": (_join([ch[0], (b"IDAT", blob[:1] + bytes([blob[1] ^ 1]) + blob[2:]), ch[-1]]), "bad zlib header"),
        "unknown critical chunk": (_join([ch[0], (b"XyZa", b"12"), *ch[1:]]), "unknown critical chunk"),
        "not a PNG": (b"GIF89a" + good[6:], "not a PNG"),
        "colour type 5": (with_ihdr(ct=5), "bad IHDR"),
        "RGB at 4 bits": (with_ihdr(depth=4), "bad IHDR"),
        "side above 16384": (with_ihdr(W=16385), "16384"),
    }


@pytest.mark.parametrize("case", sorted(_refused()))
def test_parse_png_refuses_on_the_host(case):
    from mmgt_amd import video_in
    data, word = _refused()[case]
    with pytest.raises(ValueError, match=word):
        video_in.parse_png(data)


def test_ancillary_chunks_are_skipped_and_a_batch_is_one_geometry():
    from mmgt_amd import video_in
    base = C.case_png(21, 37, 0, 8, seed=1)
    more = C.case_png(21, 37, 0, 8, seed=1, trns=b"\x00\x07", extra=((b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"k\0v")))
    assert video_in.parse_png(more).streams == video_in.parse_png(base).streams
    with pytest.raises(ValueError, match="one call decodes one geometry"):
        video_in.png_batch_operands([base, C.case_png(37, 21, 0, 8)])
    with pytest.raises(ValueError, match="one call decodes one geometry"):
        video_in.png_batch_operands([base, C.case_png(21, 37, 0, 4)])
    with pytest.raises(ValueError, match="one call decodes one geometry"):
        video_in.png_batch_operands([base, C.case_png(21, 37, 3, 8)])


def test_row_sums_give_the_adler32():
    from mmgt_amd import video_in, video_out
    rng = np.random.default_rng(8)
    f = rng.integers(0, 256, (2, 300, 41), dtype=np.uint8)
    f[1] = 255                                                                             # the largest sums
    L = f.shape[2]
    w = np.arange(L, 0, -1, dtype=np.int64)
    sums = np.stack([f.astype(np.int64).sum(axis=2), (f.astype(np.int64) * w).sum(axis=2)], axis=2)
    got = video_in.adler32_of_row_sums(sums, L)
    assert [int(v) for v in got] == [zlib.adler32(f[k].tobytes()) for k in range(2)]
    fold = 1
    for s1, s2 in sums[0].tolist():
        fold = video_out.adler32_combine(fold, ((L + s2) % 65521) << 16 | (1 + s1) % 65521, L)
    assert fold == int(got[0])


# ---- what PIL does: the definition of the pixels -----------------------------------------------------------------------------------------------------
def test_pil_convert_rgb_is_what_design_4h_says():
    """Grey of 1 / 2 / 4 bits scaled by 255 / 85 / 17, alpha dropped (not composited), tRNS ignored, palette entries copied."""
    for depth, scale in ((1, 255), (2, 85), (4, 17), (8, 1)):
        raw = C.raw_rows(37, 29, 0, depth, 1)
        png = C.make_png(C.filter_rows(raw, 1, [0] * 29).tobytes(), 37, 29, 0, depth, trns=b"\x00\x01")
        bits = np.unpackbits(raw, axis=1).reshape(29, -1, depth)
        samples = (bits << np.arange(depth - 1, -1, -1)).sum(axis=2)[:, :37]
        assert np.array_equal(C.pil_rgb(png), np.repeat((samples * scale).astype(np.uint8)[..., None], 3, axis=2)), depth
    for ct in (4, 6):
        raw = C.raw_rows(37, 29, ct, 8, 1).reshape(29, 37, -1)
        png = C.make_png(C.filter_rows(raw.reshape(29, -1), raw.shape[2], [0] * 29).tobytes(), 37, 29, ct, 8)
        want = np.repeat(raw[..., :1], 3, axis=2) if ct == 4 else raw[..., :3]
        assert raw[..., -1].min() < 128 and np.array_equal(C.pil_rgb(png), want)
    raw, pal = C.raw_rows(37, 29, 3, 8, 1), C.palette_for(8, 1)
    png = C.make_png(C.filter_rows(raw, 1, [0] * 29).tobytes(), 37, 29, 3, 8, plte=pal, trns=bytes(range(0, 200)))
    assert np.array_equal(C.pil_rgb(png), pal[raw])


def _apng(ct, dispose, blend, trns=None):
    bpp = C.filter_bpp(ct, 8)
    blobs = [C.zcompress(C.filter_rows(C.raw_rows(21, 37, ct, 8, 30 + k), bpp, [k % 5] * 37).tobytes()) for k in range(3)]
    plte = C.palette_for(8, 30) if ct == 3 else None
    stills = [C.make_png(zlib.decompress(b), 21, 37, ct, 8, plte=plte, trns=trns) for b in blobs]
    return C.make_apng(blobs, 21, 37, ct, 8, plte=plte, trns=trns, dispose=dispose, blend=blend), stills


@pytest.mark.parametrize("ct", [0, 2, 3, 4, 6])
def test_full_size_apng_frames_are_their_own_pixels_whatever_dispose_and_blend(ct):
    """The claim parse_png rests on: with every frame full size at (0, 0), PIL composes frame k to exactly frame k's own pixels for every dispose
    value and for blend SOURCE; blend OVER as well where nothing is transparent.  Where PIL disagrees (OVER with alpha or tRNS), parse_png refuses."""
    from mmgt_amd import video_in
    for dispose in (0, 1, 2):
        for blend in (0, 1):
            for trns in ((None,) if ct in (4, 6) else (None, {0: b"\x00\x07", 2: b"\x00\x07\x00\x08\x00\x09", 3: bytes(range(50, 150))}[ct])):
                apng, stills = _apng(ct, dispose, blend, trns)
                own = np.stack([C.pil_rgb(s) for s in stills])
                try:
                    h = video_in.parse_png(apng)
                except ValueError as e:
                    assert "blend OVER" in str(e) and blend == 1 and (ct in (4, 6) or trns is not None)
                    continue
                assert len(h.streams) == 3
                assert np.array_equal(C.pil_frames(apng), own), (ct, dispose, blend, trns)


# ---- the product's arithmetic in a host program under ASan + UBSan ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/pngdec_host_check.cpp with"
    exe = tmp_path_factory.mktemp("pngdec_host") / "pngdec_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "pngdec_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def run_host(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True)


def host_decode(exe, tmp_path, pngs=None, headers=None, mode="decode"):
    job, out = tmp_path / "job.bin", tmp_path / "out.bin"
    if out.exists():
        out.unlink()
    n, H, W, stride = C.write_job(job, pngs, headers)
    r = run_host(exe, mode, str(job), str(out))
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-3000:]}"
    return np.fromfile(out, np.uint8).reshape((n, H, W, 3) if mode == "decode" else (n, H * stride))


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_program_equals_pil_over_levels_strategies_and_filters(host_check, tmp_path, size):
    pngs = C.cross_batches()[size]
    assert len(pngs) == len(C.LEVELS) * len(C.STRATEGIES) * len(C.FILTERS)
    got = host_decode(host_check, tmp_path, pngs)
    want = np.stack([C.pil_rgb(p) for p in pngs])
    assert np.array_equal(got, want), f"frames {sorted(set(np.argwhere(got != want)[:, 0].tolist()))} differ"


def test_the_cross_holds_the_block_types_it_is_there_for():
    """Stored streams of several stored blocks, fixed and dynamic blocks: read off the first block header of the raw deflate bytes."""
    from mmgt_amd import video_in
    kinds = {}
    for k, png in enumerate(C.cross_batches()[(150, 150)]):
        h = video_in.parse_png(png)
        kinds.setdefault((h.streams[0][0] >> 1) & 3, []).append(len(h.streams[0]))
    assert set(kinds) == {0, 1, 2} and max(kinds[0]) > 65535 + 10


@pytest.mark.parametrize("ct,depth", C.DEPTHS)
def test_host_program_equals_pil_for_every_depth_at_every_size(host_check, tmp_path, ct, depth):
    for W, H in C.SIZES:
        pngs = C.depth_batches()[(W, H, ct, depth)]
        got = host_decode(host_check, tmp_path, pngs)
        assert np.array_equal(got, np.stack([C.pil_rgb(p) for p in pngs])), (W, H)


def test_host_program_decodes_pil_files_and_a_batch_with_per_frame_palettes(host_check, tmp_path):
    from mmgt_amd import video_in
    for name in sorted(PIL_FILES):
        data = _pil_save("P", bits=int(name[1])) if name[0] == "P" else _pil_save(name)
        assert np.array_equal(host_decode(host_check, tmp_path, [data])[0], C.pil_rgb(data)), name
    big = _pil_save("RGB", 150, 150)
    assert big.count(b"IDAT") > 1 and np.array_equal(host_decode(host_check, tmp_path, [big])[0], C.pil_rgb(big))
    pngs = C.palette_batch()
    assert len({video_in.parse_png(p).palette.tobytes() for p in pngs}) == 5
    assert np.array_equal(host_decode(host_check, tmp_path, pngs), np.stack([C.pil_rgb(p) for p in pngs]))


def test_host_program_inflates_what_zlib_never_emits(host_check, tmp_path):
    from mmgt_amd import video_in
    for name, (z, W, H) in C.token_streams().items():
        png = C.make_png(b"", W, H, 0, 8, compress=z)
        got = host_decode(host_check, tmp_path, [png], mode="filtered")
        assert got.tobytes() == zlib.decompress(z), name


def test_host_program_decodes_the_encoders_streams_and_an_apng(host_check, tmp_path):
    """The 4g yardstick's streams (one dynamic block per strip, a single length-1 distance code or none) at 1, 5 and >= H rows per strip."""
    from mmgt_amd import video_in
    frames = np.concatenate([P.smooth_frames(2, 37, 21, seed=2), P.pose_frames(1, 37, 21)])
    for strip_rows in (1, 5, 64):
        blobs = P.encode_frames(frames, strip_rows)
        got = host_decode(host_check, tmp_path, [P.png_file(b, 21, 37) for b in blobs])
        assert np.array_equal(got, frames), strip_rows
    apng, stills = _apng(2, 1, 1)
    assert np.array_equal(host_decode(host_check, tmp_path, [apng]), C.pil_frames(apng))


def test_host_program_reports_statuses_and_a_falsified_adler32(host_check, tmp_path):
    from mmgt_amd import video_in
    good = C.case_png(21, 37, 2, 8, 6, seed=1)
    h = video_in.parse_png(good)
    job, out = tmp_path / "job.bin", tmp_path / "out.bin"

    def run(header):
        C.write_job(job, headers=[header])
        return run_host(host_check, "decode", str(job), str(out))

    h.adlers[0] ^= 1
    r = run(h)
    assert r.returncode == 3 and "adler mismatch in frame 0" in r.stderr and not out.exists(), r.stderr[-2000:]
    h = video_in.parse_png(good)
    h.streams[0] = h.streams[0][:len(h.streams[0]) // 2]
    r = run(h)
    assert r.returncode == 3 and "status 6 in frame 0 (inflate)" in r.stderr, r.stderr[-2000:]
    rows = C.filter_rows(C.raw_rows(21, 37, 2, 8, 1), 3, [0] * 37)
    rows[5, 0] = 9                                                                           # a filter type above 4
    r = run(video_in.parse_png(C.make_png(rows.tobytes(), 21, 37, 2, 8)))
    assert r.returncode == 3 and "status 14 in frame 0 (unfilter)" in r.stderr, r.stderr[-2000:]
    idx = C.raw_rows(21, 37, 3, 8, 1)
    idx[7, 3] = 250                                                                          # the palette has 200 entries
    r = run(video_in.parse_png(C.make_png(C.filter_rows(idx, 1, [0] * 37).tobytes(), 21, 37, 3, 8, plte=C.palette_for(8, 1))))
    assert r.returncode == 3 and "status 15 in frame 0 (expand)" in r.stderr, r.stderr[-2000:]
    long = C.make_png(C.filter_rows(C.raw_rows(21, 38, 2, 8, 1), 3, [0] * 38).tobytes(), 21, 37, 2, 8)
    assert "status 7" in run(video_in.parse_png(long)).stderr
    short = C.make_png(C.filter_rows(C.raw_rows(21, 36, 2, 8, 1), 3, [0] * 36).tobytes(), 21, 37, 2, 8)
    assert "status 8" in run(video_in.parse_png(short)).stderr


FUZZ = {"rgb_dynamic": lambda: [C.case_png(37, 29, 2, 8, 6, seed=1), C.case_png(37, 29, 2, 8, 9, "filtered", 4, seed=2)],
        "rgb_fixed": lambda: [C.case_png(37, 29, 2, 8, 6, "fixed", seed=1)],
        "rgb_stored": lambda: [C.case_png(150, 150, 2, 8, 0, seed=1)],
        "palette_4bit": lambda: C.palette_batch(),
        "grey_1bit_rle": lambda: [C.case_png(21, 37, 0, 1, 9, "rle", 2, seed=1)],
        "encoder_strips": lambda: [P.png_file(b, 21, 37) for b in P.encode_frames(P.smooth_frames(2, 37, 21, seed=2), 5)],
        "tokens": lambda: [C.make_png(b"", W, H, 0, 8, compress=z) for z, W, H in [C.token_streams()["every_length_code"]]]}


@pytest.mark.parametrize("name", sorted(FUZZ))
def test_host_program_survives_corruptions(host_check, tmp_path, name):
    """500 seeded corruptions per batch (byte flips, shortened ranges, overwritten runs, falsified code lengths and block headers): every run ends in
    pixels, a status or an Adler-32 mismatch within the step bound; ASan / UBSan end the program otherwise."""
    C.write_job(tmp_path / "job.bin", FUZZ[name]())
    r = run_host(host_check, "fuzz", str(tmp_path / "job.bin"), "500", "20261019")
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-4000:]}"
    w = r.stdout.split()
    runs, pixels, status, adler = int(w[1]), int(w[3]), int(w[7]), int(w[11])
    assert runs == 500 and pixels + status + adler == 500 and status + adler >= 100, r.stdout
