"""GIF decode without a GPU.  The composition rules are restated in plain loops (tests/gifdec_ref.py) and held to PIL's
ImageSequence.Iterator(Image.open(f)) + convert("RGB") on seeded random files and on files PIL writes; the host parser mmgt_amd.video_in.parse_gif
is held to its scope and its refusals; and the product's own arithmetic -- csrc/gifdec_core.h, the code the kernels call -- runs in a stand-alone
host program built with AddressSanitizer and UBSan, on well-formed files against PIL on every byte and over seeded corruptions, where it must end
clean with pixels or a status.  Nothing is compared with a tolerance."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gifdec_cases as C
from tests import gifdec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rules, restated, against PIL ---------------------------------------------------------------------------------------------------------------------
def test_the_restated_rules_equal_pil_on_random_files():
    seen = set()
    for k, g in enumerate(C.random_gifs()):
        want = C.pil_frames(g)
        got = R.decode(g)
        assert got.shape == want.shape and np.array_equal(got, want), f"random file {k}"
        for f in R.walk(g)[3]:
            seen |= {("disposal", f["disposal"]), ("interlace", f["interlace"]), ("transparent", f["transparent"] is not None),
                     ("sub-rectangle", f["rect"][2:] != want.shape[2:0:-1])}
    assert seen >= {("disposal", d) for d in range(4)} | {(n, b) for n in ("interlace", "transparent", "sub-rectangle") for b in (False, True)}


@pytest.mark.parametrize("name", sorted(C.pil_written()))
def test_the_restated_rules_equal_pil_on_pil_written_files(name):
    g = C.pil_written()[name]
    want = C.pil_frames(g)
    assert np.array_equal(R.decode(g), want)
    if name == "masks":                                                                    # PIL stores the later frames as delta rectangles
        rects = [f["rect"] for f in R.walk(g)[3]]
        assert any(r[2:] != (56, 40) for r in rects[1:]), rects
    if name == "rgb":
        assert all(f["table"] is not None for f in R.walk(g)[3]) and len({f["table"].tobytes() for f in R.walk(g)[3]}) > 1


@pytest.mark.parametrize("name", sorted(C.stream_cases()))
def test_the_yardstick_lzw_reads_the_unusual_streams_as_pil_does(name):
    g = C.stream_cases()[name]
    assert np.array_equal(R.decode(g), C.pil_frames(g))


def test_the_unusual_streams_are_what_their_names_say():
    from mmgt_amd import video_in
    lzw = lambda name: video_in.parse_gif(C.stream_cases()[name]).frames[0].lzw
    first = lambda s: int.from_bytes(s[:2], "little") & 511
    assert first(lzw("no_initial_clear")) != 256 and first(lzw("no_eoi")) == 256
    plain, deferred = lzw("full_table_clears"), lzw("deferred_clear")
    # 18000 noisy indices: more codes than the table has room for, so the one stream clears and the other goes on at 12 bits without adding
    assert len(deferred) > 4096 * 12 // 8 and plain != deferred
    assert len(lzw("bytes_after_eoi")) == len(lzw("no_eoi")) + 39 + 1 or len(lzw("bytes_after_eoi")) == len(lzw("no_eoi")) + 39 + 2
    assert len(lzw("constant_kwkwk")) < 300                                                # 18000 equal indices: strings that grow by one


def test_pil_refuses_the_corrupt_streams_too():
    for name, (g, status, frame) in C.corrupt_cases().items():
        with pytest.raises(OSError):
            C.pil_frames(g)
        with pytest.raises(ValueError):
            R.decode(g)


# ---- the host parser --------------------------------------------------------------------------------------------------------------------------------------
def test_parse_gif_reads_what_the_yardstick_walker_reads():
    from mmgt_amd import video_in
    for g in C.random_gifs()[:80] + list(C.pil_written().values()):
        h = video_in.parse_gif(g)
        W, H, background, frames = R.walk(g)
        assert (h.width, h.height, h.background, len(h.frames)) == (W, H, background, len(frames))
        for a, b in zip(h.frames, frames):
            assert (a.x, a.y, a.width, a.height) == b["rect"] and a.interlace == b["interlace"] and a.min_code_size == b["mcs"]
            assert a.transparent == b["transparent"] and a.disposal == b["disposal"] and a.lzw == b["lzw"] and a.colours == len(b["table"])
            assert a.palette.shape == (256, 3) and np.array_equal(a.palette[:a.colours], b["table"]) and not a.palette[a.colours:].any()


def test_parse_gif_skips_other_extensions_and_takes_gif87a():
    from mmgt_amd import video_in
    idx = np.arange(35, dtype=np.uint8).reshape(7, 5) % 4
    table = C.random_table(np.random.default_rng(1), 4)
    plain = C.make_gif(5, 7, [dict(idx=idx)], table)
    extra = b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00" + b"\x21\xfe\x05hello\x00" + b"\x21\x01\x02ab\x00"
    more = C.make_gif(5, 7, [dict(idx=idx)], table, extra=extra)
    old = C.make_gif(5, 7, [dict(idx=idx)], table, version=b"GIF87a")
    small = C.make_gif(5, 7, [dict(idx=idx, block=3)], table)
    a = video_in.parse_gif(plain)
    for other in (more, old, small):
        b = video_in.parse_gif(other)
        assert b.frames[0].lzw == a.frames[0].lzw and len(b.frames) == 1
    assert np.array_equal(C.pil_frames(more), C.pil_frames(plain))
    no_trailer = C.make_gif(5, 7, [dict(idx=idx)], table, trailer=False)                   # PIL reads it; so does the parser
    assert len(video_in.parse_gif(no_trailer).frames) == 1 and np.array_equal(C.pil_frames(no_trailer), C.pil_frames(plain))


def _refused():
    idx = np.arange(35, dtype=np.uint8).reshape(7, 5) % 4
    table = C.random_table(np.random.default_rng(1), 4)
    good = C.make_gif(5, 7, [dict(idx=idx, disposal=1)], table)
    at = good.index(b"\x2c", 13 + 12)                                                        # the image descriptor
    data = at + 10 + 1                                                                       # its first sub-block's size byte
    screen = lambda W, H: good[:6] + W.to_bytes(2, "little") + H.to_bytes(2, "little") + good[10:]
    return {
        "bad signature": (b"GIF88a" + good[6:], "bad signature"),
        "a PNG": (b"\x89PNG\r\n\x1a\n" + good[8:], "bad signature"),
        "screen descriptor cut": (good[:10], "logical screen descriptor runs past the end"),
        "global table cut": (good[:20], "global colour table runs past the end"),
        "extension cut": (good[:13 + 12 + 4], "sub-block of extension 0xf9 runs past the end"),
        "descriptor cut": (good[:at + 5], "image descriptor of frame 0 runs past the end"),
        "image data cut": (good[:data + 3], "sub-block of the image data of frame 0 runs past the end"),
        "no block terminator": (good[:-2], "sub-block of the image data of frame 0 runs past the end"),
        "local table cut": (C.make_gif(5, 7, [dict(idx=idx, table=C.random_table(np.random.default_rng(2), 256))], table)[:200],
                            "local colour table of frame 0 runs past the end"),
        "missing trailer": (good[:at], "missing trailer"),
        "no frames": (good[:at] + b"\x3b", "no frames"),
        "no colour table": (C.make_gif(5, 7, [dict(idx=idx, mcs=2)]), "neither a local nor a global colour table"),
        "rectangle leaves the screen": (C.make_gif(5, 7, [dict(idx=idx, x=1)], table), "leaves the logical screen"),
        "rectangle below the screen": (C.make_gif(5, 7, [dict(idx=idx), dict(idx=idx, y=3)], table), "rectangle of frame 1"),
        "empty rectangle": (good[:at + 5] + b"\0\0" + good[at + 7:], "empty rectangle"),
        "code size 1": (good[:at + 10] + b"\x01" + good[at + 11:], "minimum code size 1"),
        "code size 9": (good[:at + 10] + b"\x09" + good[at + 11:], "minimum code size 9"),
        "screen of width 0": (screen(0, 7), "1 .. 16384"),
        "screen above 16384": (screen(5, 16385), "1 .. 16384"),
    }


@pytest.mark.parametrize("case", sorted(_refused()))
def test_parse_gif_refuses_on_the_host(case):
    from mmgt_amd import video_in
    data, word = _refused()[case]
    with pytest.raises(ValueError, match=word):
        video_in.parse_gif(data)


def test_operands_resolve_the_sticky_disposal_and_cut_chunks():
    from mmgt_amd import video_in
    idx = np.zeros((7, 5), np.uint8)
    table = C.random_table(np.random.default_rng(1), 4)
    frames = [dict(idx=idx, disposal=2), dict(idx=idx[:3, :2], x=1, y=2), dict(idx=idx, disposal=3, transparent=1), dict(idx=idx, disposal=0),
              dict(idx=idx, disposal=1), dict(idx=idx)]
    h = video_in.parse_gif(C.make_gif(5, 7, frames, table, background=9))
    tab, palette, data, chunks = video_in.gif_operands(h)
    assert tab.shape == (6, video_in.GIF_TAB) and palette.shape == (6, 256, 3) and data.size % 16 == 0 and chunks == [(0, 6, 5 * 35 + 6)]
    assert tab[:, 10].tolist() == [2, 2, 3, 3, 0, 0] and tab[:, 12].tolist() == [1, 0, 0, 0, 0, 0]
    assert tab[0, 11] == 0 and tab[1, 11] == int(table[0, 0]) | int(table[0, 1]) << 8 | int(table[0, 2]) << 16   # index 9 of 4: padding, then entry 0
    assert tab[:, 4].tolist() == [0, 35, 41, 76, 111, 146] and tab[-1, 6] == sum(len(f.lzw) for f in h.frames)
    _, _, _, chunks = video_in.gif_operands(h, scratch_bytes=80)
    assert chunks == [(0, 3, 76), (3, 5, 70), (5, 6, 35)]                                  # 35 + 6 + 35 indices fit 80 bytes, a fourth frame does not
    tab3, _, data3, chunks3 = video_in.gif_operands(h, limit=3, scratch_bytes=1)
    assert chunks3 == [(0, 1, 35), (1, 2, 6), (2, 3, 35)] and data3.size < data.size + 16 and np.array_equal(tab3[:, 5:], tab[:3, 5:])
    with pytest.raises(ValueError, match="no frames"):
        video_in.gif_operands(h, limit=0)


# ---- the product's arithmetic in a host program under ASan + UBSan ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/gifdec_host_check.cpp with"
    exe = tmp_path_factory.mktemp("gifdec_host") / "gifdec_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "gifdec_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


@pytest.mark.parametrize("short", [0, 4096])
def test_both_copy_paths_take_every_string(tmp_path, short):
    """csrc/gifdec_core.h copies strings of up to GD_SHORT_BYTES one per lane and longer ones by all lanes together; built with the split at either
    end, each path alone must take literals, long strings and strings that run into themselves, in bounds."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    exe = tmp_path / "gifdec_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-DGD_SHORT_BYTES={short}", "-I",
           os.path.join(ROOT, "mmgt_amd", "csrc"), os.path.join(ROOT, "tools", "gifdec_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    for name in ("mcs3", "constant_kwkwk", "deferred_clear", "surplus_pixels"):
        g = C.stream_cases()[name]
        assert np.array_equal(host_decode(str(exe), tmp_path, g), C.pil_frames(g)), name
    g = C.pil_written()["masks"]
    assert np.array_equal(host_decode(str(exe), tmp_path, g, chunk=2), C.pil_frames(g))


def run_host(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True)


def host_decode(exe, tmp_path, data, chunk=None):
    job, out = tmp_path / "job.bin", tmp_path / "out.bin"
    if out.exists():
        out.unlink()
    n, H, W = C.write_job(job, data)
    r = run_host(exe, "decode", str(job), str(out), *([str(chunk)] if chunk else []))
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-3000:]}"
    return np.fromfile(out, np.uint8).reshape(n, H, W, 3)


def test_host_program_equals_pil_on_random_files_whole_and_in_chunks(host_check, tmp_path):
    for k, g in enumerate(C.random_gifs()[:120]):
        got = host_decode(host_check, tmp_path, g, chunk=(k % 3) or None)                  # all at once, one frame at a time, two at a time
        assert np.array_equal(got, C.pil_frames(g)), f"random file {k}"


@pytest.mark.parametrize("name", sorted(C.pil_written()))
def test_host_program_equals_pil_on_pil_written_files(host_check, tmp_path, name):
    g = C.pil_written()[name]
    want = C.pil_frames(g)
    assert np.array_equal(host_decode(host_check, tmp_path, g), want)
    assert np.array_equal(host_decode(host_check, tmp_path, g, chunk=2), want)


@pytest.mark.parametrize("name", sorted(C.stream_cases()))
def test_host_program_reads_the_unusual_streams(host_check, tmp_path, name):
    g = C.stream_cases()[name]
    assert np.array_equal(host_decode(host_check, tmp_path, g), C.pil_frames(g))


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_program_at_every_size_interlaced_and_not(host_check, tmp_path, size):
    W, H = size
    rng = np.random.default_rng(W * 1000 + H)
    table = C.random_table(rng, 256)
    frames = [dict(idx=rng.integers(0, 256, (H, W)), interlace=bool(k & 1), disposal=k % 4, transparent=int(rng.integers(0, 256))) for k in range(4)]
    g = C.make_gif(W, H, frames, table)
    assert np.array_equal(host_decode(host_check, tmp_path, g), C.pil_frames(g))


def test_host_program_decodes_the_projects_own_strip_wise_streams(host_check, tmp_path):
    from tests.test_gif import distinct_palette, lzw_encode, random_indices
    idx = random_indices()                                                                  # 96 x 128
    for strip_len in (128 * 8, 1000):
        stream, _ = lzw_encode(idx, strip_len)
        g = C.make_gif(128, 96, [dict(idx=idx, stream=stream, mcs=8)], distinct_palette())
        assert np.array_equal(host_decode(host_check, tmp_path, g)[0], distinct_palette()[idx])


@pytest.mark.parametrize("name", sorted(C.corrupt_cases()))
def test_host_program_ends_corrupt_streams_in_a_status(host_check, tmp_path, name):
    g, status, frame = C.corrupt_cases()[name]
    job, out = tmp_path / "job.bin", tmp_path / "out.bin"
    C.write_job(job, g)
    r = run_host(host_check, "decode", str(job), str(out))
    assert r.returncode == 3 and f"status {status} in frame {frame}" in r.stderr and not out.exists(), r.stderr[-2000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


FUZZ = {"random_file": lambda: C.random_gifs()[3], "noise": lambda: C.pil_written()["noise"], "masks": lambda: C.pil_written()["masks"],
        "deferred_clear": lambda: C.stream_cases()["deferred_clear"], "constant": lambda: C.stream_cases()["constant_kwkwk"],
        "mcs2": lambda: C.stream_cases()["mcs2"]}


@pytest.mark.parametrize("name", sorted(FUZZ))
def test_host_program_survives_corruptions(host_check, tmp_path, name):
    """300 seeded corruptions per file (byte flips, shortened ranges, overwritten runs, another code size, falsified table rows, single bits): every
    run ends in pixels or a status within the round bound; ASan / UBSan end the program otherwise."""
    C.write_job(tmp_path / "job.bin", FUZZ[name]())
    r = run_host(host_check, "fuzz", str(tmp_path / "job.bin"), "300", "20261019")
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-4000:]}"
    w = r.stdout.split()
    runs, pixels, status = int(w[1]), int(w[3]), int(w[7])
    assert runs == 300 and pixels + status == 300 and status >= 60, r.stdout
