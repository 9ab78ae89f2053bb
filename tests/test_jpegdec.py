"""Baseline JPEG decode without a GPU: the numpy restatement tests/jpegdec_ref.py is held to PIL (libjpeg-turbo) byte for byte, the host
parser mmgt_amd.video_in.parse_jpeg to its refusals, and the product's own arithmetic -- csrc/jpegdec_core.h, the code the kernels call -- runs in a
stand-alone host program built with AddressSanitizer and UBSan: on the same files against PIL, and over seeded corruptions, where it must end
clean with pixels or a status."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image, features

from tests import jpegdec_cases as C
from tests import jpegdec_ref as R
from tests import mjpeg_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def require_turbo():
    assert features.check_feature("libjpeg_turbo"), (
        "PIL here is not built on libjpeg-turbo: tests/jpegdec_ref.py restates THAT library's default decode (slow-integer IDCT, fancy "
        "up-sampling), so a byte-for-byte comparison with another libjpeg proves nothing")


# ---- the restatement is libjpeg-turbo's decode ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names())
def test_restatement_equals_pil(name):
    require_turbo()
    data = C.streams()[name]
    got, want = R.decode(data), pil_rgb(data)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{name}: {np.count_nonzero(got != want)} bytes differ, max |d| = {np.abs(got.astype(int) - want).max()}"


def test_streams_hold_the_hard_cases():
    """The cases the list is there for cannot silently vanish: 0xFF 0x00 stuffing, restart segments that cross MCU rows, per-file Huffman tables,
    a file without DHT, one component, chroma planes of 2 samples' width."""
    S = C.streams()
    assert any(b"\xff\x00" in seg for seg in R.parse(S["ref_48x64_444_q100_noise"])["segments"])
    p = R.parse(S["pil_restart_blocks3"])
    assert p["ri"] == 3 and p["ri"] % R.geometry(p)[4] != 0 and len(p["segments"]) > 1
    assert R.parse(S["pil_optimize"])["huff"] != R.annex_k_tables() and R.parse(S["pil_default"])["huff"] == R.annex_k_tables()
    assert b"\xff\xc4" not in S["pil_default_no_dht"][:S["pil_default_no_dht"].index(b"\xff\xda")]
    assert len(R.parse(S["pil_grey"])["comps"]) == 1
    assert [R.parse(S[f"pil_subsampling{k}"])["comps"][0][1:3] for k in (0, 1, 2)] == [(1, 1), (2, 1), (2, 2)]
    assert R.parse(S["narrow_420_w3"])["W"] == 3 and R.parse(S["narrow_422_w4"])["W"] == 4


# ---- the host parser ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names())
def test_parse_jpeg_agrees_with_the_restatement(name):
    from mmgt_amd import video_in
    data = C.streams()[name]
    h, p = video_in.parse_jpeg(data + b"\0"), R.parse(data)                                  # + AVI chunk padding
    ncomp, hs, vs, rows, cols = R.geometry(p)
    assert (h.height, h.width, h.ncomp, h.hs, h.vs, h.mcu_rows, h.mcu_cols) == (p["H"], p["W"], ncomp, hs, vs, rows, cols)
    assert h.restart_interval == p["ri"] and h.scan_offset == h.segments[0][0]
    assert [data[a:b] for a, b in h.segments] == p["segments"]
    assert h.huffman == p["huff"] and (h.td, h.ta) == tuple(zip(*p["scan"]))
    for c in range(ncomp):
        assert np.array_equal(h.qtables[h.tq[c]], p["q"][p["comps"][c][3]])


def _seg(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def _find(data, marker):
    """Offset of the first header segment with that marker."""
    pos = 2
    while data[pos + 1] != marker:
        assert data[pos + 1] != 0xDA, f"no segment {marker:#x}"
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    return pos


def _patch(data, at, value):
    return data[:at] + bytes([value]) + data[at + 1:]


def _drop(data, marker):
    at = _find(data, marker)
    return data[:at] + data[at + 2 + int.from_bytes(data[at + 2:at + 4], "big"):]


def _refused():
    S = C.streams()
    good, rst = S["pil_default"], S["ref_48x64_420_q90_smooth"]                               # rst: three MCU rows = three restart intervals
    sof, sos, dqt = _find(good, 0xC0), _find(good, 0xDA), _find(good, 0xDB)
    frame = M.smooth_frame(24, 24, 3)
    r1 = rst.index(b"\xff\xd1", _find(rst, 0xDA))
    cmyk = io.BytesIO()
    Image.new("CMYK", (24, 24), (10, 60, 110, 160)).save(cmyk, format="JPEG")
    scan_len = 2 + int.from_bytes(good[sos + 2:sos + 4], "big")
    return {
        "progressive": (C.pil_jpeg(frame, progressive=True), "progressive"),
        "arithmetic": (_patch(good, sof + 1, 0xC9), "arithmetic"),
        "lossless": (_patch(good, sof + 1, 0xC3), "lossless"),
        "12-bit samples": (_patch(good, sof + 4, 12), "12-bit samples"),
        "16-bit quantiser tables": (_patch(good, dqt + 4, good[dqt + 4] | 0x10), "16-bit quantiser tables"),
        "four components": (cmyk.getvalue(), "four components"),
        "adobe transform 0": (good[:2] + _seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0])) + good[2:], "Adobe APP14 transform 0"),
        "sampling 1x2": (_patch(good, sof + 11, 0x12), "sampling factors"),
        "sampling chroma 2x1": (_patch(good, sof + 14, 0x21), "sampling factors"),
        "scan of one component": (good[:sos] + _seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + good[sos + scan_len:], "more than one scan"),
        "second scan": (good[:-2] + _seg(0xDA, bytes([1, 2, 0x11, 0, 63, 0])) + b"\x55\xff\xd9", "more than one scan"),
        "missing SOF": (_drop(good, 0xC0), "missing SOF"),
        "missing SOS": (good[:sos], "missing SOS"),
        "missing EOI": (good[:-2], "missing EOI"),
        "truncated in mid-scan": (good[:sos + scan_len + (len(good) - sos - scan_len) // 2], "missing EOI"),
        "restart out of sequence": (_patch(rst, r1 + 1, 0xD3), "restart marker out of sequence"),
        "restart without DRI": (_drop(rst, 0xDD), "restart marker out of sequence"),
        "fewer restart intervals": (rst[:r1] + b"\xff\xd9", "fewer than"),
    }


@pytest.mark.parametrize("case", sorted(_refused()))
def test_parse_jpeg_refuses_on_the_host(case):
    from mmgt_amd import video_in
    data, word = _refused()[case]
    with pytest.raises(ValueError, match=word):
        video_in.parse_jpeg(data)


def test_refusal_files_differ_from_a_good_file_only_where_stated():
    """The builders above patch the bytes they mean to: the unpatched files parse."""
    from mmgt_amd import video_in
    S = C.streams()
    assert video_in.parse_jpeg(S["pil_default"]).ncomp == 3 and len(video_in.parse_jpeg(S["ref_48x64_420_q90_smooth"]).segments) == 3
    good = S["pil_default"]
    sof = _find(good, 0xC0)
    assert good[sof + 4] == 8 and good[sof + 11] == 0x22 and good[sof + 14] == 0x11 and good[_find(good, 0xDB) + 4] >> 4 == 0


def test_a_batch_is_one_size():
    from mmgt_amd import video_in
    S = C.streams()
    with pytest.raises(ValueError, match="one call decodes one size"):
        video_in.batch_operands([S["ref_21x37_420_q90_smooth"], S["ref_16x16_420_q90_smooth"]])
    with pytest.raises(ValueError, match="one call decodes one size"):
        video_in.batch_operands([S["ref_21x37_420_q90_smooth"], S["ref_21x37_444_q90_smooth"]])


# ---- the product's arithmetic in a host program under ASan + UBSan ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/jpegdec_host_check.cpp with"
    exe = tmp_path_factory.mktemp("jpegdec_host") / "jpegdec_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "jpegdec_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def write_job(path, jpegs):
    from mmgt_amd import video_in
    headers, data, offsets, seginfo, tables = video_in.batch_operands(jpegs)
    H, W, ncomp, hs, vs = headers[0].geometry
    with open(path, "wb") as fh:
        fh.write(struct.pack("<10i", 0x314A444A, len(headers), H, W, ncomp, hs, vs, len(seginfo), video_in.TAB_INTS, 0))
        fh.write(struct.pack("<q", data.size))
        for a in (tables.astype("<i4"), seginfo.astype("<i4"), offsets.astype("<i8"), data):
            fh.write(np.ascontiguousarray(a).tobytes())
    return len(headers), H, W


def run_host(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True)


def test_host_program_equals_pil_on_every_stream(host_check, tmp_path):
    require_turbo()
    for name, data in C.streams().items():
        job, out = tmp_path / "job.bin", tmp_path / "out.rgb"
        n, H, W = write_job(job, [data])
        r = run_host(host_check, "decode", str(job), str(out))
        assert r.returncode == 0, f"{name}: {r.stdout[-500:]}{r.stderr[-3000:]}"
        got = np.fromfile(out, np.uint8).reshape(H, W, 3)
        assert np.array_equal(got, pil_rgb(data)), name


def batch_of_five():
    """Five 21 x 37 frames whose quantiser AND Huffman tables differ (different pictures and qualities under optimize=True)."""
    return [C.pil_jpeg(M.smooth_frame(21, 37, 100 + k, sigma=3.0 + 9 * k), optimize=True, quality=60 + 8 * k) for k in range(5)]


def test_host_program_decodes_a_batch_with_per_frame_tables(host_check, tmp_path):
    require_turbo()
    from mmgt_amd import video_in
    jpegs = batch_of_five()
    heads = [video_in.parse_jpeg(j) for j in jpegs]
    assert len({h.huffman[(1, 0)] for h in heads}) > 1 and len({h.qtables[0].tobytes() for h in heads}) > 1
    n, H, W = write_job(tmp_path / "job.bin", jpegs)
    r = run_host(host_check, "decode", str(tmp_path / "job.bin"), str(tmp_path / "out.rgb"))
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.fromfile(tmp_path / "out.rgb", np.uint8).reshape(n, H, W, 3)
    assert np.array_equal(got, np.stack([pil_rgb(j) for j in jpegs]))


def test_host_program_reports_a_status_for_a_cut_segment(host_check, tmp_path):
    """A stream whose markers are all in place but whose first segment lost its second half: past the host checks, so the status word speaks."""
    from mmgt_amd import video_in
    data = C.streams()["ref_48x64_420_q90_smooth"]
    a, b = video_in.parse_jpeg(data).segments[0]
    write_job(tmp_path / "job.bin", [data[:a + (b - a) // 2] + data[b:]])
    r = run_host(host_check, "decode", str(tmp_path / "job.bin"), str(tmp_path / "out.rgb"))
    assert r.returncode == 3 and "segment 0" in r.stderr, r.stderr[-3000:]
    assert not (tmp_path / "out.rgb").exists()


@pytest.mark.parametrize("name", ["ref_48x64_420_q100_noise", "pil_restart_blocks3", "pil_optimize", "pil_grey", "pil_subsampling1", "narrow_420_w3"])
def test_host_program_survives_corruptions(host_check, tmp_path, name):
    """400 seeded corruptions per stream (byte flips, shortened ranges, overwritten runs, extreme coefficients x quantisers): every run ends in
    pixels or a status; ASan / UBSan end the program otherwise."""
    write_job(tmp_path / "job.bin", [C.streams()[name]])
    r = run_host(host_check, "fuzz", str(tmp_path / "job.bin"), "400", "20261018")
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-4000:]}"
    runs, pixels, status = (int(r.stdout.split()[k]) for k in (1, 3, 7))
    assert runs == 400 and pixels + status == 400 and pixels >= 100 and status >= 1, r.stdout
