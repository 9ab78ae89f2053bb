"""Progressive JPEG decode without a GPU: the restatement tests/jpegprog_ref.py is held to PIL (libjpeg-turbo) byte for byte, every
transcoded stream of tests/jpegprog_cases.py to its baseline source under PIL, the host parser mmgt_amd.video_in.parse_jpeg(progressive=True) to the
restatement and to its refusals, and the product's own arithmetic -- csrc/jpegprog_core.h, the code the kernel calls -- runs in a stand-alone
host program built with AddressSanitizer and UBSan: on the same files against PIL, and over seeded corruptions, where every lane must end in a
status or leave everything outside its own blocks and band untouched."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image, features

from tests import jpegdec_cases as B
from tests import jpegdec_ref as R
from tests import jpegprog_cases as C
from tests import jpegprog_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def require_turbo():
    assert features.check_feature("libjpeg_turbo"), (
        "PIL here is not built on libjpeg-turbo: the restatements state THAT library's default decode, so a byte-for-byte comparison with another "
        "libjpeg proves nothing")


def script_of(p):
    return [(tuple(s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in p["scans"]]


# ---- the restatement and the fixtures -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names())
def test_restatement_equals_pil(name):
    require_turbo()
    data = C.streams()[name]
    got, want = P.decode(data), pil_rgb(data)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{name}: {np.count_nonzero(got != want)} bytes differ"


@pytest.mark.parametrize("name", C.names())
def test_every_stream_equals_its_baseline_twin_under_pil(name):
    """For a transcoded stream this is what makes it a valid fixture; for a PIL-written pair it is the fact the GPU test's twin comparison rests on."""
    twin = C.twins()[name]
    assert b"\xff\xc0" in twin[:twin.index(b"\xff\xda")] and b"\xff\xc2" in C.streams()[name]
    assert np.array_equal(pil_rgb(C.streams()[name]), pil_rgb(twin)), name


def test_streams_hold_the_hard_cases():
    S = C.streams()
    for name in S:
        p = P.parse(S[name])
        if name.startswith("pil_"):
            assert script_of(p) == (C.PIL_SCRIPT if len(p["comps"]) == 3 else C.PIL_SCRIPT_GREY), name
        else:
            assert script_of(p) == C.SCRIPTS[C.transcoded()[name][2]], name
    p = P.parse(S["pil_21x37_420_smooth"])                               # 5 x 3 own luma blocks inside a 6 x 4 padded grid
    assert [P.scan_units(p, s)[0] for s in p["scans"][:2]] == [6, 15] and R.geometry(p)[3:] == (2, 3)
    assert len({tuple(sorted(s["huff"].items())) for s in p["scans"]}) > 3                      # the tables are redefined between scans
    p = P.parse(S["pil_48x64_420_restart_rows1"])
    assert len({s["ri"] for s in p["scans"]}) > 1 and all(len(s["segments"]) > 1 for s in p["scans"])      # a DRI of its own per scan
    p = P.parse(S["tc_21x37_420_smooth_restarts"])
    assert [s["ri"] for s in p["scans"]] == C.RESTARTS["restarts"] and len(p["scans"][1]["segments"]) == 15
    assert {t for s in P.parse(S["tc_16x16_444_noise_deep"])["scans"] for t in s["td"] + s["ta"]} == {0, 1, 2, 3}
    p = P.parse(S["pil_128x128_grey_one_pixel"])                         # AC scans that are single EOB runs of 255 or 256 blocks: EOB7 + bits, EOB8
    P.coefficients(p)
    assert p["eob_runs"] and max(p["eob_runs"]) == 256 and 255 in p["eob_runs"]
    assert max(int(np.abs(c[..., 1:]).max()) for c in P.coefficients(P.parse(S["pil_16x16_444_noise_q100"]))) > 127   # AC categories up to 8


# ---- the host parser ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names())
def test_parse_jpeg_agrees_with_the_restatement(name):
    from mmgt_amd import video_in
    data = C.streams()[name]
    h, p = video_in.parse_jpeg(data + b"\0", progressive=True), P.parse(data)
    ncomp, hs, vs, rows, cols = R.geometry(p)
    assert h.progressive and (h.height, h.width, h.ncomp, h.hs, h.vs, h.mcu_rows, h.mcu_cols) == (p["H"], p["W"], ncomp, hs, vs, rows, cols)
    assert len(h.scans) == len(p["scans"])
    for a, b in zip(h.scans, p["scans"]):
        assert (a.comps, a.ss, a.se, a.ah, a.al, a.restart_interval) == (tuple(b["comps"]), b["ss"], b["se"], b["ah"], b["al"], b["ri"])
        assert (list(a.td), list(a.ta)) == (b["td"], b["ta"]) and a.huffman == b["huff"]
        assert a.units == P.scan_units(p, b)[0] and [data[x:y] for x, y in a.segments] == b["segments"]
    assert [s.level for s in h.scans] == P.levels([(s.comps, s.ss, s.se) for s in h.scans])
    for c in range(ncomp):
        assert np.array_equal(h.qtables[h.tq[c]], p["q"][p["comps"][c][3]])


def test_a_baseline_file_parses_as_before_with_the_argument():
    from mmgt_amd import video_in
    data = B.streams()["pil_restart_blocks3"]
    a, b = video_in.parse_jpeg(data), video_in.parse_jpeg(data, progressive=True)
    assert not a.progressive and not b.progressive and b.scans == [] and a.segments == b.segments and a.huffman == b.huffman


def test_levels_of_the_scripts():
    from mmgt_amd import video_in
    lv = lambda script: video_in.scan_levels([s[:3] for s in script])
    assert lv(C.PIL_SCRIPT) == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2] and lv(C.PIL_SCRIPT_GREY) == [0, 0, 0, 1, 1, 2]
    assert lv(C.SCRIPTS["spectral"]) == [0, 0, 0, 0] and lv(C.SCRIPTS["dc_split"]) == [0] * 6 and lv(C.SCRIPTS["bands"]) == [0] * 10
    assert lv(C.SCRIPTS["deep"]) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3]
    assert lv(C.SCRIPTS["chroma_first"]) == [0, 0, 0, 0, 1, 1, 1, 1]
    for script in [C.PIL_SCRIPT, C.PIL_SCRIPT_GREY, *C.SCRIPTS.values()]:
        assert lv(script) == P.levels([s[:3] for s in script])
    assert lv([((0,), 0, 0), ((0,), 1, 5), ((0,), 3, 9), ((0,), 0, 0), ((0,), 9, 9)]) == [0, 0, 1, 1, 2]      # a partial overlap of bands


def _seg(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def _markers(data):
    """[(marker, offset of its 0xFF)] of every header segment and SOS of a progressive file."""
    out, pos = [], 2
    while data[pos + 1] != 0xD9:
        m = data[pos + 1]
        out.append((m, pos))
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        if m == 0xDA:
            while not (data[pos] == 0xFF and data[pos + 1] not in (0, 0xFF) and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
    return out


def _patch(data, at, value):
    return data[:at] + bytes([value]) + data[at + 1:]


def _good():
    return C.streams()["pil_21x37_420_smooth"], C.streams()["pil_48x64_420_restart_rows1"]


def _refused():
    """name -> (file, word of the message): each file is `good` (or `rst`) patched in the one place its name states."""
    good, rst = _good()
    mk = _markers(good)
    sos = [at for m, at in mk if m == 0xDA]                              # the ten scans; scan k's Ss, Se, AhAl are its last three header bytes
    tail = lambda k: sos[k] + 2 + int.from_bytes(good[sos[k] + 2:sos[k] + 4], "big") - 3
    end = lambda k: next(at for m, at in mk if at > sos[k]) if k < 9 else len(good) - 2          # where scan k's data ends
    sof, dqt = next(at for m, at in mk if m == 0xC2), next(at for m, at in mk if m == 0xDB)
    dht1 = next(at for m, at in mk if m == 0xC4 and at > sos[0])         # the AC table scan 1 uses
    dht_len = 2 + int.from_bytes(good[dht1 + 2:dht1 + 4], "big")
    dqt_seg = good[dqt:dqt + 2 + int.from_bytes(good[dqt + 2:dqt + 4], "big")]
    rmk = _markers(rst)
    rsos = [at for m, at in rmk if m == 0xDA]
    r1 = rst.index(b"\xff\xd1", rsos[1])
    dri1 = max(at for m, at in rmk if m == 0xDD and at < rsos[1])
    dri0 = next(at for m, at in rmk if m == 0xDD)                        # before scan 0, whose restart markers then have no interval
    bands = C.streams()["tc_21x37_420_smooth_bands"]                     # scan 2 of it is component 0's band 2 - 7, its DHT before it
    bsos = [at for m, at in _markers(bands) if m == 0xC4]               # one DHT per scan: scan k is bands[bsos[k]:bsos[k + 1]]
    return {
        "arithmetic progressive": (_patch(good, sof + 1, 0xCA), "arithmetic"),
        "lossless": (_patch(good, sof + 1, 0xC3), "lossless"),
        "differential progressive": (_patch(good, sof + 1, 0xC6), "differential"),
        "12-bit samples": (_patch(good, sof + 4, 12), "12-bit samples"),
        "sampling 1x2": (_patch(good, sof + 11, 0x12), "sampling factors"),
        "adobe transform 0": (good[:2] + _seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0])) + good[2:], "Adobe APP14 transform 0"),
        "DNL": (good[:sos[1]] + _seg(0xDC, struct.pack(">H", 21)) + good[sos[1]:], "DNL"),
        "DQT after the first SOS": (good[:sos[3]] + dqt_seg + good[sos[3]:], "DQT after the first scan"),
        "Ss above Se": (_patch(good, tail(1), 6), "no legal progression"),
        "Se above 63": (_patch(good, tail(4) + 1, 64), "no legal progression"),
        "DC scan with Se 5": (_patch(good, tail(0) + 1, 5), "no legal progression"),
        "AC scan of three components": (good[:tail(0)] + bytes([1, 5]) + good[tail(0) + 2:], "an AC scan holds one component"),
        "Al 14": (_patch(good, tail(1) + 2, 0x0E), "no legal progression"),
        "Al not Ah - 1": (_patch(good, tail(5) + 2, 0x20), "no legal progression"),
        "first scan with Ah": (_patch(good, tail(1) + 2, 0x32), "has Ah != 0"),
        "refinement from the wrong Al": (_patch(good, tail(9) + 2, 0x21), "which stands at Al 1"),
        "AC before DC": (good[:sos[0]] + good[sos[1]:end(1)] + good[sos[0]:sos[1]] + good[end(1):], "before that component's DC first scan"),
        "sent twice": (good[:end(1)] + good[sos[1]:end(1)] + good[end(1):], "sent twice at the same precision"),
        "last refinement missing": (good[:end(8)] + b"\xff\xd9", "inter-block smoothing"),
        "band never sent": (bands[:bsos[2]] + bands[bsos[3]:], "coefficient 2 of component 0 is never sent.*inter-block smoothing"),
        "EOI after one scan": (good[:end(0)] + b"\xff\xd9", "inter-block smoothing"),
        "table no DHT has defined": (good[:dht1] + good[dht1 + dht_len:], "which no DHT has defined by that point"),
        "restart out of sequence": (_patch(rst, r1 + 1, 0xD3), "restart marker out of sequence"),
        "fewer restart intervals": (rst[:dri1 + 4] + struct.pack(">H", 1) + rst[dri1 + 6:], "fewer than"),
        "restart without DRI": (rst[:dri0] + rst[dri0 + 6:], "restart marker out of sequence"),
        "missing EOI": (good[:-2], "missing EOI"),
        "truncated in a scan": (good[:(sos[4] + end(4)) // 2 + 8], "missing EOI"),
    }


@pytest.mark.parametrize("case", sorted(_refused()))
def test_parse_jpeg_refuses_on_the_host(case):
    from mmgt_amd import video_in
    data, word = _refused()[case]
    with pytest.raises(ValueError, match=word):
        video_in.parse_jpeg(data, progressive=True)


def test_refusal_files_differ_from_a_good_file_only_where_stated():
    """The builders above patch the bytes they mean to: the unpatched files parse, and the bytes patched hold what the builders take them to."""
    from mmgt_amd import video_in
    good, rst = _good()
    h, hr = video_in.parse_jpeg(good, progressive=True), video_in.parse_jpeg(rst, progressive=True)
    assert [(s.comps, s.ss, s.se, s.ah, s.al) for s in h.scans] == C.PIL_SCRIPT and len(hr.scans) == 10
    assert hr.scans[1].restart_interval > 1 and len(hr.scans[1].segments) > 2
    mk = _markers(good)
    sos = [at for m, at in mk if m == 0xDA]
    assert len(sos) == 10 and [m for m, _ in mk].count(0xC2) == 1
    for k, s in enumerate(h.scans):
        t = sos[k] + 2 + int.from_bytes(good[sos[k] + 2:sos[k] + 4], "big") - 3
        assert tuple(good[t:t + 3]) == (s.ss, s.se, (s.ah << 4) | s.al) and s.segments[0][0] == t + 3
    sof = next(at for m, at in mk if m == 0xC2)
    assert good[sof + 4] == 8 and good[sof + 11] == 0x22
    assert any(m == 0xC4 and sos[0] < at < sos[1] for m, at in mk) and any(m == 0xC4 and sos[8] < at < sos[9] for m, at in mk)


def test_the_defaults_still_refuse():
    from mmgt_amd import video_in
    prog = C.streams()["pil_21x37_420_smooth"]
    with pytest.raises(ValueError, match=r"progressive JPEG \(SOF2\) is not decoded \(baseline SOF0 only\)"):
        video_in.parse_jpeg(prog)
    with pytest.raises(ValueError, match="progressive"):
        video_in.parse_jpeg(prog, progressive=False)
    with pytest.raises(ValueError, match="progressive"):
        video_in.batch_operands([prog])


def test_a_batch_is_one_size():
    from mmgt_amd import video_in
    S = C.streams()
    with pytest.raises(ValueError, match="one call decodes one size"):
        video_in.decode_jpeg_frames([S["pil_21x37_420_smooth"], S["pil_33x17_422"]], "cpu", progressive=True)
    with pytest.raises(ValueError, match="one call decodes one size"):
        video_in.decode_jpeg_frames([B.streams()["ref_21x37_444_q90_smooth"], S["pil_21x37_420_smooth"]], "cpu", progressive=True)


# ---- the product's arithmetic in a host program under ASan + UBSan ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/jpegprog_host_check.cpp with"
    exe = tmp_path_factory.mktemp("jpegprog_host") / "jpegprog_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "jpegprog_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def write_job(path, jpegs):
    """The operands of decode_jpeg_frames(jpegs, progressive=True), as mmgt_amd.video_in builds them, in the host program's file format."""
    from mmgt_amd import video_in
    heads = [video_in.parse_jpeg(j, progressive=True) for j in jpegs]
    video_in._same_geometry(heads)
    prog, base = [k for k, h in enumerate(heads) if h.progressive], [k for k, h in enumerate(heads) if not h.progressive]
    H, W, ncomp, hs, vs = heads[0].geometry
    z32, z64, z8 = np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.uint8)
    po = video_in.prog_batch_operands([jpegs[k] for k in prog], [heads[k] for k in prog]) if prog else dict(
        tables=z32, scaninfo=z32, huff=z32, seginfo=z32, levels=z64, offsets=z64, data=z8)
    bo = video_in.batch_operands([jpegs[k] for k in base], [heads[k] for k in base])[1:] if base else (z8, z64, z32, z32)
    b_data, b_offsets, b_seginfo, b_tables = bo
    with open(path, "wb") as fh:
        fh.write(struct.pack("<16i", 0x314A504A, len(heads), H, W, ncomp, hs, vs, len(prog), len(base), len(po["seginfo"]), len(po["scaninfo"]),
                             len(po["huff"]), len(po["levels"]) - 1, len(b_seginfo), video_in.TAB_INTS, 0))
        fh.write(struct.pack("<2q", po["data"].size if prog else 0, b_data.size if base else 0))
        for a, t in ((np.asarray(prog), "<i4"), (np.asarray(base), "<i4"), (po["tables"], "<i4"), (po["scaninfo"], "<i4"), (po["huff"], "<i4"),
                     (po["seginfo"], "<i4"), (po["levels"], "<i8"), (po["offsets"], "<i8"), (po["data"] if prog else z8, "u1"),
                     (b_tables, "<i4"), (b_seginfo, "<i4"), (b_offsets, "<i8"), (b_data if base else z8, "u1")):
            fh.write(np.ascontiguousarray(np.asarray(a).astype(t)).tobytes())
    return len(heads), H, W


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


def mixed_batch():
    """21 x 37 4:2:0: three progressive files under three scripts, a baseline file third of four."""
    S = C.streams()
    return [S["pil_21x37_420_smooth"], S["tc_21x37_420_smooth_deep"], C.twins()["pil_21x37_420_smooth"], S["tc_21x37_420_smooth_restarts"]]


def test_host_program_decodes_a_mixed_batch(host_check, tmp_path):
    require_turbo()
    jpegs = mixed_batch()
    n, H, W = write_job(tmp_path / "job.bin", jpegs)
    r = run_host(host_check, "decode", str(tmp_path / "job.bin"), str(tmp_path / "out.rgb"))
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.fromfile(tmp_path / "out.rgb", np.uint8).reshape(n, H, W, 3)
    assert np.array_equal(got, np.stack([pil_rgb(j) for j in jpegs]))


def cut_scan(data, k):
    """The file with the second half of scan k's (only) restart segment removed: every marker stays in place, so the parser accepts it."""
    from mmgt_amd import video_in
    a, b = video_in.parse_jpeg(data, progressive=True).scans[k].segments[0]
    return data[:a + (b - a) // 2] + data[b:]


def test_host_program_reports_a_status_for_a_scan_cut_in_half(host_check, tmp_path):
    write_job(tmp_path / "job.bin", [cut_scan(C.streams()["pil_21x37_420_smooth"], 4)])
    r = run_host(host_check, "decode", str(tmp_path / "job.bin"), str(tmp_path / "out.rgb"))
    assert r.returncode == 3 and "progressive segment 4 (scan descriptor 4)" in r.stderr, r.stderr[-3000:]
    assert not (tmp_path / "out.rgb").exists()


def test_host_program_follows_the_longest_eob_run(host_check):
    """Synthetic operands: EOB14 with all fourteen appended bits set is a run of 32767 blocks; against a segment of 32766 it is a status."""
    r = run_host(host_check, "eobrun")
    assert r.returncode == 0 and "AC status 0 over 40955 blocks, all coefficients zero 1; a segment of 32766 blocks: status 4" in r.stdout, (
        r.stdout + r.stderr[-3000:])


@pytest.mark.parametrize("name", ["pil_16x16_444_noise_q100", "pil_21x37_420_smooth", "pil_48x64_420_restart_rows1", "pil_8x8_grey",
                                  "tc_21x37_420_smooth_deep", "tc_16x16_444_noise_restarts", "pil_128x128_grey_one_pixel"])
def test_host_program_survives_corruptions(host_check, tmp_path, name):
    """300 seeded corruptions per stream (entropy bytes, byte ranges, segment and scan descriptors, Huffman blocks), decoded lane by lane: every
    lane ends in a status or clean, and the coefficients outside its frame, components, blocks and band are unchanged (exit 5 otherwise); ASan /
    UBSan end the program on anything else."""
    write_job(tmp_path / "job.bin", [C.streams()[name]])
    r = run_host(host_check, "fuzz", str(tmp_path / "job.bin"), "300", "20261020")
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-4000:]}"
    runs, clean, status = (int(r.stdout.split()[k]) for k in (1, 3, 7))
    assert runs == 300 and clean + status == 300 and clean >= 1 and status >= 50, r.stdout
    by_code = [int(v.rstrip(")")) for v in r.stdout.split("code:")[1].split()]
    assert by_code[5] >= 1 and sum(1 for v in by_code if v) >= 3, r.stdout                  # descriptors among them, and several kinds in all
