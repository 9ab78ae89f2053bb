"""Lossy WebP (VP8 key frame) decode without a GPU.  Three things are held to PIL (libwebp), the decoder of record, on every byte: the
yardstick tests/vp8dec_ref.py, over PIL-written stills and animations, the project's own writer's streams and crafted streams; the host parser
mmgt_amd.video_in.parse_webp(lossy=True), in its scope and its refusals; and the product's own arithmetic -- csrc/vp8dec_core.h, the code the
kernels call -- run in a stand-alone host program built with AddressSanitizer and UBSan, also stage by stage against the yardstick, and over
seeded corruptions, where it must end clean with pixels or a status.  Nothing is compared with a tolerance."""
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from mmgt_amd import video_in
from tests import vp8_ref as E
from tests import vp8dec_cases as C
from tests import vp8dec_ref as R
from tests import webpdec_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_stills():
    return {**C.stills(), **C.own_streams(), **C.crafted()}


# ---- the yardstick against PIL --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def yardstick():
    counters, out = R.new_counters(), {}
    for name, data in {**all_stills(), **C.animations()}.items():
        out[name] = np.stack(R.decode_file(data, counters))
    return out, counters


def test_yardstick_equals_pil_on_every_byte_of_every_case():
    got, _ = yardstick()
    assert len(C.stills()) == len(C.KINDS) * (len(C.SETTINGS) + len(C.SIZES)) + 1 and len(C.own_streams()) == 10 and len(C.crafted()) >= 38
    for name, data in {**all_stills(), **C.animations()}.items():
        want = C.pil_rgb(data)
        assert got[name].shape == want.shape and np.array_equal(got[name], want), name


def test_the_cases_reach_every_part_of_the_format():
    """A listed item that the inputs stop reaching fails here, so coverage cannot shrink silently."""
    _, c = yardstick()
    assert c["segments"] == {0, 1, 2, 3} and c["map_update"] and c["no_map_update"] and c["absolute"] and c["delta"]
    assert c["i4x4"] and c["i16"] and c["ymodes"] == {R.DC, R.TM, R.VE, R.HE} and c["uvmodes"] == {R.DC, R.TM, R.VE, R.HE}
    assert c["bmodes"] == {(m, y, x) for m in range(10) for y in range(4) for x in range(4)}      # every sub-mode in every block position
    assert c["prob_updates"] and c["skip_on"] and c["skip_off"] and c["tokens"] == set(R.TOKEN_KINDS)
    assert c["simple"] and c["normal"] and c["unfiltered"] and c["inner_skips"] and c["hev"] and c["no_hev"]
    assert c["partitions"] == {1, 2, 4, 8} and c["profiles"] == {0, 1, 2, 3} and c["sharpness"] == set(range(8))
    assert c["lf_delta"] > c["lf_delta_update"] > 0 and c["quant_deltas"] and {0, 63} <= c["levels"]


def test_crafted_bmode_frames_put_every_mode_on_every_border():
    """bmodes-0 .. 9: 3 x 3 macroblocks, all 4 x 4-predicted; over the ten files each of the nine macroblocks (top row, left and right column
    included) sees every mode in every block position."""
    seen = set()
    for f in range(10):
        d = R.decode_vp8(C.vp8_of(C.crafted()[f"bmodes-{f}"]))
        for my in range(3):
            for mx in range(3):
                assert d["mbs"][my][mx]["i4x4"]
                seen |= {(my, mx, n, m) for n, m in enumerate(d["mbs"][my][mx]["modes"])}
    assert len(seen) == 9 * 16 * 10


def test_facts_established_against_pil():
    """What DESIGN 4n lists as confirmed: each is a crafted stream whose two readings differ, and PIL decides."""
    for name, reading in (("level0-beside-filtering-segment", "a header level of 0 switches the filter off for every segment"),
                          ("segments-no-map", "segments without a map update put every macroblock in segment 0"),
                          ("colour-clamp-bits", "the colour-space and clamp-type bits are read and ignored"),
                          ("scale-bits", "the scale bits are ignored"), ("profile-3", "the profile does not select the filter: the header bit does")):
        data = C.crafted()[name]
        d = R.decode_vp8(C.vp8_of(data))
        assert np.array_equal(d["rgb"], C.pil_rgb(data)[0]), reading
    d = R.decode_vp8(C.vp8_of(C.crafted()["level0-beside-filtering-segment"]))
    assert all(np.array_equal(a, b) for a, b in zip(d["filtered"], d["unfiltered"])) and any(p[0][0] for p in d["header"]["filter"])
    d = R.decode_vp8(C.vp8_of(C.crafted()["segments-no-map"]))
    assert {mb["segment"] for row in d["mbs"] for mb in row} == {0}
    d = R.decode_vp8(C.vp8_of(C.crafted()["profile-3"]))
    assert d["header"]["filter_type"] == 1 and not all(np.array_equal(a, b) for a, b in zip(d["filtered"], d["unfiltered"]))
    # "no coefficients" comes from the parsed result: a macroblock coded without the flag but with every level zero keeps its inner edges unfiltered
    d = R.decode_vp8(C.vp8_of(C.crafted()["skip-off"]))
    quiet = [(my, mx) for my in range(3) for mx in range(3) if not d["inner"][my][mx]]
    assert quiet and not d["header"]["use_skip"]


def test_a_reader_past_its_partition_is_refused_as_pil_refuses():
    """Shortened payloads: PIL and the yardstick agree on which still decode (the last partition takes the rest, the chunk's padding byte
    included; a size past the data is cut; a reader that needs a byte past its partition's end is refused)."""
    import io
    from PIL import Image
    agree = refused = 0
    for name in ("own-33x47-p4-f0", "own-144x136-p8-fdefault", "photo-80x48-q75-m4"):
        data = all_stills()[name]
        payload = C.vp8_of(data)
        W, H = int.from_bytes(payload[6:8], "little") & 0x3FFF, int.from_bytes(payload[8:10], "little") & 0x3FFF
        for cut in (1, 2, 3, 4, 5, 6, 40, len(payload) // 2):
            short = payload[:len(payload) - cut]
            try:
                want = np.asarray(Image.open(io.BytesIO(E.webp_file([short], W, H))).convert("RGB"))
            except Exception:
                want = None
            try:
                got = R.decode_file(E.webp_file([short], W, H))[0]
            except R.Bad:
                got = None
            assert (want is None) == (got is None), (name, cut)
            if want is not None:
                assert np.array_equal(got, want), (name, cut)
                agree += 1
            else:
                refused += 1
    assert agree and refused


# ---- the host parser ------------------------------------------------------------------------------------------------------------------------------------
def test_parse_webp_lossy_reads_every_accepted_layout():
    still = C.stills()["photo-80x48-q75-m4"]
    h = video_in.parse_webp(still, lossy=True)
    assert (h.width, h.height, h.animated, len(h.frames)) == (80, 48, False, 1)
    f = h.frames[0]
    assert f.lossy and f.key and not f.alpha_is_used and f.payload[:len(C.vp8_of(still))] == C.vp8_of(still) and len(f.payload) % 2 == 0
    a = video_in.parse_webp(C.animations()["static-default"], lossy=True)
    assert a.animated and len(a.frames) == 6 and all(f.lossy for f in a.frames)
    assert any((f.x, f.y, f.width, f.height) != (0, 0, 80, 48) for f in a.frames) and all(f.x % 2 == 0 and f.y % 2 == 0 for f in a.frames)
    m = video_in.parse_webp(C.animations()["tiles-mixed"], lossy=True)
    assert [f.lossy for f in m.frames] == [k == b"VP8 " for k in C.chunk_kinds(C.animations()["tiles-mixed"])] and {f.lossy for f in m.frames} == {True, False}
    own = video_in.parse_webp(C.own_streams()["own-33x47-p4-f0"], lossy=True)
    assert (own.width, own.height) == (33, 47) and own.frames[0].lossy
    from tests import webpdec_cases as LC                                             # a lossless file parses the same under either setting
    plain = LC.stills()["photo-67x45-m0-q0"]
    assert video_in.parse_webp(plain, lossy=True) == video_in.parse_webp(plain)
    body = b"WEBP" + E._chunk(b"VP8X", b"\0\0\0\0" + struct.pack("<I", 79)[:3] + struct.pack("<I", 47)[:3]) + E._chunk(b"VP8 ", C.vp8_of(still))
    x = video_in.parse_webp(b"RIFF" + struct.pack("<I", len(body)) + body, lossy=True)   # VP8X, then VP8
    assert (x.width, x.height) == (80, 48) and x.frames[0].lossy


def _refused():
    still = C.stills()["photo-80x48-q75-m4"]
    p = bytearray(C.vp8_of(still))
    file_of = lambda payload, W=80, H=48: E.webp_file([bytes(payload)], W, H)
    inter, code, prof, hidden, big = (bytearray(p) for _ in range(5))
    inter[0] |= 1
    code[4] = 0x02
    prof[0] = (prof[0] & ~0x0E) | (4 << 1)
    hidden[0] &= ~0x10
    big[0:3] = struct.pack("<I", (len(p) << 5) | (p[0] & 31))[:3]
    anim = bytearray(C.animations()["noise-default"])
    at = bytes(anim).find(b"VP8 ") + 8
    anim[at + 6] ^= 1                                                                 # the VP8 width of frame 0 no longer equals its ANMF rectangle
    body = b"WEBP" + E._chunk(b"VP8X", b"\0\0\0\0" + struct.pack("<I", 63)[:3] + struct.pack("<I", 47)[:3]) + E._chunk(b"VP8 ", bytes(p))
    return {"not a key frame": file_of(inter), "bad VP8 start code": file_of(code), "bad VP8 profile 4": file_of(prof), "is not shown": file_of(hidden),
            "runs past its VP8 chunk": file_of(big), "no room for its frame header": file_of(p[:7]),
            "differs from its ANMF size": bytes(anim), "differs from the still's VP8 size": b"RIFF" + struct.pack("<I", len(body)) + body,
            "an ALPH chunk": C.mask_animation()}


def test_parse_webp_lossy_refuses_by_name():
    for text, data in _refused().items():
        with pytest.raises(ValueError, match=text):
            video_in.parse_webp(data, lossy=True)
    assert b"ALPH" in C.chunk_kinds(C.mask_animation())
    assert all(b"ALPH" not in C.chunk_kinds(d) for d in C.animations().values())


def test_without_the_option_the_messages_are_todays():
    for data in (C.stills()["photo-80x48-q75-m4"], C.animations()["noise-default"], C.mask_animation(), C.animations()["tiles-mixed"]):
        for call in (lambda: video_in.parse_webp(data), lambda: video_in.parse_webp(data, lossy=False), lambda: video_in.parse_webp(data, False)):
            with pytest.raises(ValueError, match=r"lossy WebP \(VP8\) is not decoded \(chunk b'(VP8 |ALPH)' at byte \d+; VP8L only\)"):
                call()
    with pytest.raises(ValueError, match="lossy WebP"):
        video_in.webp_operands([video_in.parse_webp(C.stills()["noise-1x1-q75-m4"])])
    assert video_in.WEBP_TAB == 16 and video_in.VP8_TAB == 8 and set(video_in.VP8_STATUS_TEXT) == set(range(1, 8))


# ---- the host program -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/vp8dec_host_check.cpp with"
    exe = tmp_path_factory.mktemp("vp8dec_host") / "vp8dec_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "vp8dec_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def run_host(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True)


def host_run(exe, tmp_path, files, mode="decode"):
    """-> (headers, vtab, vidx, the output file's uint32 words)."""
    headers = [video_in.parse_webp(f, lossy=True) for f in files]
    vtab, vidx, _ = C.write_job(tmp_path / "job.bin", headers)
    r = run_host(exe, mode, str(tmp_path / "job.bin"), str(tmp_path / "out.bin"))
    assert r.returncode == 0, r.stderr[-4000:]
    return headers, vtab, vidx, np.fromfile(tmp_path / "out.bin", np.uint32), r.stdout


def rgb_of(words, t):
    a = words[t[4]:t[4] + t[5] * t[6]].reshape(t[6], t[5])
    assert np.all(a >> 24 == 255)
    return np.stack([a >> 16 & 255, a >> 8 & 255, a & 255], -1).astype(np.uint8)


def _by_canvas(files):
    groups = {}
    for name, data in files.items():
        h = video_in.parse_webp(data, lossy=True)
        groups.setdefault((h.width, h.height), []).append(name)
    return groups


def test_host_program_equals_pil_on_every_still(host_check, tmp_path):
    files = all_stills()
    hev = [0, 0]
    for (W, H), names in _by_canvas(files).items():
        _, vtab, _, words, out = host_run(host_check, tmp_path, [files[n] for n in names])
        for t, n in zip(vtab, names):
            assert np.array_equal(rgb_of(words, t), C.pil_rgb(files[n])[0]), n
        w = out.split()
        hev[0] += int(w[2].rstrip(","))
        hev[1] += int(w[5])
    assert hev[0] > 0 and hev[1] > 0


def test_host_program_equals_pil_on_every_animation(host_check, tmp_path):
    for name, data in C.animations().items():
        (h,), vtab, vidx, words, _ = host_run(host_check, tmp_path, [data])
        frames, decoded, v = [], [], 0
        for k, f in enumerate(h.frames):
            frames.append({"x": f.x, "y": f.y, "blend": f.blend, "dispose": f.dispose})
            if f.lossy:
                assert vidx[v] == k
                r = rgb_of(words, vtab[v]).astype(np.uint32)
                decoded.append({"width": f.width, "height": f.height, "alpha_is_used": False, "argb": 0xFF000000 | r[..., 0] << 16 | r[..., 1] << 8 | r[..., 2]})
                v += 1
            else:
                decoded.append(L.decode_vp8l(f.payload))
        got = np.stack(L.compose(h.width, h.height, frames, decoded))[..., :3]
        assert np.array_equal(got, C.pil_rgb(data)), name


STAGED = ("photo-80x48-q75-m4", "half-80x48-q10-m6", "own-33x47-p4-fdefault", "segments-delta", "skip-off-simple", "bmodes-4")


def _frame_views(words, t):
    W, H = int(t[5]), int(t[6])
    mbw, mbh = (W + 15) // 16, (H + 15) // 16
    mbs = mbw * mbh
    raw = words[t[2]:t[2] + 64 + mbs * 296].view(np.uint8)
    hdr = words[t[2]:t[2] + 64]
    mb = raw[256:256 + 32 * mbs].reshape(mbh, mbw, 32)
    coef = raw[256 + 32 * mbs:256 + 800 * mbs].view(np.int16).reshape(mbh, mbw, 24, 16)
    planes = raw[256 + 800 * mbs:]
    Y, U, V = planes[:256 * mbs].reshape(16 * mbh, 16 * mbw), planes[256 * mbs:320 * mbs].reshape(8 * mbh, 8 * mbw), planes[320 * mbs:].reshape(8 * mbh, 8 * mbw)
    return hdr, mb, coef, (Y, U, V)


def test_host_program_equals_the_yardstick_stage_by_stage(host_check, tmp_path):
    """Header block, modes, coefficients, unfiltered planes, filtered planes, RGB: six frames of different kinds, each in a job of its own size."""
    files = all_stills()
    for name in STAGED:
        ref = R.decode_vp8(C.vp8_of(files[name]))
        _, vtab, _, words, _ = host_run(host_check, tmp_path, [files[name]], "parsed")
        hdr, mb, coef, _ = _frame_views(words, vtab[0])
        h = ref["header"]
        assert hdr[0] == 0x56384431 and (hdr[1], hdr[2]) == (len(ref["mbs"][0]), len(ref["mbs"])), name
        assert (hdr[3], hdr[4], hdr[5], hdr[6], hdr[7]) == (h["filter_type"], h["parts"], h["use_skip"], h["use_segment"], h["update_map"]), name
        for s in range(4):
            assert tuple(hdr[8 + 6 * s:14 + 6 * s]) == tuple(h["quant"][s]), name
            for i4 in (0, 1):
                assert tuple(hdr[32 + 4 * (2 * s + i4):35 + 4 * (2 * s + i4)]) == tuple(h["filter"][s][i4]), name
        for my, row in enumerate(ref["mbs"]):
            for mx, m in enumerate(row):
                rec = mb[my, mx]
                assert list(rec[:16]) == list(m["modes"]) and tuple(rec[16:20]) == (m["uvmode"], int(m["i4x4"]), m["segment"], m["skip"]), (name, my, mx)
                assert rec[30] == int(ref["inner"][my][mx]), (name, my, mx)
                if not (h["use_skip"] and m["skip"]):
                    assert np.array_equal(coef[my, mx], ref["coeffs"][my, mx]), (name, my, mx)
        for mode, key in (("unfiltered", "unfiltered"), ("filtered", "filtered")):
            _, vtab, _, words, _ = host_run(host_check, tmp_path, [files[name]], mode)
            planes = _frame_views(words, vtab[0])[3]
            assert all(np.array_equal(a, b) for a, b in zip(planes, ref[key])), (name, mode)
        _, vtab, _, words, _ = host_run(host_check, tmp_path, [files[name]])
        assert np.array_equal(rgb_of(words, vtab[0]), ref["rgb"]), name


def corruptions():
    """Four fixed corruptions of one still, (payload, status code): the GPU test runs them only because the host program shows them in bounds here."""
    p = C.vp8_of(C.own_streams()["own-33x47-p4-f0"])
    first = int.from_bytes(p[:3], "little") >> 5
    cut = max(1, first // 4)
    return {"first partition ends": (struct.pack("<I", (cut << 5) | (p[0] & 31))[:3] + p[3:10] + p[10:10 + cut] + p[10 + first:], 5),
            "token partition ends": (p[:10 + first] + b"\x01\0\0" + p[10 + first + 3:], 6),      # partition 0 declared one byte long
            "partition table past the payload": (p[:10 + first + 4], 4),
            "empty last partition": (p[:10 + first + 9], 4)}


def test_host_program_reports_statuses(host_check, tmp_path):
    good = C.own_streams()["own-33x47-p4-f0"]
    for name, (payload, code) in corruptions().items():
        headers = [video_in.parse_webp(good, lossy=True), video_in.parse_webp(E.webp_file([payload], 33, 47), lossy=True)]
        C.write_job(tmp_path / "job.bin", headers)
        r = run_host(host_check, "decode", str(tmp_path / "job.bin"), str(tmp_path / "out.bin"))
        assert r.returncode == 3 and f"status {code} in frame 1 (parse)" in r.stderr, (name, r.stderr[-500:])
        with pytest.raises(Exception):                                                # PIL refuses each of them too
            C.pil_rgb(E.webp_file([payload], 33, 47))


FUZZ = {"pil": lambda: [C.stills()[n] for n in ("photo-80x48-q75-m4", "half-80x48-q10-m6", "noise-80x48-q50-m2", "mask-80x48-q100-m4")],
        "own": lambda: [C.own_streams()[f"own-33x47-p{p}-fdefault"] for p in (2, 4)],
        "crafted": lambda: [C.crafted()[n] for n in ("segments-delta", "skip-off-simple", "bmodes-4", "lf-delta-update")],
        "edge": lambda: [C.stills()["photo-1x300-q75-m4"]]}


@pytest.mark.parametrize("name", sorted(FUZZ))
def test_host_program_survives_corruptions(host_check, tmp_path, name):
    """500 seeded corruptions per set, 2000 in all (byte flips, shortened payloads, overwritten runs, falsified header fields and frame tags, table
    rows that lie): every run ends in pixels or a status; ASan / UBSan end the program otherwise.  Every loop's trip count comes from the row's
    sizes, so there is no step bound to hold beyond the program ending."""
    C.write_job(tmp_path / "job.bin", [video_in.parse_webp(d, lossy=True) for d in FUZZ[name]()])
    r = run_host(host_check, "fuzz", str(tmp_path / "job.bin"), "500", "20261020")
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-4000:]}"
    w = r.stdout.split()
    runs, pixels, status = int(w[1]), int(w[3]), int(w[7])
    assert runs == 500 and pixels + status == runs and status >= 100 and pixels >= 50, r.stdout
