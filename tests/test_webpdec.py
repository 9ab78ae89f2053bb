"""WebP lossless / animated WebP decode without a GPU.  Three things are held to PIL (libwebp), the decoder of record, on every byte: the
yardstick tests/webpdec_ref.py, over PIL-written stills, crafted streams and hand-assembled animations; the host parser
mmgt_amd.video_in.parse_webp, in its scope and its refusals; and the product's own arithmetic -- csrc/webpdec_core.h, the code the kernels call --
run in a stand-alone host program built with AddressSanitizer and UBSan, also stage by stage against the yardstick, and over seeded corruptions,
where it must end clean with pixels or a status.  Nothing is compared with a tolerance."""
import functools
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

from mmgt_amd import decode_webp_frames, parse_webp                                    # noqa: F401  (the feature's public names)
from tests import webp_ref as E
from tests import webpdec_cases as C
from tests import webpdec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the yardstick against PIL --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def yardstick_stills():
    counters, out = R.new_counters(), {}
    for name, data in C.stills().items():
        out[name] = R.decode_file(data, counters)[0]
    return out, counters


def test_yardstick_equals_pil_on_every_pil_written_still():
    got, _ = yardstick_stills()
    assert len(got) == len(C.KINDS) * len(C.METHODS) * len(C.QUALITIES) + len(C.SIZES) * 6 + 2 + 1 + 2
    for name, data in C.stills().items():
        want = C.pil_rgba(data)[0]
        assert np.array_equal(got[name][..., :3], want[..., :3]), name
        if name.startswith("rgba"):
            assert np.array_equal(got[name], want), name


def test_the_still_corpus_reaches_every_feature():
    _, c = yardstick_stills()
    assert c["transforms"] == {0, 1, 2, 3}
    assert set(range(14)) <= c["modes"], sorted(c["modes"])
    assert c["cache_bits"] and c["cache_hits"] > 0
    assert c["groups"] >= 8 and c["max_symbol"] > 0 and c["simple_codes"] > 0 and c["one_symbol_normal_codes"] > 0 and c["far_distances"] > 0
    assert c["overlapping_copies"] > 0 and len(c["short_distance_codes"]) >= 20


@functools.lru_cache(None)
def yardstick_crafted():
    counters = {name: R.new_counters() for name in C.crafted()}
    return {name: R.decode_file(data, counters[name])[0] for name, (data, W, H) in C.crafted().items()}, counters


def test_crafted_streams_are_judged_by_pil():
    got, counters = yardstick_crafted()
    for name, (data, W, H) in C.crafted().items():
        want = C.pil_rgba(data)[0]
        assert want.shape == (H, W, 4) and np.array_equal(got[name], want), name
    for W in (20, 3):
        assert counters[f"short-distances-w{W}"]["short_distance_codes"] == set(range(1, 121))
    assert {14, 15} <= counters["modes-14-15"]["modes"]
    assert all(counters[f"palette-overflow-n{n}"]["palette_overflow"] > 0 for n in (3, 5, 20))
    assert counters["length-prefixes"]["overlapping_copies"] > 20
    assert counters["cache-bits-1"]["cache_bits"] == {1} and counters["cache-bits-11"]["cache_bits"] == {11}
    assert counters["cache-bits-1"]["cache_hits"] > 0 and counters["cache-bits-11"]["cache_hits"] > 0
    assert counters["writer-rows1-0"]["one_symbol_normal_codes"] + counters["writer-rows1-0"]["simple_codes"] > 0


def test_yardstick_composition_equals_pil_on_every_rgba_byte():
    stats = {}
    for name, data in {**C.animations(), **C.pil_animations()}.items():
        got = np.stack(R.decode_file(data, stats=stats))
        assert np.array_equal(got, C.pil_rgba(data)), name
    assert len(C.animations()) == 40
    for need in ("key: first", "key: covers", "key: after a disposed key frame", "inside the disposed rectangle", "partial-alpha blends"):
        assert stats.get(need, 0) > 0, (need, stats)


# ---- the host parser ------------------------------------------------------------------------------------------------------------------------------------
def test_parse_webp_reads_every_accepted_layout():
    from mmgt_amd import video_in
    plain = C.stills()["photo-67x45-m0-q0"]
    h = video_in.parse_webp(plain)
    assert (h.width, h.height, h.animated, len(h.frames)) == (67, 45, False, 1) and h.frames[0].key and h.frames[0].payload == C.vp8l_of(plain)
    assert not h.frames[0].alpha_is_used
    alpha = C.vp8l_of(C.stills()["rgba-67x45-m0-q0"])                                   # VP8X, then VP8L
    body = b"WEBP" + E.chunk(b"VP8X", b"\x10\0\0\0" + E.u24(66) + E.u24(44)) + E.chunk(b"VP8L", alpha)
    extended = b"RIFF" + struct.pack("<I", len(body)) + body
    g = video_in.parse_webp(extended)
    assert (g.width, g.height, len(g.frames)) == (67, 45, 1) and g.frames[0].alpha_is_used and g.frames[0].payload == alpha
    assert np.array_equal(C.pil_rgba(extended), C.pil_rgba(C.stills()["rgba-67x45-m0-q0"]))
    b = io.BytesIO()                                                                    # VP8X, ICCP, VP8L, EXIF: the others are skipped
    Image.fromarray(C.kind_image("photo", 21, 9)).save(b, format="WEBP", lossless=True, icc_profile=b"x" * 31, exif=b"Exif\0\0" + b"y" * 9)
    chunks = [k for k, _ in E.parse_chunks(b.getvalue())]
    assert b"ICCP" in chunks and b"EXIF" in chunks
    assert video_in.parse_webp(b.getvalue()).frames[0].payload == C.vp8l_of(b.getvalue())
    odd = plain[:12] + E.chunk(b"unkn", b"abc") + plain[12:]                            # an unknown chunk of odd length, and bytes behind the RIFF size
    odd = odd[:4] + struct.pack("<I", len(odd) - 8) + odd[8:] + b"trailing"
    assert video_in.parse_webp(odd).frames[0].payload == C.vp8l_of(plain)
    a = C.animations()["random-3"]
    k = video_in.parse_webp(a)
    W, H, frames = R.file_frames(a)
    assert (k.width, k.height, k.animated, len(k.frames)) == (W, H, True, 5)
    for f, want in zip(k.frames, frames):
        assert (f.x, f.y, f.width, f.height, f.blend, f.dispose, f.payload, f.duration) == (
            want["x"], want["y"], want["w"], want["h"], want["blend"], want["dispose"], want["payload"], 40)
    own = E.webp_file(E.encode_frames(E.mask_frames(3, 19, 23), 5), 23, 19, 25, loop=3)  # the project's own writer
    o = video_in.parse_webp(own)
    assert (o.width, o.height, o.loop, len(o.frames)) == (23, 19, 3, 3) and all(f.key and not f.blend for f in o.frames)


def _refused():
    plain = C.stills()["photo-67x45-m0-q0"]
    payload = C.vp8l_of(plain)
    anim = C.animations()["random-3"]
    riff = lambda body: b"RIFF" + struct.pack("<I", len(body)) + body
    lossy = io.BytesIO()
    Image.fromarray(C.kind_image("photo", 21, 9)).save(lossy, format="WEBP", quality=80)
    lossy_alpha = io.BytesIO()
    Image.fromarray(C.kind_image("rgba", 21, 9)).save(lossy_alpha, format="WEBP", quality=80)
    sig, ver = bytearray(payload), bytearray(payload)
    sig[0], ver[4] = 0x2e, payload[4] | 0x20
    frame = lambda p, *a: C.animation_file(30, 22, [(p,) + a])
    small = C.vp8l_of(C.save(C.kind_image("photo", 8, 6)))
    vp8x = lambda w, h, flags=0: E.chunk(b"VP8X", bytes([flags, 0, 0, 0]) + E.u24(w - 1) + E.u24(h - 1))
    anim_ = E.chunk(b"ANIM", bytes(6))
    return {
        "not RIFF": (b"RIFX" + plain[4:], "not a RIFF/WEBP"),
        "not WEBP": (plain[:8] + b"WAVE" + plain[12:], "not a RIFF/WEBP"),
        "RIFF size": (plain[:4] + struct.pack("<I", len(plain)) + plain[8:], "RIFF size"),
        "truncated chunk": (riff(b"WEBP" + b"VP8L" + struct.pack("<I", len(payload) + 9) + payload), "runs past the end"),
        "lossy still": (lossy.getvalue(), r"lossy WebP \(VP8\) is not decoded"),
        "lossy with alpha": (lossy_alpha.getvalue(), r"lossy WebP \(VP8\) is not decoded"),
        "lossy frame": (riff(b"WEBP" + vp8x(8, 6, 2) + anim_ + E.chunk(b"ANMF", bytes(16) + E.chunk(b"VP8 ", b"abcd"))), r"lossy WebP \(VP8\) is not decoded"),
        "ALPH in a frame": (riff(b"WEBP" + vp8x(8, 6, 2) + anim_ + E.chunk(b"ANMF", bytes(16) + E.chunk(b"ALPH", b"ab") + E.chunk(b"VP8L", small))),
                            r"lossy WebP \(VP8\) is not decoded"),
        "frame without VP8L": (riff(b"WEBP" + vp8x(8, 6, 2) + anim_ + E.chunk(b"ANMF", bytes(16))), "has no VP8L chunk"),
        "frames without ANIM": (riff(b"WEBP" + vp8x(30, 22, 2) + C.anmf(small, 0, 0, 8, 6, True, False)), "before any ANIM"),
        "ANMF without the flag": (riff(b"WEBP" + vp8x(30, 22) + anim_ + C.anmf(small, 0, 0, 8, 6, True, False)), "animation flag"),
        "signature": (C.still_file(bytes(sig)), "bad VP8L signature"),
        "version": (C.still_file(bytes(ver)), "bad VP8L version"),
        "frame size": (frame(small, 0, 0, 9, 6, True, False), "differs from its ANMF size"),
        "rectangle": (frame(small, 24, 0, 8, 6, True, False), "leaves the canvas"),
        "still canvas": (riff(b"WEBP" + vp8x(67, 44) + E.chunk(b"VP8L", payload)), "differs from the still's VP8L size"),
        "canvas too large": (riff(b"WEBP" + vp8x(16385, 30, 2) + b"".join(E.chunk(k, b) for k, b in E.parse_chunks(anim)[1:])), "16384"),
        "no frames": (riff(b"WEBP" + vp8x(8, 6)), "no frames"),
        "short": (b"RIFF\4\0\0\0WEB", "not a RIFF/WEBP"),
    }


@pytest.mark.parametrize("name", sorted(_refused()))
def test_parse_webp_refuses_by_name(name):
    from mmgt_amd import video_in
    data, text = _refused()[name]
    with pytest.raises(ValueError, match=text):
        video_in.parse_webp(data)


def test_pil_reads_alike_whatever_parse_webp_accepts():
    """Seeded damage to the containers (not to the VP8L payloads): a file that parse_webp still accepts, PIL opens too, with the frames the yardstick
    composes from what parse_webp read."""
    from mmgt_amd import video_in
    rng = np.random.default_rng(77)
    sources = [C.stills()["photo-67x45-m0-q0"], C.stills()["rgba-67x45-m0-q0"], C.animations()["random-3"], C.animations()["random-8"]]
    accepted = refused = 0
    for trial in range(240):
        src = bytearray(sources[trial % 4])
        inside = set()                                                                  # bytes of VP8L payloads past their 5 header bytes
        pos = 0
        while (pos := bytes(src).find(b"VP8L", pos)) >= 0:
            ln = int.from_bytes(src[pos + 4:pos + 8], "little")
            inside |= set(range(pos + 13, pos + 8 + ln))
            pos += 4
        where = [i for i in range(len(src)) if i not in inside]
        if trial % 3 == 2:
            src = src[:where[int(rng.integers(12, len(where)))]]
        else:
            src[where[int(rng.integers(0, len(where)))]] ^= 1 << int(rng.integers(0, 8))
        data = bytes(src)
        try:
            h = video_in.parse_webp(data)
        except ValueError:
            refused += 1
            continue
        accepted += 1
        frames = [{"x": f.x, "y": f.y, "w": f.width, "h": f.height, "blend": f.blend, "dispose": f.dispose, "payload": f.payload} for f in h.frames]
        try:
            decoded = [R.decode_vp8l(f["payload"]) for f in frames]
        except R.Bad:
            continue                                                                    # the damage reached a payload's size: the kernels' status, not the parser's
        stats = {}
        want = np.stack(R.compose(h.width, h.height, frames, decoded, stats))
        assert [f.key for f in h.frames] == stats["keys"], trial
        assert np.array_equal(C.pil_rgba(data)[..., :3], want[..., :3]), trial
    assert accepted >= 30 and refused >= 30, (accepted, refused)


# ---- the host program -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/webpdec_host_check.cpp with"
    exe = tmp_path_factory.mktemp("webpdec_host") / "webpdec_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "webpdec_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def run_host(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True)


def host_decode(exe, tmp_path, files, mode="decode"):
    from mmgt_amd import video_in
    headers = [video_in.parse_webp(f) for f in files]
    tab, chunk = C.write_job(tmp_path / "job.bin", headers)
    r = run_host(exe, mode, str(tmp_path / "job.bin"), str(tmp_path / "out.bin"))
    assert r.returncode == 0, r.stderr[-4000:]
    if mode == "decode":
        return np.fromfile(tmp_path / "out.bin", np.uint8).reshape(len(tab), headers[0].height, headers[0].width, 3)
    return tab, np.fromfile(tmp_path / "out.bin", np.uint32)


def _by_canvas(files):
    groups = {}
    for name, data in files.items():
        h = parse_webp(data)
        groups.setdefault((h.width, h.height), []).append(name)
    return groups


def test_host_program_equals_pil_on_every_still(host_check, tmp_path):
    files = {**C.stills(), **{k: v[0] for k, v in C.crafted().items()}}
    for (W, H), names in _by_canvas(files).items():
        got = host_decode(host_check, tmp_path, [files[n] for n in names])
        for k, n in enumerate(names):
            assert np.array_equal(got[k], C.pil_rgb(files[n])[0]), n


def test_host_program_equals_pil_on_every_animation(host_check, tmp_path):
    files = {**C.animations(), **C.pil_animations()}
    for (W, H), names in _by_canvas(files).items():
        got = host_decode(host_check, tmp_path, [files[n] for n in names])                # several files in one set: composition starts anew at each
        want = np.concatenate([C.pil_rgb(files[n]) for n in names])
        assert got.shape == want.shape and np.array_equal(got, want), (W, H)


STAGED = ("photo-67x45-m4-q50", "palette3-67x45-m6-q100", "palette12-67x45-m2-q50", "rgba-67x45-m6-q0", "mask-67x45-m4-q100", "noise-67x45-m0-q0")


def test_host_program_equals_the_yardstick_stage_by_stage(host_check, tmp_path):
    files = [C.stills()[n] for n in STAGED]
    refs = [R.decode_vp8l(C.vp8l_of(f)) for f in files]
    tab, scr = host_decode(host_check, tmp_path, files, "scratch")
    for t, ref, name in zip(tab, refs, STAGED):
        hdr = scr[t[6]:t[6] + 32]
        assert hdr[0] == 0x57443031 and hdr[1] == len(ref["transforms"]) and hdr[3] == ref["main"].shape[1], name
        assert np.array_equal(scr[t[6] + hdr[2]:t[6] + hdr[2] + ref["main"].size], ref["main"].reshape(-1)), name
        for k, (kind, bits, sub, w, n) in enumerate(ref["transforms"]):
            e = hdr[4 + 5 * k:9 + 5 * k]
            assert (e[0], e[1], e[3], e[4]) == (kind, bits, w, n), name
            assert np.array_equal(scr[t[6] + e[2]:t[6] + e[2] + len(sub)], np.asarray(sub, np.uint32)), name
    tab, argb = host_decode(host_check, tmp_path, files, "argb")
    for t, ref, name in zip(tab, refs, STAGED):
        assert np.array_equal(argb[t[8]:t[8] + ref["argb"].size], ref["argb"].reshape(-1)), name
    assert len({tuple(u[0] for u in r["transforms"]) for r in refs}) >= 3                # the frames of the set differ in their transforms


def test_host_program_decodes_more_groups_than_the_first_allowance_holds(host_check, tmp_path):
    """A frame's number of prefix-code groups is known only after its entropy image: the first run ends with minus the scratch words the frame
    needs as its status, the second, given them, with PIL's pixels."""
    from mmgt_amd import hip, video_in
    data = C.many_groups()
    groups = R.count_groups(C.vp8l_of(data))
    assert groups > 71 and groups * hip.WEBPDEC_GROUP_WORDS * 4 > video_in.WEBPDEC_GROUP_BYTES
    h = video_in.parse_webp(data)
    tab, _ = C.write_job(tmp_path / "job.bin", [h])
    r = run_host(host_check, "decode", str(tmp_path / "job.bin"), str(tmp_path / "out.bin"))
    assert r.returncode == 3 and "status -" in r.stderr, r.stderr[-500:]
    need = -int(r.stderr.split("status ")[1].split()[0])
    assert need > tab[0, 7] and need - groups * hip.WEBPDEC_GROUP_WORDS < tab[0, 7]
    tab, _ = C.write_job(tmp_path / "job.bin", [h], caps={0: need})
    assert tab[0, 7] == need
    r = run_host(host_check, "decode", str(tmp_path / "job.bin"), str(tmp_path / "out.bin"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", np.uint8).reshape(1, 480, 640, 3), C.pil_rgb(data))


def test_host_program_reports_statuses(host_check, tmp_path):
    from mmgt_amd import video_in
    for name, (data, code) in C.corrupt().items():
        C.write_job(tmp_path / "job.bin", [video_in.parse_webp(d) for d in data])
        r = run_host(host_check, "decode", str(tmp_path / "job.bin"), str(tmp_path / "out.bin"))
        assert r.returncode == 3 and f"status {code} in frame 1 (decode)" in r.stderr, (name, r.stderr[-500:])


FUZZ = {"stills": lambda: [C.stills()[n] for n in STAGED],
        "crafted": lambda: [C.crafted()[n][0] for n in ("cache-bits-11", "cache-bits-1")],
        "animation": lambda: [C.animations()["random-3"], C.animations()["random-8"]],
        "mixed": lambda: [C.stills()[f"mixed-200x135-m{m}-q100"] for m in (0, 6)]}


@pytest.mark.parametrize("name", sorted(FUZZ))
def test_host_program_survives_corruptions(host_check, tmp_path, name):
    """600 seeded corruptions per set, 2400 in all (byte flips, shortened payloads, overwritten runs, falsified code lengths and headers, table rows
    that lie): every run ends in pixels or a status within the step bound -- 131 loop iterations per payload bit, one per scratch word (every
    pixel of the main image and of the sub-images is one) and 16; ASan / UBSan end the program otherwise."""
    from mmgt_amd import video_in
    C.write_job(tmp_path / "job.bin", [video_in.parse_webp(d) for d in FUZZ[name]()])
    r = run_host(host_check, "fuzz", str(tmp_path / "job.bin"), "600", "20261019")
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-4000:]}"
    w = r.stdout.split()
    runs, pixels, status = int(w[1]), int(w[3]), int(w[7])
    assert runs == 600 and pixels + status == runs and status >= 150, r.stdout
