"""Lossy WebP (VP8 key frame) decode on the device (csrc/vp8dec.hip through the C ABI, mmgt_amd.video_in with lossy=True) against PIL's
ImageSequence.Iterator + convert("RGB") on every byte; each of the four launches alone against the yardstick tests/vp8dec_ref.py, so that a failure
names its stage.  Every comparison is bitwise.  What is malformed here is a short fixed list that the host program has already ended with a status
under ASan and UBSan (tests/test_vp8dec.py, tools/vp8dec_host_check.cpp)."""
import argparse
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
from PIL import Image

from mmgt_amd import decode_webp_frames, parse_webp
from tests import vp8_ref as E
from tests import vp8dec_cases as C
from tests import vp8dec_ref as R
from tests.test_vp8dec import STAGED, _frame_views, all_stills, corruptions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LOSSLESS = ("mmgt_webp_decode", "mmgt_webp_untransform")
LOSSY = ("mmgt_vp8dec_parse", "mmgt_vp8dec_reconstruct", "mmgt_vp8dec_filter", "mmgt_vp8dec_output")
ENTRIES = LOSSLESS + LOSSY + ("mmgt_webp_compose",)


def decode(files, **kw):
    out = decode_webp_frames(files, DEV, lossy=True, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    return out


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counts():
    from mmgt_amd import hip
    return {k: hip.call_count(k) for k in ENTRIES}


def delta(before):
    now = counts()
    return {k: now[k] - before[k] for k in ENTRIES}


def by_canvas(files):
    groups = {}
    for name, data in files.items():
        h = parse_webp(data, lossy=True)
        groups.setdefault((h.width, h.height), []).append(name)
    return groups


# ---- every byte against PIL -------------------------------------------------------------------------------------------------------------------------------
def test_a_lossy_still_decodes_to_pils_bytes():
    """Fails on the parent commit: there the keyword does not exist and the file is refused."""
    data = C.stills()["photo-80x48-q75-m4"]
    got = decode_webp_frames(data, DEV, lossy=True)
    assert tuple(got.shape) == (1, 48, 80, 3) and np.array_equal(got.cpu().numpy(), C.pil_rgb(data))


def test_device_equals_pil_on_every_still_and_crafted_stream():
    """One call per size class: the 80 x 48 call holds the 25 PIL settings, the 48 x 48 call every crafted stream (simple and normal filter,
    segments, deltas, 4 x 4 modes on every border, 1 .. 8 partitions)."""
    files = all_stills()
    sizes = by_canvas(files)
    assert len(sizes[(80, 48)]) == 25 and len(sizes[(48, 48)]) >= 37
    for (W, H), names in sizes.items():
        got = decode([files[n] for n in names]).cpu().numpy()
        assert got.shape[0] == len(names)
        for k, n in enumerate(names):
            assert np.array_equal(got[k], C.pil_rgb(files[n])[0]), n


def test_device_equals_pil_on_every_animation_in_one_call():
    files = C.animations()
    names = sorted(files)
    assert {parse_webp(files[n], lossy=True).width for n in names} == {80}
    before = counts()
    got = decode([files[n] for n in names]).cpu().numpy()                                   # 13 files, VP8 and VP8L frames, sub-rectangles, disposal
    want = np.concatenate([C.pil_rgb(files[n]) for n in names])
    assert got.shape == want.shape and np.array_equal(got, want)
    assert set(delta(before).values()) == {1}                                               # one set of launches, both kinds of frame in it


# ---- the launches one by one ------------------------------------------------------------------------------------------------------------------------------
def test_each_launch_alone_equals_the_yardstick_into_filled_buffers_with_guards():
    from mmgt_amd import hip, video_in
    files = [all_stills()[n] for n in STAGED if parse_webp(all_stills()[n], lossy=True).width == 48] + [all_stills()["bmodes-7"]]
    refs = [R.decode_vp8(C.vp8_of(f)) for f in files]
    assert len(files) >= 4
    headers = [parse_webp(f, lossy=True) for f in files]
    tab, ltab, vtab, lidx, vidx, data, chunks = video_in.webp_operands_lossy(headers)
    (_, _, _, _, _, _, scr_words, argb_words), = chunks
    guard = 64
    fill = lambda n: torch.full((n + 2 * guard,), -0x5A5A5A5B, dtype=torch.int32, device=DEV)        # 0xA5A5A5A5
    scratch, argb = fill(scr_words), fill(argb_words)
    d_tab, d_data = up(vtab), up(data.copy())
    for run in range(2):                                                                   # the second run goes into the dirty buffers
        view = lambda: scratch.cpu().numpy().view(np.uint32)
        assert not hip.vp8dec_parse(d_data, d_tab, scratch[guard:guard + scr_words]).any()
        scr = view()
        assert (scr[:guard] == 0xA5A5A5A5).all() and (scr[-guard:] == 0xA5A5A5A5).all()
        for t, ref in zip(vtab, refs):
            hdr, mb, coef, _ = _frame_views(scr[guard:], t)
            h = ref["header"]
            assert hdr[0] == 0x56384431 and (hdr[3], hdr[4]) == (h["filter_type"], h["parts"])
            for my, row in enumerate(ref["mbs"]):
                for mx, m in enumerate(row):
                    assert list(mb[my, mx][:16]) == list(m["modes"]) and mb[my, mx][30] == int(ref["inner"][my][mx])
                    if not (h["use_skip"] and m["skip"]):
                        assert np.array_equal(coef[my, mx], ref["coeffs"][my, mx])
        for launch, key in ((hip.vp8dec_reconstruct, "unfiltered"), (hip.vp8dec_filter, "filtered")):
            assert not launch(d_tab, scratch[guard:guard + scr_words]).any()
            scr = view()
            assert (scr[:guard] == 0xA5A5A5A5).all() and (scr[-guard:] == 0xA5A5A5A5).all()
            for t, ref in zip(vtab, refs):
                assert all(np.array_equal(a, b) for a, b in zip(_frame_views(scr[guard:], t)[3], ref[key])), key
        assert not hip.vp8dec_output(d_tab, scratch[guard:guard + scr_words], argb[guard:guard + argb_words], 48 * 48).any()
        words = argb.cpu().numpy().view(np.uint32)
        assert (words[:guard] == 0xA5A5A5A5).all() and (words[-guard:] == 0xA5A5A5A5).all()
        for t, ref in zip(vtab, refs):
            r = ref["rgb"].astype(np.uint32)
            assert np.array_equal(words[guard + t[4]:guard + t[4] + 48 * 48].reshape(48, 48), 0xFF000000 | r[..., 0] << 16 | r[..., 1] << 8 | r[..., 2])


def test_limit_and_one_frame_per_set_of_launches_carry_the_canvas(monkeypatch):
    from mmgt_amd import video_in
    files = [C.animations()[n] for n in ("hand-1", "tiles-mixed", "hand-2")]
    assert any(f.dispose for f in parse_webp(files[0], lossy=True).frames)
    want = np.concatenate([C.pil_rgb(f) for f in files])
    before = counts()
    part = decode(files, limit=7).cpu().numpy()                                             # the first file and two frames of the second
    assert part.shape[0] == 7 and np.array_equal(part, want[:7])
    assert set(delta(before).values()) == {1}
    monkeypatch.setattr(video_in, "WEBPDEC_SCRATCH_BYTES", 64)                              # one frame per set of launches: disposal crosses them
    before = counts()
    assert np.array_equal(decode(files).cpu().numpy(), want)
    d = delta(before)
    assert d["mmgt_webp_compose"] == want.shape[0] == 16 and all(d[k] == 13 for k in LOSSY) and all(d[k] == 3 for k in LOSSLESS)
    bad = [C.own_streams()["own-33x47-p4-f0"], E.webp_file([corruptions()["token partition ends"][0]], 33, 47)]
    assert np.array_equal(decode(bad, limit=1).cpu().numpy(), C.pil_rgb(bad[0]))            # a limit keeps a corrupt later frame out of the launches


# ---- the way back in of the project's own output ----------------------------------------------------------------------------------------------------------
def test_the_device_lossy_writer_round_trips(tmp_path):
    from mmgt_amd import video_in, video_out
    frames = np.stack([C.kind_image(("photo", "smooth", "noise", "half")[k % 4], 64, 64, seed=k) for k in range(8)])
    video_out.save_videos_grid(torch.from_numpy(frames)[None], str(tmp_path / "clip.webp"), n_rows=1, fps=8, webp_quality=75)
    data = (tmp_path / "clip.webp").read_bytes()
    assert set(C.chunk_kinds(data)) == {b"VP8 "}
    got = video_in.read_frames_device(tmp_path / "clip.webp", None, DEV, webp_lossy=True)
    assert np.array_equal(got.cpu().numpy(), C.pil_rgb(data)) and got.shape[0] == 8
    assert tuple(video_in.read_frames_device(tmp_path / "clip.webp", 2, DEV, webp_lossy=True).shape) == (2, 64, 64, 3)
    with pytest.raises(ValueError, match="lossy WebP"):
        video_in.read_frames_device(tmp_path / "clip.webp", None, DEV)                      # without the option: as before


def _write_inputs(tmp_path, n, H, W):
    """pose.webp (an animated lossy clip), face/ (a directory mixing lossy and lossless grey stills), lips.webp and hands.webp (lossy clips of noise on
    grey, which PIL codes without ALPH), ref.webp (a lossy still)."""
    C_save = lambda path, arr, **kw: (lambda ims: ims[0].save(path, format="WEBP", save_all=True, append_images=ims[1:], duration=40, **kw))(
        [Image.fromarray(a) for a in arr])
    C_save(tmp_path / "pose.webp", C.clip_frames("static", n, W, H), quality=75)
    (tmp_path / "face").mkdir()
    rng = np.random.default_rng(9)
    for k in range(n):
        m = np.clip(rng.normal(128, 40, (H, W)), 0, 255).astype(np.uint8)
        Image.fromarray(m).save(tmp_path / "face" / f"{k:03d}.webp", **(dict(lossless=True) if k % 2 else dict(quality=70)))
    for name in ("lips.webp", "hands.webp"):
        C_save(tmp_path / name, [np.repeat(np.clip(rng.normal(100, 50, (H, W, 1)), 0, 255).astype(np.uint8), 3, -1) for _ in range(n)], quality=75)
    Image.fromarray(C.kind_image("photo", 48, 40)).save(tmp_path / "ref.webp", quality=80)
    for name in ("pose.webp", "lips.webp", "hands.webp", "ref.webp"):
        assert b"ALPH" not in C.chunk_kinds((tmp_path / name).read_bytes()) and b"VP8 " in C.chunk_kinds((tmp_path / name).read_bytes())


def test_read_frames_device_on_a_file_a_directory_and_a_mixed_directory(tmp_path):
    from mmgt_amd import inputs, video_in
    _write_inputs(tmp_path, 6, 48, 64)
    for name in ("pose.webp", "face", "lips.webp"):
        got = video_in.read_frames_device(tmp_path / name, None, DEV, webp_lossy=True)
        want = np.stack([np.asarray(f.convert("RGB")) for f in inputs.read_frames(tmp_path / name)])
        assert np.array_equal(got.cpu().numpy(), want), name
    kinds = [C.chunk_kinds(f.read_bytes())[0] for f in sorted((tmp_path / "face").iterdir())]
    assert set(kinds) == {b"VP8 ", b"VP8L"}                                                  # the directory mixes lossy and lossless files
    assert tuple(video_in.read_frames_device(tmp_path / "face", 4, DEV, webp_lossy=True).shape) == (4, 48, 64, 3)
    with pytest.raises(ValueError, match="lossy WebP"):
        video_in.read_frames_device(tmp_path / "face", None, DEV)


def test_pose2vid_input_section_with_and_without_decode_lossy_webp(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("pose2vid_script_vp8", os.path.join(ROOT, "scripts", "pose2vid.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    _write_inputs(tmp_path, 8, 64, 64)
    a = argparse.Namespace(pose_path=str(tmp_path / "pose.webp"), face_mask_path=str(tmp_path / "face"), lips_mask_path=str(tmp_path / "lips.webp"),
                           hands_mask_path=str(tmp_path / "hands.webp"), image_path=str(tmp_path / "ref.webp"), L=8, W=64, H=64, decoder="device",
                           decode_lossy_webp=True)
    dev = torch.device(DEV)
    before = counts()
    pose_d, full_d, face_d, lips_d, L = script.load_inputs(a, dev)
    ref_d = script.load_ref_image(a, dev)
    d = delta(before)
    assert d["mmgt_webp_compose"] == 5 and all(d[k] == 5 for k in LOSSY) and all(d[k] == 1 for k in LOSSLESS)   # three files, a mixed directory, the image
    assert "decoded on the host" not in capsys.readouterr().out
    a.decoder = "pil"
    pose_h, full_h, face_h, lips_h, _ = script.load_inputs(a, dev)
    ref_h = script.load_ref_image(a, dev)
    assert delta(before) == d                                                               # --decoder pil launches none of them
    assert L == 8 and torch.equal(pose_d.cpu(), pose_h) and len(full_d) == 4 and full_d[0].std() > 0
    for x, y in zip(full_d + face_d + lips_d, full_h + face_h + lips_h):
        assert torch.equal(x, y)
    assert ref_d.is_cuda and np.array_equal(ref_d.cpu().numpy(), np.asarray(ref_h))
    # without the option: the host decodes the image and says so, as before
    a.decoder, a.decode_lossy_webp = "device", False
    lossy = script.load_ref_image(a, dev)
    assert "decoded on the host (parse_webp: lossy WebP (VP8) is not decoded" in capsys.readouterr().out
    assert np.array_equal(lossy.cpu().numpy(), np.asarray(ref_h)) and delta(before) == d
    # with it, an image with an alpha plane still goes through the host, and the note names ALPH
    Image.fromarray(np.dstack([C.kind_image("photo", 48, 40), np.full((40, 48), 128, np.uint8)])).save(tmp_path / "alpha.webp", quality=80)
    a.decode_lossy_webp, a.image_path = True, str(tmp_path / "alpha.webp")
    script.load_ref_image(a, dev)
    assert "decoded on the host (parse_webp: an ALPH chunk" in capsys.readouterr().out and delta(before) == d


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_out_of_scope_input_raises_before_any_launch():
    from tests.test_vp8dec import _refused
    good = C.stills()["photo-80x48-q75-m4"]
    decode([good])                                                                          # the library is loaded and has run
    before = counts()
    assert before["mmgt_vp8dec_parse"] >= 1
    for word, bad in _refused().items():
        with pytest.raises(ValueError, match=word):
            decode([good, bad])
    with pytest.raises(ValueError, match="one call decodes one canvas size"):
        decode([good, C.stills()["photo-16x17-q75-m4"]])
    with pytest.raises(ValueError, match="lossy WebP"):
        decode_webp_frames([good], DEV)
    assert before == counts()


@pytest.mark.parametrize("name", sorted(corruptions()))
def test_a_stream_that_does_not_decode_raises_naming_the_frame(name):
    from mmgt_amd import video_in
    payload, code = corruptions()[name]
    files = [C.own_streams()["own-33x47-p4-f0"], E.webp_file([payload], 33, 47)]
    with pytest.raises(RuntimeError, match=f"frame 1, VP8 parse: {video_in.VP8_STATUS_TEXT[code][:30]}"):
        decode(files)


def test_the_c_entries_refuse_out_of_range_arguments():
    from mmgt_amd import hip
    L = hip.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    tab = torch.zeros((2, 8), dtype=torch.int64, device=DEV)
    words = torch.zeros(8192, dtype=torch.int32, device=DEV)
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    calls = [
        (L.mmgt_vp8dec_parse, (p(buf), 4096, p(tab), p(words), 2048, p(st), 0, s)),
        (L.mmgt_vp8dec_parse, (p(buf), 4095, p(tab), p(words), 2048, p(st), 1, s)),
        (L.mmgt_vp8dec_parse, (p(buf), 4096, p(tab), p(words), 63, p(st), 1, s)),
        (L.mmgt_vp8dec_parse, (p(buf), 4096, p(tab), p(words), 2048, p(st), 65536, s)),
        (L.mmgt_vp8dec_parse, (p(buf), 2048, p(tab), p(words[1:]), 2048, p(st), 1, s)),
        (L.mmgt_vp8dec_reconstruct, (p(tab), p(words), 2048, p(st), 0, s)),
        (L.mmgt_vp8dec_reconstruct, (p(tab), p(words), 63, p(st), 1, s)),
        (L.mmgt_vp8dec_filter, (p(tab), p(words), 2048, p(st), 65536, s)),
        (L.mmgt_vp8dec_filter, (p(tab), p(words[1:]), 2048, p(st), 1, s)),
        (L.mmgt_vp8dec_output, (p(tab), p(words), 2048, p(words[4096:]), 2048, p(st), 0, 16, s)),
        (L.mmgt_vp8dec_output, (p(tab), p(words), 2048, p(words[4096:]), 0, p(st), 1, 16, s)),
        (L.mmgt_vp8dec_output, (p(tab), p(words), 2048, p(words[4096:]), 2048, p(st), 1, 0, s)),
        (L.mmgt_vp8dec_output, (p(tab), p(words), 2048, p(words[4096:]), 2048, p(st), 1, 16383 * 16383 + 1, s)),
    ]
    for k, (fn, args) in enumerate(calls):
        assert fn(*args) != 0 and "range" in L.mmgt_last_error().decode(), k
    assert L.mmgt_vp8dec_parse(None, 4096, p(tab), p(words), 2048, p(st), 1, s) != 0
    torch.cuda.synchronize()
    assert not bool(buf.any()) and not bool(words.any()) and not bool(st.any())             # nothing was launched
    # rows that name bytes or words outside the buffers, or sizes outside 1 .. 16383: status 1 from every launch, nothing touched
    rows = np.zeros((4, 8), np.int64)
    rows[0, :7] = (0, 64, 0, 4096, 0, 16, 16)                                               # more scratch words than there are
    rows[1, :7] = (0, 8192, 0, 360, 0, 16, 16)                                              # a payload past the data
    rows[2, :7] = (0, 64, 0, 359, 0, 16, 16)                                                # fewer scratch words than a 16 x 16 frame needs
    rows[3, :7] = (0, 64, 0, 2048, 0, 16384, 1)                                             # a side above 16383
    d_rows = up(rows)
    assert hip.vp8dec_parse(buf, d_rows, words[:2048]).cpu().tolist() == [1, 1, 1, 1]
    assert hip.vp8dec_reconstruct(d_rows, words[:2048]).cpu().tolist() == [1, 7, 1, 1]      # row 1 is in range here, but was never parsed
    assert hip.vp8dec_filter(d_rows, words[:2048]).cpu().tolist() == [1, 7, 1, 1]
    rows[1, 1], rows[1, 4] = 64, 2048 - 255                                                 # a good row but for its ARGB words, which leave the buffer
    assert hip.vp8dec_output(up(rows), words[:2048], words[4096:4096 + 2048], 256).cpu().tolist() == [1, 1, 1, 1]
    assert not bool(words.any())
    rows[1, 4] = 0                                                                          # now in range, but never parsed: status 7, nothing written
    assert hip.vp8dec_output(up(rows), words[:2048], words[4096:4096 + 2048], 256).cpu().tolist() == [1, 7, 1, 1]
    assert not bool(words.any())
