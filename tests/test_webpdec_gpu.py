"""WebP lossless / animated WebP decode on the device (csrc/webpdec.hip through the C ABI, mmgt_amd.video_in) against PIL's
ImageSequence.Iterator + convert("RGB") on every byte; the entropy-decode launch alone and the untransform launch alone against the yardstick
tests/webpdec_ref.py, so that a failure names its stage.  Every comparison is bitwise.  What is malformed here is a short fixed list that the host
program has already ended with a status (tests/test_webpdec.py, tools/webpdec_host_check.cpp)."""
import argparse
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
from PIL import Image

from mmgt_amd import decode_webp_frames, parse_webp
from tests import webp_ref as E
from tests import webpdec_cases as C
from tests import webpdec_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ENTRIES = ("mmgt_webp_decode", "mmgt_webp_untransform", "mmgt_webp_compose")
STAGED = ("photo-67x45-m4-q50", "palette3-67x45-m6-q100", "palette12-67x45-m2-q50", "rgba-67x45-m6-q0", "mask-67x45-m4-q100", "noise-67x45-m0-q0")


def decode(files, **kw):
    out = decode_webp_frames(files, DEV, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    return out


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def by_canvas(files):
    groups = {}
    for name, data in files.items():
        h = parse_webp(data)
        groups.setdefault((h.width, h.height), []).append(name)
    return groups


# ---- every byte against PIL -------------------------------------------------------------------------------------------------------------------------------
def test_device_equals_pil_on_every_still():
    """All PIL-written stills and all crafted streams, one call per canvas size: the 67 x 45 call holds 120 frames that differ in their transforms,
    colour caches and numbers of prefix-code groups."""
    files = {**C.stills(), **{k: v[0] for k, v in C.crafted().items()}}
    sizes = by_canvas(files)
    assert len(sizes[(67, 45)]) == 120
    for (W, H), names in sizes.items():
        names = (names * 3)[:max(3, len(names))]                                             # three frames a call at the least
        got = decode([files[n] for n in names]).cpu().numpy()
        assert got.shape[0] == len(names) >= 3
        for k, n in enumerate(names):
            assert np.array_equal(got[k], C.pil_rgb(files[n])[0]), n


def test_more_groups_than_the_first_allowance_holds_are_decoded_in_a_second_run(monkeypatch):
    from mmgt_amd import hip, video_in
    data = C.many_groups()                                                                  # 89 groups, PIL's method 4
    assert R.count_groups(C.vp8l_of(data)) > 71
    before = {k: hip.call_count(k) for k in ENTRIES}
    assert np.array_equal(decode([data]).cpu().numpy(), C.pil_rgb(data))
    assert all(hip.call_count(k) - before[k] == 2 for k in ENTRIES)
    files = [C.stills()["photo-160x120-m4-q75"], C.save(C.kind_image("photo", 160, 120), method=0), C.stills()["photo-160x120-m4-q75"]]
    want = np.concatenate([C.pil_rgb(f) for f in files])
    monkeypatch.setattr(video_in, "WEBPDEC_GROUP_BYTES", 2 * 4 * hip.WEBPDEC_GROUP_WORDS)   # room for two groups: frames 0 and 2 have eight
    before = {k: hip.call_count(k) for k in ENTRIES}
    assert np.array_equal(decode(files).cpu().numpy(), want)
    assert all(hip.call_count(k) - before[k] == 2 for k in ENTRIES)


def test_device_equals_pil_on_every_animation():
    files = {**C.animations(), **C.pil_animations()}
    for (W, H), names in by_canvas(files).items():
        got = decode([files[n] for n in names]).cpu().numpy()                               # 40 files in one call: composition starts anew at each
        want = np.concatenate([C.pil_rgb(files[n]) for n in names])
        assert got.shape == want.shape and want.shape[0] >= 3 and np.array_equal(got, want), (W, H)


# ---- the launches one by one ------------------------------------------------------------------------------------------------------------------------------
def _operands(files, **kw):
    from mmgt_amd import video_in
    headers = [parse_webp(f) for f in files]
    tab, data, chunks = video_in.webp_operands(headers, **kw)
    return headers, tab, data, chunks


def test_each_launch_alone_equals_the_yardstick_into_filled_buffers_with_guards():
    from mmgt_amd import hip
    files = [C.stills()[n] for n in STAGED]
    refs = [R.decode_vp8l(C.vp8l_of(f)) for f in files]
    assert len({tuple(u[0] for u in r["transforms"]) for r in refs}) >= 3                    # the frames of the call differ in their transforms
    headers, tab, data, chunks = _operands(files)
    (f0, f1, scr_words, argb_words), = chunks
    guard = 64
    fill = lambda n: torch.full((n + 2 * guard,), -0x5A5A5A5B, dtype=torch.int32, device=DEV)        # 0xA5A5A5A5
    scratch, argb = fill(scr_words), fill(argb_words)
    d_tab, d_data = up(tab), up(data.copy())
    status = hip.webp_decode(d_data, d_tab, scratch[guard:guard + scr_words])
    assert not status.any()
    scr = scratch.cpu().numpy().view(np.uint32)
    assert (scr[:guard] == 0xA5A5A5A5).all() and (scr[-guard:] == 0xA5A5A5A5).all()
    for t, ref, name in zip(tab, refs, STAGED):
        base = guard + t[6]
        hdr = scr[base:base + 32]
        assert hdr[0] == 0x57443031 and hdr[1] == len(ref["transforms"]) and hdr[3] == ref["main"].shape[1], name
        assert np.array_equal(scr[base + hdr[2]:base + hdr[2] + ref["main"].size], ref["main"].reshape(-1)), name
        for k, (kind, bits, sub, w, n) in enumerate(ref["transforms"]):
            e = hdr[4 + 5 * k:9 + 5 * k]
            assert (e[0], e[1], e[3], e[4]) == (kind, bits, w, n), name
            assert np.array_equal(scr[base + e[2]:base + e[2] + len(sub)], np.asarray(sub, np.uint32)), name
    _, status = hip.webp_untransform(d_tab, scratch[guard:guard + scr_words], out=(argb[guard:guard + argb_words], None))
    assert not status.any()
    words = argb.cpu().numpy().view(np.uint32)
    assert (words[:guard] == 0xA5A5A5A5).all() and (words[-guard:] == 0xA5A5A5A5).all()
    for t, ref, name in zip(tab, refs, STAGED):
        assert np.array_equal(words[guard + t[8]:guard + t[8] + ref["argb"].size], ref["argb"].reshape(-1)), name
    out = torch.full((len(files) + 2, 45, 67, 3), 0xA5, dtype=torch.uint8, device=DEV)
    carry = torch.full((45, 67), -0x5A5A5A5B, dtype=torch.int32, device=DEV)
    hip.webp_compose(d_tab, argb[guard:guard + argb_words], carry, 45, 67, out=out[1:-1])
    got = out.cpu().numpy()
    assert (got[0] == 0xA5).all() and (got[-1] == 0xA5).all()
    assert np.array_equal(got[1:-1], np.stack([C.pil_rgb(f)[0] for f in files]))
    # a second run into the same, now dirty, buffers gives the same bytes
    assert np.array_equal(decode(files, out=out[1:-1]).cpu().numpy(), got[1:-1])


def test_limit_and_one_frame_per_set_of_launches_carry_the_canvas(monkeypatch):
    from mmgt_amd import hip, video_in
    def crosses(data):                                                                      # a blended frame that is no key frame, after a disposed one
        f = parse_webp(data).frames
        return any(f[k - 1].dispose and f[k].blend and not f[k].key and f[k].alpha_is_used for k in range(1, len(f)))
    names = [n for n in sorted(C.animations()) if crosses(C.animations()[n])][:3]
    assert len(names) == 3
    files = [C.animations()[n] for n in names]
    want = np.concatenate([C.pil_rgb(f) for f in files])
    whole = decode(files).cpu().numpy()
    assert np.array_equal(whole, want)
    before = {k: hip.call_count(k) for k in ENTRIES}
    part = decode(files, limit=7).cpu().numpy()                                             # the first file and two frames of the second
    assert part.shape[0] == 7 and np.array_equal(part, want[:7])
    assert all(hip.call_count(k) - before[k] == 1 for k in ENTRIES)
    monkeypatch.setattr(video_in, "WEBPDEC_SCRATCH_BYTES", 64)                              # one frame per set of launches: blend and dispose cross them
    before = {k: hip.call_count(k) for k in ENTRIES}
    assert np.array_equal(decode(files).cpu().numpy(), want)
    assert all(hip.call_count(k) - before[k] == want.shape[0] == 15 for k in ENTRIES)
    bad = C.corrupt()["truncated"][0]                                                       # a limit keeps a corrupt later frame out of the launches
    assert np.array_equal(decode(bad, limit=1).cpu().numpy(), C.pil_rgb(bad[0]))


# ---- the way back in of the project's own output ----------------------------------------------------------------------------------------------------------
def test_the_device_webp_writer_round_trips(tmp_path):
    import mmgt_amd
    from mmgt_amd import video_in, video_out
    frames = np.concatenate([E.mask_frames(3, 40, 56), np.random.default_rng(4).integers(0, 256, (2, 40, 56, 3)).astype(np.uint8)])
    videos = torch.from_numpy(frames)[None]
    video_out.save_videos_grid(videos, str(tmp_path / "clip.webp"), n_rows=1, fps=8)
    sent = video_out.frames_uint8(videos, 1)
    got = mmgt_amd.read_frames_device(tmp_path / "clip.webp", None, DEV)
    assert np.array_equal(got.cpu().numpy(), sent) and np.array_equal(sent, C.pil_rgb((tmp_path / "clip.webp").read_bytes()))
    assert tuple(video_in.read_frames_device(tmp_path / "clip.webp", 2, DEV).shape) == (2,) + sent.shape[1:]
    with pytest.raises(RuntimeError, match="no frames"):
        video_in.read_frames_device(tmp_path / "clip.webp", 0, DEV)
    blobs = video_out.encode_webp_frames(torch.from_numpy(frames).to(DEV), strip_rows=7)
    video_out.write_webp(str(tmp_path / "still.webp"), blobs[:1], 56, 40, 8)
    assert np.array_equal(video_in.read_frames_device(tmp_path / "still.webp", None, DEV).cpu().numpy(), frames[:1])
    video_out.write_webp(str(tmp_path / "strips.webp"), blobs, 56, 40, 8, loop=2)
    assert np.array_equal(video_in.read_frames_device(tmp_path / "strips.webp", None, DEV).cpu().numpy(), frames)


def _mask_clip(n, H, W, seed):
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        cx, cy = W * (0.3 + 0.05 * k) + seed, H * 0.5 - seed
        out[k][(xx - cx) ** 2 + (yy - cy) ** 2 < (H / (4 + seed)) ** 2] = 255
    return out


def _save_clip(path, arr):
    ims = [Image.fromarray(a) for a in arr]
    ims[0].save(path, format="WEBP", save_all=True, append_images=ims[1:], lossless=True, duration=40)


def _write_inputs(tmp_path, n, H, W):
    """pose.webp (an animated RGB clip), face/ (a directory of grey stills), lips.webp and hands.webp (animated grey clips), ref.webp."""
    _save_clip(tmp_path / "pose.webp", C.shapes_clip(n, W, H))
    (tmp_path / "face").mkdir()
    for k, m in enumerate(_mask_clip(n, H, W, 0)):
        Image.fromarray(m).save(tmp_path / "face" / f"{k:03d}.webp", lossless=True)
    _save_clip(tmp_path / "lips.webp", _mask_clip(n, H, W, 1))
    _save_clip(tmp_path / "hands.webp", _mask_clip(n, H, W, 2))
    Image.fromarray(C.kind_image("photo", 48, 40)).save(tmp_path / "ref.webp", lossless=True, method=4)


def test_read_frames_device_on_a_file_a_directory_and_a_mixed_directory(tmp_path):
    from mmgt_amd import inputs, video_in
    _write_inputs(tmp_path, 6, 48, 64)
    for name in ("pose.webp", "face", "lips.webp"):
        got = video_in.read_frames_device(tmp_path / name, None, DEV)
        want = np.stack([np.asarray(f.convert("RGB")) for f in inputs.read_frames(tmp_path / name)])
        assert np.array_equal(got.cpu().numpy(), want), name
    assert tuple(video_in.read_frames_device(tmp_path / "face", 4, DEV).shape) == (4, 48, 64, 3)
    Image.fromarray(np.zeros((48, 64, 3), np.uint8)).save(tmp_path / "face" / "006.png")
    with pytest.raises(RuntimeError, match="read_frames"):
        video_in.read_frames_device(tmp_path / "face", None, DEV)


def test_webp_clips_through_the_device_input_helpers(tmp_path):
    from mmgt_amd import inputs, video_in
    _write_inputs(tmp_path, 6, 48, 64)
    read = lambda name: video_in.read_frames_device(tmp_path / name, None, DEV)
    pose = inputs.pose_tensor_device(read("pose.webp"), 64, 48)
    ref = inputs.pose_tensor(inputs.read_frames(tmp_path / "pose.webp"), 64, 48)
    assert pose.is_cuda and tuple(pose.shape) == (1, 3, 6, 48, 64) and torch.equal(pose.cpu(), ref)
    host = {k: inputs.read_frames(tmp_path / k) for k in ("face", "lips.webp", "hands.webp")}
    for hands in ("hands.webp", None):
        a = inputs.motion_masks_device(read("face"), read("lips.webp"), read(hands) if hands else None, 6, 64)
        b = inputs.motion_masks(host["face"], host["lips.webp"], host[hands] if hands else None, 6, torch.device(DEV), 64)
        for la, lb in zip(a, b):
            for x, y in zip(la, lb):
                assert torch.equal(x, y)
    assert a[1][0].std() > 0


def test_pose2vid_input_section_on_webp_inputs_with_both_decoders(tmp_path, capsys):
    from mmgt_amd import hip
    spec = importlib.util.spec_from_file_location("pose2vid_script_webp", os.path.join(ROOT, "scripts", "pose2vid.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    _write_inputs(tmp_path, 8, 64, 64)
    a = argparse.Namespace(pose_path=str(tmp_path / "pose.webp"), face_mask_path=str(tmp_path / "face"), lips_mask_path=str(tmp_path / "lips.webp"),
                           hands_mask_path=str(tmp_path / "hands.webp"), image_path=str(tmp_path / "ref.webp"), L=8, W=64, H=64, decoder="device")
    dev = torch.device(DEV)
    before = {k: hip.call_count(k) for k in ENTRIES}
    pose_d, full_d, face_d, lips_d, L = script.load_inputs(a, dev)
    ref_d = script.load_ref_image(a, dev)
    assert all(hip.call_count(k) - before[k] == 5 for k in ENTRIES)                           # three files, a directory and the reference image
    assert "decoded on the host" not in capsys.readouterr().out
    a.decoder = "pil"
    pose_h, full_h, face_h, lips_h, _ = script.load_inputs(a, dev)
    ref_h = script.load_ref_image(a, dev)
    assert all(hip.call_count(k) - before[k] == 5 for k in ENTRIES)                           # --decoder pil launches none of them
    assert L == 8 and torch.equal(pose_d.cpu(), pose_h) and len(full_d) == 4 and full_d[0].std() > 0
    for x, y in zip(full_d + face_d + lips_d, full_h + face_h + lips_h):
        assert torch.equal(x, y)
    assert ref_d.is_cuda and np.array_equal(ref_d.cpu().numpy(), np.asarray(ref_h))
    # out of the decoder's scope: the host decodes it and says so
    Image.fromarray(C.kind_image("photo", 48, 40)).save(tmp_path / "lossy.webp", quality=80)
    a.decoder, a.image_path = "device", str(tmp_path / "lossy.webp")
    lossy = script.load_ref_image(a, dev)
    assert "decoded on the host (parse_webp: lossy WebP (VP8) is not decoded" in capsys.readouterr().out
    assert np.array_equal(lossy.cpu().numpy(), np.asarray(Image.open(a.image_path).convert("RGB")))
    assert all(hip.call_count(k) - before[k] == 5 for k in ENTRIES)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_out_of_scope_input_raises_before_any_launch(tmp_path):
    from mmgt_amd import hip, video_in
    good = C.stills()["photo-67x45-m0-q0"]
    decode([good])                                                                          # the library is loaded and has run
    before = {k: hip.call_count(k) for k in ENTRIES}
    assert before["mmgt_webp_decode"] >= 1
    lossy = tmp_path / "lossy.webp"
    Image.fromarray(C.kind_image("photo", 67, 45)).save(lossy, quality=80)
    sig = bytearray(good)
    sig[20] = 0x2e
    for bad, word in ((lossy.read_bytes(), "lossy WebP"), (bytes(sig), "bad VP8L signature"), (C.stills()["photo-16x17-m0-q50"], "one call decodes one canvas size"),
                      (good[:-20], "RIFF size"), (b"GIF89a" + good[6:], "not a RIFF/WEBP")):
        with pytest.raises(ValueError, match=word):
            decode([good, bad])
    with pytest.raises(ValueError, match="lossy WebP"):
        video_in.read_frames_device(lossy, None, DEV)
    assert before == {k: hip.call_count(k) for k in ENTRIES}


@pytest.mark.parametrize("name", sorted(C.corrupt()))
def test_a_stream_that_does_not_decode_raises_naming_the_frame(name):
    from mmgt_amd import video_in
    files, code = C.corrupt()[name]
    with pytest.raises(RuntimeError, match=f"frame 1, image data: {video_in.WEBP_STATUS_TEXT[code][:30]}"):
        decode(files)


def test_the_c_entries_refuse_out_of_range_arguments():
    from mmgt_amd import hip
    L = hip.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    tab = torch.zeros((2, 16), dtype=torch.int64, device=DEV)
    words = torch.zeros(4096, dtype=torch.int32, device=DEV)
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    calls = [
        (L.mmgt_webp_decode, (p(buf), 4096, p(tab), p(words), 2048, p(st), 0, s)),
        (L.mmgt_webp_decode, (p(buf), 4095, p(tab), p(words), 2048, p(st), 1, s)),
        (L.mmgt_webp_decode, (p(buf), 4096, p(tab), p(words), 31, p(st), 1, s)),
        (L.mmgt_webp_decode, (p(buf), 4096, p(tab), p(words), 2048, p(st), 65536, s)),
        (L.mmgt_webp_decode, (p(buf[1:]), 2048, p(tab), p(words), 2048, p(st), 1, s)),
        (L.mmgt_webp_decode, (p(buf), 2048, p(tab), p(words[1:]), 2048, p(st), 1, s)),
        (L.mmgt_webp_untransform, (p(tab), p(words), 2048, p(words[2048:]), 2048, p(st), 0, s)),
        (L.mmgt_webp_untransform, (p(tab), p(words), 31, p(words[2048:]), 2048, p(st), 1, s)),
        (L.mmgt_webp_untransform, (p(tab), p(words), 2048, p(words[2048:]), 0, p(st), 1, s)),
        (L.mmgt_webp_compose, (p(tab), p(words), 2048, p(words[2048:]), p(buf), 0, 4, 4, s)),
        (L.mmgt_webp_compose, (p(tab), p(words), 2048, p(words[2048:]), p(buf), 1, 0, 4, s)),
        (L.mmgt_webp_compose, (p(tab), p(words), 2048, p(words[2048:]), p(buf), 1, 4, 16385, s)),
        (L.mmgt_webp_compose, (p(tab), p(words), 0, p(words[2048:]), p(buf), 1, 4, 4, s)),
    ]
    for k, (fn, args) in enumerate(calls):
        assert fn(*args) != 0 and "range" in L.mmgt_last_error().decode(), k
    assert L.mmgt_webp_decode(None, 4096, p(tab), p(words), 2048, p(st), 1, s) != 0
    torch.cuda.synchronize()
    assert not bool(buf.any()) and not bool(words.any()) and not bool(st.any())             # nothing was launched
    # rows that name bytes or words outside the buffers: status 12, nothing touched
    rows = np.zeros((2, 16), np.int64)
    rows[0, :9] = (0, 0, 4, 4, 0, 64, 0, 4096, 0)                                           # more scratch words than there are
    rows[1, :9] = (0, 0, 4, 4, 0, 8192, 0, 1024, 0)                                         # a stream past the data
    status = hip.webp_decode(buf, up(rows), words[:2048])
    assert status.cpu().tolist() == [12, 12] and not bool(words.any())
