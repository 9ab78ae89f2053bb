"""PNG / APNG decode on the device (csrc/pngdec.hip through the C ABI, mmgt_amd.video_in) against PIL's Image.open(f).convert("RGB") on
every byte; the inflate launch alone against zlib.decompress and the unfilter launch alone against tests/pngdec_cases.unfilter_ref, so that a
failure names its stage.  Every comparison is bitwise.  The streams here are well formed: what bad data does is proven on the host
(tests/test_pngdec.py, tools/pngdec_host_check.cpp)."""
import argparse
import functools
import importlib.util
import io
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests import png_ref as P
from tests import pngdec_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ENTRIES = ("mmgt_png_inflate", "mmgt_png_unfilter", "mmgt_png_expand")


def decode(pngs, **kw):
    from mmgt_amd import video_in
    out = video_in.decode_png_frames(pngs, DEV, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    return out


@functools.lru_cache(maxsize=None)
def pil_batch(key):
    pngs = C.cross_batches()[key] if len(key) == 2 else C.depth_batches()[key]
    return np.stack([C.pil_rgb(p) for p in pngs])


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stages(pngs):
    """The three launches one by one -> (filtered bytes as inflated, reconstructed bytes, row sums, pixels), all on the host, and the headers."""
    from mmgt_amd import hip, video_in
    headers, (H, W, ct, depth), data, offsets, adlers, palette, plte_len = video_in.png_batch_operands(pngs)
    stride = headers[0].stride
    filt, st0 = hip.png_inflate(up(data.copy()), up(offsets), H * stride)
    inflated = filt.cpu().numpy().copy()
    sums, st1 = hip.png_unfilter(filt, H, W, ct, depth)
    pix, st2 = hip.png_expand(filt, H, W, ct, depth, up(palette) if ct == 3 else None, up(plte_len) if ct == 3 else None)
    assert not st0.any() and not st1.any() and not st2.any()
    return headers, inflated, filt.cpu().numpy(), sums.cpu().numpy(), pix.cpu().numpy(), adlers


# ---- every byte against PIL -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_pil_over_levels_strategies_and_filters(size):
    got = decode(C.cross_batches()[size]).cpu().numpy()
    want = pil_batch(size)
    assert got.shape == want.shape and np.array_equal(got, want), f"frames {sorted(set(np.argwhere(got != want)[:, 0].tolist()))} differ"


@pytest.mark.parametrize("ct,depth", C.DEPTHS)
def test_device_equals_pil_for_every_depth_at_every_size(ct, depth):
    for W, H in C.SIZES:
        got = decode(C.depth_batches()[(W, H, ct, depth)]).cpu().numpy()
        assert np.array_equal(got, pil_batch((W, H, ct, depth))), (W, H)


@pytest.mark.parametrize("size", [(37, 29), (150, 150)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_each_launch_alone(size):
    """Inflate against zlib.decompress, unfilter against the numpy unfilter, the row sums against zlib's Adler-32, the pixels against PIL."""
    from mmgt_amd import video_in
    pngs = C.cross_batches()[size][::7 if size[0] > 100 else 1]
    headers, inflated, recon, sums, pix, adlers = stages(pngs)
    W, H = size
    for k, h in enumerate(headers):
        want = zlib.decompressobj(-15).decompress(h.streams[0])
        assert inflated[k].tobytes() == want, f"inflate, frame {k}"
    for k in range(0, len(pngs), 5 if size[0] > 100 else 1):
        rows = np.frombuffer(inflated[k].tobytes(), np.uint8).reshape(H, -1)
        assert np.array_equal(recon[k].reshape(H, -1)[:, 1:], C.unfilter_ref(rows, 3)), f"unfilter, frame {k}"
        assert np.array_equal(recon[k].reshape(H, -1)[:, 0], rows[:, 0])
    assert np.array_equal(video_in.adler32_of_row_sums(sums, headers[0].stride), adlers)
    assert np.array_equal(pix, np.stack([C.pil_rgb(p) for p in pngs]))


def test_sub_byte_and_two_and_four_byte_pixels_unfilter_alone():
    for ct, depth in ((0, 1), (3, 4), (4, 8), (6, 8)):
        pngs = C.depth_batches()[(21, 37, ct, depth)]
        headers, inflated, recon, sums, pix, adlers = stages(pngs)
        for k in range(len(pngs)):
            rows = inflated[k].reshape(37, -1)
            assert np.array_equal(recon[k].reshape(37, -1)[:, 1:], C.unfilter_ref(rows, C.filter_bpp(ct, depth))), (ct, depth, k)


def test_inflate_of_what_zlib_never_emits():
    from mmgt_amd import hip, video_in
    for name, (z, W, H) in C.token_streams().items():
        h = video_in.parse_png(C.make_png(b"", W, H, 0, 8, compress=z))
        _, _, data, offsets, _, _, _ = video_in.png_batch_operands(None, [h])
        filt, st = hip.png_inflate(up(data.copy()), up(offsets), H * (1 + W))
        assert int(st[0]) == 0 and filt.cpu().numpy().tobytes() == zlib.decompress(z), name


def test_pil_files_the_encoders_streams_and_per_frame_palettes():
    from mmgt_amd import video_in
    rng = np.random.default_rng(3)
    for mode in ("1", "L", "LA", "RGB", "RGBA"):
        ch = {"1": 0, "L": 0, "LA": 2, "RGB": 3, "RGBA": 4}[mode]
        a = rng.integers(0, 2, (29, 37)).astype(bool) if mode == "1" else rng.integers(0, 256, (29, 37, ch) if ch else (29, 37)).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(a, None if mode == "1" else mode).save(b, format="PNG")
        data = b.getvalue()
        assert np.array_equal(decode([data])[0].cpu().numpy(), C.pil_rgb(data)), mode
    pngs = C.palette_batch()
    assert len({video_in.parse_png(p).palette.tobytes() for p in pngs}) == 5
    assert np.array_equal(decode(pngs).cpu().numpy(), np.stack([C.pil_rgb(p) for p in pngs]))
    frames = np.concatenate([P.smooth_frames(2, 37, 21, seed=2), P.pose_frames(1, 37, 21)])
    for strip_rows in (1, 5, 64):
        got = decode([P.png_file(b, 21, 37) for b in P.encode_frames(frames, strip_rows)])
        assert np.array_equal(got.cpu().numpy(), frames), strip_rows


# ---- repeatable, and nothing outside its buffers ----------------------------------------------------------------------------------------------------------
def test_second_run_into_prefilled_buffers_and_guard_words():
    from mmgt_amd import hip, video_in
    pngs = C.cross_batches()[(37, 29)][:40] + C.cross_batches()[(37, 29)][100:]
    want = pil_batch((37, 29))
    want = np.concatenate([want[:40], want[100:]])
    a = decode(pngs)
    buf = torch.full((len(pngs), 29, 37, 3), 0xA5, dtype=torch.uint8, device=DEV)
    b = decode(pngs, out=buf)
    assert b.data_ptr() == buf.data_ptr() and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want)
    # the launches themselves, into scratch pre-filled with 0xA5 and with guard words behind every buffer
    headers, (H, W, ct, depth), data, offsets, adlers, _, _ = video_in.png_batch_operands(pngs)
    n, fb, G = len(pngs), H * headers[0].stride, 64
    filt_all = torch.full((n * fb + G,), 0xA5, dtype=torch.uint8, device=DEV)
    out_all = torch.full((n * H * W * 3 + G,), 0xA5, dtype=torch.uint8, device=DEV)
    sums_all = torch.full((n * H * 2 + 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    st_all = torch.full((3 * n + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    filt = filt_all[:n * fb].view(n, fb)
    hip.png_inflate(up(data.copy()), up(offsets), fb, out=(filt, st_all[:n]))
    hip.png_unfilter(filt, H, W, ct, depth, out=(sums_all[:n * H * 2].view(n, H, 2), st_all[n:2 * n]))
    pix, _ = hip.png_expand(filt, H, W, ct, depth, out=(out_all[:n * H * W * 3].view(n, H, W, 3), st_all[2 * n:3 * n]))
    assert torch.equal(pix, a)
    assert bool((filt_all[n * fb:] == 0xA5).all()) and bool((out_all[n * H * W * 3:] == 0xA5).all())
    assert bool((sums_all[n * H * 2:] == 0x5A5A5A5A5A5A5A5A).all()) and bool((st_all[3 * n:] == 0x5A5A5A5A).all()) and not bool(st_all[:3 * n].any())


def test_groups_under_the_scratch_budget(monkeypatch):
    from mmgt_amd import hip, video_in
    pngs = C.cross_batches()[(21, 37)][:10]
    before = hip.call_count("mmgt_png_inflate")
    monkeypatch.setattr(video_in, "PNGDEC_SCRATCH_BYTES", 3 * 37 * (1 + 63 + 16))             # three frames per set of launches
    got = decode(pngs)
    assert hip.call_count("mmgt_png_inflate") - before == 4
    assert np.array_equal(got.cpu().numpy(), pil_batch((21, 37))[:10])


# ---- the way back in of the project's own lossless outputs -------------------------------------------------------------------------------------------------
def test_apng_and_png_directory_round_trip(tmp_path):
    from mmgt_amd import video_in, video_out
    import mmgt_amd
    frames = np.concatenate([P.smooth_frames(4, 40, 56, seed=6), P.pose_frames(2, 40, 56)])
    videos = torch.from_numpy(frames)[None]                                                # (b, t, h, w, 3) uint8
    video_out.save_videos_grid(videos, str(tmp_path / "clip.apng"), n_rows=1, fps=8)
    sent = video_out.frames_uint8(videos, 1)
    assert np.array_equal(sent, frames)
    got = mmgt_amd.read_frames_device(tmp_path / "clip.apng", None, DEV)
    assert tuple(got.shape) == sent.shape and np.array_equal(got.cpu().numpy(), sent) and np.array_equal(sent, C.pil_frames((tmp_path / "clip.apng").read_bytes()))
    assert tuple(video_in.read_frames_device(tmp_path / "clip.apng", 4, DEV).shape) == (4,) + sent.shape[1:]
    blobs = video_out.encode_png_frames(torch.from_numpy(frames).to(DEV))
    video_out.write_png_sequence(tmp_path / "clip_png", blobs, 56, 40)                       # what --format pngs writes
    got = video_in.read_frames_device(tmp_path / "clip_png", None, DEV)
    assert np.array_equal(got.cpu().numpy(), frames)
    assert np.array_equal(video_in.read_frames_device(tmp_path / "clip_png" / "0002.png", None, DEV).cpu().numpy(), frames[2:3])


def _mask_clip(n, H, W, seed):
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        cx, cy = W * (0.3 + 0.05 * k) + seed, H * 0.5 - seed
        out[k][(xx - cx) ** 2 + (yy - cy) ** 2 < (H / (4 + seed)) ** 2] = 255
    return out


def _write_inputs(tmp_path, n, H, W):
    """pose/ (RGB .png), face/ lips/ hands/ (grey .png, as binary masks are stored), ref.png (palette, 4 bits)."""
    for name, arr in (("pose", P.smooth_frames(n, H, W, seed=8)), ("face", _mask_clip(n, H, W, 0)), ("lips", _mask_clip(n, H, W, 1)),
                      ("hands", _mask_clip(n, H, W, 2))):
        (tmp_path / name).mkdir()
        for k in range(n):
            Image.fromarray(arr[k]).save(tmp_path / name / f"{k:03d}.png")
    (tmp_path / "ref.png").write_bytes(C.case_png(48, 40, 3, 4, seed=4))


def test_png_directories_through_the_device_input_helpers(tmp_path):
    from mmgt_amd import inputs, video_in
    _write_inputs(tmp_path, 6, 48, 64)
    read = lambda name: video_in.read_frames_device(tmp_path / name, None, DEV)
    pose = inputs.pose_tensor_device(read("pose"), 64, 48)
    ref = inputs.pose_tensor(inputs.read_frames(tmp_path / "pose"), 64, 48)
    assert pose.is_cuda and tuple(pose.shape) == (1, 3, 6, 48, 64) and torch.equal(pose.cpu(), ref)
    host = {k: inputs.read_frames(tmp_path / k) for k in ("face", "lips", "hands")}
    for hands in ("hands", None):
        a = inputs.motion_masks_device(read("face"), read("lips"), read(hands) if hands else None, 6, 64)
        b = inputs.motion_masks(host["face"], host["lips"], host[hands] if hands else None, 6, torch.device(DEV), 64)
        for la, lb in zip(a, b):
            for x, y in zip(la, lb):
                assert torch.equal(x, y)
    assert a[1][0].std() > 0


def test_pose2vid_input_section_on_png_inputs_with_both_decoders(tmp_path, capsys):
    from mmgt_amd import hip
    spec = importlib.util.spec_from_file_location("pose2vid_script_png", os.path.join(ROOT, "scripts", "pose2vid.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    _write_inputs(tmp_path, 8, 64, 64)
    a = argparse.Namespace(pose_path=str(tmp_path / "pose"), face_mask_path=str(tmp_path / "face"), lips_mask_path=str(tmp_path / "lips"),
                           hands_mask_path=str(tmp_path / "hands"), image_path=str(tmp_path / "ref.png"), L=8, W=64, H=64, decoder="device")
    dev = torch.device(DEV)
    before = {k: hip.call_count(k) for k in ENTRIES}
    pose_d, full_d, face_d, lips_d, L = script.load_inputs(a, dev)
    ref_d = script.load_ref_image(a, dev)
    assert all(hip.call_count(k) - before[k] == 5 for k in ENTRIES)                           # four directories and the reference image
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
    rows = C.filter_rows(C.raw_rows(48, 40, 0, 8, 1), 1, [0] * 40)
    sixteen = np.repeat(rows[:, 1:], 2, axis=1)
    data16 = np.concatenate([np.zeros((40, 1), np.uint8), sixteen], axis=1).tobytes()
    (tmp_path / "deep.png").write_bytes(C.make_png(data16, 48, 40, 0, 16))
    a.decoder, a.image_path = "device", str(tmp_path / "deep.png")
    ref16 = script.load_ref_image(a, dev)
    assert "decoded on the host (parse_png: bit depth 16" in capsys.readouterr().out
    assert np.array_equal(ref16.cpu().numpy(), np.asarray(Image.open(a.image_path).convert("RGB")))
    assert all(hip.call_count(k) - before[k] == 5 for k in ENTRIES)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_out_of_scope_input_raises_before_any_launch(tmp_path):
    import struct
    from mmgt_amd import hip, video_in
    good = C.case_png(21, 37, 2, 8, seed=1)
    decode([good])                                                                          # the library is loaded and has run
    before = {k: hip.call_count(k) for k in ENTRIES}
    assert before["mmgt_png_inflate"] >= 1
    laced = good[:8] + P.chunk(b"IHDR", struct.pack(">IIBBBBB", 21, 37, 8, 2, 0, 0, 1)) + good[33:]
    crc = bytearray(good)
    crc[good.index(b"IDAT") + 10] ^= 1
    for bad, word in ((laced, "Adam7 interlace"), (bytes(crc), "bad CRC"), (C.case_png(37, 21, 2, 8), "one call decodes one geometry"),
                      (good[:-12], "missing IEND")):
        with pytest.raises(ValueError, match=word):
            decode([good, bad])
    (tmp_path / "laced.png").write_bytes(laced)
    with pytest.raises(ValueError, match="Adam7 interlace"):
        video_in.read_frames_device(tmp_path / "laced.png", None, DEV)
    assert before == {k: hip.call_count(k) for k in ENTRIES}


def test_a_falsified_trailer_and_a_palette_index_beyond_plte_raise():
    from mmgt_amd import video_in
    good = C.case_png(21, 37, 2, 8, seed=1)
    h = video_in.parse_png(good)
    h.adlers[0] ^= 1
    with pytest.raises(RuntimeError, match="frame 0: the image data's Adler-32"):
        video_in._decode_png_operands(video_in.png_batch_operands(None, [h]), DEV)
    idx = C.raw_rows(21, 37, 3, 8, 1)
    idx[7, 3] = 250                                                                          # the palette has 200 entries
    bad = C.make_png(C.filter_rows(idx, 1, [0] * 37).tobytes(), 21, 37, 3, 8, plte=C.palette_for(8, 1))
    with pytest.raises(RuntimeError, match="frame 1, pixels: a palette index beyond PLTE"):
        decode([C.case_png(21, 37, 3, 8, seed=1), bad])


def test_the_c_entries_refuse_out_of_range_arguments():
    import ctypes
    from mmgt_amd import hip
    L = hip.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    off = torch.tensor([0, 16], dtype=torch.int64, device=DEV)
    words = torch.zeros(64, dtype=torch.int64, device=DEV)
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    calls = [
        L.mmgt_png_inflate(p(buf), 4096, p(off), p(buf[2048:]), p(st), 0, 64, s),
        L.mmgt_png_inflate(p(buf), 4095, p(off), p(buf[2048:]), p(st), 1, 64, s),
        L.mmgt_png_inflate(p(buf), 4096, p(off), p(buf[2048:]), p(st), 1, 0, s),
        L.mmgt_png_inflate(p(buf), 4096, p(off), p(buf[2048:]), p(st), 1, 16384 * 65537 + 1, s),
        L.mmgt_png_inflate(p(buf[1:]), 2048, p(off), p(buf[2048:]), p(st), 1, 64, s),
        L.mmgt_png_inflate(p(buf), 2048, p(off), p(buf[2049:]), p(st), 1, 64, s),
        L.mmgt_png_unfilter(p(buf), p(words), p(st), 1, 0, 4, 2, 8, s),
        L.mmgt_png_unfilter(p(buf), p(words), p(st), 1, 4, 16385, 2, 8, s),
        L.mmgt_png_unfilter(p(buf), p(words), p(st), 1, 4, 4, 2, 4, s),
        L.mmgt_png_unfilter(p(buf), p(words), p(st), 1, 4, 4, 5, 8, s),
        L.mmgt_png_unfilter(p(buf), p(words), p(st), 0, 4, 4, 2, 8, s),
        L.mmgt_png_expand(p(buf), None, None, p(buf[2048:]), p(st), 1, 4, 4, 6, 16, s),
        L.mmgt_png_expand(p(buf), None, None, p(buf[2048:]), p(st), 1, 4, 4, 0, 3, s),
        L.mmgt_png_expand(p(buf), None, None, p(buf[2048:]), p(st), 1, 16385, 4, 0, 8, s),
    ]
    for k, rc in enumerate(calls):
        assert rc != 0, k
    for fn, args in ((L.mmgt_png_inflate, (p(buf), 4096, p(off), p(buf[2048:]), p(st), 0, 64, s)),
                     (L.mmgt_png_unfilter, (p(buf), p(words), p(st), 1, 0, 4, 2, 8, s)),
                     (L.mmgt_png_expand, (p(buf), None, None, p(buf[2048:]), p(st), 1, 4, 4, 0, 3, s))):
        assert fn(*args) != 0 and "range" in L.mmgt_last_error().decode()
    assert L.mmgt_png_expand(p(buf), None, None, p(buf[2048:]), p(st), 1, 4, 4, 3, 8, s) != 0      # colour type 3 without a palette
    torch.cuda.synchronize()
    assert not bool(buf.any()) and not bool(st.any())                                       # nothing was launched


def test_a_mixed_directory_still_raises(tmp_path):
    from mmgt_amd import video_in
    d = tmp_path / "frames"
    d.mkdir()
    Image.fromarray(P.smooth_frames(1, 29, 37)[0]).save(d / "000.png")
    Image.fromarray(P.smooth_frames(1, 29, 37)[0]).save(d / "001.jpg")
    with pytest.raises(RuntimeError, match="read_frames"):
        video_in.read_frames_device(d, None, DEV)
    (d / "001.jpg").unlink()
    assert tuple(video_in.read_frames_device(d, None, DEV).shape) == (1, 29, 37, 3)
