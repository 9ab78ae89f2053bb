"""Baseline JPEG decode on the device (csrc/jpegdec.hip through the C ABI, mmgt_amd.video_in) against the numpy restatement
tests/jpegdec_ref.py, which tests/test_jpegdec.py holds to PIL (libjpeg-turbo) byte for byte.  Every comparison is bitwise.  The streams here are
well formed: what bad data does is proven on the host (tests/test_jpegdec.py, tools/jpegdec_host_check.cpp)."""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import jpegdec_cases as C
from tests import jpegdec_ref as R
from tests import mjpeg_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def decode(jpegs, **kw):
    from mmgt_amd import video_in
    out = video_in.decode_jpeg_frames(jpegs, DEV, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    return out


@pytest.mark.parametrize("name", C.names())
def test_device_equals_restatement(name):
    data = C.streams()[name]
    want = R.decode(data)
    got = decode([data])
    assert tuple(got.shape) == (1,) + want.shape
    assert np.array_equal(got[0].cpu().numpy(), want), name


def test_batch_with_per_frame_tables_is_repeatable():
    """Five frames whose quantiser and Huffman tables differ; the second run writes into a buffer pre-filled with 0xA5."""
    from mmgt_amd import video_in
    jpegs = [C.pil_jpeg(M.smooth_frame(21, 37, 100 + k, sigma=3.0 + 9 * k), optimize=True, quality=60 + 8 * k) for k in range(5)]
    heads = [video_in.parse_jpeg(j) for j in jpegs]
    assert len({h.huffman[(1, 0)] for h in heads}) > 1 and len({h.qtables[0].tobytes() for h in heads}) > 1
    want = np.stack([R.decode(j) for j in jpegs])
    a = decode(jpegs)
    buf = torch.full((5, 21, 37, 3), 0xA5, dtype=torch.uint8, device=DEV)
    b = decode(jpegs, out=buf)
    assert b.data_ptr() == buf.data_ptr()
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want) and torch.equal(a, b)


def test_512_square_frames_with_32_segments_and_with_one():
    from mmgt_amd import video_in, video_out
    frame = M.smooth_frame(512, 512, 5)
    ours = video_out.encode_jpeg_frames(torch.from_numpy(frame)[None].to(DEV), 90, "4:2:0")[0]
    pil = C.pil_jpeg(frame, quality=85)
    h_ours, h_pil = video_in.parse_jpeg(ours), video_in.parse_jpeg(pil)
    assert len(h_ours.segments) == 32 and h_ours.restart_interval == 32 and len(h_pil.segments) == 1 and h_pil.restart_interval == 0
    assert np.array_equal(decode([ours])[0].cpu().numpy(), R.decode(ours))
    assert np.array_equal(decode([pil])[0].cpu().numpy(), R.decode(pil))


def _mask_clip(n, H, W, seed):
    """Grey mask frames as RGB: a bright disc that moves, on black."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W, 3), np.uint8)
    for k in range(n):
        cx, cy = W * (0.3 + 0.05 * k) + seed, H * 0.5 - seed
        out[k][(xx - cx) ** 2 + (yy - cy) ** 2 < (H / (4 + seed)) ** 2] = 255
    return out


def _write_avi(path, frames, quality=90):
    from mmgt_amd import video_out
    jpegs = video_out.encode_jpeg_frames(torch.from_numpy(frames).to(DEV), quality, "4:2:0")
    video_out.write_avi(str(path), jpegs, frames.shape[2], frames.shape[1], 25)
    return jpegs


def test_avi_round_trip_and_the_device_input_helpers(tmp_path):
    from PIL import Image
    from mmgt_amd import inputs, video_in
    import mmgt_amd
    frames = np.stack([M.smooth_frame(48, 64, 30 + k) for k in range(6)])
    _write_avi(tmp_path / "clip.avi", frames)
    chunks = inputs.mjpeg_avi_frames(tmp_path / "clip.avi")
    want = np.stack([R.decode(c) for c in chunks])
    got = mmgt_amd.read_frames_device(tmp_path / "clip.avi", None, DEV)
    assert tuple(got.shape) == (6, 48, 64, 3) and np.array_equal(got.cpu().numpy(), want)
    assert M.psnr(want, frames) > 25                                                       # it is the clip that went in
    assert tuple(video_in.read_frames_device(tmp_path / "clip.avi", 4, DEV).shape) == (4, 48, 64, 3)

    pose = inputs.pose_tensor_device(got, 64, 48)
    ref = inputs.pose_tensor([Image.fromarray(f) for f in want], 64, 48)
    assert pose.is_cuda and pose.dtype == torch.float32 and tuple(pose.shape) == (1, 3, 6, 48, 64) and torch.equal(pose.cpu(), ref)
    with pytest.raises(ValueError, match="pose_tensor"):
        inputs.pose_tensor_device(got, 32, 32)

    masks = {}
    for name, seed in (("face", 0), ("lips", 1), ("hands", 2)):
        _write_avi(tmp_path / f"{name}.avi", _mask_clip(6, 48, 64, seed))
        masks[name] = video_in.read_frames_device(tmp_path / f"{name}.avi", None, DEV)
    host = {k: [Image.fromarray(f) for f in v.cpu().numpy()] for k, v in masks.items()}
    for hands in ("hands", None):
        a = inputs.motion_masks_device(masks["face"], masks["lips"], masks[hands] if hands else None, 6, 64)
        b = inputs.motion_masks(host["face"], host["lips"], host[hands] if hands else None, 6, torch.device(DEV), 64)
        for la, lb in zip(a, b):
            assert len(la) == len(lb) == 4
            for x, y in zip(la, lb):
                assert torch.equal(x, y)
    assert a[1][0].std() > 0


def test_a_directory_of_jpg_frames_and_what_is_not_read(tmp_path):
    from mmgt_amd import video_in
    frames = [M.smooth_frame(21, 37, 60 + k) for k in range(3)]
    d = tmp_path / "frames"
    d.mkdir()
    for k, f in enumerate(frames):
        (d / f"{k:03d}.jpg").write_bytes(C.pil_jpeg(f, quality=80 + k))
    got = video_in.read_frames_device(d, None, DEV)
    assert np.array_equal(got.cpu().numpy(), np.stack([R.decode((d / f"{k:03d}.jpg").read_bytes()) for k in range(3)]))
    np.save(tmp_path / "clip.npy", np.stack(frames))
    with pytest.raises(RuntimeError, match="read_frames"):
        video_in.read_frames_device(tmp_path / "clip.npy", None, DEV)
    from PIL import Image
    Image.fromarray(frames[0]).save(d / "003.png")
    with pytest.raises(RuntimeError, match="read_frames"):
        video_in.read_frames_device(d, None, DEV)


def test_out_of_scope_input_raises_before_any_launch():
    from mmgt_amd import hip
    S = C.streams()
    decode([S["ref_16x16_420_q90_smooth"]])                                               # the library is loaded and has run
    before = {k: hip.call_count(k) for k in ("mmgt_jpegdec_sizes", "mmgt_jpegdec_entropy", "mmgt_jpegdec_idct", "mmgt_jpegdec_color")}
    assert before["mmgt_jpegdec_entropy"] >= 1
    with pytest.raises(ValueError, match="one call decodes one size"):
        decode([S["ref_21x37_420_q90_smooth"], S["ref_16x16_420_q90_smooth"]])
    with pytest.raises(ValueError, match="progressive"):
        decode([S["ref_21x37_420_q90_smooth"], C.pil_jpeg(M.smooth_frame(21, 37, 1), progressive=True)])
    assert before == {k: hip.call_count(k) for k in before}


def test_pose2vid_input_section_with_the_device_decoder(tmp_path):
    """scripts/pose2vid.py's input section at 64 x 64 x 8 frames from .avi files: --decoder device gives the pose tensor and masks of --decoder pil
    (PIL on libjpeg-turbo decodes to the same bytes; elsewhere the restatement stands in for PIL)."""
    from PIL import Image, features
    from mmgt_amd import inputs
    spec = importlib.util.spec_from_file_location("pose2vid_script", os.path.join(ROOT, "scripts", "pose2vid.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    _write_avi(tmp_path / "pose.avi", np.stack([M.smooth_frame(64, 64, 80 + k) for k in range(8)]))
    for name, seed in (("face", 0), ("lips", 1), ("hands", 2)):
        _write_avi(tmp_path / f"{name}.avi", _mask_clip(8, 64, 64, seed))
    a = argparse.Namespace(pose_path=str(tmp_path / "pose.avi"), face_mask_path=str(tmp_path / "face.avi"), lips_mask_path=str(tmp_path / "lips.avi"),
                           hands_mask_path=str(tmp_path / "hands.avi"), L=8, W=64, H=64, decoder="device")
    dev = torch.device(DEV)
    pose_d, full_d, face_d, lips_d, L = script.load_inputs(a, dev)
    assert L == 8 and tuple(pose_d.shape) == (1, 3, 8, 64, 64)
    if features.check_feature("libjpeg_turbo"):
        a.decoder = "pil"
        pose_h, full_h, face_h, lips_h, _ = script.load_inputs(a, dev)
    else:
        read = lambda p: [Image.fromarray(R.decode(c)) for c in inputs.mjpeg_avi_frames(p)]
        pose_h = inputs.pose_tensor(read(a.pose_path), 64, 64)
        full_h, face_h, lips_h = inputs.motion_masks(read(a.face_mask_path), read(a.lips_mask_path), read(a.hands_mask_path), 8, dev, 64)
    assert torch.equal(pose_d.cpu(), pose_h)
    for x, y in zip(full_d + face_d + lips_d, full_h + face_h + lips_h):
        assert torch.equal(x, y)
    assert len(full_d) == 4 and full_d[0].std() > 0
