"""Progressive JPEG decode on the device (csrc/jpegprog.hip through the C ABI, mmgt_amd.video_in) against the restatement
tests/jpegprog_ref.py, which tests/test_jpegprog.py holds to PIL (libjpeg-turbo) byte for byte, and against the device decode of each stream's
baseline twin.  Every comparison is bitwise.  One stream is cut so that a lane ends in a status word; what other bad data does is proven on the
host (tests/test_jpegprog.py, tools/jpegprog_host_check.cpp)."""
import argparse
import functools
import importlib.util
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, features

from tests import jpegdec_ref as R
from tests import jpegprog_cases as C
from tests import jpegprog_ref as P
from tests import mjpeg_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ENTRIES = ("mmgt_jpegprog_entropy", "mmgt_jpegdec_entropy", "mmgt_jpegdec_idct", "mmgt_jpegdec_color")


def decode(jpegs, **kw):
    from mmgt_amd import video_in
    out = video_in.decode_jpeg_frames(jpegs, DEV, progressive=True, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    return out


def counts():
    from mmgt_amd import hip
    return {k: hip.call_count(k) for k in ENTRIES}


def calls_of(fn):
    before = counts()
    out = fn()
    return out, {k: v - before[k] for k, v in counts().items()}


@functools.lru_cache(maxsize=None)
def want(name):
    return P.decode(C.streams()[name])


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", C.names())
def test_device_equals_restatement_pil_and_the_baseline_twin(name):
    from mmgt_amd import video_in
    data, twin = C.streams()[name], C.twins()[name]
    got = decode([data])
    assert tuple(got.shape) == (1,) + want(name).shape
    assert np.array_equal(got[0].cpu().numpy(), want(name)), name
    if features.check_feature("libjpeg_turbo"):
        assert np.array_equal(got[0].cpu().numpy(), pil_rgb(data)), name
    assert torch.equal(got, video_in.decode_jpeg_frames([twin], DEV)), name


def mixed_batch():
    S = C.streams()
    names = ["pil_21x37_420_smooth", "tc_21x37_420_smooth_deep", None, "tc_21x37_420_smooth_restarts"]
    return [S[n] if n else C.twins()["pil_21x37_420_smooth"] for n in names], names


def test_three_scripts_and_a_baseline_file_in_one_call():
    """Three progressive files under three scripts (3, 4 and 3 levels) and a baseline one, third of four; the second run writes into a buffer
    pre-filled with 0xA5."""
    jpegs, names = mixed_batch()
    ref = np.stack([want(n) if n else R.decode(jpegs[2]) for n in names])
    a, n = calls_of(lambda: decode(jpegs))
    assert n == {"mmgt_jpegprog_entropy": 4, "mmgt_jpegdec_entropy": 1, "mmgt_jpegdec_idct": 2, "mmgt_jpegdec_color": 2}
    buf = torch.full((4, 21, 37, 3), 0xA5, dtype=torch.uint8, device=DEV)
    b = decode(jpegs, out=buf)
    assert b.data_ptr() == buf.data_ptr()
    assert np.array_equal(a.cpu().numpy(), ref) and torch.equal(a, b)


def test_launch_counts():
    S = C.streams()
    pil = [S["pil_21x37_420_smooth"], C.pil_jpeg(M.smooth_frame(21, 37, 77), progressive=True, quality=60, subsampling=2)]
    out, n = calls_of(lambda: decode(pil))
    assert n == {"mmgt_jpegprog_entropy": 3, "mmgt_jpegdec_entropy": 0, "mmgt_jpegdec_idct": 1, "mmgt_jpegdec_color": 1}
    assert np.array_equal(out.cpu().numpy(), np.stack([P.decode(j) for j in pil]))
    twin = C.twins()["pil_21x37_420_smooth"]
    out, n = calls_of(lambda: decode([twin, twin]))
    assert n == {"mmgt_jpegprog_entropy": 0, "mmgt_jpegdec_entropy": 1, "mmgt_jpegdec_idct": 1, "mmgt_jpegdec_color": 1}
    assert np.array_equal(out[1].cpu().numpy(), R.decode(twin))
    for script, levels in (("spectral", 1), ("chroma_first", 2), ("deep", 4)):
        _, n = calls_of(lambda: decode([S[f"tc_21x37_420_smooth_{script}"]]))
        assert n["mmgt_jpegprog_entropy"] == levels and n["mmgt_jpegdec_entropy"] == 0, script
    _, n = calls_of(lambda: decode([S["tc_21x37_420_smooth_spectral"], S["tc_21x37_420_smooth_deep"], S["tc_21x37_420_smooth_chroma_first"]]))
    assert n["mmgt_jpegprog_entropy"] == 4                                                   # max level + 1 over the batch


def test_a_directory_of_progressive_jpg_frames(tmp_path):
    from mmgt_amd import video_in
    d = tmp_path / "frames"
    d.mkdir()
    files = [C.pil_jpeg(M.smooth_frame(21, 37, 60 + k), progressive=True, quality=80 + k) for k in range(2)] + [C.pil_jpeg(M.smooth_frame(21, 37, 62))]
    for k, f in enumerate(files):
        (d / f"{k:03d}.jpg").write_bytes(f)
    got = video_in.read_frames_device(d, None, DEV, jpeg_progressive=True)
    assert np.array_equal(got.cpu().numpy(), np.stack([P.decode(files[0]), P.decode(files[1]), R.decode(files[2])]))
    assert tuple(video_in.read_frames_device(d, 1, DEV, jpeg_progressive=True).shape) == (1, 21, 37, 3)
    before = counts()
    with pytest.raises(ValueError, match=r"progressive JPEG \(SOF2\) is not decoded"):
        video_in.read_frames_device(d, None, DEV)
    with pytest.raises(ValueError, match="progressive"):
        video_in.decode_jpeg_frames(files, DEV)
    assert before == counts()


def test_out_of_scope_input_raises_before_any_launch():
    S = C.streams()
    decode([S["pil_8x8_grey"]])
    before = counts()
    with pytest.raises(ValueError, match="one call decodes one size"):
        decode([S["pil_21x37_420_smooth"], S["pil_33x17_422"]])
    good = S["pil_21x37_420_smooth"]
    with pytest.raises(ValueError, match="inter-block smoothing"):
        decode([good, good[:good.rindex(b"\xff\xc4")] + b"\xff\xd9"])                        # the last refinement missing
    assert before == counts()


def test_pose2vid_reference_image_with_and_without_the_flag(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("pose2vid_script", os.path.join(ROOT, "scripts", "pose2vid.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    path = tmp_path / "ref.jpg"
    path.write_bytes(C.streams()["pil_48x64_420_restart_rows1"])
    a = argparse.Namespace(image_path=str(path), decoder="device", decode_progressive_jpeg=True)
    dev = torch.device(DEV)
    ref, n = calls_of(lambda: script.load_ref_image(a, dev))
    assert n["mmgt_jpegprog_entropy"] == 3 and "decoded on the host" not in capsys.readouterr().out
    assert ref.is_cuda and ref.dtype == torch.uint8 and np.array_equal(ref.cpu().numpy(), want("pil_48x64_420_restart_rows1"))
    if features.check_feature("libjpeg_turbo"):
        assert np.array_equal(ref.cpu().numpy(), np.asarray(Image.open(path).convert("RGB")))
    a.decode_progressive_jpeg = False
    host, n = calls_of(lambda: script.load_ref_image(a, dev))
    assert n["mmgt_jpegprog_entropy"] == 0 and "is decoded on the host (parse_jpeg: progressive JPEG" in capsys.readouterr().out
    assert host.is_cuda and np.array_equal(host.cpu().numpy(), np.asarray(Image.open(path).convert("RGB")))


def test_a_truncated_scan_raises_and_the_next_decode_is_correct():
    """Frame 1's scan 4 (luma 6 - 63, its first scan) loses the second half of its bytes; every marker stays, so the parser accepts the file and
    the lane's status word speaks: an error path, as the baseline decoder's cut-segment case."""
    from mmgt_amd import video_in
    good = C.streams()["pil_21x37_420_smooth"]
    a, b = video_in.parse_jpeg(good, progressive=True).scans[4].segments[0]
    cut = good[:a + (b - a) // 2] + good[b:]
    assert len(video_in.parse_jpeg(cut, progressive=True).scans) == 10
    with pytest.raises(RuntimeError, match=r"decode_jpeg_frames: frame 1, scan 4, restart segment 0: "):
        decode([good, cut])
    assert np.array_equal(decode([good])[0].cpu().numpy(), want("pil_21x37_420_smooth"))
