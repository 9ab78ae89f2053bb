"""The device image resize on the GPU (csrc/resize.hip through the C ABI, mmgt_amd.inputs / conditioning / pipeline) against PIL itself:
every uint8 comparison is bitwise, and so is every float result whose float stage the host route defines (ToTensor, the VAE's 2x - 1, CLIP's
rescale and normalize).  tests/test_resize.py holds the arithmetic and the indexing to PIL and to exact buffers on the host."""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import resize_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CASES = [(s, f) for s in R.SHAPES for f in R.FILTERS]
CASE_IDS = [f"{R.shape_id(s)}-{f}" for s, f in CASES]
SENTINEL = 0xA5


def _carve(nbytes, guard):
    """A buffer of `nbytes` inside a larger one filled with the sentinel, `guard` bytes either side (61: a base that is not 4-byte aligned)."""
    big = torch.full((guard + nbytes + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
    return big, big[guard:guard + nbytes]


def _guards_intact(big, nbytes, guard):
    return bool((big[:guard] == SENTINEL).all()) and bool((big[guard + nbytes:] == SENTINEL).all())


def _resize_guarded(x, hd, wd, filt, guard):
    from mmgt_amd import conditioning as C, hip
    n, hs, ws, c = x.shape
    ws_bytes = hip.resize_u8_workspace(n, hs, ws, hd, wd, c)
    assert ws_bytes == (n * hs * wd * c if (hs != hd and ws != wd) else 0)
    big_o, out = _carve(n * hd * wd * c, guard)
    big_t, tmp = _carve(ws_bytes, guard)
    got = hip.resize_u8(x, hd, wd, C.resample_tables_device(ws, wd, filt, x.device), C.resample_tables_device(hs, hd, filt, x.device),
                        out=out.view(n, hd, wd, c), tmp=tmp if ws_bytes else None)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert _guards_intact(big_o, out.numel(), guard), "bytes outside the output were written"
    assert _guards_intact(big_t, ws_bytes, guard), "bytes outside the workspace were written"
    return got


@pytest.mark.parametrize("shape,filt", CASES, ids=CASE_IDS)
def test_device_equals_pil(shape, filt):
    """Noise and 0 / 255 edges, 1 and 3 bands, batches of 1 and of 3 different frames; output and workspace lie between guard bytes, once 4-byte
    aligned (the 4-byte vertical items where the pitch allows) and once not (byte items); two runs give the same bytes."""
    (hs, ws), (hd, wd) = shape
    for kind in R.KINDS:
        for c in (1, 3):
            for n, guard in ((1, 64), (3, 61), (3, 64)):
                fr = R.frames(n, hs, ws, c, kind)
                want = np.stack([R.pil_resize(f, hd, wd, filt) for f in fr])
                x = torch.from_numpy(fr).to(DEV)
                a = _resize_guarded(x, hd, wd, filt, guard)
                assert np.array_equal(a.cpu().numpy(), want), (kind, c, n, guard, int(np.count_nonzero(a.cpu().numpy() != want)))
                b = _resize_guarded(x, hd, wd, filt, guard)
                assert torch.equal(a, b)


@pytest.mark.parametrize("filt", R.FILTERS)
def test_a_1080p_frame(filt):
    """1080 x 1920 -> 512 x 512: 2160 workgroups in the horizontal launch, 768 in the vertical, on 256 CUs."""
    from mmgt_amd import inputs
    fr = R.frames(1, 1080, 1920, 3, "noise")
    got = inputs.resize_frames_device(torch.from_numpy(fr).to(DEV), 512, 512, filt)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1, 512, 512, 3)
    assert np.array_equal(got[0].cpu().numpy(), R.pil_resize(fr[0], 512, 512, filt))


def test_bad_arguments_return_before_any_launch():
    from mmgt_amd import conditioning as C, hip
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    tabs = C.resample_tables_device(8, 4, "bilinear", x.device)
    with pytest.raises(RuntimeError, match="tables_x"):
        hip.resize_u8(x, 8, 4)
    with pytest.raises(RuntimeError, match="bounds"):
        hip.resize_u8(x, 8, 4, tables_x=(tabs[0][:3], tabs[1]))
    with pytest.raises(RuntimeError, match="1 or 3 bands"):
        hip.resize_u8(torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device=DEV), 8, 4, tables_x=tabs)
    with pytest.raises(RuntimeError, match="16384"):
        hip.resize_u8(x, 8, 16385, tables_x=tabs)
    with pytest.raises(RuntimeError, match="lut"):
        hip.resize_u8(x, 8, 4, tables_x=tabs, lut=torch.zeros((1, 256), device=DEV))
    lib = hip.lib()
    p, t0, t1 = x.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr()
    assert lib.mmgt_resize_u8(p, None, None, None, None, 1, 8, 8, 8, 4, 3, t0, t1, 3, None, None, 0, None) == 1          # no output
    assert b"exactly one" in lib.mmgt_last_error()
    o = torch.zeros(96, dtype=torch.uint8, device=DEV)
    assert lib.mmgt_resize_u8(p, None, o.data_ptr(), None, None, 1, 8, 8, 4, 4, 3, t0, t1, 3, t0, t1, 3, None) == 1     # two passes, no workspace
    assert b"workspace" in lib.mmgt_last_error()
    assert lib.mmgt_resize_u8(p, None, o.data_ptr(), None, None, 1, 8, 8, 8, 4, 3, None, None, 0, None, None, 0, None) == 1   # no tables
    assert lib.mmgt_resize_u8(p, None, None, o.data_ptr(), None, 1, 8, 8, 8, 4, 3, t0, t1, 3, None, None, 0, None) == 1       # float without a table
    torch.cuda.synchronize()
    assert not o.any()


# ---- the public interface -----------------------------------------------------------------------------------------------------------------------------
def test_pose_tensor_device_with_resize_is_pose_tensor():
    from PIL import Image
    from mmgt_amd import inputs
    fr = R.frames(5, 48, 80, 3, "noise")
    want = inputs.pose_tensor([Image.fromarray(f) for f in fr], 64, 48)
    got = inputs.pose_tensor_device(torch.from_numpy(fr).to(DEV), 64, 48, resize=True)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 5, 48, 64) and torch.equal(got.cpu(), want)
    want = inputs.pose_tensor([Image.fromarray(f) for f in fr], 40, 30)                                  # both passes
    assert torch.equal(inputs.pose_tensor_device(torch.from_numpy(fr).to(DEV), 40, 30, resize=True).cpu(), want)
    same = inputs.pose_tensor_device(torch.from_numpy(fr).to(DEV), 80, 48)                              # no pass: the lookup alone
    assert torch.equal(same.cpu(), inputs.pose_tensor([Image.fromarray(f) for f in fr], 80, 48))


@pytest.fixture(scope="module")
def ref_image():
    from PIL import Image
    return Image.fromarray(R.image(100, 150, 3, "noise", seed=7))


def test_vae_input_of_the_reference_image(ref_image):
    from mmgt_amd import inputs
    from mmgt_amd.pipeline import _pil_to_tensor
    vae_in, _ = inputs.ref_image_tensors_device(torch.from_numpy(np.asarray(ref_image).copy()).to(DEV), 64, 64)
    assert vae_in.is_cuda and vae_in.dtype == torch.float32 and tuple(vae_in.shape) == (1, 3, 64, 64) and vae_in.is_contiguous()
    assert torch.equal(vae_in.cpu()[0], _pil_to_tensor(ref_image, 64, 64, True))


def test_clip_pixel_values_of_the_reference_image(ref_image):
    """uint8 stage: PIL's default (bicubic) resize, exactly.  Float stage against (v / 255 - mean) / std in fp64: three fp32 roundings on |v| <= 2.7,
    the earlier two amplified by 1 / std <= 3.9 -- about 6e-7, held to 1e-6; against CLIPImageProcessor (itself within 1e-6 of fp64) 2e-6."""
    from transformers import CLIPImageProcessor
    from mmgt_amd import inputs
    dev_img = torch.from_numpy(np.asarray(ref_image).copy()).to(DEV)
    u8 = inputs.resize_frames_device(dev_img[None], 224, 224, "bicubic")[0].cpu().numpy()
    pil224 = ref_image.resize((224, 224))
    assert np.array_equal(u8, np.asarray(pil224))
    _, clip_in = inputs.ref_image_tensors_device(dev_img, 64, 64)
    assert clip_in.is_cuda and clip_in.dtype == torch.float32 and tuple(clip_in.shape) == (1, 3, 224, 224)
    got = clip_in.cpu().numpy().astype(np.float64)
    mean, std = np.array(inputs.CLIP_MEAN, np.float64), np.array(inputs.CLIP_STD, np.float64)
    f64 = ((u8.astype(np.float64) / 255.0 - mean) / std).transpose(2, 0, 1)[None]
    d64 = np.abs(got - f64).max()
    proc = CLIPImageProcessor().preprocess(pil224, return_tensors="pt").pixel_values.numpy().astype(np.float64)
    dproc = np.abs(got - proc).max()
    print(f"clip pixel values: max |d| vs fp64 {d64:.3e}, vs CLIPImageProcessor {dproc:.3e} (the processor vs fp64 {np.abs(proc - f64).max():.3e})")
    assert d64 <= 1e-6 and dproc <= 2e-6


def test_pose_frames_device_at_other_sizes():
    """256 x 256 (512 * 256 bytes of intermediate: beyond the pyramid kernel's LDS) and 192 x 256 (not square) go through the tiled resize and equal
    PIL's bilinear resize of the 512 x 512 drawing; 64 x 64 stays on the pyramid kernel with the result it had."""
    from PIL import Image
    from mmgt_amd import conditioning as C, hip
    from tests.test_dwpose import make_keypoints
    kp = torch.from_numpy(make_keypoints(0, 3).reshape(3, -1)).to(DEV)
    drawn = hip.dwpose_draw(kp.reshape(3, 134, 3).contiguous())[0].cpu().numpy()                        # (3, 512, 512, 3)
    assert drawn.any()

    def want(h, w):
        u8 = np.stack([np.asarray(Image.fromarray(f).resize((w, h), Image.BILINEAR)) for f in drawn])
        return torch.from_numpy(u8).permute(3, 0, 1, 2)[None].float() / 255.0
    for h, w in ((256, 256), (192, 256)):
        before = hip.call_count("mmgt_resize_u8")
        pose, face, lips, hands = C.pose_frames_device(kp, h, w)
        assert hip.call_count("mmgt_resize_u8") == before + 1
        assert tuple(pose.shape) == (1, 3, 3, h, w) and pose.is_contiguous() and torch.equal(pose.cpu(), want(h, w))
        assert tuple(face.shape) == (3, 512, 512)
    before = hip.call_count("mmgt_resize_u8"), hip.call_count("mmgt_resample_u8")
    pose = C.pose_frames_device(kp, 64, 64)[0]
    assert (hip.call_count("mmgt_resize_u8"), hip.call_count("mmgt_resample_u8")) == (before[0], before[1] + 3)
    # the pyramid kernel divides by 255 on the device: PIL's bytes exactly, the quotient to the last ulp (as tests/test_conditioning.py holds it)
    assert torch.equal((pose.cpu() * 255).round().to(torch.uint8), (want(64, 64) * 255).round().to(torch.uint8))
    torch.testing.assert_close(pose.cpu(), want(64, 64), rtol=0, atol=1e-7)


def _load_script():
    spec = importlib.util.spec_from_file_location("pose2vid_script_resize", os.path.join(ROOT, "scripts", "pose2vid.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def test_pipeline_takes_the_reference_image_as_a_device_tensor(ref_image):
    """64 x 64, 8 frames, 4 DDIM steps, CLIP and the VAE encoder in the pipeline: ref_image as a uint8 tensor gives the latents of the PIL image of
    the same pixels, bitwise -- both float stages are lookups in tables the host route's own operations filled (the tests above hold the VAE table to
    _pil_to_tensor and show the CLIP table's distance from CLIPImageProcessor; here the processor's values must be reproduced exactly)."""
    from transformers import CLIPImageProcessor
    from mmgt_amd import inputs
    from mmgt_amd.synthetic import hash_uniform, synth_masks
    dev = torch.device(DEV)
    dev_img = torch.from_numpy(np.asarray(ref_image).copy()).to(dev)
    _, clip_in = inputs.ref_image_tensors_device(dev_img, 64, 64)
    assert torch.equal(clip_in.cpu(), CLIPImageProcessor().preprocess(ref_image.resize((224, 224)), return_tensors="pt").pixel_values)
    pipe = _load_script().build_synthetic(dev, torch.float32)
    lips, face = synth_masks("p.lips", 8, 8), synth_masks("p.face", 8, 8)
    kw = dict(motion_scale=[1.0, 1.0, 2.0], latents=hash_uniform("p.noise", (1, 4, 8, 8, 8), 1.7), decode=False)
    args = (hash_uniform("p.pose", (1, 3, 8, 64, 64), 0.5) + 0.5, hash_uniform("p.audio", (1, 8, 32, 768), 1.7), [1 + l for l in lips], face, lips,
            64, 64, 8, 4, 3.5)
    a = pipe(ref_image, *args, **kw).videos.cpu()
    b = pipe(dev_img, *args, **kw).videos.cpu()
    assert torch.isfinite(a).all() and a.std() > 0
    assert torch.equal(a, b)


def _write_avi(path, frames, quality=90):
    from mmgt_amd import video_out
    jpegs = video_out.encode_jpeg_frames(torch.from_numpy(frames).to(DEV), quality, "4:2:0")
    video_out.write_avi(str(path), jpegs, frames.shape[2], frames.shape[1], 25)


def test_pose2vid_input_section_with_the_device_decoder_and_another_frame_size(tmp_path):
    """scripts/pose2vid.py's input section on 96 x 128 .avi inputs at W = H = 64: --decoder device gives the pose tensor and masks of --decoder pil;
    the reference image comes back as a device tensor of the file's pixels, a .jpg through the device decoder."""
    from PIL import Image, features
    from tests import mjpeg_ref as M
    assert features.check_feature("libjpeg_turbo"), "PIL here is not built on libjpeg-turbo: the device decoder restates THAT library's decode"
    script = _load_script()
    _write_avi(tmp_path / "pose.avi", np.stack([M.smooth_frame(96, 128, 80 + k) for k in range(8)]))
    yy, xx = np.mgrid[0:96, 0:128]
    for name, seed in (("face", 0), ("lips", 1), ("hands", 2)):
        clip = np.zeros((8, 96, 128, 3), np.uint8)
        for k in range(8):
            clip[k][(xx - 128 * (0.3 + 0.05 * k) - seed) ** 2 + (yy - 48 + seed) ** 2 < (96 / (4 + seed)) ** 2] = 255
        _write_avi(tmp_path / f"{name}.avi", clip)
    a = argparse.Namespace(pose_path=str(tmp_path / "pose.avi"), face_mask_path=str(tmp_path / "face.avi"), lips_mask_path=str(tmp_path / "lips.avi"),
                           hands_mask_path=str(tmp_path / "hands.avi"), L=8, W=64, H=64, decoder="device")
    dev = torch.device(DEV)
    pose_d, full_d, face_d, lips_d, L = script.load_inputs(a, dev)
    assert L == 8 and pose_d.is_cuda and tuple(pose_d.shape) == (1, 3, 8, 64, 64)
    a.decoder = "pil"
    pose_h, full_h, face_h, lips_h, _ = script.load_inputs(a, dev)
    assert torch.equal(pose_d.cpu(), pose_h)
    for x, y in zip(full_d + face_d + lips_d, full_h + face_h + lips_h):
        assert torch.equal(x, y)
    assert len(full_d) == 4 and full_d[0].std() > 0

    ref = M.smooth_frame(100, 150, 5)
    Image.fromarray(ref).save(tmp_path / "ref.png")
    Image.fromarray(ref).save(tmp_path / "ref.jpg", quality=92)
    for name in ("ref.png", "ref.jpg"):
        a.image_path, a.decoder = str(tmp_path / name), "device"
        got = script.load_ref_image(a, dev)
        assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.uint8
        a.decoder = "pil"
        assert np.array_equal(got.cpu().numpy(), np.asarray(script.load_ref_image(a, dev)))
