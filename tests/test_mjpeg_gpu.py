"""The device-side Motion-JPEG encoder (csrc/mjpeg.hip, mmgt_amd.video_out) on the GPU against the fp64 restatement tests/mjpeg_ref.py, an
independent decoder (PIL / libjpeg-turbo) and PIL's own encoder; then the layers above it: decode_video_jpeg, the pipeline's
output_type="jpeg" and both scripts with --format avi.

Margins of test_quality_and_size_against_pils_encoder.  libjpeg's integer DCT and colour tables round differently from a float encoder, so
PSNR and size are close to PIL's but not equal.  The margins come from the REFERENCE, not the device: tests/mjpeg_ref.py against PIL's encoder
(same quality, sampling, restart_marker_rows=1) on the CPU over PIL_CASES gave, at worst,
    PSNR shortfall  0.018 dB  (4:4:4, 17 x 9, quality 90)     -> 2 x = 0.036 dB, below the floor: margin 0.05 dB
    size excess     8.47 %    (4:2:0, 40 x 56, quality 90)    -> 2 x: margin 16.95 %
(on MCU-multiple sizes the restatement is 0.05 % .. 1.3 % SMALLER than PIL; off the multiple it is larger because the frame is extended by edge
replication, as the encoder is specified, where libjpeg pads with DC-only dummy blocks)."""
import io
import json
import os
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch
from PIL import Image

from tests import mjpeg_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PSNR_MARGIN_DB = 0.05
SIZE_MARGIN = 0.1695
PIL_CASES = [(128, 128, 11), (40, 56, 12), (17, 9, 13), (96, 208, 14)]            # (H, W, seed) of R.smooth_frame
PIL_QUALITIES = (50, 75, 90)
SAMPLINGS = ("4:2:0", "4:4:4")


def _dev(frames):
    return torch.from_numpy(np.ascontiguousarray(frames)).cuda()


def _pil_jpeg(frame, quality, subsampling):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", quality=quality, subsampling={"4:2:0": 2, "4:4:4": 0}[subsampling], restart_marker_rows=1)
    return b.getvalue()


def _decode(data):
    img = Image.open(io.BytesIO(data))
    img.load()
    return img


def _vae_frames(n=4, latent=8):
    """uint8 frames out of the VAE decoder + frames_to_u8 (random-init weights): (n, 8 latent, 8 latent, 3) on the device."""
    from mmgt_amd.synthetic import hash_uniform, synth_state_dict
    from mmgt_amd.vae import AutoencoderKL, vae_decoder_spec
    vae = AutoencoderKL(device="cuda:0", dtype=torch.bfloat16)
    vae.load_state_dict(synth_state_dict(vae_decoder_spec(), prefix="vae.", device="cuda:0"))
    lat = hash_uniform("mjpeg.lat", (1, 4, n, latent, latent), 1.7)
    return vae, lat, vae.decode_video_uint8(lat)[0].contiguous()


# ---- coefficients --------------------------------------------------------------------------------------------------------------------------------
def _check_coefficients(frame, quality, subsampling, what):
    from mmgt_amd import hip
    got = hip.jpeg_dct_quant(_dev(frame[None]), quality, subsampling)[0].cpu().numpy().astype(np.int64)
    want, ratio = R.coefficients(frame, quality, subsampling, with_ratio=True)
    assert got.shape == want.shape
    band = R.tie_band(ratio)                                   # defined by the fp64 reference alone
    diff = np.abs(got - want)
    print(f"{what} {subsampling} q{quality}: {want.size} coefficients, tie band holds {100 * band.mean():.3f} %, "
          f"{int((diff != 0).sum())} differ ({int((diff[~band] != 0).sum())} outside the band), max |d| {int(diff.max())}")
    assert band.mean() < 0.01, "the tie band must stay a sliver, or it could hide a wrong kernel"
    assert (diff[~band] == 0).all()
    assert diff.max() <= 1


@pytest.mark.parametrize("subsampling", SAMPLINGS)
@pytest.mark.parametrize("quality", [50, 90, 95])
def test_coefficients_match_fp64_outside_the_tie_band(subsampling, quality):
    for H, W, seed in ((256, 256, 1), (40, 56, 2), (17, 9, 3), (72, 200, 4)):
        _check_coefficients(R.smooth_frame(H, W, seed), quality, subsampling, f"smooth {H}x{W}")


def test_coefficients_of_vae_output_frames():
    _, _, frames = _vae_frames(4, 16)
    frames = frames.cpu().numpy()
    assert frames.shape == (4, 128, 128, 3) and frames.std() > 0
    for k in range(frames.shape[0]):
        for ss in SAMPLINGS:
            _check_coefficients(frames[k], 90, ss, f"vae frame {k}")


# ---- bit stream ----------------------------------------------------------------------------------------------------------------------------------
def _device_files_and_coefficients(frames, quality, subsampling):
    from mmgt_amd import hip, video_out
    x = _dev(frames)
    files = video_out.encode_jpeg_frames(x, quality, subsampling)
    coef = hip.jpeg_dct_quant(x, quality, subsampling).cpu().numpy()
    return files, coef


BITSTREAM_CASES = {
    "smooth_on_multiple": (lambda: R.smooth_frame(64, 64, 21)[None], 90),
    "smooth_off_multiple": (lambda: R.smooth_frame(40, 56, 22)[None], 75),
    "tiny_off_multiple": (lambda: R.smooth_frame(17, 9, 23)[None], 50),
    "wide_two_chunks": (lambda: R.smooth_frame(24, 1000, 24)[None], 90),           # more than 256 blocks in an MCU row: the carry between chunks
    "all_black": (lambda: np.zeros((1, 48, 80, 3), np.uint8), 90),
    "noise_q100": (lambda: R.noise_frame(96, 112, 25)[None], 100),                  # long codes, stuffing
    "noise_q100_wide": (lambda: R.noise_frame(16, 1100, 26)[None], 100),
    "quality_1": (lambda: R.smooth_frame(64, 48, 27)[None], 1),
    "clip_24_frames": (lambda: np.stack([R.smooth_frame(144, 80, 100 + k) for k in range(24)]), 90),   # 9 / 18 MCU rows: RST numbering wraps
}


@pytest.mark.parametrize("subsampling", SAMPLINGS)
@pytest.mark.parametrize("case", sorted(BITSTREAM_CASES))
def test_bit_stream_equals_the_restatements_coder_on_the_devices_coefficients(case, subsampling):
    make, quality = BITSTREAM_CASES[case]
    frames = make()
    n, H, W, _ = frames.shape
    files, coef = _device_files_and_coefficients(frames, quality, subsampling)
    assert len(files) == n
    for k in range(n):
        want = R.file_from_coefficients(coef[k], W, H, quality, subsampling)
        assert files[k] == want, f"{case} frame {k}: {len(files[k])} B vs {len(want)} B, first difference at " \
                                 f"{next((i for i, (a, b) in enumerate(zip(files[k], want)) if a != b), min(len(files[k]), len(want)))}"
        # an independent decoder: true size and mode, and the same picture as from the restatement's own file
        img = _decode(files[k])
        assert img.format == "JPEG" and img.size == (W, H) and img.mode == "RGB"
        assert np.array_equal(np.asarray(img), np.asarray(_decode(want)))
        if k < 3:                                              # and against the restatement end to end (its own fp64 coefficients)
            ref_coef = R.coefficients(frames[k], quality, subsampling)
            if np.array_equal(coef[k], ref_coef):
                assert files[k] == R.encode(frames[k], quality, subsampling)
            else:                                              # only coefficients inside the tie band may differ (the coefficient tests)
                print(f"{case} frame {k}: {int((coef[k] != ref_coef).sum())} of {ref_coef.size} coefficients differ from fp64")
    if case == "noise_q100":
        assert files[0].count(b"\xff\x00") > 0
    if case == "clip_24_frames":
        rows = R.geometry(H, W, subsampling)[0]
        scan = files[5][files[5].index(b"\xff\xda"):]
        assert [scan.count(bytes([0xFF, 0xD0 + m])) for m in range(8)] == [(rows - 1 - m + 7) // 8 for m in range(8)]


def test_uniform_noise_at_quality_100_comes_back_whole_at_512():
    """A 512 x 512 frame of uniform noise at quality 100: nothing is truncated (the segment bound holds for any input) and PIL decodes all of it."""
    from mmgt_amd import video_out
    frame = R.noise_frame(512, 512, 31)
    for ss in SAMPLINGS:
        data = video_out.encode_jpeg_frames(_dev(frame[None]), 100, ss)[0]
        img = _decode(data)
        assert img.size == (512, 512)
        pil = _decode(_pil_jpeg(frame, 100, ss))
        got, ref = R.psnr(np.asarray(img), frame), R.psnr(np.asarray(pil), frame)
        print(f"noise 512x512 q100 {ss}: {len(data)} B (raw {frame.size} B), PSNR {got:.2f} dB, PIL's encoder {ref:.2f} dB / {len(_pil_jpeg(frame, 100, ss))} B")
        assert got > ref - PSNR_MARGIN_DB
        # every MCU row is there: the bottom rows of the picture are as good as the top ones
        assert R.psnr(np.asarray(img)[-64:], frame[-64:]) > ref - 1.0


@pytest.mark.parametrize("subsampling", SAMPLINGS)
def test_quality_and_size_against_pils_encoder(subsampling):
    """Held to the margins the restatement needs against PIL (module docstring), not to anything measured on the device."""
    from mmgt_amd import video_out
    for H, W, seed in PIL_CASES:
        frame = R.smooth_frame(H, W, seed)
        for q in PIL_QUALITIES:
            mine = video_out.encode_jpeg_frames(_dev(frame[None]), q, subsampling)[0]
            pil = _pil_jpeg(frame, q, subsampling)
            p_mine, p_pil = R.psnr(np.asarray(_decode(mine)), frame), R.psnr(np.asarray(_decode(pil)), frame)
            print(f"{subsampling} {H}x{W} q{q}: device {len(mine)} B {p_mine:.3f} dB, PIL {len(pil)} B {p_pil:.3f} dB")
            assert p_mine >= p_pil - PSNR_MARGIN_DB
            assert len(mine) <= len(pil) * (1 + SIZE_MARGIN)


def test_ten_calls_into_poisoned_buffers_give_the_same_bytes():
    from mmgt_amd import hip, video_out
    frames = _dev(np.stack([R.smooth_frame(72, 200, 40 + k) for k in range(6)]))
    first = video_out.encode_jpeg_frames(frames, 90)
    rows = hip.jpeg_geometry(72, 200, "4:2:0")[0]
    coef = hip.jpeg_dct_quant(frames, 90)
    stride = hip.jpeg_segment_stride(200, "4:2:0")
    head = video_out.jfif_headers(200, 72, 90)
    for call in range(10):
        segs = torch.full((6 * rows, stride), 0xA5 + call, device="cuda", dtype=torch.uint8)
        sizes = torch.full((6 * rows,), -7, device="cuda", dtype=torch.int32)
        coef2 = torch.full_like(coef, 0x5A5A)
        _check = hip.lib().mmgt_jpeg_dct_quant(frames.data_ptr(), coef2.data_ptr(), 6, 72, 200, 420, 90, torch.cuda.current_stream().cuda_stream)
        assert _check == 0 and torch.equal(coef2, coef)
        hip.jpeg_entropy(coef2, 72, 200, out=(segs, sizes))
        data, off = hip.jpeg_compact(segs, sizes, rows)
        data, off = data.cpu().numpy().tobytes(), off.tolist()
        assert [head + data[off[k * rows]:off[(k + 1) * rows]] for k in range(6)] == first
        assert video_out.encode_jpeg_frames(frames, 90) == first


def test_bad_arguments_raise():
    from mmgt_amd import hip, video_out
    x = _dev(R.smooth_frame(16, 16, 0)[None])
    for q in (0, 101):
        with pytest.raises(RuntimeError, match="quality"):
            hip.jpeg_dct_quant(x, q)
    with pytest.raises(RuntimeError, match="subsampling"):
        video_out.encode_jpeg_frames(x, 90, "4:2:2")
    with pytest.raises(ValueError, match="uint8"):
        video_out.encode_jpeg_frames(x.float(), 90)
    out = torch.empty((1, 1, 1, 6, 64), device="cuda", dtype=torch.int16)
    rc = hip.lib().mmgt_jpeg_dct_quant(x.data_ptr(), out.data_ptr(), 40000, 65535, 65535, 420, 90, None)
    assert rc != 0 and b"index range" in hip.lib().mmgt_last_error()
    assert video_out.encode_jpeg_frames(R.smooth_frame(16, 16, 0)[None], 90) == video_out.encode_jpeg_frames(x, 90)     # host data is uploaded


# ---- the layers above ----------------------------------------------------------------------------------------------------------------------------
def test_decode_video_jpeg_equals_encoding_the_uint8_frames():
    from mmgt_amd import video_out
    vae, lat, _ = _vae_frames(11, 8)
    for q, ss in ((90, "4:2:0"), (60, "4:4:4")):
        got = vae.decode_video_jpeg(lat, q, ss, frames_per_batch=4)
        want = video_out.encode_jpeg_frames(vae.decode_video_uint8(lat, frames_per_batch=4)[0], q, ss)
        assert len(got) == 11 and got == want
    with pytest.raises(ValueError, match="batch 1"):
        vae.decode_video_jpeg(torch.cat([lat, lat]))


def test_save_videos_grid_avi_of_several_clips(tmp_path):
    """A grid of three clips has a size off the MCU multiple ((h + 2) * rows + 2); .mp4 still raises as before."""
    from mmgt_amd import inputs, video_out
    clips = np.stack([np.stack([R.smooth_frame(40, 40, 10 * c + k) for k in range(5)]) for c in range(3)])      # (3, 5, 40, 40, 3)
    path = tmp_path / "grid.avi"
    video_out.save_videos_grid(torch.from_numpy(clips), str(path), n_rows=2, fps=8, quality=95)
    want = video_out.frames_uint8(torch.from_numpy(clips), 2)
    assert want.shape == (5, 86, 86, 3)
    back = inputs.read_frames(str(path))
    assert len(back) == 5 and back[0].size == (86, 86)
    for img, f in zip(back, want):
        assert R.psnr(np.asarray(img), f) > 30.0
    with pytest.raises(RuntimeError, match="PyAV"):
        video_out.save_videos_grid(torch.from_numpy(clips), str(tmp_path / "x.mp4"))


def test_pipeline_output_type_jpeg_64x64x8():
    from tests.test_pipeline_gpu import _build, _inputs, build_weights
    from mmgt_amd import video_out
    pipe = _build(build_weights("cuda:0"), torch.bfloat16)
    inp = _inputs(8, 8)
    kw = dict(motion_scale=[1.0, 1.0, 2.0], latents=inp["latents"], clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"])
    args = (None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, 8, 2, 3.5)
    jpegs = pipe(*args, output_type="jpeg", jpeg_quality=85, **kw).videos
    u8 = pipe(*args, output_type="uint8", **kw).videos
    assert isinstance(jpegs, list) and len(jpegs) == 8 and all(isinstance(j, bytes) for j in jpegs)
    assert jpegs == video_out.encode_jpeg_frames(u8[0], 85)
    for j, f in zip(jpegs, u8[0].numpy()):
        img = _decode(j)
        assert img.size == (64, 64) and img.mode == "RGB"


def _run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), *args], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _avi_audio(path):
    """Concatenated bodies of the 01wb chunks of an AVI's movi list."""
    from mmgt_amd.inputs import _riff_chunks
    buf = open(path, "rb").read()
    out = b""
    for cc, off, size in _riff_chunks(buf, 12, len(buf)):
        if cc == b"LIST" and buf[off:off + 4] == b"movi":
            out = b"".join(buf[o:o + s] for c, o, s in _riff_chunks(buf, off + 4, off + size) if c == b"01wb")
    return out


def test_audio2vid_format_avi_carries_the_wavs_samples(tmp_path):
    from mmgt_amd import inputs
    t = np.arange(16000) / 16000.0
    pcm = (0.4 * np.sin(2 * np.pi * 220 * t) * 32767).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    L = 8
    rec = _run("audio2vid.py", "--synthetic", "--audio_path", str(tmp_path / "a.wav"), "-W", "64", "-H", "64", "-L", str(L), "--steps", "2",
               "--format", "avi", "--quality", "92", "--out_dir", str(tmp_path))
    assert rec["saved"].endswith(".avi") and rec["bytes"] == os.path.getsize(rec["saved"]) and rec["encode_s"] >= 0
    frames = inputs.read_frames(rec["saved"])
    assert len(frames) == L and all(f.size == (64, 64) and f.mode == "RGB" for f in frames)
    assert np.asarray(frames[0]).std() > 0
    assert _avi_audio(rec["saved"]) == pcm[:L * 16000 // 25].tobytes()               # the wav's first L / fps seconds, bit-exact
    buf = open(rec["saved"], "rb").read()
    assert struct.unpack("<I", buf[32:36])[0] == 40000 and struct.unpack("<I", buf[48:52])[0] == L        # avih: usec per frame, frames


def test_pose2vid_format_avi_and_avi_as_pose_input(tmp_path):
    """pose2vid writes an .avi, and takes one as --pose_path (what audio2vid wrote)."""
    from mmgt_amd import inputs, video_out
    rng = np.random.default_rng(0)
    L = 8
    Image.fromarray(rng.integers(0, 255, (96, 80, 3), dtype=np.uint8)).save(tmp_path / "ref.png")
    pose = np.stack([R.smooth_frame(72, 72, 50 + i) for i in range(L)])
    video_out.write_avi(str(tmp_path / "pose.avi"), video_out.encode_jpeg_frames(pose, 95), 72, 72, 25)
    yy, xx = np.mgrid[0:128, 0:128]
    blob = lambda cx, cy, r: (((xx - cx) ** 2 + (yy - cy) ** 2) < r * r).astype(np.uint8) * 255
    np.save(tmp_path / "face.npy", np.stack([blob(64 + i, 50, 30) for i in range(L)]))
    np.save(tmp_path / "lips.npy", np.stack([blob(64 + i, 70, 8) for i in range(L)]))
    rec = _run("pose2vid.py", "--random-weights", "--image_path", str(tmp_path / "ref.png"), "--pose_path", str(tmp_path / "pose.avi"),
               "--face_mask_path", str(tmp_path / "face.npy"), "--lips_mask_path", str(tmp_path / "lips.npy"), "-W", "64", "-H", "64", "-L", str(L),
               "--num_c", "8", "--steps", "2", "--format", "avi", "--out_dir", str(tmp_path))
    assert rec["video"] == [1, L, 64, 64, 3] and rec["frames"] == L and rec["bytes"] == os.path.getsize(rec["saved"])
    frames = inputs.read_frames(rec["saved"])
    assert len(frames) == L and frames[0].size == (64, 64) and np.asarray(frames[0]).std() > 0
