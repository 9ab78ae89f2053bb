"""End to end at BASELINE config 1 (64x64 px, 8 frames, 4 DDIM steps): the HIP Pose2VideoPipeline (ReferenceNet ->
banks, PoseGuider, windowed CFG denoising, DDIM, VAE decode) against the oracle pipeline on the same weights and noise."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmgt_amd.synthetic import hash_uniform, synth_masks, synth_state_dict  # noqa: E402
from tests.oracle_cache import cached  # noqa: E402


def _inputs(frames, latent):
    lips = synth_masks("p.lips", frames, latent)
    face = synth_masks("p.face", frames, latent)
    return dict(clip=hash_uniform("p.clip", (1, 768), 1.0), ref_lat=hash_uniform("p.reflat", (1, 4, latent, latent), 1.0),
                pose=hash_uniform("p.pose", (1, 3, frames, latent * 8, latent * 8), 0.5) + 0.5,
                audio=hash_uniform("p.audio", (1, frames, 32, 768), 1.7), full=[1 + l for l in lips], face=face, lips=lips,
                latents=hash_uniform("p.noise", (1, 4, frames, latent, latent), 1.7))


def build_weights(dev):
    from mmgt_amd.side_models import pose_guider_spec
    from mmgt_amd.unet3d_spec import unet2d_reference_spec, unet3d_spec
    from mmgt_amd.vae import vae_decoder_spec
    pg_spec = pose_guider_spec(320, (16, 32, 96, 256))
    return dict(unet=synth_state_dict(unet3d_spec(), device=dev),
                refnet=synth_state_dict(unet2d_reference_spec(), prefix="refnet.", device=dev),
                pose=synth_state_dict(pg_spec, prefix="pose_guider.", device=dev),
                vae=synth_state_dict(vae_decoder_spec(), prefix="vae.", device=dev))


@pytest.fixture(scope="module")
def weights():
    sds = build_weights("cuda:0")
    return sds, {k: {n: t.cpu() for n, t in v.items()} for k, v in sds.items()}


def oracle_pipeline_fp32(sds_cpu, frames, ctx, ov):
    """(latent trajectory, decoded video) of the oracle pipeline for test_pipeline_fp32_matches_oracle."""
    from oracle import pipeline_ref
    inp = _inputs(frames, 8)
    traj = []
    with torch.no_grad():
        want = pipeline_ref.pose2vid(sds_cpu["unet"], sds_cpu["refnet"], sds_cpu["pose"], sds_cpu["vae"],
                                     clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"], pose_images=inp["pose"],
                                     audio_tensor=inp["audio"], full_mask=inp["full"], face_mask=inp["face"],
                                     lip_mask=inp["lips"], latents=inp["latents"], num_inference_steps=4, guidance_scale=3.5,
                                     motion_scale=[1.0, 1.0, 2.0], context_frames=ctx, context_overlap=ov, trajectory=traj)
    return {"traj": traj, "want": want}


def oracle_pipeline_bf16_floor(sds_cpu):
    """(fp32 oracle final latents, |CPU-bf16 oracle - fp32 oracle|) for test_pipeline_bf16_within_measured_noise_floor."""
    from oracle import pipeline_ref
    inp = _inputs(8, 8)
    kw = dict(clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"], pose_images=inp["pose"],
              audio_tensor=inp["audio"], full_mask=inp["full"], face_mask=inp["face"], lip_mask=inp["lips"],
              latents=inp["latents"], num_inference_steps=4, guidance_scale=3.5, motion_scale=[1.0, 1.0, 2.0], decode=False)
    with torch.no_grad():
        want = pipeline_ref.pose2vid(sds_cpu["unet"], sds_cpu["refnet"], sds_cpu["pose"], sds_cpu["vae"], **kw)
        floor = (pipeline_ref.pose2vid(sds_cpu["unet"], sds_cpu["refnet"], sds_cpu["pose"], sds_cpu["vae"],
                                       unet_dtype=torch.bfloat16, **kw) - want).abs()
    return {"want": want, "floor": floor}


def oracle_long_video(sds_cpu):
    """Latent trajectory of the oracle for test_long_video_96_frames_six_wrapping_windows (L = 96, 2 steps)."""
    from oracle import pipeline_ref
    inp = _inputs(96, 8)
    traj = []
    with torch.no_grad():
        pipeline_ref.pose2vid(sds_cpu["unet"], sds_cpu["refnet"], sds_cpu["pose"], sds_cpu["vae"],
                              clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"], pose_images=inp["pose"],
                              audio_tensor=inp["audio"], full_mask=inp["full"], face_mask=inp["face"], lip_mask=inp["lips"],
                              latents=inp["latents"], num_inference_steps=2, guidance_scale=3.5,
                              motion_scale=[1.0, 1.0, 2.0], context_frames=24, context_overlap=8, decode=False,
                              trajectory=traj)
    return {"traj": traj}


def oracle_pipeline_320px(sds_cpu):
    """Latent trajectory of the fp32 oracle pipeline at 320 x 320 px x 5 frames, 2 DDIM steps, and the two scalars of its CPU-bf16 floor on
    the final latents (max and mean of |denoiser under CPU bf16 - fp32|), for the two tests at that size."""
    from oracle import pipeline_ref
    from tests import geometry_cases as gx
    inp = _inputs(gx.PIPELINE_320["frames"], gx.PIPELINE_320["latent"])
    kw = dict(clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"], pose_images=inp["pose"], audio_tensor=inp["audio"],
              full_mask=inp["full"], face_mask=inp["face"], lip_mask=inp["lips"], latents=inp["latents"],
              num_inference_steps=gx.PIPELINE_320["steps"], guidance_scale=3.5, motion_scale=[1.0, 1.0, 2.0], decode=False)
    traj = []
    with torch.no_grad():
        want = pipeline_ref.pose2vid(sds_cpu["unet"], sds_cpu["refnet"], sds_cpu["pose"], sds_cpu["vae"], trajectory=traj, **kw)
        floor = (pipeline_ref.pose2vid(sds_cpu["unet"], sds_cpu["refnet"], sds_cpu["pose"], sds_cpu["vae"],
                                       unet_dtype=torch.bfloat16, **kw) - want).abs()
    return {"traj": traj, "floor_max": floor.max(), "floor_mean": floor.mean()}


def _build(sds, dtype):
    from mmgt_amd.pipeline import Pose2VideoPipeline
    from mmgt_amd.reference_unet import UNet2DConditionModel
    from mmgt_amd.scheduler import DDIMScheduler
    from mmgt_amd.side_models import PoseGuider
    from mmgt_amd.unet3d import UNet3DConditionModel
    from mmgt_amd.vae import AutoencoderKL
    dev = "cuda:0"
    unet = UNet3DConditionModel(device=dev, dtype=dtype)
    unet.load_state_dict(sds["unet"])
    unet.enable_gradient_checkpointing()
    ref = UNet2DConditionModel(device=dev, dtype=dtype)
    ref.load_state_dict(sds["refnet"])
    pg = PoseGuider(320, block_out_channels=(16, 32, 96, 256), device=dev, dtype=dtype)
    pg.load_state_dict(sds["pose"])
    vae = AutoencoderKL(device=dev, dtype=dtype)
    vae.load_state_dict(sds["vae"])
    return Pose2VideoPipeline(vae=vae, image_encoder=None, reference_unet=ref, denoising_unet=unet, pose_guider=pg,
                              scheduler=DDIMScheduler())


@pytest.mark.parametrize("frames,ctx,ov", [(8, 12, 4), (14, 8, 2)])
def test_pipeline_fp32_matches_oracle(weights, frames, ctx, ov):
    sds, sds_cpu = weights
    inp = _inputs(frames, 8)
    ref = cached(f"pipeline_fp32_{frames}_{ctx}_{ov}", lambda: oracle_pipeline_fp32(sds_cpu, frames, ctx, ov))
    traj, want = ref["traj"], ref["want"]
    pipe = _build(sds, torch.float32)
    got_traj = []
    out = pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, frames, 4, 3.5,
               motion_scale=[1.0, 1.0, 2.0], context_frames=ctx, context_overlap=ov, latents=inp["latents"],
               clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"],
               callback=lambda i, t, lat: got_traj.append(lat.cpu().clone()))
    assert len(got_traj) == 4
    for a, b in zip(got_traj, traj):
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-4)           # latent trajectory, every DDIM step
    assert out.videos.shape == (1, 3, frames, 64, 64)
    torch.testing.assert_close(out.videos, want, rtol=1e-3, atol=2e-4)


def test_pipeline_bf16_within_measured_noise_floor(weights):
    """bf16 product mode, 4 DDIM steps: final latents against the fp32 oracle, gated at 1.5x the error the SAME oracle makes
    when its denoiser runs under PyTorch CPU bf16 on the same inputs (measured here, not quoted)."""
    sds, sds_cpu = weights
    inp = _inputs(8, 8)
    ref = cached("pipeline_bf16_floor", lambda: oracle_pipeline_bf16_floor(sds_cpu))
    want, floor = ref["want"], ref["floor"]
    pipe = _build(sds, torch.bfloat16)
    got = pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, 8, 4, 3.5,
               motion_scale=[1.0, 1.0, 2.0], latents=inp["latents"], clip_image_embeds=inp["clip"],
               ref_image_latents=inp["ref_lat"], decode=False).videos.cpu()
    d = (got - want).abs()
    print(f"bf16 pipeline final latents: HIP max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e}; CPU-bf16 floor max "
          f"{floor.max().item():.3e} mean {floor.mean().item():.3e}; mean|x| {want.abs().mean().item():.3f}")
    assert torch.isfinite(got).all()
    assert d.max() <= 1.5 * floor.max() and d.mean() <= 1.5 * floor.mean()


def _run_320px(sds, dtype, callback=None):
    from tests import geometry_cases as gx
    g = gx.PIPELINE_320
    inp = _inputs(g["frames"], g["latent"])
    pipe = _build(sds, dtype)
    return pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 8 * g["latent"], 8 * g["latent"], g["frames"],
                g["steps"], 3.5, motion_scale=[1.0, 1.0, 2.0], latents=inp["latents"], clip_image_embeds=inp["clip"],
                ref_image_latents=inp["ref_lat"], decode=False, callback=callback).videos.cpu()


def test_pipeline_320px_fp32_matches_oracle(weights):
    """320 x 320 px x 5 frames, 2 DDIM steps, fp32 mode: the PoseGuider's stride-2 chain from 320 x 320 pixels, the ReferenceNet hand-off at
    1600 / 400 / 100 / 25 bank keys, one 5-frame window through the accumulate + CFG + DDIM step at 40 x 40 -- the latent trajectory of
    every step against the oracle pipeline at the north-star tolerance."""
    from tests import geometry_cases as gx
    sds, sds_cpu = weights
    traj = cached("pipeline_320px", lambda: oracle_pipeline_320px(sds_cpu))["traj"]
    got = []
    out = _run_320px(sds, torch.float32, callback=lambda i, t, lat: got.append(lat.cpu().clone()))
    assert len(got) == len(traj) == gx.PIPELINE_320["steps"]
    for i, (a, b) in enumerate(zip(got, traj)):
        print(f"320 px fp32 pipeline, step {i}: max|d| {(a - b).abs().max().item():.3e} mean|x| {b.abs().mean().item():.3f}")
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(out, traj[-1], rtol=1e-3, atol=1e-4)


def test_pipeline_320px_bf16_within_measured_noise_floor(weights):
    """The same run in bf16 product mode: final latents within 1.5x the error of the oracle pipeline with its denoiser under CPU bf16."""
    sds, sds_cpu = weights
    ref = cached("pipeline_320px", lambda: oracle_pipeline_320px(sds_cpu))
    want, fmax, fmean = ref["traj"][-1], ref["floor_max"].item(), ref["floor_mean"].item()
    got = _run_320px(sds, torch.bfloat16)
    d = (got - want).abs()
    print(f"320 px bf16 pipeline final latents: HIP max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e}; CPU-bf16 floor max "
          f"{fmax:.3e} mean {fmean:.3e}; mean|x| {want.abs().mean().item():.3f}")
    assert torch.isfinite(got).all()
    assert d.max() <= 1.5 * fmax and d.mean() <= 1.5 * fmean


def test_long_video_96_frames_six_wrapping_windows(weights):
    """BASELINE config 5 at its real window geometry (L = 96, context 24, overlap 8 => 6 closed-loop windows, the last one
    wrapping 80..7; context.py:15-42, pipeline_pose2vid_long.py:522-635) at 64x64 px, 2 DDIM steps, fp32 mode against the
    oracle's latent trajectory.  The same run through the window-parallel branch (1-rank group, CFG rows split: 12 units)
    must agree with it to fp32 rounding."""
    import os
    import torch.distributed as dist
    from mmgt_amd.context import uniform
    sds, sds_cpu = weights
    L = 96
    wins = list(uniform(0, 2, L, 24, 1, 8))
    assert len(wins) == 6 and wins[-1][0] == 80 and wins[-1][-1] == 7
    inp = _inputs(L, 8)
    traj = cached("long_video_96", lambda: oracle_long_video(sds_cpu))["traj"]
    pipe = _build(sds, torch.float32)
    kw = dict(motion_scale=[1.0, 1.0, 2.0], context_frames=24, context_overlap=8, latents=inp["latents"],
              clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"], decode=False)
    got = []
    pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, L, 2, 3.5,
         callback=lambda i, t, lat: got.append(lat.cpu().clone()), **kw)
    assert len(got) == 2
    for a_, b_ in zip(got, traj):
        torch.testing.assert_close(a_, b_, rtol=1e-3, atol=1e-4)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29400 + os.getpid() % 500))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        par = pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, L, 2, 3.5,
                   window_group=True, cfg_split=True, **kw).videos.cpu()
    finally:
        dist.destroy_process_group()
    torch.testing.assert_close(par, traj[-1], rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(par, got[-1], rtol=1e-5, atol=1e-6)


def test_long_video_config5_at_full_size_512x512x96(weights):
    """BASELINE config 5 at its STATED size on one GPU: 512x512 px, L = 96, context 24, overlap 8 => 6 windows per DDIM step (the
    last one wrapping), bf16 product mode, 2 steps (pipeline_pose2vid_long.py:522-635).  No oracle finishes this size in test
    time, so the checks are the size-independent ones: finite latents, bitwise reproducible run to run, and the window-parallel
    branch (1-rank group, CFG rows split into 12 half-units per step) equal to the serial loop to bf16-kernel rounding: the
    half-batch forwards take other GEMM tile shapes, so the sums are re-associated, not the algorithm."""
    import os
    import time
    import torch.distributed as dist
    from mmgt_amd.context import uniform
    sds, _ = weights
    L, lat = 96, 64
    assert len(list(uniform(0, 2, L, 24, 1, 8))) == 6
    inp = _inputs(L, lat)
    pipe = _build(sds, torch.bfloat16)
    kw = dict(motion_scale=[1.0, 1.0, 2.0], context_frames=24, context_overlap=8, latents=inp["latents"],
              clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"], decode=False)
    run = lambda steps=2, g=3.5, **k: pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 512, 512, L, steps, g, **kw, **k).videos
    a = run()
    torch.cuda.synchronize()
    t0 = time.time()
    b_ = run()
    torch.cuda.synchronize()
    print(f"config 5 (512x512x96, 6 windows/step), 2 steps incl. prologue: {time.time() - t0:.2f} s")
    assert a.shape == (1, 4, L, lat, lat) and torch.isfinite(a).all()
    assert torch.equal(a, b_), "512x512x96 sampler is not bitwise reproducible"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29400 + os.getpid() % 500))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        par = run(window_group=True, cfg_split=True)
        # The tight gate: ONE step at guidance 1 (+ 2^-20: the reference loop insists on > 1) from t = 999, where the DDIM update
        # returns x0 = -v: the latents ARE the (negated) predictions, no amplification.  The 12 (window, CFG row) units run single-row
        # forwards (other GEMM tiles, no shared-row / twin paths), so against the batched forwards of the serial loop they are a second
        # bf16 evaluation of the same function: the two must agree within the measured bf16 noise floor of this operator at this shape
        # (tests/golden/unet3d_full_cfg2_bf16floor.npz: max 2.2e-2, mean 3.5e-3 against fp32) in EVERY frame of every window -- a wrong
        # window weight, a frame off by one in one of the six windows or a swapped CFG row is an O(0.1 .. 1) difference.
        one_serial = run(1, 1.0 + 2.0 ** -20)
        one_split = run(1, 1.0 + 2.0 ** -20, window_group=True, cfg_split=True)
    finally:
        dist.destroy_process_group()
    import numpy as np
    fl = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet3d_full_cfg2_bf16floor.npz"))
    fmax, fmean = float(fl["max_abs"]), float(fl["mean_abs"])
    d1 = (one_split.float() - one_serial.float()).abs()
    per_frame = d1.mean(dim=(0, 1, 3, 4))
    print(f"one step at guidance 1, cfg_split units vs serial: max|d| {d1.max().item():.3e} mean {d1.mean().item():.3e} (bf16 floor {fmax:.3e} / "
          f"{fmean:.3e}); per-frame mean {per_frame.min().item():.3e} .. {per_frame.max().item():.3e}")
    assert d1.max() <= 1.5 * fmax and d1.mean() <= 1.5 * fmean and per_frame.max() <= 2.0 * fmean
    d = (par.float() - a.float()).abs()
    print(f"cfg_split path vs serial at 512x512x96: max|d| {d.max().item():.3e} mean {d.mean().item():.3e} on mean|x| {a.abs().mean().item():.3f}")
    # measured: mean 2.4 % of mean|x|, max 3.5 % of the range after 2 guided steps (guidance 3.5 amplifies the per-forward bf16
    # re-association noise); a wrong window / CFG row / counter would be O(1)
    assert torch.isfinite(par).all() and d.mean() <= 6e-2 * a.abs().mean() and d.max() <= 0.25 * a.abs().max()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_operator_single_cfg_row_equals_batched_rows(weights, dtype):
    """denoise_window(cfg_row=r) on one CFG row == row r of the CFG-batched call: the unconditional row never reads the
    banks, the conditional row reads bank row 1 in every frame (mutual_self_attention.py:150-188)."""
    from mmgt_amd.unet3d import UNet3DConditionModel
    from tests import golden_cases as gc
    sds, _ = weights
    case = dict(gc.UNET_CASES["full_cfg1"], frames=3)
    inp = gc.unet_inputs(case)
    mv = lambda t: t.cuda()
    m = UNet3DConditionModel(device="cuda:0", dtype=dtype)
    m.load_state_dict(sds["unet"])
    m.enable_gradient_checkpointing()
    m.set_banks({k: mv(v) for k, v in inp["banks"].items()})
    f = case["frames"]
    both = m.denoise_window(mv(inp["sample"]), 499, mv(inp["ehs"]), mv(inp["audio"]), mv(inp["pose"]),
                            [mv(x) for x in inp["full"]], [mv(x) for x in inp["face"]], [mv(x) for x in inp["lips"]],
                            inp["motion_scale"])[..., :4].float()
    for row in (0, 1):
        cut = lambda L: [mv(x).view(2, f, -1)[row].contiguous() for x in L]
        one = m.denoise_window(mv(inp["sample"][row:row + 1]), 499, mv(inp["ehs"]), mv(inp["audio"][row:row + 1]),
                               mv(inp["pose"][row:row + 1]), cut(inp["full"]), cut(inp["face"]), cut(inp["lips"]),
                               inp["motion_scale"], cfg_row=row)[..., :4].float()
        # same arithmetic per row; the GEMM tile choice may differ with M, which only reorders nothing today (bit-equal), but
        # the gate allows a couple of bf16 ulps so that a future tile with another MFMA shape stays legal
        tol = dict(rtol=1e-5, atol=1e-6) if dtype == torch.float32 else dict(rtol=1.6e-2, atol=2e-3)
        torch.testing.assert_close(one, both[row * f:(row + 1) * f], **tol)


def test_window_parallel_group_path_equals_serial_loop(weights):
    """SURVEY 8e config 5 on the device: the window-parallel branch (RCCL all-gather per round; here a 1-rank group, the
    multi-rank dealing is covered by the gloo test) leaves the latents bit-identical to the serial window loop."""
    import os
    import torch.distributed as dist
    sds, _ = weights
    inp = _inputs(14, 8)
    pipe = _build(sds, torch.bfloat16)
    kw = dict(motion_scale=[1.0, 1.0, 2.0], context_frames=8, context_overlap=2, latents=inp["latents"],
              clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"])
    serial = pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, 14, 2, 3.5, **kw).videos
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29400 + os.getpid() % 500))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        par = pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, 14, 2, 3.5,
                   window_group=True, **kw).videos
    finally:
        dist.destroy_process_group()
    assert torch.equal(serial, par)
