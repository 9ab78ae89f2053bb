"""The HIP denoise-step operator (mmgt_amd.UNet3DConditionModel, through the C ABI) against the oracle on identical
weights, latents and conditioning.

  * fp32-I/O mode: rtol 1e-3 / atol 1e-4 (the north-star tolerance) at BASELINE config-1 geometry, full width, and at the
    benchmarked BASELINE config-2 shape (512x512x24) against the REFERENCE's own output (G4 golden).
  * bf16 mode: no bf16 implementation of this 1.4 B-parameter network meets 1e-3 / 1e-4 against an fp32 reference, so it is
    gated against the MEASURED bf16 noise floor: the oracle run under PyTorch CPU bf16 on the same inputs (inside the test
    at config-1 size; at 512x512 the floor is the committed tools/gen_bf16_floor.py measurement at the full shape).  The HIP
    bf16 max|d| and mean|d| must stay within 1.5x that floor.
  * between those two sizes (48-, 24- and 40-wide latents, tests/geometry_cases.py) both modes again, the bf16 floor measured by the
    oracle at each case, and the launches of a bf16 forward counted against the restated gates.
"""
import os

import numpy as np
import pytest
import torch

from tests.oracle_cache import cached  # noqa: E402

pytestmark = pytest.mark.gpu

from mmgt_amd.synthetic import synth_state_dict  # noqa: E402
from oracle import unet3d_ref as R  # noqa: E402
from tests import geometry_cases as gx  # noqa: E402
from tests import golden_cases as gc  # noqa: E402


@pytest.fixture(scope="module")
def full_sd():
    from mmgt_amd.unet3d_spec import unet3d_spec
    sd_gpu = synth_state_dict(unet3d_spec(), device="cuda:0")
    sd_cpu = {k: v.cpu() for k, v in sd_gpu.items()}
    return sd_gpu, sd_cpu


def _to_dev(inp):
    mv = lambda t: t.cuda() if torch.is_tensor(t) else t
    out = {k: ([mv(x) for x in v] if isinstance(v, list) and torch.is_tensor(v[0]) else mv(v)) for k, v in inp.items()
           if k != "banks"}
    out["banks"] = {k: v.cuda() for k, v in inp["banks"].items()}
    return out


def _run_hip(sd_gpu, case, dtype, weighted=True):
    from mmgt_amd.unet3d import UNet3DConditionModel
    m = UNet3DConditionModel(device="cuda:0", dtype=dtype)
    m.load_state_dict(sd_gpu)
    if weighted:
        m.enable_gradient_checkpointing()          # scripts/pose2vid.py:183-184
    else:
        m.eval()
    inp = _to_dev(gc.unet_inputs(case))
    m.set_banks(inp["banks"])
    out = m(inp["sample"], inp["timestep"], encoder_hidden_states=inp["ehs"], audio_embedding=inp["audio"],
            pose_cond_fea=inp["pose"], full_mask=inp["full"], face_mask=inp["face"], body_mask=inp["lips"],
            motion_scale=inp["motion_scale"], return_dict=False)[0]
    torch.cuda.synchronize()
    return out.float().cpu()


def _run_oracle(sd_cpu, case, weighted=True, dtype=torch.float32):
    """dtype=bfloat16: every weight and activation of the oracle in bf16 (PyTorch CPU kernels) = the measured noise floor."""
    cfg = R.UNet3DConfig()
    inp = gc.unet_inputs(case)
    c = (lambda t: t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t) if dtype != torch.float32 else (lambda t: t)
    cl = lambda L: [c(x) for x in L]
    sd = sd_cpu if dtype == torch.float32 else {k: c(v) for k, v in sd_cpu.items()}
    with torch.no_grad():
        return R.unet3d_forward(sd, cfg, c(inp["sample"]), inp["timestep"], c(inp["ehs"]), c(inp["audio"]), c(inp["pose"]),
                                cl(inp["full"]), cl(inp["face"]), cl(inp["lips"]), inp["motion_scale"],
                                {k: c(v) for k, v in inp["banks"].items()}, weighted=weighted).float()


FLOOR_SLACK = 1.5      # HIP bf16 error <= 1.5 x the measured CPU-bf16 error of the same oracle on the same inputs


def _floor_cfg2(golden_dir):
    f = np.load(os.path.join(golden_dir, "unet3d_full_cfg2_bf16floor.npz"))
    return float(f["max_abs"]), float(f["mean_abs"])


def test_unet_fp32_mode_matches_oracle_config1(full_sd):
    sd_gpu, sd_cpu = full_sd
    case = gc.UNET_CASES["full_cfg1"]
    ref = _run_oracle(sd_cpu, case)
    out = _run_hip(sd_gpu, case, torch.float32)
    print("fp32 mode: max|d|", (out - ref).abs().max().item(), "mean|x|", ref.abs().mean().item())
    torch.testing.assert_close(out, ref, rtol=1e-3, atol=1e-4)


def test_unet_bf16_forward_is_bitwise_reproducible(full_sd):
    """No atomics, fixed-order reductions, deterministic tile schedules: two forwards of the whole UNet on the same inputs are
    bitwise identical (a race in any kernel's staging would show here as well as in the parity gates)."""
    sd_gpu, _ = full_sd
    case = gc.UNET_CASES["full_cfg1"]
    a = _run_hip(sd_gpu, case, torch.bfloat16)
    b = _run_hip(sd_gpu, case, torch.bfloat16)
    assert torch.equal(a, b)


def test_unet_window_state_keeps_step_invariant_work(full_sd):
    """denoise_window(window_state=...): the audio K / V projections and the MM-HAA mask rows are derived once per window and kept in the
    CALLER's dict; later steps reuse them -- bitwise the stateless result, at a different timestep too -- and a different window's inputs
    with their own dict are not affected."""
    from mmgt_amd.unet3d import UNet3DConditionModel
    sd_gpu, _ = full_sd
    m = UNet3DConditionModel(device="cuda:0", dtype=torch.bfloat16)
    m.load_state_dict(sd_gpu)
    m.enable_gradient_checkpointing()
    inp = _to_dev(gc.unet_inputs(gc.UNET_CASES["full_cfg1"]))
    m.set_banks(inp["banks"])

    def run(ts, audio, state):
        return m.denoise_window(inp["sample"], ts, inp["ehs"], audio, inp["pose"], inp["full"], inp["face"], inp["lips"],
                                inp["motion_scale"], window_state=state).clone()
    t0, t1 = inp["timestep"], inp["timestep"] * 0 + 321
    state = {}
    first = run(t0, inp["audio"], state)
    assert any(k[0] == "kv3" for k in state) and any(k[0] == "mask_rows" for k in state)
    assert torch.equal(first, run(t0, inp["audio"], None))
    assert torch.equal(run(t1, inp["audio"], state), run(t1, inp["audio"], None))
    other = inp["audio"] * 0.5                                        # another window: its own dict
    assert torch.equal(run(t0, other, {}), run(t0, other, None))
    assert not torch.equal(run(t0, other, None), first)


def test_unet_zero_audio_rows_are_skipped_exactly(full_sd):
    """audio_zero_rows = 1 (the unconditional CFG row, whose audio embedding the reference sets to zeros): that row's audio cross-attention is
    exactly zero, so not computing it gives bitwise the result of computing it -- in the CFG pair and for the rows run alone (cfg_row)."""
    from mmgt_amd.unet3d import UNet3DConditionModel
    sd_gpu, _ = full_sd
    m = UNet3DConditionModel(device="cuda:0", dtype=torch.bfloat16)
    m.load_state_dict(sd_gpu)
    m.enable_gradient_checkpointing()
    inp = _to_dev(gc.unet_inputs(gc.UNET_CASES["full_cfg1"]))
    m.set_banks(inp["banks"])
    audio = inp["audio"].clone()
    assert audio.shape[0] == 2
    audio[0] = 0

    def run(zero_rows, **kw):
        return m.denoise_window(inp["sample"], inp["timestep"], inp["ehs"], audio, inp["pose"], inp["full"], inp["face"], inp["lips"],
                                inp["motion_scale"], audio_zero_rows=zero_rows, **kw).clone()
    full = run(0)
    assert torch.equal(run(1), full)
    assert torch.equal(run(1, window_state={}), full)
    f = inp["sample"].shape[2]
    half = lambda t: t.view(2, f, -1)[0].contiguous()
    row0 = dict(sample=inp["sample"][:1], audio=audio[:1], pose=inp["pose"][:1], full=[half(t) for t in inp["full"]],
                face=[half(t) for t in inp["face"]], lips=[half(t) for t in inp["lips"]])

    def run_row0(zero_rows):
        return m.denoise_window(row0["sample"], inp["timestep"], inp["ehs"], row0["audio"], row0["pose"], row0["full"], row0["face"],
                                row0["lips"], inp["motion_scale"], cfg_row=0, audio_zero_rows=zero_rows).clone()
    assert torch.equal(run_row0(1), run_row0(0))
    with pytest.raises(RuntimeError, match="audio_zero_rows"):
        run(3)


def test_unet_cfg_rows_share_input(full_sd):
    """cfg_rows_share_input: with identical latents / pose in both CFG rows, conv_in and the first resnet run once and are duplicated.
    Bitwise the full computation when the convs take the same reduction order (tail split off: 24 frames of rows fill the persistent grid
    differently from 48), at rounding level otherwise."""
    from mmgt_amd import hip
    from mmgt_amd.unet3d import UNet3DConditionModel
    sd_gpu, _ = full_sd
    m = UNet3DConditionModel(device="cuda:0", dtype=torch.bfloat16)
    m.load_state_dict(sd_gpu)
    m.enable_gradient_checkpointing()
    inp = _to_dev(gc.unet_inputs(gc.UNET_CASES["full_cfg1"]))
    m.set_banks(inp["banks"])
    sample = inp["sample"][:1].repeat(2, 1, 1, 1, 1)
    pose = inp["pose"][:1].repeat(2, 1, 1, 1, 1)

    def run(share):
        return m.denoise_window(sample, inp["timestep"], inp["ehs"], inp["audio"], pose, inp["full"], inp["face"], inp["lips"],
                                inp["motion_scale"], cfg_rows_share_input=share).float()
    hip.tune("tailsplit", 0)
    try:
        assert torch.equal(run(True), run(False))       # includes the first reference-attention reader on ONE attention pass (twin)
        m._twin = False
        assert torch.equal(run(True), run(False))
        m._twin = True
    finally:
        hip.tune("tailsplit", 1)
    a, b = run(True), run(False)
    d = (a - b).abs()
    assert d.max() <= 0.05 * b.abs().max() and d.mean() <= 5e-3 * b.abs().mean().clamp_min(1e-3), (d.max().item(), d.mean().item())


def test_unet_fp32_mode_eval_semantics(full_sd):
    """eval() => motion_scale ignored."""
    sd_gpu, sd_cpu = full_sd
    case = gc.UNET_CASES["full_cfg1"]
    ref = _run_oracle(sd_cpu, case, weighted=False)
    out = _run_hip(sd_gpu, case, torch.float32, weighted=False)
    torch.testing.assert_close(out, ref, rtol=1e-3, atol=1e-4)


def test_unet_matches_reference_golden_config1(full_sd, golden_dir):
    """Straight against the REFERENCE's own output (tests/golden/unet3d_full_cfg1.npz)."""
    import numpy as np, os
    sd_gpu, _ = full_sd
    g = torch.from_numpy(np.load(os.path.join(golden_dir, "unet3d_full_cfg1.npz"))["script"])
    out = _run_hip(sd_gpu, gc.UNET_CASES["full_cfg1"], torch.float32)
    torch.testing.assert_close(out, g, rtol=1e-3, atol=1e-4)


def test_unet_bf16_mode_within_measured_noise_floor(full_sd):
    sd_gpu, sd_cpu = full_sd
    case = gc.UNET_CASES["full_cfg1"]
    ref = _run_oracle(sd_cpu, case)
    floor = (_run_oracle(sd_cpu, case, dtype=torch.bfloat16) - ref).abs()
    out = _run_hip(sd_gpu, case, torch.bfloat16)
    d = (out - ref).abs()
    print(f"bf16 mode: HIP max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e}; CPU-bf16 floor max {floor.max().item():.3e} "
          f"mean {floor.mean().item():.3e}; mean|x| {ref.abs().mean().item():.3f}")
    assert torch.isfinite(out).all()
    assert d.max() <= FLOOR_SLACK * floor.max() and d.mean() <= FLOOR_SLACK * floor.mean()


def test_unet_wider_geometry_fp32(full_sd):
    """16x16 latent (128x128 px), 5 frames: exercises multi-tile attention, ragged GEMM tiles and window length != 8."""
    sd_gpu, sd_cpu = full_sd
    case = dict(gc.UNET_CASES["full_cfg1"], frames=5, latent=16, timestep=21)
    ref = _run_oracle(sd_cpu, case)
    out = _run_hip(sd_gpu, case, torch.float32)
    torch.testing.assert_close(out, ref, rtol=1e-3, atol=1e-4)


SIX_FRAME_CASE = dict(gc.UNET_CASES["full_cfg1"], frames=6, latent=64, timestep=499)


def test_unet_full_resolution_512x512_six_frames(full_sd, golden_dir):
    """BASELINE config-2 spatial size (512x512 px = 64x64 latent, 4096 tokens and 4096 bank keys at level 0) on 6 frames:
    the shapes at which the production tile configurations are chosen (128x320 conv tile from 49152 output rows, 256x128
    for the GEGLU / long-K GEMMs, 64-key attention tiles without ragged-tail code).  fp32-I/O mode against the CPU oracle
    at the north-star tolerance, bf16 product mode against the same reference at the bf16 noise floor."""
    sd_gpu, sd_cpu = full_sd
    case = SIX_FRAME_CASE
    ref = cached("unet_512x512_six_frames", lambda: _run_oracle(sd_cpu, case))
    out = _run_hip(sd_gpu, case, torch.float32)
    d = (out - ref).abs()
    print("512x512x6 fp32 mode: max|d|", d.max().item(), "mean|x|", ref.abs().mean().item())
    torch.testing.assert_close(out, ref, rtol=1e-3, atol=1e-4)
    out16 = _run_hip(sd_gpu, case, torch.bfloat16)
    d16 = (out16 - ref).abs()
    fmax, fmean = _floor_cfg2(golden_dir)       # CPU-bf16 floor of the oracle at 512x512 (24 frames: tools/gen_bf16_floor.py)
    print(f"512x512x6 bf16 mode: max|d| {d16.max().item():.3e} mean|d| {d16.mean().item():.3e} (floor {fmax:.3e} / {fmean:.3e})")
    assert torch.isfinite(out16).all()
    assert d16.max() <= FLOOR_SLACK * fmax and d16.mean() <= FLOOR_SLACK * fmean


def test_groupnorm_tables_from_conv_epilogues_512x512_six_frames(full_sd, golden_dir):
    """The GroupNorm tables that come out of a fused conv's epilogue (csrc/rconv.hip: conv1 -> the resnet's norm2, conv2 -> the `norm` of
    the transformer block that reads the resnet's output) against the same forward with a statistics pass over every tensor
    (`rconv_stats` = 0): both within the bf16 floor of the oracle, and the folds must have been the path taken (counted: 10 resnets on
    the fused launch + the 5 level-0 transformer norms)."""
    from mmgt_amd import hip
    sd_gpu, sd_cpu = full_sd
    case = SIX_FRAME_CASE
    ref = cached("unet_512x512_six_frames", lambda: _run_oracle(sd_cpu, case))
    fmax, fmean = _floor_cfg2(golden_dir)
    n0 = hip.call_count("mmgt_gn_stats_finalize_unet")
    out = _run_hip(sd_gpu, case, torch.bfloat16)
    folds = hip.call_count("mmgt_gn_stats_finalize_unet") - n0
    assert folds == 15, f"{folds} GroupNorm tables came from conv epilogues (15 expected)"
    try:
        hip.tune("rconv_stats", 0)
        n0 = hip.call_count("mmgt_gn_stats_finalize_unet")
        passes = _run_hip(sd_gpu, case, torch.bfloat16)
        assert hip.call_count("mmgt_gn_stats_finalize_unet") == n0
    finally:
        hip.tune("rconv_stats", 1)
    for o in (out, passes):
        d = (o - ref).abs()
        assert d.max() <= FLOOR_SLACK * fmax and d.mean() <= FLOOR_SLACK * fmean
    d = (out - passes).abs()
    print(f"epilogue statistics against passes: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e}")
    assert d.mean() <= fmean


FUSED_BLOCKS = ("down_blocks.0.", "down_blocks.2.", "up_blocks.1.", "up_blocks.3.")    # 64 x 64 and 16 x 16 pixels, 320 and 1280 wide: 10 resnets


def _rimg_keys(model):
    return {k for k in model.w if k.endswith(".rimg")}


def _fused_leg_keys(model):
    return {r + cv + ".rimg" for r in model._resnets if r.startswith(FUSED_BLOCKS) for cv in (".conv1", ".conv2")}


def _six_frame_model(sd_gpu):
    from mmgt_amd.unet3d import UNet3DConditionModel
    m = UNet3DConditionModel(device="cuda:0", dtype=torch.bfloat16)
    m.load_state_dict(sd_gpu)
    m.enable_gradient_checkpointing()
    inp = _to_dev(gc.unet_inputs(SIX_FRAME_CASE))
    m.set_banks(inp["banks"])
    run = lambda: m(inp["sample"], inp["timestep"], encoder_hidden_states=inp["ehs"], audio_embedding=inp["audio"], pose_cond_fea=inp["pose"],
                    full_mask=inp["full"], face_mask=inp["face"], body_mask=inp["lips"], motion_scale=inp["motion_scale"], return_dict=False)[0]
    return m, run


def test_fused_leg_images_exist_where_a_forward_read_them_512x512_six_frames(full_sd):
    """The weight images of the fused GroupNorm -> SiLU -> conv3x3 legs (csrc/rconv.hip) are built by the first forward that runs the leg: none
    after load_state_dict, then conv1 and conv2 of exactly the ten resnets whose level is in the `rconv` mask and whose pixels tile into
    16 x 16 (the 8 x 8 level never does at 64 x 64 latents), one fused launch each; a second forward builds nothing and repeats the first bit
    for bit; a repeated load drops the images of the previous weights."""
    from mmgt_amd import hip
    sd_gpu, _ = full_sd
    m, run = _six_frame_model(sd_gpu)
    assert not _rimg_keys(m)
    n0 = hip.call_count("mmgt_gn_silu_conv3x3_unet")
    first = run()
    launches = hip.call_count("mmgt_gn_silu_conv3x3_unet") - n0
    want = _fused_leg_keys(m)
    assert len(want) == 20 and _rimg_keys(m) == want
    assert launches == 20, f"{launches} fused launches in one forward (20 expected: 10 resnets x 2 legs)"
    assert torch.equal(run(), first) and _rimg_keys(m) == want
    m.load_state_dict(sd_gpu)
    assert not _rimg_keys(m)


def test_fused_leg_switched_off_builds_no_image(full_sd):
    """`rconv` = 0, read once by the constructor: no fused launch and no image."""
    from mmgt_amd import hip
    sd_gpu, _ = full_sd
    mask = hip.tune_get("rconv")
    try:
        hip.tune("rconv", 0)
        m, run = _six_frame_model(sd_gpu)
    finally:
        hip.tune("rconv", mask)
    n0 = hip.call_count("mmgt_gn_silu_conv3x3_unet")
    assert torch.isfinite(run()).all()
    assert hip.call_count("mmgt_gn_silu_conv3x3_unet") == n0 and not _rimg_keys(m)


def test_reference_net_builds_fused_leg_images_for_its_fused_resnets_only():
    """The ReferenceNet shares the UNet's blocks: after `write_banks` at 64 x 64 latents its images are those of the same ten resnets."""
    from mmgt_amd.reference_unet import UNet2DConditionModel
    from mmgt_amd.synthetic import hash_uniform
    from mmgt_amd.unet3d_spec import unet2d_reference_spec
    m = UNet2DConditionModel(device="cuda:0", dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(unet2d_reference_spec(), device="cuda:0"))
    assert not _rimg_keys(m)
    bank = m.write_banks(hash_uniform("refnet.lat", (2, 4, 64, 64), 1.0).cuda(), 0, hash_uniform("refnet.ehs", (2, 1, 768), 1.0).cuda())
    assert len(bank) == 16 and all(torch.isfinite(v).all() for v in bank.values())
    want = _fused_leg_keys(m)
    assert len(want) == 20 and _rimg_keys(m) == want


TWELVE_FRAME_CASE = dict(gc.UNET_CASES["full_cfg1"], frames=12, latent=64, timestep=499)


def test_unet_shipped_window_512x512_twelve_frames(full_sd, golden_dir):
    """The reference's SHIPPED window (`context_frames=12`: /root/reference/src/pipelines/pipeline_pose2vid_long.py:360-362) at the benchmarked
    spatial size: M = 98 304 token rows at level 0 -- `tleg320_kernel<12>` (4 pixels x 12 frames per wave), the 192-row `gemm16` tiles and
    every dispatcher branch that differs from the 24-frame shape.  fp32-I/O mode against the CPU oracle at the north-star tolerance; bf16
    product mode within 1.5x the CPU-bf16 floor; the fused temporal leg must have been the path taken (its launch count is read back), and
    the three-launch form of the same legs must agree with it at the rounding level of the floor."""
    from mmgt_amd import hip
    sd_gpu, sd_cpu = full_sd
    case = TWELVE_FRAME_CASE
    ref = cached("unet_512x512_twelve_frames", lambda: _run_oracle(sd_cpu, case))
    out = _run_hip(sd_gpu, case, torch.float32)
    d = (out - ref).abs()
    print("512x512x12 fp32 mode: max|d|", d.max().item(), "mean|x|", ref.abs().mean().item())
    torch.testing.assert_close(out, ref, rtol=1e-3, atol=1e-4)
    del out
    fmax, fmean = _floor_cfg2(golden_dir)
    n0 = hip.call_count("mmgt_temporal_leg320")
    out16 = _run_hip(sd_gpu, case, torch.bfloat16)
    legs = hip.call_count("mmgt_temporal_leg320") - n0
    assert legs == 10, f"the fused temporal leg ran {legs} times in a 12-frame forward (5 level-0 motion modules x 2 legs expected)"
    d16 = (out16 - ref).abs()
    print(f"512x512x12 bf16 mode: max|d| {d16.max().item():.3e} mean|d| {d16.mean().item():.3e} (floor {fmax:.3e} / {fmean:.3e})")
    assert torch.isfinite(out16).all()
    assert d16.max() <= FLOOR_SLACK * fmax and d16.mean() <= FLOOR_SLACK * fmean
    assert torch.equal(_run_hip(sd_gpu, case, torch.bfloat16), out16)
    try:
        hip.tune("tleg", 0)
        n0 = hip.call_count("mmgt_temporal_leg320")
        three = _run_hip(sd_gpu, case, torch.bfloat16)
        assert hip.call_count("mmgt_temporal_leg320") == n0
    finally:
        hip.tune("tleg", 1)
    d3 = (three - ref).abs()
    assert d3.max() <= FLOOR_SLACK * fmax and d3.mean() <= FLOOR_SLACK * fmean
    assert not torch.equal(three, out16)            # two different computations of the same legs


def test_unet_benchmarked_shape_512x512x24_matches_reference_golden(full_sd, golden_dir):
    """G4: BASELINE config 2 = exactly what bench.py times -- latent (2,4,24,64,64), M = 196608 token rows at
    level 0, the tile choices that only trigger at 24 frames.  The fixture is a strided sub-sample + moments of the
    REFERENCE's own fp32 output (tools/refgen/gen_golden.py --only full_cfg2: 233 s of the reference's UNet3DConditionModel
    on the build container's CPU); the oracle agrees with that full tensor to max|d| 4.5e-6.
    fp32-I/O mode at the north-star tolerance; bf16 product mode within 1.5x the CPU-bf16 floor measured at this shape."""
    sd_gpu, _ = full_sd
    case = gc.UNET_CASES["full_cfg2"]
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "unet3d_full_cfg2.npz")).items()}
    out = _run_hip(sd_gpu, case, torch.float32)
    assert out.shape == (2, 4, 24, 64, 64)
    got = gc.g4_summary(out)
    d = (got["sub"] - g["sub"]).abs()
    print(f"512x512x24 fp32 mode vs reference golden: max|d| {d.max().item():.3e} over {d.numel()} samples")
    torch.testing.assert_close(got["sub"], g["sub"], rtol=1e-3, atol=1e-4)
    for k in ("mean_bc", "std_bc", "absmax_bc", "mean_bf", "std_bf", "mean_abs"):
        torch.testing.assert_close(got[k], g[k], rtol=1e-3, atol=1e-4)
    del out
    out16 = _run_hip(sd_gpu, case, torch.bfloat16)
    d16 = (gc.g4_summary(out16)["sub"] - g["sub"]).abs()
    fmax, fmean = _floor_cfg2(golden_dir)
    print(f"512x512x24 bf16 mode vs reference golden: max|d| {d16.max().item():.3e} mean|d| {d16.mean().item():.3e} "
          f"(CPU-bf16 floor {fmax:.3e} / {fmean:.3e})")
    assert torch.isfinite(out16).all()
    assert d16.max() <= FLOOR_SLACK * fmax and d16.mean() <= FLOOR_SLACK * fmean
    # the production configuration twice: bitwise reproducible (persistent workgroups walking many tiles, 64-query attention)
    assert torch.equal(_run_hip(sd_gpu, case, torch.bfloat16), out16)


def test_mmhaa_merged_bias_term_keeps_fp32_accuracy_with_blurred_masks(full_sd):
    """in the merged MM-HAA out-projection the term sum_i mask_i s_i (Wz_i b_o,i) met a bf16-rounded mask and a bf16-rounded
    bias (2^-8 relative) where the three-launch path multiplies fp32 by fp32.  With the head / tail columns the bf16 GEMM of the bias
    columns alone (what a zero-audio row consists of) reproduces the fp32 product to ~2^-15 of its scale, for non-binary masks."""
    from mmgt_amd import hip
    from mmgt_amd.unet3d import UNet3DConditionModel, mask_bias_columns
    sd_gpu, _ = full_sd
    m = UNet3DConditionModel(device="cuda:0", dtype=torch.bfloat16)
    m.load_state_dict(sd_gpu)
    t = m._audio[0] + ".transformer_blocks.0"
    wb = m.w[t + ".oz3.wb"]
    g = torch.Generator(device="cuda").manual_seed(11)
    rows = 4096
    masks = torch.rand((3, rows), device="cuda", generator=g) ** 2               # blurred: anything in [0, 1], not 8-bit values
    scales = torch.tensor([1.0, 1.0, 2.0], device="cuda")
    rs = (masks * scales[:, None]).contiguous()
    cols = mask_bias_columns(rs, wb.shape[1], torch.bfloat16)
    zero = torch.zeros((rows, wb.shape[0]), device="cuda", dtype=torch.bfloat16)
    got = hip.gemm(cols, wb, None, residual=zero).double()
    bias = torch.stack([m.w[f"{t}.oz{i}.bias"] for i in range(3)]).double()      # (3, C) fp32 merged biases Wz_i b_o,i
    ref = rs.double().t() @ bias
    scale = ref.abs().max()
    err = (got - ref).abs().max() / scale
    naive = ((rs.bfloat16().double().t() @ bias.float().bfloat16().double()) - ref).abs().max() / scale
    got32 = hip.gemm(cols.float(), wb.float(), None).double()                    # the operand columns carry the fp32 product ...
    err32 = (got32 - ref).abs().max() / scale
    print(f"merged bias term: max err / scale {err.item():.2e} bf16 out, {err32.item():.2e} fp32 out (one bf16 column per branch: "
          f"{naive.item():.2e})")
    assert err32 <= 2 ** -14 and naive >= 8 * err32
    assert err <= 2 ** -8 * 1.01                                                 # ... and the bf16 output adds its one rounding


# ---------------------------------------------------------------------------------- 384 / 192 / 320 px: the gates between 8 x 8 and 64 x 64 latents

def oracle_with_bf16_floor(sd_cpu, case):
    """The fp32 oracle's prediction for `case` and the two scalars of its CPU-bf16 floor, max and mean of |oracle under bf16 - fp32 oracle|
    (tests/golden/oracle_cache/unet_<case>.pt): the reference side measures the gate of the bf16 product mode, never the code under test."""
    ref = _run_oracle(sd_cpu, case)
    floor = (_run_oracle(sd_cpu, case, dtype=torch.bfloat16) - ref).abs()
    return {"ref": ref, "floor_max": floor.max(), "floor_mean": floor.mean()}


def _geometry_oracle(sd_cpu, name):
    return cached("unet_" + name, lambda: oracle_with_bf16_floor(sd_cpu, gx.UNET_GEOMETRY[name]))


def _geometry_model(sd_gpu, case, dtype):
    from mmgt_amd.unet3d import UNet3DConditionModel
    m = UNet3DConditionModel(device="cuda:0", dtype=dtype)
    m.load_state_dict(sd_gpu)
    m.enable_gradient_checkpointing()
    inp = _to_dev(gc.unet_inputs(case))
    m.set_banks(inp["banks"])

    def run():
        out = m(inp["sample"], inp["timestep"], encoder_hidden_states=inp["ehs"], audio_embedding=inp["audio"], pose_cond_fea=inp["pose"],
                full_mask=inp["full"], face_mask=inp["face"], body_mask=inp["lips"], motion_scale=inp["motion_scale"], return_dict=False)[0]
        torch.cuda.synchronize()
        return out.float().cpu()
    return m, run


@pytest.mark.parametrize("name", list(gx.UNET_GEOMETRY))
def test_unet_geometry_fp32_mode_matches_oracle(full_sd, name):
    """fp32-I/O mode at the north-star tolerance at 48 x 48 x 12, 24 x 24 x 24 and 40 x 40 x 5 latents: odd sides under the stride-2 convs and
    the 2x up-sampling (20 -> 10 -> 5, 12 -> 6 -> 3), 9 .. 2304 bank keys, windows of 5, 12 and 24 frames."""
    sd_gpu, sd_cpu = full_sd
    case = gx.UNET_GEOMETRY[name]
    ref = _geometry_oracle(sd_cpu, name)["ref"]
    out = _run_hip(sd_gpu, case, torch.float32)
    assert out.shape == ref.shape == (2, 4, case["frames"], case["latent"], case["latent"])
    print(f"{name} fp32 mode: max|d| {(out - ref).abs().max().item():.3e} mean|x| {ref.abs().mean().item():.3f}")
    torch.testing.assert_close(out, ref, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("name", list(gx.UNET_GEOMETRY))
def test_unet_geometry_bf16_mode_floor_paths_and_repeatability(full_sd, name):
    """bf16 product mode at the same three geometries, default switches: the launches of one forward are those the restated gates predict
    (tests/geometry_cases.expected_paths: which blocks ran fused is asserted, not assumed), the result is finite and within 1.5x the
    CPU-bf16 floor of the oracle at this very case, and a second forward repeats the first bit for bit."""
    from mmgt_amd import hip
    sd_gpu, sd_cpu = full_sd
    case = gx.UNET_GEOMETRY[name]
    o = _geometry_oracle(sd_cpu, name)
    ref, fmax, fmean = o["ref"], o["floor_max"].item(), o["floor_mean"].item()
    m, run = _geometry_model(sd_gpu, case, torch.bfloat16)
    before = {k: hip.call_count(k) for k in gx.PATHS}
    out = run()
    got = {k: hip.call_count(k) - before[k] for k in gx.PATHS}
    d = (out - ref).abs()
    print(f"{name} bf16 mode: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e} (floor {fmax:.3e} / {fmean:.3e}); launches {got}")
    assert got == gx.expected_paths(case["latent"], case["frames"], torch.bfloat16)
    assert torch.isfinite(out).all()
    assert d.max() <= FLOOR_SLACK * fmax and d.mean() <= FLOOR_SLACK * fmean
    assert torch.equal(run(), out)


def test_unet_matches_reference_golden_lat40(full_sd, golden_dir):
    """Straight against the REFERENCE's own output at a 40 x 40 latent, 2 frames, script mode (tests/golden/unet3d_full_lat40.npz)."""
    sd_gpu, _ = full_sd
    g = torch.from_numpy(np.load(os.path.join(golden_dir, "unet3d_full_lat40.npz"))["script"])
    out = _run_hip(sd_gpu, gx.GOLDEN_LAT40, torch.float32)
    print("lat40 fp32 mode vs reference golden: max|d|", (out - g).abs().max().item())
    torch.testing.assert_close(out, g, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unet_refuses_latent_side_20_before_any_launch(full_sd, dtype):
    """A side that is no multiple of 8 cannot pass the three stride-2 convs and come back through the up-sampling (unet_3d.py:461-469): the
    named error, and nothing has been launched when it is raised."""
    from mmgt_amd import hip
    sd_gpu, _ = full_sd
    m, run = _geometry_model(sd_gpu, dict(gc.UNET_CASES["full_cfg1"], frames=2, latent=20), dtype)
    before = dict(hip._calls)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        run()
    assert dict(hip._calls) == before
