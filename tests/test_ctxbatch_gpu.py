"""Several context windows per forward (`context_batch_size`, DESIGN.md "Several windows per forward") on the device: the group accumulate
kernel, the operator on 2 B rows against the oracle's forward of each window ALONE, the bank rows, the shared-input / twin path at b = 4,
the sampler's trajectory against the oracle, the window_state memo per group, one full-size forward, and the script flag.

Row order of a group: [uncond w0 .. uncond w(B-1), cond w0 .. cond w(B-1)], each window with its Fw frames.  The windows of a group
share the banks, the CLIP pair and the timestep (one clip)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmgt_amd.synthetic import synth_state_dict  # noqa: E402
from tests import golden_cases as gc  # noqa: E402
from tests import test_pipeline_gpu as TP  # noqa: E402
from tests import test_unet_gpu as TU  # noqa: E402
from tests.oracle_cache import cached  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG1 = gc.UNET_CASES["full_cfg1"]


@pytest.fixture(scope="module")
def full_sd():
    from mmgt_amd.unet3d_spec import unet3d_spec
    sd_gpu = synth_state_dict(unet3d_spec(), device="cuda:0")
    return sd_gpu, {k: v.cpu() for k, v in sd_gpu.items()}


@pytest.fixture(scope="module")
def weights():
    sds = TP.build_weights("cuda:0")
    return sds, {k: {n: t.cpu() for n, t in v.items()} for k, v in sds.items()}


def _window_inputs(case, k):
    """Window k of a group: window 0 is the existing case's own input set (tag "u"), the others are other frames of the same clip -- their
    own latents, audio, pose and masks; the banks, the CLIP pair and the timestep are window 0's."""
    w0 = gc.unet_inputs(case)
    if k == 0:
        return w0
    w = gc.unet_inputs(case, tag=f"u.w{k}")
    w["banks"], w["ehs"], w["timestep"] = w0["banks"], w0["ehs"], w0["timestep"]
    return w


def _group(wins):
    """The windows' inputs as ONE batch in CFG row major order (every per-window tensor is [uncond | cond] along dim 0)."""
    rows = lambda key: torch.cat([w[key][:1] for w in wins] + [w[key][1:] for w in wins])
    f = wins[0]["sample"].shape[2]
    masks = lambda key: [torch.cat([w[key][l][:f] for w in wins] + [w[key][l][f:] for w in wins]) for l in range(len(wins[0][key]))]
    return dict(sample=rows("sample"), audio=rows("audio"), pose=rows("pose"), full=masks("full"), face=masks("face"), lips=masks("lips"),
                ehs=wins[0]["ehs"], timestep=wins[0]["timestep"], motion_scale=wins[0]["motion_scale"], banks=wins[0]["banks"])


def _model(sd_gpu, dtype, banks):
    from mmgt_amd.unet3d import UNet3DConditionModel
    m = UNet3DConditionModel(device="cuda:0", dtype=dtype)
    m.load_state_dict(sd_gpu)
    m.enable_gradient_checkpointing()
    m.set_banks({k: v.cuda() for k, v in banks.items()})
    return m


def _forward(m, inp, **kw):
    """denoise_window on the inputs -> (b, 4, f, h, w) fp32 on the host."""
    from mmgt_amd import hip
    d = TU._to_dev(inp)
    x = m.denoise_window(d["sample"], d["timestep"], d["ehs"], d["audio"], d["pose"], d["full"], d["face"], d["lips"], d["motion_scale"], **kw)
    out = hip.nhwc_to_ncfhw(x, d["sample"].shape[0], 4).float().cpu()
    torch.cuda.synchronize()
    return out


def _window_slice(out, k, nwin):
    """[uncond, cond] rows of window k from a group output."""
    return out[[k, nwin + k]]


_oracle_memo = {}


def _oracle_window(sd_cpu, case, k, dtype=torch.float32):
    """The oracle's forward of window k ALONE (what tests/test_unet_gpu.py::_run_oracle does for its case), memoised in the session."""
    key = (repr(sorted(case.items())), k, dtype)
    if key not in _oracle_memo:
        from oracle import unet3d_ref as R
        inp = _window_inputs(case, k)
        c = (lambda t: t.to(dtype) if torch.is_tensor(t) and t.is_floating_point() else t) if dtype != torch.float32 else (lambda t: t)
        sd = sd_cpu if dtype == torch.float32 else {n: c(v) for n, v in sd_cpu.items()}
        with torch.no_grad():
            _oracle_memo[key] = R.unet3d_forward(sd, R.UNet3DConfig(), c(inp["sample"]), inp["timestep"], c(inp["ehs"]), c(inp["audio"]),
                                                 c(inp["pose"]), [c(x) for x in inp["full"]], [c(x) for x in inp["face"]],
                                                 [c(x) for x in inp["lips"]], inp["motion_scale"],
                                                 {n: c(v) for n, v in inp["banks"].items()}).float()
    return _oracle_memo[key]


# ------------------------------------------------------------------------------------------------ kernel: accumulate
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_accumulate_windows_is_bitwise_the_sequential_windows(dtype):
    """mmgt_accumulate_windows against B calls of mmgt_accumulate_window on overlapping and wrapping index lists, into a random NaN-free
    pred_sum: the adds happen in list order, so bitwise."""
    from mmgt_amd import hip
    g = torch.Generator(device="cuda").manual_seed(5)
    F, fw, C, h, w = 20, 6, 4, 8, 8
    lists = [[0, 1, 2, 3, 4, 5], [3, 4, 5, 6, 7, 8], [6, 7, 8, 9, 10, 11], [17, 18, 19, 0, 1, 2], [19, 0, 1, 2, 3, 4]]
    for B in (1, 2, 5):
        idx = torch.tensor(lists[-B:] if B == 2 else lists[:B], device="cuda", dtype=torch.int32)
        pred = (torch.randn((2 * B * fw, h, w, 64), device="cuda", generator=g) * 3).to(dtype)
        ps0 = torch.randn((2, C, F, h, w), device="cuda", generator=g)
        c0 = torch.randint(0, 3, (F,), device="cuda", generator=g).float()
        a, ca = ps0.clone(), c0.clone()
        hip.accumulate_windows(pred, a, ca, idx, C)
        b, cb = ps0.clone(), c0.clone()
        p = pred.view(2, B, fw, h, w, 64)
        for k in range(B):
            hip.accumulate_window(p[:, k].reshape(2 * fw, h, w, 64).contiguous(), b, cb, idx[k].contiguous(), C)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(ca, cb), (B, (a - b).abs().max().item())
        assert not torch.equal(a, ps0) and (ca - c0).sum() == B * fw


# ------------------------------------------------------------------------------------------------ operator against the oracle
@pytest.mark.parametrize("nwin", [2, 3])
def test_operator_group_fp32_matches_oracle_window_by_window(full_sd, nwin):
    """fp32 mode: every window's slice of a 2- / 3-window forward against the oracle's forward of that window alone, at rtol 1e-3 /
    atol 1e-4.  Also printed, as a record: max|batched - sequential HIP forward| (3.8e-6 in fp32, 1.4e-2 in bf16 on MI355X; DESIGN)."""
    sd_gpu, sd_cpu = full_sd
    wins = [_window_inputs(CFG1, k) for k in range(nwin)]
    m = _model(sd_gpu, torch.float32, wins[0]["banks"])
    out = _forward(m, _group(wins))
    assert out.shape[0] == 2 * nwin
    for k in range(nwin):
        ref = _oracle_window(sd_cpu, CFG1, k)
        got = _window_slice(out, k, nwin)
        seq = _forward(m, wins[k])
        print(f"fp32 group of {nwin}, window {k}: max|d| vs oracle {(got - ref).abs().max().item():.3e}; max|batched - sequential| "
              f"{(got - seq).abs().max().item():.3e}")
        torch.testing.assert_close(got, ref, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("nwin", [2, 3])
def test_operator_group_bf16_within_the_lone_window_floor(full_sd, nwin):
    """bf16 mode: every window's slice within FLOOR_SLACK x the CPU-bf16 floor of the oracle on THAT window's inputs -- the gate and the floor
    tests/test_unet_gpu.py::test_unet_bf16_mode_within_measured_noise_floor applies to a lone window.  Window state, zero-audio skip and
    shared rows on, as the sampler calls the operator."""
    sd_gpu, sd_cpu = full_sd
    wins = [_window_inputs(CFG1, k) for k in range(nwin)]
    m = _model(sd_gpu, torch.bfloat16, wins[0]["banks"])
    out = _forward(m, _group(wins), audio_zero_rows=nwin, cfg_rows_share_input=True, window_state={})
    assert torch.isfinite(out).all()
    for k in range(nwin):
        ref = _oracle_window(sd_cpu, CFG1, k)
        floor = (_oracle_window(sd_cpu, CFG1, k, torch.bfloat16) - ref).abs()
        d = (_window_slice(out, k, nwin) - ref).abs()
        seq = _forward(m, wins[k], audio_zero_rows=1, cfg_rows_share_input=True)
        print(f"bf16 group of {nwin}, window {k}: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e} (floor {floor.max().item():.3e} / "
              f"{floor.mean().item():.3e}); max|batched - sequential| {(_window_slice(out, k, nwin) - seq).abs().max().item():.3e}")
        assert d.max() <= TU.FLOOR_SLACK * floor.max() and d.mean() <= TU.FLOOR_SLACK * floor.mean()


# ------------------------------------------------------------------------------------------------ bank rows
@pytest.mark.parametrize("dtype,latent", [(torch.float32, 8), (torch.bfloat16, 8), (torch.bfloat16, 16)])
def test_every_conditional_window_reads_bank_row_1(full_sd, dtype, latent):
    """Bank row 0 filled with a large constant, row 1 real: the whole group output is unchanged to the bit against the all-real bank -- every
    conditional window reads row 1 (an index past it would read other memory, row 0 would change the result), and the unconditional
    rows do not read the bank at all."""
    sd_gpu, _ = full_sd
    case = dict(CFG1, latent=latent, frames=4)
    wins = [_window_inputs(case, k) for k in range(3)]
    inp = _group(wins)
    m = _model(sd_gpu, dtype, inp["banks"])
    real = _forward(m, inp)
    poisoned = {k: v.clone() for k, v in inp["banks"].items()}
    for v in poisoned.values():
        v[0] = 1.0e4
    m.set_banks({k: v.cuda() for k, v in poisoned.items()})
    assert torch.equal(_forward(m, inp), real)
    # ... and the conditional rows DO read the bank: another row 1 changes them and leaves the unconditional rows alone
    other = {k: v.clone() for k, v in inp["banks"].items()}
    for v in other.values():
        v[1] = v[1] * 0.5 + 0.1
    m.set_banks({k: v.cuda() for k, v in other.items()})
    moved = _forward(m, inp)
    assert torch.equal(moved[:3], real[:3])
    for k in range(3):
        assert not torch.equal(moved[3 + k], real[3 + k]), f"conditional window {k} did not read the bank"


# ------------------------------------------------------------------------------------------------ shared input / twin at b = 4
def test_group_cfg_rows_share_input_b4(full_sd):
    """cfg_rows_share_input with TWO windows (b = 4): the second half of the batch is a copy of the first, conv_in and the first resnet run
    once on B Fw frames.  The relations tests/test_unet_gpu.py::test_unet_cfg_rows_share_input asserts at b = 2: bitwise when the convs take
    the same reduction order (tail split off), with and without the twin pass; at rounding level otherwise."""
    from mmgt_amd import hip
    sd_gpu, _ = full_sd
    wins = [_window_inputs(CFG1, k) for k in range(2)]
    inp = TU._to_dev(_group(wins))
    m = _model(sd_gpu, torch.bfloat16, wins[0]["banks"])
    assert torch.equal(inp["sample"][:2], inp["sample"][2:]) and torch.equal(inp["pose"][:2], inp["pose"][2:])

    def run(share):
        return m.denoise_window(inp["sample"], inp["timestep"], inp["ehs"], inp["audio"], inp["pose"], inp["full"], inp["face"], inp["lips"],
                                inp["motion_scale"], cfg_rows_share_input=share).float()
    hip.tune("tailsplit", 0)
    try:
        assert torch.equal(run(True), run(False))
        m._twin = False
        assert torch.equal(run(True), run(False))
        m._twin = True
    finally:
        hip.tune("tailsplit", 1)
    a, b = run(True), run(False)
    d = (a - b).abs()
    assert d.max() <= 0.05 * b.abs().max() and d.mean() <= 5e-3 * b.abs().mean().clamp_min(1e-3), (d.max().item(), d.mean().item())


def test_group_twin_pass_runs_for_two_windows(full_sd):
    """At 16 x 16 latents (256 tokens: the smallest shape with a twin kernel) the first reference-attention reader of a 2-window group runs
    as ONE attention pass over B Fw frames (mmgt_attention_twin is counted), and the result agrees with the unshared batch at the
    rounding level the b = 2 test uses."""
    from mmgt_amd import hip
    sd_gpu, _ = full_sd
    case = dict(CFG1, latent=16, frames=4)
    wins = [_window_inputs(case, k) for k in range(2)]
    inp = TU._to_dev(_group(wins))
    m = _model(sd_gpu, torch.bfloat16, wins[0]["banks"])

    def run(share):
        return m.denoise_window(inp["sample"], inp["timestep"], inp["ehs"], inp["audio"], inp["pose"], inp["full"], inp["face"], inp["lips"],
                                inp["motion_scale"], cfg_rows_share_input=share).float()
    n0 = hip.call_count("mmgt_attention_twin")
    a = run(True)
    assert hip.call_count("mmgt_attention_twin") == n0 + 1
    b = run(False)
    assert hip.call_count("mmgt_attention_twin") == n0 + 1
    d = (a - b).abs()
    print(f"twin pass, 2 windows: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e} on max|x| {b.abs().max().item():.3f}")
    assert d.max() <= 0.05 * b.abs().max() and d.mean() <= 5e-3 * b.abs().mean().clamp_min(1e-3), (d.max().item(), d.mean().item())


# ------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("batch", [2, "all"])
def test_pipeline_fp32_trajectory_matches_oracle_with_batched_windows(weights, batch):
    """test_pipeline_fp32_matches_oracle's (14, 8, 2) case -- several overlapping windows -- at context_batch_size 2 and "all windows": every
    step's latents at rtol 1e-3 / atol 1e-4 and the video at 1e-3 / 2e-4 against the cached oracle, the numbers of B = 1."""
    from mmgt_amd.context import uniform
    sds, sds_cpu = weights
    frames, ctx, ov = 14, 8, 2
    nw = len(list(uniform(0, 4, frames, ctx, 1, ov)))
    assert nw >= 2
    B = nw if batch == "all" else batch
    inp = TP._inputs(frames, 8)
    ref = cached(f"pipeline_fp32_{frames}_{ctx}_{ov}", lambda: TP.oracle_pipeline_fp32(sds_cpu, frames, ctx, ov))
    pipe = TP._build(sds, torch.float32)
    got = []
    out = pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, frames, 4, 3.5, motion_scale=[1.0, 1.0, 2.0],
               context_frames=ctx, context_overlap=ov, context_batch_size=B, latents=inp["latents"], clip_image_embeds=inp["clip"],
               ref_image_latents=inp["ref_lat"], callback=lambda i, t, lat: got.append(lat.cpu().clone()))
    assert len(got) == 4
    for a, b in zip(got, ref["traj"]):
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(out.videos, ref["want"], rtol=1e-3, atol=2e-4)


def test_pipeline_bf16_batched_within_measured_noise_floor(weights):
    """bf16, context_batch_size = 2, against the cached floor of test_pipeline_bf16_within_measured_noise_floor (its case and its gate).  That
    case is 8 frames in ONE window, so this is the degenerate group of one window (B larger than the window count); the sampler with groups
    that really hold several windows is gated by test_pipeline_bf16_several_windows_batched_within_measured_noise_floor below."""
    sds, sds_cpu = weights
    inp = TP._inputs(8, 8)
    ref = cached("pipeline_bf16_floor", lambda: TP.oracle_pipeline_bf16_floor(sds_cpu))
    want, floor = ref["want"], ref["floor"]
    pipe = TP._build(sds, torch.bfloat16)
    got = pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, 8, 4, 3.5, motion_scale=[1.0, 1.0, 2.0],
               context_batch_size=2, latents=inp["latents"], clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"],
               decode=False).videos.cpu()
    d = (got - want).abs()
    print(f"bf16 pipeline, context_batch_size 2: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e}; floor {floor.max().item():.3e} / "
          f"{floor.mean().item():.3e}")
    assert torch.isfinite(got).all()
    assert d.max() <= 1.5 * floor.max() and d.mean() <= 1.5 * floor.mean()


def _oracle_bf16_floor_several_windows(sds_cpu, frames, ctx, ov):
    """(fp32 oracle final latents, |CPU-bf16 oracle - fp32 oracle|) of the (frames, ctx, ov) sampler run, measured the way
    tests/test_pipeline_gpu.py::oracle_pipeline_bf16_floor measures its single-window case (about 20 s of CPU: computed in the test)."""
    from oracle import pipeline_ref
    inp = TP._inputs(frames, 8)
    kw = dict(clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"], pose_images=inp["pose"], audio_tensor=inp["audio"],
              full_mask=inp["full"], face_mask=inp["face"], lip_mask=inp["lips"], latents=inp["latents"], num_inference_steps=4,
              guidance_scale=3.5, motion_scale=[1.0, 1.0, 2.0], context_frames=ctx, context_overlap=ov, decode=False)
    with torch.no_grad():
        want = pipeline_ref.pose2vid(sds_cpu["unet"], sds_cpu["refnet"], sds_cpu["pose"], sds_cpu["vae"], **kw)
        floor = (pipeline_ref.pose2vid(sds_cpu["unet"], sds_cpu["refnet"], sds_cpu["pose"], sds_cpu["vae"], unet_dtype=torch.bfloat16, **kw) - want).abs()
    return want, floor


def test_pipeline_bf16_several_windows_batched_within_measured_noise_floor(weights):
    """bf16, context_batch_size = 2 on the (14, 8, 2) case -- SEVERAL windows, so the groups really hold two windows and a trailing short one:
    final latents against the fp32 oracle, gated at 1.5 x the error the same oracle makes when its denoiser runs under CPU bf16 on the same
    inputs (the gate of test_pipeline_bf16_within_measured_noise_floor; the floor is measured here for this case).  A wrong mask, audio or
    pose row order in the group's conditioning is an O(0.1 .. 1) difference."""
    from mmgt_amd.context import uniform
    sds, sds_cpu = weights
    frames, ctx, ov = 14, 8, 2
    nw = len(list(uniform(0, 4, frames, ctx, 1, ov)))
    assert nw >= 2 and nw % 2 == 1, nw                       # whole groups of two and a short last group
    inp = TP._inputs(frames, 8)
    want, floor = _oracle_bf16_floor_several_windows(sds_cpu, frames, ctx, ov)
    pipe = TP._build(sds, torch.bfloat16)
    run = lambda B: pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, frames, 4, 3.5,
                         motion_scale=[1.0, 1.0, 2.0], context_frames=ctx, context_overlap=ov, context_batch_size=B, latents=inp["latents"],
                         clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"], decode=False).videos.cpu()
    for B in (2, nw):
        got = run(B)
        d = (got - want).abs()
        print(f"bf16 pipeline, {nw} windows, context_batch_size {B}: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e}; floor "
              f"{floor.max().item():.3e} / {floor.mean().item():.3e}")
        assert torch.isfinite(got).all()
        assert d.max() <= 1.5 * floor.max() and d.mean() <= 1.5 * floor.mean()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("nwin", [2, 3])
def test_operator_single_cfg_row_of_a_group_equals_batched_rows(full_sd, dtype, nwin):
    """denoise_window(cfg_row=r) on the B rows of ONE CFG row of a group == that half of the CFG-batched group
    (tests/test_pipeline_gpu.py::test_operator_single_cfg_row_equals_batched_rows with several windows, its tolerances), with bank row 0
    filled with a large constant: the conditional rows of every window read bank row 1 (k2_bdiv = nb on the one-row slice), the
    unconditional rows read no bank."""
    sd_gpu, _ = full_sd
    case = dict(CFG1, frames=3)
    wins = [_window_inputs(case, k) for k in range(nwin)]
    inp = _group(wins)
    banks = {k: v.clone() for k, v in inp["banks"].items()}
    m = _model(sd_gpu, dtype, banks)
    both = _forward(m, inp)
    for v in banks.values():
        v[0] = 1.0e4
    m.set_banks({k: v.cuda() for k, v in banks.items()})
    f = case["frames"]
    tol = dict(rtol=1e-5, atol=1e-6) if dtype == torch.float32 else dict(rtol=1.6e-2, atol=2e-3)
    for row in (0, 1):
        half = slice(row * nwin, (row + 1) * nwin)
        cut = lambda L: [x.view(2, nwin * f, -1)[row].contiguous() for x in L]
        one = dict(inp, sample=inp["sample"][half], audio=inp["audio"][half], pose=inp["pose"][half], full=cut(inp["full"]),
                   face=cut(inp["face"]), lips=cut(inp["lips"]))
        got = _forward(m, one, cfg_row=row)
        assert got.shape[0] == nwin
        print(f"{dtype}, {nwin} windows, cfg_row {row}: max|d| vs batched {(got - both[half]).abs().max().item():.3e}")
        torch.testing.assert_close(got, both[half], **tol)


def test_window_state_is_kept_per_group_and_per_clip(weights):
    """The memo of the audio K / V and MM-HAA mask rows is one dict per GROUP, owned by one denoise() call: two steps with it equal two steps
    without it bitwise, and a second clip with other audio and masks through the same pipeline object gets its own state."""
    from mmgt_amd import hip
    sds, _ = weights
    pipe = TP._build(sds, torch.bfloat16)
    clip1 = TP._inputs(14, 8)
    clip2 = dict(clip1, audio=clip1["audio"].flip(1) * 0.5, full=[t.flip(0) for t in clip1["full"]], face=[t.flip(0) for t in clip1["face"]],
                 lips=[t.flip(0) for t in clip1["lips"]])

    def run(inp):
        return pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, 14, 2, 3.5, motion_scale=[1.0, 1.0, 2.0],
                    context_frames=8, context_overlap=2, context_batch_size=2, latents=inp["latents"], clip_image_embeds=inp["clip"],
                    ref_image_latents=inp["ref_lat"], decode=False).videos.clone()
    assert hip.tune_get("window_state") == 1
    with1, with2 = run(clip1), run(clip2)
    hip.tune("window_state", 0)
    try:
        without1, without2 = run(clip1), run(clip2)
    finally:
        hip.tune("window_state", 1)
    assert torch.equal(with1, without1) and torch.equal(with2, without2)
    assert not torch.equal(with1, with2)


# ------------------------------------------------------------------------------------------------ full size, once
def test_two_shipped_windows_in_one_forward_512x512(full_sd, golden_dir):
    """512 x 512, bf16, two 12-frame windows in one forward (b = 4): window 0 = the inputs of test_unet_shipped_window_512x512_twelve_frames,
    window 1 other frames.  Finite and bitwise repeatable; window 0 within that test's gate against the same cached oracle output;
    window 1 within the same band of its own lone HIP forward; bank row 0 is never read."""
    sd_gpu, sd_cpu = full_sd
    case = TU.TWELVE_FRAME_CASE
    wins = [_window_inputs(case, k) for k in range(2)]
    inp = _group(wins)
    fmax, fmean = TU._floor_cfg2(golden_dir)
    m = _model(sd_gpu, torch.bfloat16, inp["banks"])
    kw = dict(audio_zero_rows=2, cfg_rows_share_input=True)
    out = _forward(m, inp, **kw)
    assert out.shape == (4, 4, 12, 64, 64) and torch.isfinite(out).all()
    assert torch.equal(_forward(m, inp, **kw), out), "two windows in one forward are not bitwise repeatable"
    ref = cached("unet_512x512_twelve_frames", lambda: TU._run_oracle(sd_cpu, case))
    d0 = (_window_slice(out, 0, 2) - ref).abs()
    lone = _forward(m, wins[1], audio_zero_rows=1, cfg_rows_share_input=True)
    d1 = (_window_slice(out, 1, 2) - lone).abs()
    print(f"512x512, 2 x 12 frames: window 0 vs oracle max|d| {d0.max().item():.3e} mean|d| {d0.mean().item():.3e}; window 1 vs lone forward "
          f"max|d| {d1.max().item():.3e} mean|d| {d1.mean().item():.3e} (floor {fmax:.3e} / {fmean:.3e})")
    assert d0.max() <= TU.FLOOR_SLACK * fmax and d0.mean() <= TU.FLOOR_SLACK * fmean
    assert d1.max() <= TU.FLOOR_SLACK * fmax and d1.mean() <= TU.FLOOR_SLACK * fmean
    poisoned = {k: v.clone() for k, v in inp["banks"].items()}
    for v in poisoned.values():
        v[0] = 1.0e4
    m.set_banks({k: v.cuda() for k, v in poisoned.items()})
    assert torch.equal(_forward(m, inp, **kw), out)


# ------------------------------------------------------------------------------------------------ script
def test_pose2vid_script_takes_context_batch_size(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pose2vid.py"), "--synthetic", "-W", "64", "-H", "64", "-L", "20",
                        "--num_c", "8", "--steps", "2", "--context_batch_size", "2", "--out_dir", str(tmp_path)], capture_output=True,
                       text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["context_batch_size"] == 2 and rec["windows_per_step"] >= 2 and rec["video"] == [1, 3, 20, 64, 64] and rec["finite"]
