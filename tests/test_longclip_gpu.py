"""The long-clip options of the sampler on the device: the two window accumulations of csrc/elementwise.hip with weights against fp64 and
bit for bit against each other, and with unit weights against weights=None; their refusals; the loop without weights over a stand-in whose prediction
depends on the frame's position in its window; the real operator's steps restated from its own recorded predictions; the script flags.

THE BOUNDS ARE DERIVED, NOT MEASURED (tests/longclip_ref.py states each next to the code that evaluates it).  u = 2^-24.
  kernels     a target element covered by m windows is a chain of m fmaf: |sum - ref| <= m u sum_k |w_k p_k|; counter: m u sum_k w_k, and exact
              for pyramid (small integers).  Compared WITHOUT a factor.
  the loop    tests/sampler_ref.py's per-step bound compounded over six steps, the weighted average's error (the products of the stand-in, the
              fmaf chain, the counter, the division) handed in as d_eu / d_ec; gate |out - ref| <= 2 B on every element.
  operator    one step at a time from the latents as stored and the predictions as recorded (exact in fp64): the fmaf chain, the counter, the
              division and cfg_ddim_kernel's fourteen roundings; the same gate."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import longclip_ref as LR  # noqa: E402
from tests import sampler_ref as R  # noqa: E402
from tests import step_gate as G  # noqa: E402
from tests import test_pipeline_gpu as TP  # noqa: E402
from tests.test_step_contract_gpu import guard_rows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
ENTRIES = ("mmgt_accumulate_window", "mmgt_accumulate_windows")
C, CPAD = 4, 64

# ---- the kernels --------------------------------------------------------------------------------------------------------------------------------------

WINDOW_CASES = {"open14": (14, LR.open_windows(14, 8, 2)), "open20": (20, LR.open_windows(20, 8, 2)), "uniform14": (14, LR.uniform_windows(14, 8, 2))}


def test_window_cases_are_what_they_are_named():
    assert WINDOW_CASES["open14"][1] == [list(range(0, 8)), list(range(6, 14))]
    assert len(WINDOW_CASES["open20"][1]) == 3
    assert WINDOW_CASES["uniform14"][1][-1] == [12, 13, 0, 1, 2, 3, 4, 5] and len(WINDOW_CASES["uniform14"][1]) == 3


def _kernel_case(tag, name, hw, dt, rows):
    """pred ((rows B Fw), h, w, 64) in CFG row major order with 1e9 in the pad channels, idx (B, Fw) int32, per window (rows, C, Fw, h, w)"""
    F, wins = WINDOW_CASES[name]
    h, w = {64: (8, 8), 15: (3, 5)}[hw]
    B, Fw = len(wins), len(wins[0])
    pred = torch.full((rows * B * Fw, h, w, CPAD), 1e9, device=DEV, dtype=F32)
    pred[..., :C] = G.rnd(f"longclip.{tag}.{name}.{hw}.{rows}", (rows * B * Fw, h, w, C), 1.5, device=DEV)
    pred = pred.to(dt).contiguous()
    per_window = [pred.view(rows, B, Fw, h, w, CPAD)[:, k, ..., :C].permute(0, 4, 1, 2, 3) for k in range(B)]
    idx = torch.tensor(wins, device=DEV, dtype=torch.int32)
    return F, wins, (h, w), pred, per_window, idx


def _slice(pred, rows, B, Fw, k):
    """the ((rows Fw), h, w, cpad) slice of window k that a single-window launch takes"""
    return pred.view((rows, B, Fw) + tuple(pred.shape[1:]))[:, k].reshape((rows * Fw,) + tuple(pred.shape[1:])).contiguous()


@pytest.mark.parametrize("rows,row0", [(2, 0), (1, 1)], ids=["pair", "cond"])
@pytest.mark.parametrize("fuse", ["pyramid", "ramp"])
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hw", [64, 15])
@pytest.mark.parametrize("name", list(WINDOW_CASES))
def test_weighted_accumulation_against_fp64(name, hw, dt, fuse, rows, row0):
    """the group launch and B single-window launches: each within the bound of the fp64 sum, and bit for bit each other; NaN behind every
    operand; with rows = 1, row0 = 1 the unconditional row of pred_sum keeps its prefilled bits, and the same two hold with weights=None"""
    from mmgt_amd import hip
    F, wins, (h, w), pred, per_window, idx = _kernel_case("k", name, hw, dt, rows)
    B, Fw = idx.shape
    w32 = LR.weights(fuse, Fw, 2).to(DEV)
    S, W, B_s, B_w = LR.accumulate_reference(per_window, wins, w32, F)
    ps0 = torch.zeros((2, C, F, h, w), device=DEV, dtype=F32)
    if rows == 1:
        ps0[0] = G.rnd(f"longclip.row0.{name}.{hw}", (C, F, h, w), 1.0, device=DEV)
    ps_g, cnt_g = ps0.clone(), torch.zeros(F, device=DEV)
    before = [hip.call_count(n) for n in ENTRIES]
    hip.accumulate_windows(G.guarded(pred, extra_rows=1), ps_g, cnt_g, guard_rows(idx), C, rows=rows, row0=row0, weights=guard_rows(w32))
    ps_s, cnt_s = ps0.clone(), torch.zeros(F, device=DEV)
    for k in range(B):
        hip.accumulate_window(G.guarded(_slice(pred, rows, B, Fw, k), extra_rows=1), ps_s, cnt_s, guard_rows(idx[k]), C, rows=rows, row0=row0,
                              weights=guard_rows(w32))
    torch.cuda.synchronize()
    assert [hip.call_count(n) - b for n, b in zip(ENTRIES, before)] == [B, 1]
    for what, ps, cnt in (("group", ps_g, cnt_g), ("single", ps_s, cnt_s)):
        d = (ps[row0:row0 + rows].double() - S).abs()
        print(f"{what} {name} hw {hw} {fuse}: max |d| / B {(d / B_s.clamp_min(1e-300)).max().item():.3f}, counter |d| {(cnt.double() - W).abs().max().item():.2e}")
        assert torch.isfinite(ps).all() and (d <= B_s).all()
        assert ((cnt.double() - W).abs() <= B_w).all()
        if fuse == "pyramid":
            assert torch.equal(cnt.double(), W)
        if rows == 1:
            assert G.same_bits((ps[0], cnt), (ps0[0], cnt)), "CFG row 0 was written by a launch for row 1"
    assert G.same_bits((ps_g, cnt_g), (ps_s, cnt_s)), "the group launch differs from sequential single-window launches"
    assert S.abs().max() > 1 and W.min() > 0 and float(W.sum()) == pytest.approx(B * float(w32.double().sum()))     # every frame covered
    if rows == 1:                                                # the same pair of launches with weights=None: a single row of the group form
        ps_g, cnt_g, ps_s, cnt_s = ps0.clone(), torch.zeros(F, device=DEV), ps0.clone(), torch.zeros(F, device=DEV)
        hip.accumulate_windows(G.guarded(pred, extra_rows=1), ps_g, cnt_g, guard_rows(idx), C, rows=rows, row0=row0)
        for k in range(B):
            hip.accumulate_window(G.guarded(_slice(pred, rows, B, Fw, k), extra_rows=1), ps_s, cnt_s, guard_rows(idx[k]), C, rows=rows, row0=row0)
        assert G.same_bits((ps_g, cnt_g), (ps_s, cnt_s)), "weights=None: the group launch differs from sequential single-window launches"
        assert G.same_bits((ps_g[0], cnt_g), (ps0[0], cnt_s)) and not torch.equal(ps_g[1], ps0[1]) and cnt_g.min() >= 1, "weights=None: CFG row 0 was written"


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(WINDOW_CASES))
def test_unit_weights_are_bitwise_the_unweighted_entries(name, dt):
    """on a prefilled pred_sum and counter, weights of 1 against weights=None of the same entry: the group launch and the single launch, each for
    both CFG rows and for either row alone"""
    from mmgt_amd import hip
    F, wins, (h, w), pred, _, idx = _kernel_case("unit", name, 15, dt, 2)
    B, Fw = idx.shape
    ones = torch.ones(Fw, device=DEV)
    ps0 = G.rnd(f"longclip.ps0.{name}", (2, C, F, h, w), 2.0, device=DEV)
    cnt0 = (torch.arange(F, device=DEV) % 3).to(F32)
    for rows, row0 in ((2, 0), (1, 1), (1, 0)):
        a, ca, b, cb = ps0.clone(), cnt0.clone(), ps0.clone(), cnt0.clone()
        p = pred.view(2, B * Fw, h, w, CPAD)[row0:row0 + rows].reshape(rows * B * Fw, h, w, CPAD).contiguous()
        hip.accumulate_windows(p, a, ca, idx, C, rows=rows, row0=row0, weights=ones)
        hip.accumulate_windows(p, b, cb, idx, C, rows=rows, row0=row0)
        assert G.same_bits((a, ca), (b, cb)) and not torch.equal(a, ps0), (rows, row0)
        a, ca, b, cb = ps0.clone(), cnt0.clone(), ps0.clone(), cnt0.clone()
        for k in range(B):
            p = _slice(pred, 2, B, Fw, k)[row0 * Fw:(row0 + rows) * Fw].contiguous()
            hip.accumulate_window(p, a, ca, idx[k], C, rows=rows, row0=row0, bump_counter=k != 1, weights=ones)
            hip.accumulate_window(p, b, cb, idx[k], C, rows=rows, row0=row0, bump_counter=k != 1)
        assert G.same_bits((a, ca), (b, cb)) and not torch.equal(a, ps0), (rows, row0)


def test_refusals_launch_nothing():
    from mmgt_amd import hip
    F, wins, (h, w), pred, _, idx = _kernel_case("refuse", "open14", 15, F32, 2)
    B, Fw = idx.shape
    w32 = LR.weights("pyramid", Fw).to(DEV)
    ps, cnt = torch.zeros((2, C, F, h, w), device=DEV), torch.zeros(F, device=DEV)
    one = _slice(pred, 2, B, Fw, 0)
    group = lambda p, ps, cnt, ix, w, C, **k: hip.accumulate_windows(p, ps, cnt, ix, C, weights=w, **k)
    single = lambda p, ps, cnt, ix, w, C, **k: hip.accumulate_window(p, ps, cnt, ix, C, weights=w, **k)
    before = dict(hip._calls)
    for fn, p, ix in ((group, pred, idx), (single, one, idx[0].contiguous())):
        with pytest.raises(RuntimeError, match="pred must be float32 or bfloat16"):
            fn(p.half(), ps, cnt, ix, w32, C)
        with pytest.raises(RuntimeError, match="pred must be contiguous"):
            fn(p[1:], ps, cnt, ix, w32, C)                                           # a row short
        with pytest.raises(RuntimeError, match="pred must be contiguous"):
            fn(p[..., :32], ps, cnt, ix, w32, C)                                     # a strided view
        with pytest.raises(RuntimeError, match="pred must be contiguous"):
            fn(p, ps, cnt, ix, w32, C, rows=1, row0=1)                               # both rows handed over for one
        with pytest.raises(RuntimeError, match="rows must be"):
            fn(p, ps, cnt, ix, w32, C, rows=2, row0=1)
        with pytest.raises(RuntimeError, match="rows must be"):
            fn(p, ps, cnt, ix, w32, C, rows=3, row0=0)
        with pytest.raises(RuntimeError, match="rows must be"):
            fn(p, ps, cnt, ix, w32, C, rows=1, row0=2)
        with pytest.raises(RuntimeError, match="idx must be contiguous int32"):
            fn(p, ps, cnt, ix.long(), w32, C)
        with pytest.raises(RuntimeError, match="pred_sum must be"):
            fn(p, ps.double(), cnt, ix, w32, C)
        with pytest.raises(RuntimeError, match="pred_sum must be"):
            fn(p, ps[:, :3].contiguous(), cnt, ix, w32, C)
        with pytest.raises(RuntimeError, match="pixels per frame"):
            fn(p, ps[..., :w - 1].contiguous(), cnt, ix, w32, C)
        with pytest.raises(RuntimeError, match="counter must be"):
            fn(p, ps, cnt[:F - 1].contiguous(), ix, w32, C)
        with pytest.raises(RuntimeError, match="weights must be"):
            fn(p, ps, cnt, ix, w32[:Fw - 1].contiguous(), C)
        with pytest.raises(RuntimeError, match="weights must be"):
            fn(p, ps, cnt, ix, w32.double(), C)
        with pytest.raises(RuntimeError, match="GPU"):
            fn(p, ps, cnt, ix, w32.cpu(), C)
    with pytest.raises(RuntimeError, match=r"idx must be \(B, Fw\)"):
        group(pred, ps, cnt, idx[0].contiguous(), w32, C)
    with pytest.raises(RuntimeError, match=r"idx must be \(Fw,\)"):
        single(one, ps, cnt, idx, w32, C)
    assert hip._calls == before
    assert not ps.any() and not cnt.any()


# ---- the loop, end to end, without weights ------------------------------------------------------------------------------------------------------------

L, CTX, OV, STEPS, HW, S_U, S_C = 20, 8, 2, 6, 8, 0.5, 2.0
TABLE = R.alphas_cumprod()
INTERVAL = (0.3, 0.8)


class _PositionUNet:
    """tests/test_sampler_gpu.py's Gaussian stand-in with a gain that depends on the frame's position k in its window of n: fp32(c(t) (1 + 0.25
    (k - (n - 1) / 2) / n)) per row kind, so the windows that cover a frame disagree and the fuse changes the latents.  Takes cfg_row=1 (the
    conditional rows alone).  Records (timestep, rows, cfg_row) of every call."""
    device = torch.device(DEV)

    def __init__(self, mu=None):
        self.calls, self.mu = [], mu

    def denoise_window(self, latent_in, t, encoder_hidden_states, audio_embedding, pose_cond_fea, full_mask, face_mask, body_mask, motion_scale,
                       cfg_row=None):
        rows, c, f, h, w = latent_in.shape
        assert cfg_row in (None, 1) and latent_in.dtype == F32 and (cfg_row == 1 or rows % 2 == 0)
        a_t = R.a_of(TABLE, int(t))
        kinds = [S_C] * rows if cfg_row == 1 else [S_U] * (rows // 2) + [S_C] * (rows // 2)
        gain = torch.tensor([[LR.position_gain(R.gaussian_v_gain(a_t, s), k, f) for k in range(f)] for s in kinds], device=DEV, dtype=F32)
        v = latent_in * gain.view(rows, 1, f, 1, 1)
        if self.mu is not None:
            v = v + torch.tensor([R.f32(R.gaussian_v_mean_gain(a_t, s)) for s in kinds], device=DEV, dtype=F32).view(rows, 1, 1, 1, 1) * self.mu
        out = torch.full((rows * f, h, w, 64), 1e9, device=DEV, dtype=F32)
        out[..., :c] = v.permute(0, 2, 3, 4, 1).reshape(rows * f, h, w, c)
        self.calls.append((int(t), rows, cfg_row))
        return out


def _x_T():
    return G.rnd("longclip.loop.xT", (1, 4, L, HW, HW), 1.7, device=DEV).contiguous()


def _mu():
    return G.rnd("longclip.loop.mu", (1, 4, 1, HW, HW), 1.0, device=DEV)


def _denoise(scheduler, mu=None, **kw):
    from mmgt_amd.pipeline import Pose2VideoPipeline
    scheduler.set_timesteps(STEPS)
    unet = _PositionUNet(mu)
    pipe = Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=unet, pose_guider=None, scheduler=scheduler)
    out = pipe.denoise(_x_T(), scheduler.timesteps, torch.zeros(2, 1, 8, device=DEV), None, torch.zeros(2, L, 1, 1, device=DEV), [], [], [], R.GUIDANCE,
                       None, context_frames=CTX, context_stride=1, context_overlap=OV, num_inference_steps=STEPS, **kw)
    torch.cuda.synchronize()
    return out, unet


def _windows(schedule):
    return LR.open_windows(L, CTX, OV) if schedule == "open" else LR.uniform_windows(L, CTX, OV)


def _reference(schedule, fuse, rule, interval=None, phi=0.0, eta=0.0, noises=None, mu=None):
    flags = LR.guided_flags(R.trailing_timesteps(STEPS), interval)
    return LR.gaussian_loop(_x_T(), TABLE, STEPS, rule, R.GUIDANCE, phi, S_U, S_C, _windows(schedule), LR.weights(fuse, CTX, OV), flags, eta, noises, mu)


def _check(out, ref, bound, what):
    assert ref.abs().max() > 0.1 and (bound < 1e-3 * (ref.abs() + 1)).all()
    G.check(out, ref, bound, what)


def test_the_loop_case():
    assert len(_windows("open")) == 3 and len(_windows("uniform")) == 4 and _windows("uniform")[-1] == [18, 19, 0, 1, 2, 3, 4, 5]
    assert LR.guided_flags(R.trailing_timesteps(STEPS), INTERVAL) == [False, False, True, True, True, False]


def test_loop_open_pyramid_default_ddim():
    """the default update (cfg_ddim_step) behind the weighted accumulation; flat on the same windows gives other latents, by far more than the bounds"""
    from mmgt_amd import hip
    from mmgt_amd.scheduler import DDIMScheduler
    before = {n: hip.call_count(n) for n in ENTRIES + ("mmgt_cfg_ddim_step", "mmgt_sampler_step")}
    out, unet = _denoise(DDIMScheduler(), context_schedule="open", context_fuse="pyramid")
    assert hip.call_count(ENTRIES[0]) - before[ENTRIES[0]] == STEPS * 3 and hip.call_count(ENTRIES[1]) == before[ENTRIES[1]]
    assert hip.call_count("mmgt_cfg_ddim_step") - before["mmgt_cfg_ddim_step"] == STEPS and hip.call_count("mmgt_sampler_step") == before["mmgt_sampler_step"]
    ref, bound = _reference("open", "pyramid", "cfg_ddim")
    _check(out, ref, bound, "denoise open + pyramid, ddim")
    two, u2 = _denoise(DDIMScheduler(), context_schedule="open", context_fuse="pyramid", context_batch_size=2)
    assert torch.equal(out, two) and len(u2.calls) == STEPS * 2 and len(unet.calls) == STEPS * 3
    assert hip.call_count(ENTRIES[1]) - before[ENTRIES[1]] == STEPS * 2
    # the fuse must matter on this stand-in, or the test shows nothing
    ref_f, bound_f = _reference("open", "flat", "cfg_ddim")
    assert ((ref - ref_f).abs() > 2 * (bound + bound_f)).any() and (ref - ref_f).abs().max() > 1e-2
    flat, _ = _denoise(DDIMScheduler(), context_schedule="open")
    _check(flat, ref_f, bound_f, "denoise open + flat, ddim")
    assert ((out.double() - flat.double()).abs() > 2 * (bound + bound_f)).any()


def test_loop_open_ramp_dpm():
    from mmgt_amd.scheduler import DPMSolverMultistepScheduler
    out, _ = _denoise(DPMSolverMultistepScheduler(), context_schedule="open", context_fuse="ramp")
    _check(out, *_reference("open", "ramp", "dpm"), "denoise open + ramp, dpmpp2m")
    two, _ = _denoise(DPMSolverMultistepScheduler(), context_schedule="open", context_fuse="ramp", context_batch_size=2)
    assert torch.equal(out, two)


@pytest.mark.parametrize("eta", [0.0, 0.5], ids=["eta0", "eta0.5"])
def test_loop_uniform_pyramid_interval_rescale(eta):
    """wrapping windows, pyramid, guidance in (0.3, 0.8] of the schedule, rescale 0.7 (a per-element mean, as tests/test_sampler_gpu.py: with mean 0 the
    prediction at t = 999 has no variance), with and without eta: the unguided steps run half the rows and launch no moments"""
    from mmgt_amd import hip
    from mmgt_amd.scheduler import DDIMScheduler
    kw = dict(context_fuse="pyramid", guidance_interval=INTERVAL, guidance_rescale=0.7)
    gen = lambda: dict(eta=eta, generator=torch.Generator(device=DEV).manual_seed(5)) if eta else {}
    mu = _mu()
    before = hip.call_count("mmgt_cfg_moments")
    out, unet = _denoise(DDIMScheduler(), mu, **kw, **gen())
    flags = LR.guided_flags(R.trailing_timesteps(STEPS), INTERVAL)
    assert hip.call_count("mmgt_cfg_moments") - before == sum(flags) == 3
    want = [(t, 2 if f else 1, None if f else 1) for t, f in zip(R.trailing_timesteps(STEPS), flags) for _ in range(4)]
    assert unet.calls == want
    noises = None
    if eta:
        twin = torch.Generator(device=DEV).manual_seed(5)
        noises = [torch.randn((1, 4, L, HW, HW), generator=twin, device=DEV, dtype=F32) for _ in range(STEPS)]
    _check(out, *_reference("uniform", "pyramid", "ddim", INTERVAL, 0.7, eta, noises, mu), f"denoise uniform + pyramid + interval + rescale, eta {eta}")
    two, u2 = _denoise(DDIMScheduler(), mu, context_batch_size=2, **kw, **gen())
    assert torch.equal(out, two)
    assert u2.calls == [(t, 4 if f else 2, None if f else 1) for t, f in zip(R.trailing_timesteps(STEPS), flags) for _ in range(2)]


def test_loop_defaults_touch_none_of_the_new_entries(monkeypatch):
    """the defaults hand the two accumulations no weight vector (the weighted path is an operand now, not an entry of its own)"""
    from mmgt_amd import hip
    from mmgt_amd.scheduler import DDIMScheduler
    given = []

    def recording(name, real):
        def fn(*a, weights=None, **k):
            given.append((name, weights is not None))
            return real(*a, weights=weights, **k)
        return fn
    for name in ("accumulate_window", "accumulate_windows"):
        monkeypatch.setattr(hip, name, recording(name, getattr(hip, name)))
    before = [hip.call_count(n) for n in ENTRIES]
    for kw in ({}, dict(context_batch_size=2), dict(context_schedule="open")):
        out, unet = _denoise(DDIMScheduler(), **kw)
        assert torch.isfinite(out).all() and all(cfg_row is None for _, _, cfg_row in unet.calls)
    assert [hip.call_count(n) - b for n, b in zip(ENTRIES, before)] == [STEPS * (4 + 3), STEPS * 2]
    assert len(given) == STEPS * (4 + 3 + 2) and {name for name, _ in given} == {"accumulate_window", "accumulate_windows"}
    assert not any(weighted for _, weighted in given)


# ---- the real operator --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipes():
    sds = TP.build_weights(DEV)
    built = {}
    return lambda dtype: built.setdefault(dtype, TP._build(sds, dtype))


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_operator_open_pyramid_interval(pipes, dtype, batch):
    """14 frames, 8 / 2, 4 DDIM steps at 64 x 64 px: every step's weighted average and update restated in fp64 from the predictions the operator itself
    returned (so nothing but the pipeline's new arithmetic and routing is held here), cfg_row=1 on steps 0 and 3, two windows per step."""
    frames, ctx, ov, steps, g = 14, 8, 2, 4, 3.5
    pipe, inp = pipes(dtype), TP._inputs(14, 8)
    unet = pipe.denoising_unet
    calls, traj = [], []
    inner = unet.denoise_window

    def recording(sample, t, *a, **kw):
        out = inner(sample, t, *a, **kw)
        calls.append((int(t), sample.shape[0], kw.get("cfg_row"), out.clone()))
        return out
    unet.denoise_window = recording
    try:
        pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, frames, steps, g, motion_scale=[1.0, 1.0, 2.0],
             context_frames=ctx, context_overlap=ov, context_batch_size=batch, latents=inp["latents"], clip_image_embeds=inp["clip"],
             ref_image_latents=inp["ref_lat"], decode=False, context_schedule="open", context_fuse="pyramid", guidance_interval=INTERVAL,
             callback=lambda i, t, lat: traj.append(lat.clone()))
    finally:
        del unet.denoise_window
    torch.cuda.synchronize()
    wins, w32 = LR.open_windows(frames, ctx, ov), LR.weights("pyramid", ctx, ov)
    ts = R.trailing_timesteps(steps)
    flags = [False, True, True, False]
    assert len(wins) == 2 and len(LR.uniform_windows(frames, ctx, ov)) == 3 and LR.guided_flags(ts, INTERVAL) == flags
    per_step = len(wins) // batch
    assert len(calls) == steps * per_step and len(traj) == steps
    x = inp["latents"].to(DEV).float()
    for i, t in enumerate(ts):
        rows = 2 if flags[i] else 1
        step_calls = calls[i * per_step:(i + 1) * per_step]
        assert [(c[0], c[1], c[2]) for c in step_calls] == [(t, rows * batch, None if flags[i] else 1)] * per_step
        preds = {0: [], 1: []}
        for _, _, _, out in step_calls:
            assert out.shape[0] == rows * batch * ctx
            o = out.view(rows, batch, ctx, 8, 8, out.shape[-1])[..., :4]
            for k in range(batch):
                for r in range(rows):
                    preds[r if rows == 2 else 1].append(o[r, k].permute(3, 0, 1, 2)[None])
        ref, B = LR.step_from_predictions(preds[0] if flags[i] else None, preds[1], wins, w32, x, g, LR.ddim_scalars(TABLE, t, steps))
        G.check(traj[i], ref, B, f"operator {dtype} batch {batch} step {i}")
        x = traj[i]
    assert torch.isfinite(traj[-1]).all() and traj[-1].abs().max() > 0.1


# ---- the script ---------------------------------------------------------------------------------------------------------------------------------------

def test_pose2vid_script_takes_the_long_clip_options(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pose2vid.py"), "--synthetic", "-W", "64", "-H", "64", "-L", "14", "--num_c", "8",
                        "--steps", "4", "--context_schedule", "open", "--context_fuse", "pyramid", "--guidance_interval", "0.3", "0.8", "--out_dir",
                        str(tmp_path)], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["context_schedule"] == "open" and rec["context_fuse"] == "pyramid" and rec["guidance_interval"] == [0.3, 0.8]
    assert rec["windows_per_step"] == 3 and rec["video"] == [1, 3, 14, 64, 64] and rec["finite"]
