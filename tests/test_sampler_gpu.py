"""csrc/sampler.hip on the device (through mmgt_amd.hip and Pose2VideoPipeline.denoise) against the fp64 yardstick tests/sampler_ref.py.

THE BOUND IS DERIVED, NOT MEASURED.  sampler_step_kernel as written, u = 2^-24, every fp32 result contributing u of its magnitude, carried through the
linear operations behind it by the magnitudes of their coefficients (tests/sampler_ref.py states the same chain next to the code that evaluates it):
    eu = ps0 / cnt, ec = ps1 / cnt         d_eu = u |eu|, d_ec = u |ec|
    vg = eu + g (ec - eu)                  d_vg = d_eu + |g| (d_eu + d_ec + u |ec - eu|) + u |g (ec - eu)| + u |vg|
    rho = phi sqrt(Var_c / Var_g) + 1 - phi    the fp64 moments see the fp32 ec, vg:  d_Var = 2 mean(|y - mean| d_y) + (D + 3) 2^-53 2 mean(y^2),
                                           D the longest chain of fp64 adds;  d_rho = phi sqrt(Var_c / Var_g) / 2 (d_Var_c / Var_c + d_Var_g / Var_g) + u |rho|
    v = rho vg                             d_v = |rho| d_vg + d_rho |vg| + u |v|                  (rescale 0: v = vg, d_v = d_vg)
    x0 = sa_t x - sb_t v                   d_x0 = u |sa_t x| + |sb_t| d_v + u |sb_t v| + u |x0|
    o = k_x x + k_0 x0                     d_o = u |k_x x| + |k_0| d_x0 + u |k_0 x0| + u |o|
    o += k_1 xp; o += k_v v; o += k_z z    each  |k| d_operand + u |k operand| + u |o|
    B = d_o (1 + 2^-10),  B_x0 = d_x0 (1 + 2^-10);  the gate: |out - ref| <= 2 B and |x0_out - x0| <= 2 B_x0 on EVERY element (tests/step_gate.py's
gate).  An fma drops terms of these sums, so one B covers the contracted and the uncontracted code.  tests/test_sampler.py shows on the CPU that this
bound accepts the kernel's arithmetic and rejects a wrong sign on k_1, a stale x0_prev and a rho taken from the unconditional row's variance.
The moments: per sum, sum_i of the elements' own bounds plus D 2^-53 sum |term|; on `exact_moment_case` every operation is exact and the bound is 0.
The loop: the per-step bound with the errors so far handed in as d_x, d_xp, d_eu, d_ec (sampler_ref.gaussian_loop), six steps."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sampler_ref as R  # noqa: E402
from tests import step_gate as G  # noqa: E402
from tests.test_step_contract_gpu import guard_rows, sentinels  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
NEW = ("mmgt_sampler_step", "mmgt_cfg_moments")


def _guard(t):
    """a contiguous view with one NaN row of the leading dimension behind it"""
    return G.guarded(t, extra_rows=1)


# ---- the step kernel ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_sampler_step(shape, kind):
    """(4, 130, 64, 64) = 2 129 920 elements: a second sweep of the grid-stride loop; (4, 7, 5, 3) = 420: one ragged workgroup.  Counters mix 1 and 2;
    NaN behind every operand; out and x0_out inside sentinel-filled buffers that must come back untouched, every element written."""
    from mmgt_amd import hip
    C, F, H, W = shape
    c = R.step_case(kind, C, F, H, W, DEV)
    if F == 130:
        assert C * F * H * W > G.SWEEP
    ref, x0, B, B0 = R.step_reference(c["ps"], c["counter"], c["x"], c["g"], c["phi"], c["co"], c["x0_prev"], c["z"])
    (obuf, out), (xbuf, x0_out) = sentinels((1, C, F, H, W), F32), sentinels((1, C, F, H, W), F32)
    before = [hip.call_count(n) for n in NEW]
    got = hip.sampler_step(_guard(c["ps"]), guard_rows(c["counter"]), _guard(c["x"]), c["g"], *c["co"], rescale=c["phi"],
                           prev_x0=None if c["x0_prev"] is None else _guard(c["x0_prev"]), noise=None if c["z"] is None else _guard(c["z"]),
                           x0_out=x0_out, out=out)
    assert got is out
    assert [hip.call_count(n) - b for n, b in zip(NEW, before)] == [1, 1 if c["phi"] else 0]
    G.assert_untouched(obuf, out)
    G.assert_untouched(xbuf, x0_out)
    G.check(out, ref, B, f"sampler_step {kind} {shape}")
    G.check(x0_out, x0, B0, f"sampler_step {kind} {shape} x0")


def test_sampler_step_skips_operands_with_a_zero_coefficient_and_takes_given_moments():
    """a first-order step handed a NaN-filled prev_x0 and noise (k_1 = k_z = 0) does not read them; x0_out=None writes no x0; moments handed over are
    the ones of `cfg_moments`"""
    from mmgt_amd import hip
    c = R.step_case("dpm-first", 4, 7, 5, 3, DEV)
    nan = torch.full_like(c["x"], G.NAN)
    ref, _, B, _ = R.step_reference(c["ps"], c["counter"], c["x"], c["g"], 0.0, c["co"])
    G.check(hip.sampler_step(c["ps"], c["counter"], c["x"], c["g"], *c["co"], prev_x0=nan, noise=nan), ref, B, "first order, NaN operands unused")
    c = R.step_case("dpm-second-rescale", 4, 7, 5, 3, DEV)
    mom = hip.cfg_moments(c["ps"], c["counter"], c["g"])
    a = hip.sampler_step(c["ps"], c["counter"], c["x"], c["g"], *c["co"], rescale=c["phi"], prev_x0=c["x0_prev"], moments=mom)
    b = hip.sampler_step(c["ps"], c["counter"], c["x"], c["g"], *c["co"], rescale=c["phi"], prev_x0=c["x0_prev"])
    assert torch.equal(a, b)


# ---- the moments --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_cfg_moments_against_fp64(shape):
    from mmgt_amd import hip
    c = R.step_case("dpm-second", *shape, DEV)
    ref, bound = R.moments_reference(c["ps"], c["counter"], c["g"])
    got = hip.cfg_moments(_guard(c["ps"]), guard_rows(c["counter"]), c["g"])
    assert got.dtype == torch.float64 and got.shape == (4,) and got.is_cuda
    x = G.ratio(got, ref, bound)
    print(f"cfg_moments {shape}: |d| / B {x.tolist()}")
    assert (x <= 1.0).all()
    assert torch.equal(hip.cfg_moments(c["ps"], c["counter"], c["g"]), got)                 # two launches: the same bits


@pytest.mark.parametrize("shape", R.SHAPES[1:], ids=str)
def test_cfg_moments_exact_on_a_mean_of_fifty_standard_deviations(shape):
    """every fp32 operation of the kernel and every fp64 partial sum is exact on this input (sampler_ref.exact_moment_case): the four sums must be THE
    sums, in any order.  A reduction in fp32, or with the squares in fp32, cannot give them (tests/test_sampler.py)."""
    from mmgt_amd import hip
    from tests.test_sampler import _exact_case
    ps, g, sums, cnt = _exact_case(shape, DEV)
    got = hip.cfg_moments(_guard(ps), guard_rows(cnt), g)
    assert torch.equal(got, sums), (got - sums).tolist()
    assert torch.equal(hip.cfg_moments(ps, cnt, g), got)
    n = ps[0].numel()
    var = got[1] / n - (got[0] / n) ** 2
    assert (got[0] / n) / var.sqrt() > 45


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    from mmgt_amd import hip
    c = R.step_case("dpm-second-rescale", 4, 7, 5, 3, DEV)
    ps, cnt, lat, xp = c["ps"], c["counter"], c["x"], c["x0_prev"]
    step = lambda *a, **k: hip.sampler_step(*a, c["g"], *c["co"], **k)
    before = dict(hip._calls)
    with pytest.raises(RuntimeError, match="latents must be"):
        step(ps, cnt, torch.cat([lat, lat]), prev_x0=xp)
    with pytest.raises(RuntimeError, match="pred_sum must be"):
        step(ps[:, :3].contiguous(), cnt, lat, prev_x0=xp)
    with pytest.raises(RuntimeError, match="pred_sum must be"):
        step(ps.double(), cnt, lat, prev_x0=xp)
    with pytest.raises(RuntimeError, match="counter has"):
        step(ps, cnt[:6].contiguous(), lat, prev_x0=xp)
    with pytest.raises(RuntimeError, match="prev_x0 must be"):
        step(ps, cnt, lat, prev_x0=xp[:, :, :6].contiguous())
    with pytest.raises(RuntimeError, match="noise must be"):
        step(ps, cnt, lat, prev_x0=xp, noise=lat[:, :3].contiguous())
    with pytest.raises(RuntimeError, match="noise must be"):
        step(ps, cnt, lat, prev_x0=xp, noise=lat.double())
    with pytest.raises(RuntimeError, match="prev_x0"):
        step(ps, cnt, lat)                                                              # k_1 != 0 without it
    for bad in (-0.25, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="rescale"):
            step(ps, cnt, lat, prev_x0=xp, rescale=bad)
    with pytest.raises(RuntimeError, match="x0_out"):
        step(ps, cnt, lat, prev_x0=xp, x0_out=xp)
    with pytest.raises(RuntimeError, match="pred_sum must be"):
        hip.cfg_moments(ps.double(), cnt, c["g"])
    with pytest.raises(RuntimeError, match="counter has"):
        hip.cfg_moments(ps, cnt[:6].contiguous(), c["g"])
    assert hip._calls == before


def test_torch_op_returns_latents_and_x0():
    import mmgt_amd.torch_ops  # noqa: F401
    c = R.step_case("dpm-second-rescale", 4, 7, 5, 3, DEV)
    ref, x0, B, B0 = R.step_reference(c["ps"], c["counter"], c["x"], c["g"], c["phi"], c["co"], c["x0_prev"], c["z"])
    out, x0_out = torch.ops.mmgt_hip.sampler_step(c["ps"], c["counter"], c["x"], c["x0_prev"], None, c["g"], c["phi"], list(c["co"]))
    G.check(out, ref, B, "torch.ops.mmgt_hip.sampler_step")
    G.check(x0_out, x0, B0, "torch.ops.mmgt_hip.sampler_step x0")


# ---- the loop, end to end, without weights ------------------------------------------------------------------------------------------------------------

L, CTX, OV, STEPS, HW, S_U, S_C = 20, 12, 4, 6, 8, 0.5, 2.0
TABLE = R.alphas_cumprod()


class _GaussianUNet:
    """A stand-in for the operator (no `boc`): the exact v-prediction of data N(0, 0.5^2) for the unconditional rows and N(0, 2^2) for the conditional
    ones, v = fp32(c(t)) x in fp32 on the device, in the operator's layout ((rows Fw), h, w, 64) with garbage in the pad channels."""
    device = torch.device(DEV)

    def __init__(self, mu=None):
        self.calls, self.mu = 0, mu

    def denoise_window(self, latent_in, t, encoder_hidden_states, audio_embedding, pose_cond_fea, full_mask, face_mask, body_mask, motion_scale,
                       cfg_row=None):
        rows, c, f, h, w = latent_in.shape
        assert cfg_row is None and rows % 2 == 0 and latent_in.dtype == F32
        a_t = R.a_of(TABLE, int(t))
        per_row = lambda fn: torch.tensor([R.f32(fn(a_t, S_U))] * (rows // 2) + [R.f32(fn(a_t, S_C))] * (rows // 2), device=DEV, dtype=F32).view(rows, 1, 1, 1, 1)
        v = latent_in * per_row(R.gaussian_v_gain)
        if self.mu is not None:
            v = v + per_row(R.gaussian_v_mean_gain) * self.mu
        out = torch.full((rows * f, h, w, 64), 1e9, device=DEV, dtype=F32)
        out[..., :c] = v.permute(0, 2, 3, 4, 1).reshape(rows * f, h, w, c)
        self.calls += 1
        return out


def _x_T():
    return G.rnd("sampler.loop.xT", (1, 4, L, HW, HW), 1.7, device=DEV).contiguous()


def _mu():
    """per (channel, pixel) means, the same for every frame (the stand-in sees windows, not frame numbers)"""
    return G.rnd("sampler.loop.mu", (1, 4, 1, HW, HW), 1.0, device=DEV)


def _denoise(scheduler, mu=None, **kw):
    from mmgt_amd.pipeline import Pose2VideoPipeline
    scheduler.set_timesteps(STEPS)
    unet = _GaussianUNet(mu)
    pipe = Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=unet, pose_guider=None, scheduler=scheduler)
    out = pipe.denoise(_x_T(), scheduler.timesteps, torch.zeros(2, 1, 8, device=DEV), None, torch.zeros(2, L, 1, 1, device=DEV), [], [], [], R.GUIDANCE,
                       None, context_frames=CTX, context_stride=1, context_overlap=OV, num_inference_steps=STEPS, **kw)
    torch.cuda.synchronize()
    return out, unet


def _loop_check(out, what, rule, phi=0.0, eta=0.0, noises=None, mu=None):
    ref, bound = R.gaussian_loop(_x_T(), TABLE, STEPS, rule, R.GUIDANCE, phi, S_U, S_C, eta, noises, mu)
    assert ref.abs().max() > 0.1 and (bound < 1e-3 * (ref.abs() + 1)).all()              # six compounded steps stay far below any wrong rule
    G.check(out, ref, bound, what)


def test_loop_has_counters_one_and_two():
    from mmgt_amd.context import get_context_scheduler
    wins = list(get_context_scheduler("uniform")(0, STEPS, L, CTX, 1, OV))
    cnt = torch.zeros(L)
    for w in wins:
        cnt[torch.tensor(w)] += 1
    assert set(cnt.tolist()) == {1.0, 2.0}


@pytest.mark.parametrize("phi", [0.0, 0.7], ids=["plain", "rescale"])
def test_loop_dpm(phi):
    """The rescale run gives both Gaussians a per-element mean: with mean 0 the exact prediction at t = 999 is v = 0 everywhere, Var v_g = 0 and rho the
    IEEE 0 / 0, which no reference can be compared with.  Everything else is as the plain run: s = 0.5 / 2, six steps, counters 1 and 2."""
    from mmgt_amd.scheduler import DPMSolverMultistepScheduler
    mu = _mu() if phi else None
    out, _ = _denoise(DPMSolverMultistepScheduler(), mu, guidance_rescale=phi)
    _loop_check(out, f"denoise dpmpp2m rescale {phi}", "dpm", phi, mu=mu)


def test_loop_ddim_eta_with_a_device_generator():
    from mmgt_amd.scheduler import DDIMScheduler
    out, _ = _denoise(DDIMScheduler(), eta=0.5, generator=torch.Generator(device=DEV).manual_seed(3))
    twin = torch.Generator(device=DEV).manual_seed(3)
    noises = [torch.randn((1, 4, L, HW, HW), generator=twin, device=DEV, dtype=F32) for _ in range(STEPS)]
    _loop_check(out, "denoise ddim eta 0.5", "ddim", eta=0.5, noises=noises)


def test_loop_dpm_context_batch_two_is_bit_equal():
    from mmgt_amd.scheduler import DPMSolverMultistepScheduler
    one, u1 = _denoise(DPMSolverMultistepScheduler())
    two, u2 = _denoise(DPMSolverMultistepScheduler(), context_batch_size=2)
    assert torch.equal(one, two) and u2.calls < u1.calls


def test_loop_default_ddim_stays_on_cfg_ddim_step():
    from mmgt_amd import hip
    from mmgt_amd.scheduler import DDIMScheduler
    before = {n: hip.call_count(n) for n in NEW + ("mmgt_cfg_ddim_step",)}
    out, _ = _denoise(DDIMScheduler())
    assert hip.call_count("mmgt_cfg_ddim_step") - before["mmgt_cfg_ddim_step"] == STEPS
    assert all(hip.call_count(n) == before[n] for n in NEW)
    assert torch.isfinite(out).all()
