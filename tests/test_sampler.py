"""The sampler's update rules on the CPU: DPM-Solver++ 2M, DDIM with eta, guidance rescale (mmgt_amd/scheduler.py, the plumbing of mmgt_amd/pipeline.py)
against the fp64 yardstick tests/sampler_ref.py; and the CPU twin of tests/test_sampler_gpu.py, which shows that the derived bound of the step kernel
accepts the kernel's arithmetic and rejects three subtly wrong kernels, and that the exact moments case rejects fp32 reductions."""
import importlib.util
import os
import sys

import pytest
import torch

from mmgt_amd.scheduler import SAMPLERS, DDIMScheduler, DPMSolverMultistepScheduler, with_sampler
from tests import sampler_ref as R
from tests.mm_gate import ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = R.alphas_cumprod()


# ---- the schedule and the closed form -------------------------------------------------------------------------------------------------------------

def test_the_yardstick_restates_the_schedule():
    s = DDIMScheduler()
    assert torch.equal(s.alphas_cumprod, TABLE) and float(TABLE[999]) == 0.0
    for n in (4, 5, 10, 12, 20, 25, 30, 40):
        s.set_timesteps(n)
        assert s.timesteps.tolist() == R.trailing_timesteps(n)


def _err(rule, n, s):
    return abs(R.gaussian_gain(rule, TABLE, n, s) - s) / s


def test_closed_form_gaussian_dpm_beats_ddim():
    """Data N(0, s^2): every sampler is x_final = c x_T and the exact solution from the zero-SNR start is c = s.  Conditions on ORDER, no tolerance.
    (|c - s| / s of this yardstick at s = 2: DPM 2.24e-2 / 5.57e-3 / 2.20e-3 at N = 10 / 20 / 40, DDIM 3.34e-2 at N = 40; both tend to 0 with N.)"""
    for s in (0.25, 0.5, 2.0):
        for n in (5, 10, 12, 20, 25, 40):
            d, e = _err("dpm", n, s), _err("ddim", n, s)
            print(f"s {s} N {n}: |c - s| / s  dpm {d:.3e}  ddim {e:.3e}")
            assert d < e, (s, n, d, e)
    assert _err("dpm", 10, 2.0) < _err("ddim", 40, 2.0)
    assert _err("dpm", 10, 2.0) > _err("dpm", 20, 2.0) > _err("dpm", 40, 2.0)


# ---- coefficients -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 25, 30])
def test_dpm_orders_e_and_r0(n):
    """steps 0, 1 and the last are first order (no earlier x0; the earlier point at lambda = -inf; sigma_s = 0), every other step second; e is finite
    at a_t = 0 and 0 on the last step"""
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(n)
    tr = R.dpm_triples(TABLE, n)
    for i, t in enumerate(s.timesteps.tolist()):
        co64, e, r0 = s.step_details(t)
        first = i in (0, 1, n - 1)
        assert (r0 is None) == first and (co64[4] == 0.0) == first and R.dpm_order(*tr[i]) == (1 if first else 2)
        assert e == pytest.approx(R.dpm_e(*tr[i][1:]), rel=1e-14, abs=0)
        if not first:
            assert r0 == pytest.approx(R.dpm_r0(*tr[i]), rel=1e-13) and r0 > 0
        assert s.update_coefficients(t) == R.f32s(R.dpm_k(*tr[i]))
    assert s.step_details(s.timesteps[0])[1] == 0.0 and s.step_details(s.timesteps[-1])[1] == 0.0
    assert s.update_coefficients(s.timesteps[-1])[2:5] == (0.0, 1.0, 0.0)            # the last step returns x0


@pytest.mark.parametrize("n", [4, 25, 30])
@pytest.mark.parametrize("eta", [0.0, 0.7, 1.0])
def test_ddim_coefficients(n, eta):
    s = DDIMScheduler()
    s.set_timesteps(n)
    pairs = R.ddim_pairs(TABLE, n)
    g = torch.Generator().manual_seed(n)
    x, v, z = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(3))
    for (a_t, a_s), t in zip(pairs, s.timesteps.tolist()):
        co = s.update_coefficients(t, eta)
        assert co == R.f32s(R.ddim_k(a_t, a_s, eta))
        if eta == 0.0:                          # the update of `step_coefficients`, to 1e-6
            sa_t, sb_t, sa_p, sb_p = s.step_coefficients(t)
            old = sa_p * (sa_t * x - sb_t * v) + sb_p * (sa_t * v + sb_t * x)
            new = co[2] * x + co[3] * (co[0] * x - co[1] * v) + co[5] * v
            assert co[4] == 0.0 and co[6] == 0.0 and (old - new).abs().max() < 1e-6
    if eta == 1.0:
        first, last = s.update_coefficients(999, 1.0), s.update_coefficients(s.timesteps[-1], 1.0)
        assert first[2] == 0.0 and first[5] == 0.0 and first[6] ** 2 == pytest.approx(1 - pairs[0][1], rel=1e-6)
        assert last[6] == 0.0


def test_the_linear_form_is_the_rule():
    """k_x x + k_0 x0 + k_1 x0_prev + k_v v + k_z z against the rules as the issue states them, fp64"""
    g = torch.Generator().manual_seed(1)
    x, v, z, x0p = (torch.randn(32, generator=g, dtype=torch.float64) for _ in range(4))
    form = lambda co: co[2] * x + co[3] * (co[0] * x - co[1] * v) + co[4] * x0p + co[5] * v + co[6] * z
    for a_t, a_s in R.ddim_pairs(TABLE, 12):
        assert (form(R.ddim_k(a_t, a_s, 0.6)) - R.ddim_update(x, v, z, a_t, a_s, 0.6)[0]).abs().max() < 1e-13
    for tr in R.dpm_triples(TABLE, 12):
        assert (form(R.dpm_k(*tr)) - R.dpm_update(x, v, x0p, *tr)[0]).abs().max() < 1e-13


def test_unbuilt_settings_and_eta_are_refused():
    for kw in (dict(algorithm_type="sde-dpmsolver++"), dict(solver_order=3), dict(solver_type="heun"), dict(timestep_spacing="leading")):
        with pytest.raises(NotImplementedError):
            DPMSolverMultistepScheduler(**kw)
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(5)
    with pytest.raises(ValueError, match="eta"):
        s.update_coefficients(999, 0.5)
    d = DDIMScheduler()
    assert with_sampler(d, "ddim") is d and set(SAMPLERS) == {"ddim", "dpmpp2m"}
    m = with_sampler(d, "dpmpp2m")
    assert type(m) is DPMSolverMultistepScheduler and m.alphas_cumprod is d.alphas_cumprod and m.order == 1 and m.init_noise_sigma == 1.0


# ---- the CPU twin of the GPU gate -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", R.SHAPES[:2], ids=str)
def test_step_bound_accepts_the_kernel_arithmetic_and_rejects_mutants(kind, shape):
    c = R.step_case(kind, *shape)
    ref, x0, B, B0 = R.step_reference(c["ps"], c["counter"], c["x"], c["g"], c["phi"], c["co"], c["x0_prev"], c["z"])
    out, x0s = R.step_simulate(c["ps"], c["counter"], c["x"], c["g"], c["phi"], c["co"], c["x0_prev"], c["z"])
    assert ratio(out, ref, B).max() <= 2.0 and ratio(x0s, x0, B0).max() <= 2.0
    assert (B <= 64 * R.U * (ref.abs() + 8)).all()               # the bound stays a few dozen fp32 roundings of values of order one
    muts = R.step_mutants(c)
    assert set(muts) == {"dpm-second": {"k_1 with the wrong sign", "a stale x0_prev (the buffer of two steps ago)"},
                         "dpm-second-rescale": {"k_1 with the wrong sign", "a stale x0_prev (the buffer of two steps ago)",
                                                "rho from the unconditional row's variance"}}.get(kind, set())
    for name, (m, _) in muts.items():
        worst = ratio(m.float(), ref, B).max().item()
        print(f"{kind} {shape} {name}: {worst:.3g} B")
        assert worst > 2.0, name


def _exact_case(shape, device="cpu"):
    from tests.mm_gate import rnd
    C, F, H, W = shape
    iu = 3000 + (rnd(f"sampler.mom.u.{shape}", (C, F, H, W), 111.0, device=device)).round()
    ic = 3200 + (rnd(f"sampler.mom.c.{shape}", (C, F, H, W), 111.0, device=device)).round()
    cnt = (1.0 + (torch.arange(F, device=device) % 2).float()).contiguous()
    return R.exact_moment_case(iu, ic, cnt) + (cnt,)


def test_exact_moment_case_rejects_fp32_reductions():
    """v_c with a mean of 50 standard deviations: the fp64 sums are exact (bound 0); a reduction in fp32, and one that keeps only the squares in fp32,
    miss them"""
    ps, g, sums, cnt = _exact_case(R.SHAPES[1])
    eu, ec = ps[0] / cnt[None, :, None, None], ps[1] / cnt[None, :, None, None]
    vg = eu + g * (ec - eu)
    assert abs(ec.double().mean() / ec.double().std()) > 45
    good = torch.stack([ec.double().sum(), (ec.double() ** 2).sum(), vg.double().sum(), (vg.double() ** 2).sum()])
    assert torch.equal(good, sums)
    ref, bound = R.moments_reference(ps, cnt, g)
    assert ((ref - sums).abs() <= bound).all()
    all32 = torch.stack([ec.sum(), (ec * ec).sum(), vg.sum(), (vg * vg).sum()]).double()
    sq32 = torch.stack([ec.double().sum(), (ec * ec).sum().double(), vg.double().sum(), (vg * vg).sum().double()])
    assert not torch.equal(all32, sums) and not torch.equal(sq32, sums)


@pytest.mark.parametrize("rule,phi,eta", [("dpm", 0.0, 0.0), ("dpm", 0.7, 0.0), ("ddim", 0.0, 0.5)], ids=["dpm", "dpm-rescale", "ddim-eta"])
def test_loop_bound_accepts_an_fp32_loop_and_rejects_a_first_order_one(rule, phi, eta):
    """the twin of the GPU loop test: six steps of the kernel's arithmetic in fp32 stay inside the compounded bound; the same loop with every DPM step
    first order does not"""
    n, s_u, s_c, g = 6, 0.5, 2.0, R.GUIDANCE
    gen = torch.Generator().manual_seed(5)
    x_T = torch.randn(1, 4, 20, 8, 8, generator=gen)
    noises = [torch.randn(1, 4, 20, 8, 8, generator=gen) for _ in range(n)] if eta else None
    mu = torch.randn(1, 4, 1, 8, 8, generator=gen) if phi else None      # a zero-mean Gaussian predicts v = 0 at t = 999: no variance to rescale by
    ref, bound = R.gaussian_loop(x_T, TABLE, n, rule, g, phi, s_u, s_c, eta, noises, mu)
    assert ref.abs().max() > 0.1 and (bound < 1e-3 * (ref.abs() + 1)).all()

    def loop(first_order_only=False):
        x, x0p, one = x_T.clone(), None, torch.ones(20)
        steps = R.ddim_pairs(TABLE, n) if rule == "ddim" else R.dpm_triples(TABLE, n)
        for i, st in enumerate(steps):
            a_t = st[-2]
            ps = torch.cat([R.f32(R.gaussian_v_gain(a_t, s)) * x + (0.0 if mu is None else R.f32(R.gaussian_v_mean_gain(a_t, s)) * mu) for s in (s_u, s_c)])
            if rule == "dpm" and first_order_only:
                st = (None,) + st[1:]
            co = R.f32s(R.ddim_k(*st, eta) if rule == "ddim" else R.dpm_k(*st))
            x, x0p = R.step_simulate(ps, one, x, g, phi, co, x0p, None if noises is None else noises[i])
        return x
    worst = ratio(loop(), ref, bound).max().item()
    print(f"{rule} rescale {phi} eta {eta}: fp32 loop {worst:.3f} B")
    assert worst <= 2.0
    if rule == "dpm":
        assert ratio(loop(True), ref, bound).max() > 2.0


# ---- pipeline plumbing over CPU doubles ---------------------------------------------------------------------------------------------------------------

L, CTX, OV, STEPS, HW = 20, 12, 4, 5, 4


class _UNet:
    """CPU double of denoise_window (the pattern of tests/test_ctxbatch.py): a deterministic function of each row's latents and CFG row"""
    device = torch.device("cpu")

    def denoise_window(self, latent_in, t, encoder_hidden_states, audio_embedding, pose_cond_fea, full_mask, face_mask, body_mask, motion_scale,
                       cfg_row=None):
        rows, c, f, h, w = latent_in.shape
        out = torch.full((rows * f, h, w, 64), 1e9)
        for r in range(rows):
            pred = latent_in[r] * (0.9 - 1e-4 * float(t)) + 0.05 * (r // (rows // 2))
            out[r * f:(r + 1) * f, :, :, :c] = pred.permute(1, 2, 3, 0)
        return out


def _run(monkeypatch, scheduler, **kw):
    """-> (calls of cfg_ddim_step, calls of sampler_step, final latents) of a 5-step run over the doubles"""
    from mmgt_amd import pipeline as PL
    from tests import loop_doubles
    loop_doubles.install(monkeypatch, PL.hip)
    old, new = [], []
    ddim = PL.hip.cfg_ddim_step

    def cfg_ddim_step(*a, **k):
        assert len(a) == 8 and not k
        old.append(a)
        return ddim(*a)

    def sampler_step(pred_sum, counter, latents, g, sa_t, sb_t, k_x, k_0, k_1, k_v, k_z, *, rescale=0.0, moments=None, prev_x0=None, noise=None,
                     x0_out=None, out=None):
        new.append(dict(co=(sa_t, sb_t, k_x, k_0, k_1, k_v, k_z), rescale=rescale, prev_x0=prev_x0, noise=None if noise is None else noise.clone(),
                        x0_out=x0_out, prev_x0_value=None if prev_x0 is None else prev_x0.clone()))
        c = dict(ps=pred_sum, counter=counter, x=latents, g=g, phi=rescale)
        o, x0, _, _ = R.step_reference(c["ps"], counter, latents, g, rescale, (sa_t, sb_t, k_x, k_0, k_1, k_v, k_z), prev_x0, noise)
        if x0_out is not None:
            x0_out.copy_(x0[0:1].float())
        new[-1]["x0_value"] = x0.float().clone()
        return o.float()
    monkeypatch.setattr(PL.hip, "cfg_ddim_step", cfg_ddim_step)
    monkeypatch.setattr(PL.hip, "sampler_step", sampler_step)
    scheduler.set_timesteps(STEPS)
    pipe = PL.Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=_UNet(), pose_guider=None, scheduler=scheduler)
    g = torch.Generator().manual_seed(7)
    lat = torch.randn(1, 4, L, HW, HW, generator=g)
    audio, masks, ehs = torch.zeros(2, L, 3, 5), [torch.zeros(2 * L, HW * HW)], torch.zeros(2, 1, 8)
    out = pipe.denoise(lat, scheduler.timesteps, ehs, None, audio, masks, masks, masks, 3.5, None, context_frames=CTX, context_stride=1,
                       context_overlap=OV, num_inference_steps=STEPS, **kw)
    return old, new, out


def test_default_call_is_cfg_ddim_step_with_its_eight_arguments(monkeypatch):
    for kw in ({}, dict(eta=0.0, guidance_rescale=0.0)):
        old, new, _ = _run(monkeypatch, DDIMScheduler(), **kw)
        assert len(old) == STEPS and not new


def test_dpm_hands_every_x0_to_the_next_step(monkeypatch):
    old, new, out = _run(monkeypatch, DPMSolverMultistepScheduler(), guidance_rescale=0.3)
    assert not old and len(new) == STEPS and torch.isfinite(out).all()
    bufs = {c["x0_out"].data_ptr() for c in new}
    assert len(bufs) == 2                                          # two buffers for the clip, allocated once
    assert new[0]["prev_x0"] is None and [c["co"][4] != 0.0 for c in new] == [False, False, True, True, False]
    for a, b in zip(new, new[1:]):
        assert b["prev_x0"] is a["x0_out"] and b["prev_x0"] is not b["x0_out"]
        assert torch.equal(b["prev_x0_value"], a["x0_value"])
    assert all(c["rescale"] == 0.3 and c["noise"] is None for c in new)


def test_eta_draws_one_noise_per_step_in_order(monkeypatch):
    gen = torch.Generator().manual_seed(11)
    first = torch.randn(1, 4, L, HW, HW, generator=gen)                                   # the initial latents come first
    old, new, _ = _run(monkeypatch, DDIMScheduler(), eta=0.5, generator=gen)
    assert not old and len(new) == STEPS
    twin = torch.Generator().manual_seed(11)
    assert torch.equal(torch.randn(1, 4, L, HW, HW, generator=twin), first)
    for c in new:
        assert c["noise"].dtype == torch.float32 and torch.equal(c["noise"], torch.randn(1, 4, L, HW, HW, generator=twin))
    assert [c["co"][6] > 0 for c in new] == [True] * (STEPS - 1) + [False] and all(c["prev_x0"] is None and c["x0_out"] is None for c in new)


def test_the_three_refusals_name_both_arguments(monkeypatch):
    from mmgt_amd import pipeline as PL
    with pytest.raises(ValueError, match=r"(?s)eta.*DPMSolverMultistepScheduler"):
        _run(monkeypatch, DPMSolverMultistepScheduler(), eta=0.5)
    with pytest.raises(ValueError, match=r"(?s)eta.*window_group"):
        _run(monkeypatch, DDIMScheduler(), eta=0.5, window_group=True)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"(?s)guidance_rescale.*guidance_scale|guidance_scale.*guidance_rescale"):
            _run(monkeypatch, DDIMScheduler(), guidance_rescale=bad)
    pipe = PL.Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=_UNet(), pose_guider=None,
                                 scheduler=DPMSolverMultistepScheduler())
    with pytest.raises(ValueError, match="eta"):                                       # __call__ refuses before the prologue
        pipe(None, None, None, [], [], [], 32, 32, L, STEPS, 3.5, eta=0.3)
    with pytest.raises(ValueError, match="guidance_rescale"):
        pipe(None, None, None, [], [], [], 32, 32, L, STEPS, 3.5, guidance_rescale=2.0)


@pytest.mark.parametrize("script", ["pose2vid.py", "audio2vid.py"])
def test_scripts_parse_the_sampler_flags(monkeypatch, script):
    path = os.path.join(ROOT, "scripts", script)
    spec = importlib.util.spec_from_file_location("sampler_flags_" + script[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", [path, "--synthetic"])
    a = mod.parse_args()
    assert (a.sampler, a.eta, a.guidance_rescale) == ("ddim", 0.0, 0.0)
    monkeypatch.setattr(sys, "argv", [path, "--synthetic", "--sampler", "dpmpp2m", "--eta", "0.25", "--guidance_rescale", "0.7"])
    a = mod.parse_args()
    assert (a.sampler, a.eta, a.guidance_rescale) == ("dpmpp2m", 0.25, 0.7)
    monkeypatch.setattr(sys, "argv", [path, "--sampler", "euler"])
    with pytest.raises(SystemExit):
        mod.parse_args()
