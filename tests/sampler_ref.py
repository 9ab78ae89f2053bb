"""The fp64 yardstick of the sampler's update rules (mmgt_amd/scheduler.py `update_coefficients`, csrc/sampler.hip): plain torch and math, nothing
imported from the code under test.  Three layers:

RULES (a = alphas_cumprod as fp64, alpha = sqrt(a), sigma = sqrt(1 - a); a step goes from a_t to a_s, a_s = 1 behind the last timestep)
  DDIM, eta          x0 = alpha_t x - sigma_t v;  s_eta = eta sqrt((1 - a_s) / (1 - a_t)) sqrt(1 - a_t / a_s)
                     x_s = alpha_s x0 + sqrt(max(0, 1 - a_s - s_eta^2)) (alpha_t v + sigma_t x) + s_eta z             (`ddim_update`)
  DPM-Solver++ 2M    e = alpha_t sigma_s / (sigma_t alpha_s)   (no logarithm)
                     first order   x_s = (sigma_s / sigma_t) x + alpha_s (1 - e) x0          -- no earlier x0, or a_prev == 0, or sigma_s == 0
                     second order  r0 = (lambda_t - lambda_prev) / (lambda_s - lambda_t),  lambda = log(alpha / sigma)
                                   x_s = (sigma_s / sigma_t) x - alpha_s (e - 1) x0 - 1/2 alpha_s (e - 1) (x0 - x0_prev) / r0   (`dpm_update`)
  `ddim_k` / `dpm_k` restate both as (sa_t, sb_t, k_x, k_0, k_1, k_v, k_z) of  x_s = k_x x + k_0 x0 + k_1 x0_prev + k_v v + k_z z.

THE STEP KERNEL (`step_reference`): the contract of mmgt_sampler_step in fp64 on the operands as stored, and the bound B per element of what the fp32
kernel may differ by.  u = 2^-24.  csrc/sampler.hip, sampler_step_kernel, operation by operation (every result contributes u of its magnitude, carried
through the linear steps behind it by the magnitudes of their coefficients; an fma drops one of these terms, so one B covers both forms):
  eu = ps0 / cnt, ec = ps1 / cnt               d_eu = u |eu|, d_ec = u |ec|                      (callers may hand in larger d_eu, d_ec, d_x, d_xp)
  diff = ec - eu                               d_diff = d_eu + d_ec + u |diff|
  gd = g diff                                  d_gd = |g| d_diff + u |gd|
  vg = eu + gd                                 d_vg = d_eu + d_gd + u |vg|
  rho (rescale phi > 0)                        n Var = S2 - S1^2 / n from the fp64 moments.  The moments see the kernel's fp32 ec and vg, i.e. data
                                               perturbed by d_ec, d_vg:  d_Var = 2 mean(|y - mean| d_y)  to first order, plus the fp64 summation itself,
                                               (D + 3) 2^-53 2 mean(y^2) with D = `moment_depth(n)` the longest chain of adds.  r = sqrt(Var_c / Var_g):
                                               d_r = r/2 (d_Var_c / Var_c + d_Var_g / Var_g);  rho = phi r + (1 - phi) rounded once: d_rho = phi d_r + u |rho|
  v = rho vg                                   d_v = |rho| d_vg + d_rho |vg| + u |v|
  x0 = sa_t x - sb_t v                         d_x0 = |sa_t| d_x + u |sa_t x| + |sb_t| d_v + u |sb_t v| + u |x0|
  o = k_x x + k_0 x0                           d_o = |k_x| d_x + u |k_x x| + |k_0| d_x0 + u |k_0 x0| + u |o|
  o += k_1 xp;  o += k_v v;  o += k_z z        each: |k| d_operand + u |k operand| + u |o|
  B = d_o (1 + 2^-10) (the second-order terms), B_x0 = d_x0 (1 + 2^-10).  The gate is |out - ref| <= 2 B on every element, as tests/step_gate.py.

THE MOMENTS (`moments_reference`): the four fp64 sums and, per sum, sum_i (d_y or 2 |y| d_y + d_y^2) + D 2^-53 sum_i |term|.  `exact_moment_case` is
an input on which every fp32 operation of the kernel is exact and every fp64 partial sum is an integer multiple of 2^-16 below 2^53 2^-16: there the
bound is 0 in any summation order, and a reduction that keeps a sum or a sum of squares in fp32 cannot meet it.

THE LOOP (`gaussian_loop`): N steps on exact Gaussian v-predictions with the step bound compounded: the error of the latents and of x0 after a step
enters the next as d_x, d_xp, d_eu, d_ec.
"""
import math

import torch

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
SLACK = 1 + 2.0 ** -10


# ---- the schedule (mmgt_amd/scheduler.py restated: the fp32 table IS the definition of a) -----------------------------------------------------------

def alphas_cumprod(num_train=1000, beta_start=0.00085, beta_end=0.012):
    """the zero-terminal-SNR table of animation.yaml:80-89 as the fp32 tensor the scheduler holds"""
    betas = torch.linspace(beta_start, beta_end, num_train, dtype=F32)
    s = torch.cumprod(1.0 - betas, dim=0).sqrt()
    s0, sT = s[0].clone(), s[-1].clone()
    s = (s - sT) * (s0 / (s0 - sT))
    ab = s ** 2
    alphas = torch.cat([ab[0:1], ab[1:] / ab[:-1]])
    return torch.cumprod(1.0 - (1 - alphas), dim=0)


def trailing_timesteps(n, num_train=1000):
    return [int(round(num_train - i * (num_train / n))) - 1 for i in range(n)]


def a_of(table, t):
    return float(table[t]) if t >= 0 else 1.0


def ddim_pairs(table, n):
    """[(a_t, a_s)] of DDIM's N steps: s = t - 1000 // N"""
    return [(a_of(table, t), a_of(table, t - len(table) // n)) for t in trailing_timesteps(n, len(table))]


def dpm_triples(table, n):
    """[(a_prev or None, a_t, a_s)] of DPM's N steps: s = the next timestep"""
    ts = trailing_timesteps(n, len(table))
    return [(a_of(table, ts[i - 1]) if i else None, a_of(table, ts[i]), a_of(table, ts[i + 1]) if i + 1 < n else 1.0) for i in range(n)]


# ---- the rules ----------------------------------------------------------------------------------------------------------------------------------------

def ddim_sigma(a_t, a_s, eta):
    return eta * math.sqrt((1 - a_s) / (1 - a_t)) * math.sqrt(1 - a_t / a_s)


def ddim_update(x, v, z, a_t, a_s, eta):
    al_t, sg_t = math.sqrt(a_t), math.sqrt(1 - a_t)
    x0 = al_t * x - sg_t * v
    s = ddim_sigma(a_t, a_s, eta)
    out = math.sqrt(a_s) * x0 + math.sqrt(max(0.0, 1 - a_s - s * s)) * (al_t * v + sg_t * x)
    return (out + s * z if s else out), x0


def dpm_e(a_t, a_s):
    return math.sqrt(a_t) * math.sqrt(1 - a_s) / (math.sqrt(1 - a_t) * math.sqrt(a_s))


def dpm_order(a_prev, a_t, a_s):
    return 1 if a_prev is None or a_prev == 0.0 or a_s == 1.0 else 2


def dpm_r0(a_prev, a_t, a_s):
    lam = lambda a: math.log(math.sqrt(a) / math.sqrt(1 - a))
    return (lam(a_t) - lam(a_prev)) / (lam(a_s) - lam(a_t))


def dpm_update(x, v, x0_prev, a_prev, a_t, a_s):
    al_t, sg_t, al_s, sg_s = math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_s), math.sqrt(1 - a_s)
    x0 = al_t * x - sg_t * v
    e = dpm_e(a_t, a_s)
    if dpm_order(a_prev, a_t, a_s) == 1:
        return (sg_s / sg_t) * x + al_s * (1 - e) * x0, x0
    r0 = dpm_r0(a_prev, a_t, a_s)
    return (sg_s / sg_t) * x - al_s * (e - 1) * x0 - 0.5 * al_s * (e - 1) * (x0 - x0_prev) / r0, x0


def ddim_k(a_t, a_s, eta):
    s = ddim_sigma(a_t, a_s, eta)
    c = math.sqrt(max(0.0, 1 - a_s - s * s))
    return math.sqrt(a_t), math.sqrt(1 - a_t), c * math.sqrt(1 - a_t), math.sqrt(a_s), 0.0, c * math.sqrt(a_t), s


def dpm_k(a_prev, a_t, a_s):
    al_s, e = math.sqrt(a_s), dpm_e(a_t, a_s)
    k_x = math.sqrt(1 - a_s) / math.sqrt(1 - a_t)
    if dpm_order(a_prev, a_t, a_s) == 1:
        return math.sqrt(a_t), math.sqrt(1 - a_t), k_x, al_s * (1 - e), 0.0, 0.0, 0.0
    r0 = dpm_r0(a_prev, a_t, a_s)
    return math.sqrt(a_t), math.sqrt(1 - a_t), k_x, al_s * (1 - e) * (1 + 0.5 / r0), -al_s * (1 - e) * 0.5 / r0, 0.0, 0.0


def f32(v):
    """a Python float as the fp32 kernel argument it becomes (back as a Python float)"""
    return float(torch.tensor(v, dtype=F32))


def f32s(vals):
    return tuple(f32(v) for v in vals)


# ---- the closed form: data ~ N(0, s^2) ------------------------------------------------------------------------------------------------------------------

def gaussian_v_gain(a, s):
    """v = c x for the exact denoiser x0 = alpha s^2 x / (alpha^2 s^2 + sigma^2):  v = (alpha x - x0) / sigma"""
    al, sg = math.sqrt(a), math.sqrt(1 - a)
    return (al - al * s * s / (al * al * s * s + sg * sg)) / sg


def gaussian_v_mean_gain(a, s):
    """data ~ N(mu, s^2) per element: x0 = mu + alpha s^2 (x - alpha mu) / (alpha^2 s^2 + sigma^2), so v = c x + m mu with c = `gaussian_v_gain` and
    m = -sigma / (alpha^2 s^2 + sigma^2).  (At the zero-SNR start v = -mu: with mu = 0 the prediction is 0 everywhere and has no variance.)"""
    return -math.sqrt(1 - a) / (a * s * s + 1 - a)


def gaussian_gain(rule, table, n, s):
    """c of x_final = c x_T under `rule` ("ddim" or "dpm") with the exact denoiser; the exact probability-flow solution from the zero-SNR start is c = s"""
    x, x0p = torch.ones((), dtype=F64), None
    if rule == "ddim":
        for a_t, a_s in ddim_pairs(table, n):
            x, _ = ddim_update(x, gaussian_v_gain(a_t, s) * x, None, a_t, a_s, 0.0)
    else:
        for a_prev, a_t, a_s in dpm_triples(table, n):
            x, x0p = dpm_update(x, gaussian_v_gain(a_t, s) * x, x0p, a_prev, a_t, a_s)
    return float(x)


# ---- the step kernel ------------------------------------------------------------------------------------------------------------------------------------

MOMENT_BLOCKS_MAX = 512


def moment_depth(n):
    """the longest chain of fp64 adds behind a moment (csrc/sampler.hip): a thread's elements, six butterfly stages, three wave adds, the fold"""
    blocks = min(max(1, -(-n // 1024)), MOMENT_BLOCKS_MAX)
    return -(-n // (blocks * 256)) + 6 + 3 + blocks


def guided(ps, counter, g, d_eu=None, d_ec=None):
    """(eu, ec, vg, d_eu, d_ec, d_vg) in fp64; g as the fp32 argument"""
    cnt = counter.double()[None, None, :, None, None]
    eu, ec = ps[0:1].double() / cnt, ps[1:2].double() / cnt
    d_eu = U * eu.abs() if d_eu is None else d_eu
    d_ec = U * ec.abs() if d_ec is None else d_ec
    g = f32(g)
    diff = ec - eu
    d_diff = d_eu + d_ec + U * diff.abs()
    gd = g * diff
    d_gd = abs(g) * d_diff + U * gd.abs()
    vg = eu + gd
    return eu, ec, vg, d_eu, d_ec, d_eu + d_gd + U * vg.abs()


def _var(y, d_y):
    n = y.numel()
    m = y.mean()
    var = ((y - m) ** 2).mean()
    d_var = 2 * ((y - m).abs() * d_y).mean() + (d_y ** 2).mean() + (moment_depth(n) + 3) * 2.0 ** -53 * 2 * (y ** 2).mean()
    return var, d_var


def rescale_rho(ec, vg, d_ec, d_vg, phi):
    """(rho, d_rho): rho = phi sqrt(Var ec / Var vg) + (1 - phi), phi as the fp32 argument"""
    phi = f32(phi)
    vc, d_vc = _var(ec, d_ec)
    vv, d_vv = _var(vg, d_vg)
    r = math.sqrt(float(vc / vv))
    d_r = 0.5 * r * float(d_vc / vc + d_vv / vv) * SLACK
    rho = phi * r + (1 - phi)
    return rho, phi * d_r + U * abs(rho)


def step_reference(ps, counter, x, g, phi, co, x0_prev=None, z=None, d_x=0.0, d_xp=0.0, d_eu=None, d_ec=None, rho_from="cond"):
    """-> (out, x0, B_out, B_x0) in fp64.  co = (sa_t, sb_t, k_x, k_0, k_1, k_v, k_z) as handed to the kernel; x0_prev / z enter when their
    coefficient is not zero.  rho_from="uncond" is the mutant that takes the variance of the unconditional row."""
    sa_t, sb_t, k_x, k_0, k_1, k_v, k_z = f32s(co)
    eu, ec, vg, d_eu, d_ec, d_vg = guided(ps, counter, g, d_eu, d_ec)
    rho, d_rho = (1.0, 0.0) if phi == 0 else rescale_rho(ec if rho_from == "cond" else eu, vg, d_ec if rho_from == "cond" else d_eu, d_vg, phi)
    xi = x.double()
    v = rho * vg
    d_v = d_vg if phi == 0 else abs(rho) * d_vg + d_rho * vg.abs() + U * v.abs()
    p1, p2 = sa_t * xi, sb_t * v
    x0 = p1 - p2
    d_x0 = abs(sa_t) * d_x + U * p1.abs() + abs(sb_t) * d_v + U * p2.abs() + U * x0.abs()
    t1, t2 = k_x * xi, k_0 * x0
    o = t1 + t2
    d_o = abs(k_x) * d_x + U * t1.abs() + abs(k_0) * d_x0 + U * t2.abs() + U * o.abs()
    for k, operand, d_op in ((k_1, x0_prev, d_xp), (k_v, v, d_v), (k_z, z, 0.0)):
        if k != 0.0 or (operand is v):
            if operand is None:
                raise ValueError("a non-zero coefficient without its operand")
            t = k * operand.double()
            o = o + t
            d_o = d_o + abs(k) * d_op + U * t.abs() + U * o.abs()
    return o, x0, d_o * SLACK, d_x0 * SLACK


def step_simulate(ps, counter, x, g, phi, co, x0_prev=None, z=None):
    """the kernel's arithmetic in torch fp32 (separate multiplies and adds), rho from the fp64 moments of the fp32 values -> (out, x0) fp32"""
    c = [torch.tensor(v, dtype=F32, device=x.device) for v in co]
    sa_t, sb_t, k_x, k_0, k_1, k_v, k_z = c
    g32 = torch.tensor(g, dtype=F32, device=x.device)
    cnt = counter[None, None, :, None, None]
    eu, ec = ps[0:1] / cnt, ps[1:2] / cnt
    vg = eu + g32 * (ec - eu)
    rho = torch.ones((), dtype=F32, device=x.device)
    if phi != 0:
        n = vg.numel()
        nvar = lambda y: (y.double() ** 2).sum() - y.double().sum() ** 2 / n
        rho = (float(f32(phi)) * torch.sqrt(nvar(ec) / nvar(vg)) + (1.0 - f32(phi))).to(F32)
    v = rho * vg
    x0 = sa_t * x - sb_t * v
    o = k_x * x + k_0 * x0
    if co[4] != 0.0:
        o = o + k_1 * x0_prev
    o = o + k_v * v
    if co[6] != 0.0:
        o = o + k_z * z
    return o, x0


KINDS = ("ddim-eta", "dpm-first", "dpm-second", "dpm-second-rescale")
SHAPES = [(4, 5, 8, 8), (4, 7, 5, 3), (4, 130, 64, 64)]
GUIDANCE = 3.5


def step_case(kind, C, F, H, W, device="cpu", steps=20):
    """The operands of one step-kernel case, a pure function of (kind, shape): counters mixing 1 and 2, pred_sum = counter x hash_uniform, the guided
    row's spread unlike the conditional one's.  -> dict(ps, counter, x, g, phi, co, x0_prev, z); co as fp32-rounded Python floats.
    ddim-eta: step 10 of 20, eta 0.7 (noise);  dpm-first: step 1 (the earlier point is the zero-SNR start);  dpm-second(-rescale): step 10 (rescale 0.7)."""
    from tests.mm_gate import rnd
    table = alphas_cumprod()
    tag = f"sampler.{kind}.{C}.{F}.{H}.{W}"
    cnt = (1.0 + (torch.arange(F, device=device) * 7 % 3 == 1).to(F32)).contiguous()
    ps = (rnd(tag + ".ps", (2, C, F, H, W), 1.0, device=device) * torch.tensor([[0.6], [1.4]], device=device).view(2, 1, 1, 1, 1) + 0.05) * cnt[None, None, :, None, None]
    case = dict(ps=ps.contiguous(), counter=cnt, x=rnd(tag + ".x", (1, C, F, H, W), 1.5, device=device), g=GUIDANCE, phi=0.0, x0_prev=None, z=None)
    if kind == "ddim-eta":
        case["co"] = f32s(ddim_k(*ddim_pairs(table, steps)[10], 0.7))
        case["z"] = rnd(tag + ".z", (1, C, F, H, W), 1.7, device=device)
    else:
        tr = dpm_triples(table, steps)[1 if kind == "dpm-first" else 10]
        case["co"] = f32s(dpm_k(*tr))
        if kind != "dpm-first":
            case["x0_prev"] = rnd(tag + ".x0p", (1, C, F, H, W), 1.2, device=device)
        if kind.endswith("rescale"):
            case["phi"] = 0.7
    assert (case["co"][4] != 0.0) == (case["x0_prev"] is not None) and (case["co"][6] != 0.0) == (case["z"] is not None)
    assert {1.0, 2.0} == set(cnt.tolist())
    return case


def step_mutants(case):
    """{name: (out, x0) fp64} of three subtly wrong kernels (the first two need a second-order step, the last a rescale)"""
    c = case
    ref = lambda **kw: step_reference(c["ps"], c["counter"], c["x"], c["g"], c["phi"], kw.pop("co", c["co"]), x0_prev=kw.pop("x0_prev", c["x0_prev"]),
                                      z=c["z"], **kw)[:2]
    m = {}
    if c["co"][4] != 0.0:
        co = list(c["co"])
        co[4] = -co[4]
        m["k_1 with the wrong sign"] = ref(co=tuple(co))
        m["a stale x0_prev (the buffer of two steps ago)"] = ref(x0_prev=c["x0_prev"].flip(2) * 0.97)
    if c["phi"] != 0.0:
        m["rho from the unconditional row's variance"] = ref(rho_from="uncond")
    return m


# ---- the moments ----------------------------------------------------------------------------------------------------------------------------------------

def moments_reference(ps, counter, g):
    """-> (sums fp64 (4,), bounds fp64 (4,)) of (sum ec, sum ec^2, sum vg, sum vg^2)"""
    _, ec, vg, _, d_ec, d_vg = guided(ps, counter, g)
    D = moment_depth(ec.numel()) * 2.0 ** -53
    sums = torch.stack([ec.sum(), (ec ** 2).sum(), vg.sum(), (vg ** 2).sum()])
    bounds = torch.stack([d_ec.sum() + D * ec.abs().sum(), (2 * ec.abs() * d_ec + d_ec ** 2).sum() + D * (ec ** 2).sum(),
                          d_vg.sum() + D * vg.abs().sum(), (2 * vg.abs() * d_vg + d_vg ** 2).sum() + D * (vg ** 2).sum()])
    return sums, bounds * SLACK


def exact_moment_case(unit_ints_u, unit_ints_c, counter):
    """pred_sum (2, C, F, H, W) fp32 from INTEGER tensors (units of 2^-8, |.| < 2^13) and a counter of 1s and 2s, with guidance 2: ps / cnt, ec - eu,
    2 (ec - eu) and eu + 2 (ec - eu) are integers below 2^15 in those units, exact in fp32 with or without an fma; their squares are integers below
    2^30 in units of 2^-16, so every fp64 partial sum of up to 2^22 of them is exact.  -> (ps, guidance, exact sums fp64 (4,)).  v_c has a mean of 50
    standard deviations when unit_ints_c = 3200 +- uniform 111."""
    cnt = counter.double()[None, :, None, None]
    eu, ec = unit_ints_u.double(), unit_ints_c.double()
    ps = torch.stack([eu * cnt, ec * cnt]).to(F32) / 256.0
    vg = 2 * ec - eu
    sums = torch.stack([ec.sum() / 2 ** 8, (ec ** 2).sum() / 2 ** 16, vg.sum() / 2 ** 8, (vg ** 2).sum() / 2 ** 16])
    assert (ec ** 2).sum() < 2 ** 53 and (vg ** 2).sum() < 2 ** 53 and max(eu.abs().max(), ec.abs().max()) < 2 ** 13
    return ps.contiguous(), 2.0, sums


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------------------------

def gaussian_loop(x_T, table, n, rule, g, phi, s_u, s_c, eta=0.0, noises=None, mu=None):
    """The sampler on exact Gaussian v-predictions (unconditional data N(mu, s_u^2), conditional N(mu, s_c^2); mu None = 0, else a tensor that
    broadcasts against the latents): the model's output is fp32(c(t)) x (+ fp32(m(t)) mu) in fp32, and every frame's window average returns it
    exactly (a sum of one or two equal values over 1 or 2).  -> (latents fp64, bound): per step `step_reference` with counter 1, the errors so far
    handed in as d_x, d_xp and d_eu = |c_u| d_x + u (|c_u x| + |m_u mu| + 2 |eu|) (the model's two products and its sum, the division; without mu
    one product: 2 u |eu|), d_ec likewise."""
    x = x_T.double()
    d_x = torch.zeros_like(x)
    x0p, d_xp = None, 0.0
    one = torch.ones((x.shape[2],), dtype=F32, device=x.device)
    steps = ddim_pairs(table, n) if rule == "ddim" else dpm_triples(table, n)
    for i, st in enumerate(steps):
        a_t = st[-2]
        rows, errs = [], []
        for s in (s_u, s_c):
            c = f32(gaussian_v_gain(a_t, s))
            if mu is None:
                e = c * x
                d = abs(c) * d_x + 2 * U * e.abs()
            else:
                mt = f32(gaussian_v_mean_gain(a_t, s)) * mu.double()
                e = c * x + mt
                d = abs(c) * d_x + U * ((c * x).abs() + mt.abs() + 2 * e.abs())
            rows.append(e)
            errs.append(d)
        ps = torch.cat(rows)
        co = f32s(ddim_k(*st, eta) if rule == "ddim" else dpm_k(*st))
        d_eu, d_ec = errs
        x, x0, d_x, d_x0 = step_reference(ps, one, x, g, phi, co, x0_prev=x0p, z=None if noises is None else noises[i], d_x=d_x, d_xp=d_xp,
                                          d_eu=d_eu, d_ec=d_ec)
        x0p, d_xp = x0, d_x0
    return x, d_x
