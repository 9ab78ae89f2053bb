"""The fp64 yardstick of the long-clip options of the sampler: open-ended windows, weighted window blending and the guidance interval,
restated in plain torch and integers; nothing imported from the code under test (tests/sampler_ref.py supplies the update rules and their bounds).

WINDOWS     `open_windows`: one window when L <= ctx, else starts 0, s, 2 s, ... below L - ctx with s = ctx - ov, then L - ctx.
            `uniform_windows`: the closed loop at context_stride 1: starts 0, s, ... below L, every index modulo L (the last window wraps).
WEIGHTS     `weights`: pyramid min(k + 1, n - k); ramp min(1, (k + 1) / (o + 1), (n - k) / (o + 1)); flat 1; in double, rounded once to fp32.
INTERVAL    `guided_flags`: the step at timestep t is guided iff lo < (t + 1) / 1000 <= hi.

THE ACCUMULATION (`accumulate_reference`).  csrc/elementwise.hip, the two weighted kernels: a target element that m windows cover is the chain
s_0 = 0, s_j = fmaf(w_j, p_j, s_(j-1)) over those windows in list order: m roundings, each of a partial sum of magnitude <= sum_k |w_k p_k|; the
products are not rounded.  counter likewise collects m weights.  u = 2^-24:
    B_sum = m u sum_k |w_k p_k|          B_cnt = m u sum_k w_k      (pyramid: the weights are small integers and every partial sum is exact, B_cnt = 0)
The first fma and the first add are exact additions to zero, so both bounds hold with room; they are compared WITHOUT a factor.

THE LOOP (`gaussian_loop`): tests/sampler_ref.py's loop with a stand-in whose prediction depends on the frame's POSITION k in its window of n:
    p = fp32(c(t) (1 + 0.25 (k - (n - 1) / 2) / n)) x  (+ fp32(m(t)) mu)              one product (two and a sum with mu), in fp32
so the windows that cover a frame disagree and the fuse matters.  A frame's average is e = sum_k w_k p_k / sum_k w_k.  Its error, handed to
`sampler_ref.step_reference` as d_eu / d_ec with counter 1:
    d_p  = |gain_k| d_x + u |gain_k x|                      (with mu: + u |m mu| + u |p|)
    d_S  = sum_k w_k d_p_k + m u sum_k |w_k p_k|            (the fmaf chain above)
    d_W  = m u sum_k w_k
    d_e  = (d_S + |e| d_W) / W (1 + 2^-10) + u |e|          (the division of the update kernel; second-order terms in the slack)
An unguided step is the same update at guidance 1 with a zero unconditional row (d_eu = 0) and no rescale: v = 0 + 1 (e_c - 0).

THE OPERATOR (`step_from_predictions`): the same average from predictions AS RECORDED (any dtype, exact in fp64, d_p = 0) and one update of the
latents as stored (d_x = 0), for the DDIM update of `cfg_ddim_kernel` (tests/step_gate.py CfgDdim states its fourteen roundings; here with d_eu, d_ec
handed in)."""
import torch

from tests import sampler_ref as R

F32, F64 = torch.float32, torch.float64
U = R.U
SLACK = R.SLACK


def open_windows(L, ctx, ov):
    if L <= ctx:
        return [list(range(L))]
    starts = list(range(0, L - ctx, ctx - ov)) + [L - ctx]
    return [list(range(j, j + ctx)) for j in starts]


def uniform_windows(L, ctx, ov):
    """context.uniform at context_stride 1 and step 0"""
    if L <= ctx:
        return [list(range(L))]
    return [[e % L for e in range(j, j + ctx)] for j in range(0, L, ctx - ov)]


def weights(name, n, o=4):
    """-> fp32 (n,) on the CPU"""
    if name == "flat":
        w = [1.0] * n
    elif name == "pyramid":
        w = [float(min(k + 1, n - k)) for k in range(n)]
    elif name == "ramp":
        w = [min(1.0, (k + 1) / (o + 1), (n - k) / (o + 1)) for k in range(n)]
    else:
        raise ValueError(name)
    return torch.tensor(w, dtype=F64).to(F32)


def guided_flags(timesteps, interval, num_train=1000):
    if interval is None:
        return [True] * len(timesteps)
    lo, hi = interval
    return [lo < (int(t) + 1) / num_train <= hi for t in timesteps]


def cover(windows, F):
    """per frame the list of (window number, position) that hold it, in list order"""
    cov = [[] for _ in range(F)]
    for n, win in enumerate(windows):
        for k, f in enumerate(win):
            cov[f].append((n, k))
    return cov


def accumulate_reference(preds, windows, w32, F):
    """preds: one tensor per window, (rows, C, Fw, ...) of any dtype; w32 fp32 (Fw,).  -> (sum fp64 (rows, C, F, ...), counter fp64 (F,), B_sum, B_cnt)
    for pred_sum and counter that start at zero."""
    p0 = preds[0]
    shape = tuple(p0.shape[:2]) + (F,) + tuple(p0.shape[3:])
    dev = p0.device
    S, A = torch.zeros(shape, dtype=F64, device=dev), torch.zeros(shape, dtype=F64, device=dev)
    W, m = torch.zeros(F, dtype=F64, device=dev), torch.zeros(F, dtype=F64, device=dev)
    w = w32.double().to(dev)
    wv = w.view((1, 1, -1) + (1,) * (p0.dim() - 3))
    for win, p in zip(windows, preds):
        idx = torch.tensor(win, device=dev)
        t = wv * p.double()
        S[:, :, idx] += t
        A[:, :, idx] += t.abs()
        W[idx] += w
        m[idx] += 1
    mv = m.view((1, 1, -1) + (1,) * (p0.dim() - 3))
    return S, W, mv * U * A, m * U * W


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------------------

def position_gain(c, k, n):
    """the stand-in's gain at position k of a window of n frames, as the fp32 number it multiplies with (back as a Python float)"""
    return R.f32(c * (1 + 0.25 * (k - (n - 1) / 2) / n))


def _fused_row(x, d_x, a_t, s, windows, w32, mu):
    """(e, d_e) of one row kind: x (1, C, F, h, w) fp64"""
    F = x.shape[2]
    n = len(windows[0])
    c = R.gaussian_v_gain(a_t, s)
    mt = None if mu is None else R.f32(R.gaussian_v_mean_gain(a_t, s)) * mu.double()
    S, A, D = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    W, m = torch.zeros(F, dtype=F64, device=x.device), torch.zeros(F, dtype=F64, device=x.device)
    w = w32.double().to(x.device)
    for win in windows:
        idx = torch.tensor(win, device=x.device)
        gain = torch.tensor([position_gain(c, k, n) for k in range(n)], dtype=F64, device=x.device).view(1, 1, n, 1, 1)
        xw, dxw = x[:, :, idx], d_x[:, :, idx]
        prod = gain * xw
        if mt is None:
            p = prod
            d_p = gain.abs() * dxw + U * prod.abs()
        else:
            p = prod + mt
            d_p = gain.abs() * dxw + U * (prod.abs() + mt.abs() + p.abs())
        wv = w.view(1, 1, n, 1, 1)
        S[:, :, idx] += wv * p
        A[:, :, idx] += wv * p.abs()
        D[:, :, idx] += wv * d_p
        W[idx] += w
        m[idx] += 1
    Wv, mv = W.view(1, 1, F, 1, 1), m.view(1, 1, F, 1, 1)
    e = S / Wv
    d_e = (D + mv * U * A + e.abs() * mv * U * Wv) / Wv * SLACK + U * e.abs()
    return e, d_e


def gaussian_loop(x_T, table, n_steps, rule, g, phi, s_u, s_c, windows, w32, flags=None, eta=0.0, noises=None, mu=None):
    """-> (latents fp64, bound).  windows: the clip's window list; w32: fp32 (Fw,) weights; flags: per step, whether it is guided (None: all).
    rule: "ddim" / "dpm" are mmgt_sampler_step's updates (sampler_ref.step_reference); "cfg_ddim" is the default path's cfg_ddim_kernel
    (`ddim_step_reference`; eta 0, no rescale)."""
    x = x_T.double()
    d_x = torch.zeros_like(x)
    x0p, d_xp = None, 0.0
    one = torch.ones((x.shape[2],), dtype=F32, device=x.device)
    steps = R.dpm_triples(table, n_steps) if rule == "dpm" else R.ddim_pairs(table, n_steps)
    ts = R.trailing_timesteps(n_steps, len(table))
    flags = [True] * n_steps if flags is None else flags
    for i, st in enumerate(steps):
        a_t = st[-2]
        ec, d_ec = _fused_row(x, d_x, a_t, s_c, windows, w32, mu)
        if flags[i]:
            eu, d_eu = _fused_row(x, d_x, a_t, s_u, windows, w32, mu)
            g_i, phi_i = g, phi
        else:
            eu, d_eu = torch.zeros_like(ec), torch.zeros_like(ec)
            g_i, phi_i = 1.0, 0.0
        if rule == "cfg_ddim":
            assert phi == 0.0 and eta == 0.0 and noises is None
            x, d_x = ddim_step_reference(eu, ec, d_eu, d_ec, x, g_i, *ddim_scalars(table, ts[i], n_steps), d_x=d_x)
            continue
        co = R.f32s(R.ddim_k(*st, eta) if rule == "ddim" else R.dpm_k(*st))
        x, x0, d_x, d_x0 = R.step_reference(torch.cat([eu, ec]), one, x, g_i, phi_i, co, x0_prev=x0p, z=None if noises is None else noises[i],
                                            d_x=d_x, d_xp=d_xp, d_eu=d_eu, d_ec=d_ec)
        x0p, d_xp = x0, d_x0
    return x, d_x


# ---- the operator's steps from its own recorded predictions -------------------------------------------------------------------------------------------

def ddim_step_reference(eu, ec, d_eu, d_ec, x, g, sa_t, sb_t, sa_p, sb_p, d_x=0.0):
    """cfg_ddim_kernel on averages eu, ec (fp64) with their errors handed in, the latents x as stored -> (new latents fp64, B): tests/step_gate.py
    CfgDdim.reference with d_eu, d_ec (and d_x, the error of the latents so far) from the caller; scalars as the fp32 arguments they become."""
    G_, SA_T, SB_T, SA_P, SB_P = R.f32s((g, sa_t, sb_t, sa_p, sb_p))
    u, xi = U, x.double()
    diff = ec - eu
    d_diff = d_eu + d_ec + u * diff.abs()
    gd = G_ * diff
    d_gd = abs(G_) * d_diff + u * gd.abs()
    v = eu + gd
    d_v = d_eu + d_gd + u * v.abs()
    p1, p2 = SA_T * xi, SB_T * v
    x0 = p1 - p2
    d_x0 = abs(SA_T) * d_x + u * p1.abs() + abs(SB_T) * d_v + u * p2.abs() + u * x0.abs()
    p3, p4 = SA_T * v, SB_T * xi
    e = p3 + p4
    d_e = abs(SA_T) * d_v + u * p3.abs() + abs(SB_T) * d_x + u * p4.abs() + u * e.abs()
    q1, q2 = SA_P * x0, SB_P * e
    ref = q1 + q2
    B = abs(SA_P) * d_x0 + u * q1.abs() + abs(SB_P) * d_e + u * q2.abs() + u * ref.abs()
    return ref, B * SLACK


def ddim_scalars(table, t, n_steps):
    """(sqrt a_t, sqrt(1 - a_t), sqrt a_s, sqrt(1 - a_s)) of the step leaving timestep t, s = t - 1000 // N, in the fp32 arithmetic of the fp32 table
    (scheduler.step_coefficients restated: the table and these four roundings ARE the definition of the kernel's arguments); a = 1 below timestep 0"""
    prev = int(t) - len(table) // n_steps
    a_t = table[int(t)]
    a_p = table[prev] if prev >= 0 else torch.tensor(1.0, dtype=F32)
    f = lambda v: float(v.to(F32))
    return f(a_t ** 0.5), f((1 - a_t) ** 0.5), f(a_p ** 0.5), f((1 - a_p) ** 0.5)


def step_from_predictions(preds_u, preds_c, windows, w32, x, g, co4):
    """One DDIM step (eta 0) of the pipeline from the operator's recorded predictions.  preds_c: per window (1, C, Fw, h, w) of the conditional row;
    preds_u: the same for the unconditional row, or None on an unguided step (guidance 1 over a zero row).  x: the latents before the step, as stored;
    co4: `ddim_scalars`.  -> (latents fp64, B)."""
    F = x.shape[2]

    def avg(preds):
        S, W, B_s, B_w = accumulate_reference(preds, windows, w32, F)
        Wv = W.view(1, 1, F, 1, 1)
        e = S / Wv
        return e, (B_s + e.abs() * B_w.view(1, 1, F, 1, 1)) / Wv * SLACK + U * e.abs()

    ec, d_ec = avg(preds_c)
    if preds_u is None:
        eu, d_eu, g = torch.zeros_like(ec), torch.zeros_like(ec), 1.0
    else:
        eu, d_eu = avg(preds_u)
    return ddim_step_reference(eu, ec, d_eu, d_ec, x, g, *co4)
