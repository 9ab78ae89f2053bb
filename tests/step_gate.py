"""The numeric gate of the kernels that run AROUND the hot bf16 kernels in every denoise step and every VAE decode (csrc/elementwise.hip, and
`mmgt_gemm_bf16_f32` of csrc/gemm16.hip), torch only, any device.  In the style of tests/mm_gate.py, whose U, U32, `ratio`, `check`, `guarded`,
`out_in_sentinels` and `assert_untouched` are reused.

Every kernel is a case class with `contract()` (the operation in fp64 on the operands AS STORED, only the kernel's own rounding points modelled),
`bound()` (B per element; `reference()` returns both, computed once), `simulate()` (the kernel's arithmetic in torch fp32 / bf16) and `mutants()`
({name: fp64 result of a subtly wrong kernel}).  The gate is  |out - ref| <= 2 B  on EVERY element.  u32 = 2^-24 is the fp32 unit roundoff, U = 2^-8
mm_gate's bf16 one.  Nothing below is fitted to kernel output; every term is read from the line it cites.  The file is built without fast-math
(csrc/Makefile:4): `expf`, `sinf`, `cosf` are the library functions (1 ulp = 2 u32 of the result each), `a * b + c` may or may not be contracted
into an fma, so both forms are bounded.

EXACT kernels (B = 0: the gate is torch.equal, `expected()` is what the kernel must store bit for bit)
  ncfhw_to_nhwc     elementwise.hip:44 one fp32 multiply, :48 / :51 the storage rounding  ==  (x * scale).to(dt) in fp32; pad channels 0 (:44).
  accumulate_window(s)   without weights, elementwise.hip:130 one fmaf(1, v, s) = s + v per target and window, :169-174 the windows that hold a frame
                    in list order  ==  the same adds by torch in that order; `accumulate_windows` == B sequential `accumulate_window` calls; a
                    frame in no window is not written (:175 `if (any)`), its counter not either in the value (:178-181 adds nothing).  The
                    counter: + 1.f per window.
  qk_split3         elementwise.hip:250-252 sum = (qk0 + qk1) + bias in fp32, :254 hi = bf16(sum), :257 lo = bf16(sum - hi), :264-269 the pieces
                    [hi | hi | lo] of Qp and [hi | lo | hi] of Kp.
  gemm_bf16_f32 on integers in {-2 .. 2}: every partial sum is an integer of magnitude <= 4 K < 2^24, exact in fp32 in any order.

BOUNDED kernels
  nhwc_to_ncfhw     elementwise.hip:68 v = x * scale + shift, :69 the clamp (exact, 1-Lipschitz).  Two roundings: u32 |x scale| (absent when the
                    compiler contracts to an fma) and u32 |v|:   B = u32 (|x scale| + |v|).
  timestep_features elementwise.hip:80 freq = expf(-9.210340371976184f * (float)k / (float)half): the constant's rounding, the product and the
                    quotient are (1 + u32)^3 - 1 =: r3 on the exponent e, expf is 1 ulp:  |d freq| <= freq (expm1(r3 |e|) + 2 u32);
                    :81 a = ts * freq rounds once more: |d a| <= |a| (expm1(r3 |e|) + 3 u32); :82 cosf / sinf are 1-Lipschitz and 1 ulp:
                        B = |a| (expm1(r3 |e|) + 3 u32) + 2 u32 |ref| + U |ref| (bf16 storage, common.h:42)
  silu              common.h:104 x / (1 + __expf(-x)): mm_gate's SiLU term (2^-21 + 2^-23 |x|) |ref| + U |ref| (bf16).  Where e^-x reaches 2^127
                    `__expf` may return inf and the quotient -0: B += |ref| there (|ref| < 2^-120).
  cfg_ddim_step     elementwise.hip:96-103.  Contracted, ten operations (two divisions, the difference, three fmas behind three products,
                    :103's product and fma); uncontracted fourteen.  Every one of the fourteen results contributes u32 of its magnitude, carried
                    through the linear steps behind it by the magnitudes of their coefficients (`CfgDdim.reference`): the contracted form
                    drops terms of this sum, so one B covers both.
  softmax_rows / softmax_rows_f32_bf16   elementwise.hip:193-200, :213-233.  z = x scale.  The reference maximum cancels in the quotient, so only
                    the ARGUMENT of every exponential matters: u32 |z| for the product (:194 / :218, absent in an fma), u32 |z - m| for the
                    difference, then `__expf` = v_exp_f32 (1 ulp) behind one multiply by log2 e (2 u32 |z - m|, as mm_gate states for SiLU):
                        eps_j = u32 (|z_j| + 3 |z_j - m| + 2)
                    The sum: cols / 64 serial adds per lane (:197 / :226) + six shuffle adds (common.h:155-159) of positive terms: D u32,
                    D = ceil(cols / 64) + 6, plus the terms' own errors sum_j p_j eps_j.  :199 one division (2 u32: a reciprocal of 1 ulp
                    if not correctly rounded), :200 / :233 one product (u32), then the storage rounding (U |ref|, bf16).  An exponential or a
                    probability below 2^-126 may be flushed: 2^-125 absolute.
                        B_j = p_j expm1(eps_j + sum_i p_i eps_i + (D + 3) u32) + U p_j (bf16) + 2^-125
  gemm_bf16_f32     gemm16.hip:720-737 raw fp32 accumulators of exact bf16 x bf16 products: (K + 2) u32 sum_k |a||w| (mm_gate LINEAR, no epilogue).
  logits chain      vae.py:267-275  t -> gemm_bf16_f32 with [Wq_hi; Wq_lo; Wk_hi; Wk_lo] -> qk_split3 -> gemm_bf16_f32, against the fp64
                    (t Wq^T + bq)(t Wk^T + bk)^T of the fp32 weights.  hi = bf16(x), lo = bf16(x - hi): |x - hi| <= U |x|, |x - hi - lo| <= U^2 |x| = 2^-16 |x|.
                        d_q = 2^-16 A_q + (C + 2) u32 A_q + 2 u32 (A_q + |bq|) + 2^-16 |q|,   A_q = sum_c |t_c||Wq_c|   (d_k likewise)
                          (the weight pieces; the first GEMM's accumulation of the hi and lo columns; elementwise.hip:250 two adds; the split)
                        B = sum_c (d_q |k| + |q| d_k) + (2^-16 + (3 C + 2) u32 (1 + 2^-7)) sum_c |q_c||k_c|
                          (the dropped lo x lo term; the second GEMM's accumulation over 3 C exact products)
                    i.e. a few 2^-16 sum_c |q_c||k_c| at C = 512 (worst case; the pieces keep 16 bits at least, 17 on average).

GRID-STRIDE.  `grid_for` (elementwise.hip:22-25) launches at most SWEEP = 8192 x 256 threads; the rest is walked in a grid-stride loop.  The mutant
`second sweep not written` leaves the sentinel in everything a thread index >= sweep writes; cases take `sweep` so that small CPU twins have one."""
import math

import torch

from tests.mm_gate import BF16, NAN, SENT, U, U32, _Case, assert_untouched, check, guarded, out_in_sentinels, ratio, rnd  # noqa: F401

F32, F64 = torch.float32, torch.float64
SWEEP = 8192 * 256
FLT_MAX = 3.4028234663852886e38
R3 = (1 + U32) ** 3 - 1
LN10000_F32 = 9.210340371976184          # elementwise.hip:80 (rounded to fp32 by `f32c`)
TINY = 2.0 ** -125


def f32c(v, device="cpu"):
    """a Python float as the fp32 kernel argument it becomes"""
    return torch.tensor(v, dtype=F32, device=device)


def rejected(mut, ref, B, dt, factor=2.0):
    """the gate refuses the mutant stored in `dt` (what a wrong kernel would leave in memory): some element not finite or beyond factor * B"""
    m = mut.to(F32).to(dt)
    if not torch.isfinite(m.float()).all():
        return True
    return bool((ratio(m, ref, B) > factor).any())


def worst(mut, ref, B, dt):
    m = mut.to(F32).to(dt)
    x = ratio(m, ref, B)
    return float("inf") if not torch.isfinite(m.float()).all() else x.max().item()


def flat_accepts(out, ref, rtol, atol):
    """torch.testing.assert_close's criterion"""
    return bool(((out.double() - ref).abs() <= atol + rtol * ref.abs()).all())


def unswept(t, per_thread, sweep):
    """`t` with the sentinel in everything that thread indices >= sweep write (per_thread consecutive elements each)"""
    flat = t.clone().reshape(-1)
    flat[sweep * per_thread:] = SENT
    return flat.reshape(t.shape)


def _gather_or_nan(flat, idx):
    """flat[idx] with NaN where idx runs past the allocation (what lies there is not the kernel's to read)"""
    ext = torch.cat([flat.reshape(-1), torch.full((1,), NAN, dtype=flat.dtype, device=flat.device)])
    return ext[torch.where(idx < flat.numel(), idx, torch.full_like(idx, flat.numel()))]


class _Exact(_Case):
    """B = 0: `expected()` bit for bit"""

    def reference(self):
        e = self.expected().double()
        return e, torch.zeros_like(e)

    def simulate(self):
        return self.expected()


# ---- layout ----------------------------------------------------------------------------------------------------------------------------------

class ToNhwc(_Exact):
    """x (B, C, F, H, W) fp32 -> (B F, H, W, cpad) dt = (x * scale).to(dt), pad channels zero"""

    def __init__(self, what, x, cpad, dt, scale=1.0, sweep=SWEEP):
        self.what, self.x, self.cpad, self.dt, self.scale, self.sweep = what, x, cpad, dt, scale, sweep

    def expected(self):
        B, C, F, H, W = self.x.shape
        out = torch.zeros((B * F, H, W, self.cpad), dtype=self.dt, device=self.x.device)
        out[..., :C] = (self.x * f32c(self.scale, self.x.device)).to(self.dt).permute(0, 2, 3, 4, 1).reshape(B * F, H, W, C)
        return out

    def mutants(self):
        x, dev = self.x, self.x.device
        B, C, F, H, W = x.shape
        HW, cp = H * W, self.cpad
        exp = self.expected().double()
        m = {}
        if B * F * HW * (cp // 8) > self.sweep:
            m["second sweep not written"] = unswept(exp, 8, self.sweep)
        if cp > C:      # elementwise.hip:44 `c < Cpad`: the pad channels read the planes behind channel C - 1
            b = torch.arange(B, device=dev)[:, None, None, None]
            f = torch.arange(F, device=dev)[None, :, None, None]
            p = torch.arange(HW, device=dev)[None, None, :, None]
            c = torch.arange(cp, device=dev)[None, None, None, :]
            v = _gather_or_nan(x, ((b * C + c) * F + f) * HW + p)
            m["channel tail compared against Cpad"] = (v * f32c(self.scale, dev)).to(self.dt).double().reshape(B * F, H, W, cp)
        if self.dt == BF16 and math.log2(abs(self.scale)) % 1:
            t = exp.clone()
            t[..., :C] = (x.to(BF16).float() * f32c(self.scale, dev)).to(BF16).double().permute(0, 2, 3, 4, 1).reshape(B * F, H, W, C)
            m["scale applied after the rounding"] = t
        if F > 1 and C > 1:
            t = exp.clone()
            t[..., :C] = (x * f32c(self.scale, dev)).to(self.dt).double().reshape(B, F, C, HW).permute(0, 1, 3, 2).reshape(B * F, H, W, C)
            m["f and c exchanged"] = t
        return m


class FromNhwc(_Case):
    """x (B F, H, W, cpad) dt -> (B, C, F, H, W) fp32 = clamp(x * scale + shift)"""

    def __init__(self, what, x, B, C, scale=1.0, shift=0.0, clamp01=False, sweep=SWEEP):
        self.what, self.x, self.B, self.C, self.scale, self.shift, self.clamp01, self.sweep = what, x, B, C, scale, shift, clamp01, sweep
        self.dt = F32
        self._ref = None

    def _ncfhw(self, v):
        BF, H, W, C = v.shape
        return v.reshape(self.B, BF // self.B, H, W, C).permute(0, 4, 1, 2, 3).contiguous()

    def _affine(self, xs, clamp_first=False):
        dev = xs.device
        s, sh = f32c(self.scale, dev).double(), f32c(self.shift, dev).double()
        if clamp_first:
            return (xs * s).clamp(0.0, 1.0) + sh
        v = xs * s + sh
        return v.clamp(0.0, 1.0) if self.clamp01 else v

    def reference(self):
        if self._ref is None:
            xs = self._ncfhw(self.x[..., :self.C]).double()
            s, sh = f32c(self.scale, xs.device).double(), f32c(self.shift, xs.device).double()
            self._ref = (self._affine(xs), U32 * ((xs * s).abs() + (xs * s + sh).abs()))
        return self._ref

    def simulate(self):
        dev = self.x.device
        v = self._ncfhw(self.x[..., :self.C]).float() * f32c(self.scale, dev) + f32c(self.shift, dev)
        return v.clamp(0.0, 1.0) if self.clamp01 else v

    def mutants(self):
        ref, _ = self.reference()
        x, dev = self.x, self.x.device
        BF, H, W, cp = x.shape
        B, C, F, HW = self.B, self.C, BF // self.B, H * W
        m = {}
        if ref.numel() > self.sweep:
            m["second sweep not written"] = unswept(ref, 1, self.sweep)
        if cp > C and B > 1:      # elementwise.hip:66-67 `t % Cpad`, `t / Cpad` (one batch entry: t < C, nothing changes)
            i = torch.arange(B * C * F * HW, device=dev)
            p, t = i % HW, i // HW
            f, t = t % F, t // F
            c, b = t % cp, t // cp
            m["channel tail compared against Cpad"] = self._affine(_gather_or_nan(x.double(), ((b * F + f) * HW + p) * cp + c)).reshape(ref.shape)
        if self.clamp01:
            m["clamp before shift"] = self._affine(self._ncfhw(x[..., :C]).double(), clamp_first=True)
        if F > 1 and C > 1:
            m["f and c exchanged"] = ref.permute(0, 2, 1, 3, 4).contiguous().reshape(ref.shape)
        return m


# ---- timestep features, SiLU -------------------------------------------------------------------------------------------------------------------

class Timestep(_Case):
    """ts (B,) fp32 -> (B, dim) dt = [cos(ts freq_k) | sin(ts freq_k)], freq_k = exp(-ln(10000) k / half)"""

    def __init__(self, what, ts, dim, dt, sweep=SWEEP):
        self.what, self.ts, self.dim, self.dt, self.sweep = what, ts, dim, dt, sweep
        self._ref = None

    def _feat(self, const=math.log(10000.0), den=None, sin_first=False, arg_rel=0.0):
        half = self.dim // 2
        k = torch.arange(half, dtype=F64, device=self.ts.device)
        e = -const * k / (half if den is None else den)
        a = self.ts.double()[:, None] * torch.exp(e)[None, :] * (1.0 + arg_rel)
        parts = [torch.sin(a), torch.cos(a)] if sin_first else [torch.cos(a), torch.sin(a)]
        return torch.cat(parts, 1), a, e

    def reference(self):
        if self._ref is None:
            ref, a, e = self._feat()
            da = a.abs() * (torch.expm1(R3 * e.abs())[None, :] + 3 * U32)
            B = torch.cat([da, da], 1) + 2 * U32 * ref.abs() + (U * ref.abs() if self.dt == BF16 else 0.0)
            self._ref = (ref, B)
        return self._ref

    def simulate(self):
        dev = self.ts.device
        half = self.dim // 2
        k = torch.arange(half, dtype=F32, device=dev)
        freq = torch.exp(-f32c(LN10000_F32, dev) * k / f32c(float(half), dev))
        a = self.ts[:, None] * freq[None, :]
        return torch.cat([torch.cos(a), torch.sin(a)], 1).to(self.dt)

    def mutants(self):
        ref, _ = self.reference()
        m = {"denominator half - 1": self._feat(den=self.dim // 2 - 1)[0],
             "sin first": self._feat(sin_first=True)[0],
             "ln(10000) replaced by 9.21": self._feat(const=9.21)[0],
             "argument with a 2^-12 relative error (a native sin)": self._feat(arg_rel=2.0 ** -12)[0]}
        if ref.numel() > self.sweep:
            m["second sweep not written"] = unswept(ref, 1, self.sweep)
        return m


class Silu(_Case):
    """x (n,) dt -> x / (1 + exp(-x)) in dt"""

    def __init__(self, what, x, sweep=SWEEP):
        self.what, self.x, self.dt, self.sweep = what, x, x.dtype, sweep
        self._ref = None

    def reference(self):
        if self._ref is None:
            x = self.x.double()
            ref = x * torch.sigmoid(x)
            B = (2.0 ** -21 + 2.0 ** -23 * x.abs()) * ref.abs() + (U * ref.abs() if self.dt == BF16 else 0.0)
            B = B + torch.where(-x >= 127 * math.log(2.0), ref.abs(), torch.zeros_like(ref))
            self._ref = (ref, B)
        return self._ref

    def simulate(self):
        x = self.x.float()
        return (x / (1.0 + torch.exp(-x))).to(self.dt)

    def mutants(self):
        ref, _ = self.reference()
        x = self.x.double()
        m = {"quick_gelu's 1.702 x in the exponential": x * torch.sigmoid(1.702 * x)             }
        if self.dt == F32:          # (a relative 2^-9 is below what a bf16 output can show)
            m["the exponential rounded to bf16"] = x / (1.0 + torch.exp(-x).float().to(BF16).double())
        if ref.numel() > self.sweep:
            m["second sweep not written"] = unswept(ref, 1, self.sweep)
        return m


# ---- CFG + DDIM ----------------------------------------------------------------------------------------------------------------------------------

class CfgDdim(_Case):
    """pred_sum (2, C, F, H, W), counter (F,), latents (1, C, F, H, W) fp32, the five fp32 scalars -> new latents (elementwise.hip:92-105)"""

    def __init__(self, what, ps, counter, lat, g, sa_t, sb_t, sa_p, sb_p, sweep=SWEEP):
        self.what, self.ps, self.counter, self.lat, self.sc, self.sweep = what, ps, counter, lat, (g, sa_t, sb_t, sa_p, sb_p), sweep
        self.dt = F32
        self._ref = None

    def _scalars(self):
        return [f32c(v, self.lat.device).double() for v in self.sc]

    def _cnt(self, frames=None):
        """the counter of every element (1, 1, F, 1, 1), or of `frames` (a flat per-element frame index)"""
        c = self.counter.double()
        if frames is None:
            return c[None, None, :, None, None]
        return c[frames].reshape(self.lat.shape)

    def _step(self, eu, ec, swap_p=False, x0_sb=False):
        g, sa_t, sb_t, sa_p, sb_p = self._scalars()
        xi = self.lat.double()
        v = eu + g * (ec - eu)
        x0 = sa_t * xi - sb_t * v
        e = sa_t * v + sb_t * xi
        return sb_p * x0 + sa_p * e if x0_sb else sa_p * x0 + sb_p * e

    def reference(self):
        if self._ref is None:
            g, sa_t, sb_t, sa_p, sb_p = [s.abs() for s in self._scalars()]
            G_, SA_T, SB_T, SA_P, SB_P = self._scalars()
            xi, cnt = self.lat.double(), self._cnt()
            eu, ec = self.ps[0:1].double() / cnt, self.ps[1:2].double() / cnt
            u = U32
            d_eu, d_ec = u * eu.abs(), u * ec.abs()                                   # :98 two divisions
            diff = ec - eu
            d_diff = d_eu + d_ec + u * diff.abs()                                     # :99 ec - eu
            gd = G_ * diff
            d_gd = g * d_diff + u * gd.abs()                                          # :99 g * (..)   (no rounding in an fma)
            v = eu + gd
            d_v = d_eu + d_gd + u * v.abs()                                           # :99 eu + ..
            p1, p2 = SA_T * xi, SB_T * v
            x0 = p1 - p2
            d_x0 = u * p1.abs() + sb_t * d_v + u * p2.abs() + u * x0.abs()            # :101 two products, one difference
            p3, p4 = SA_T * v, SB_T * xi
            e = p3 + p4
            d_e = sa_t * d_v + u * p3.abs() + u * p4.abs() + u * e.abs()              # :102
            q1, q2 = SA_P * x0, SB_P * e
            ref = q1 + q2
            B = sa_p * d_x0 + u * q1.abs() + sb_p * d_e + u * q2.abs() + u * ref.abs()   # :103
            self._ref = (ref, B * (1 + 2.0 ** -20))                                   # (the second-order terms: below 16 u32 of B)
        return self._ref

    def simulate(self):
        g, sa_t, sb_t, sa_p, sb_p = [f32c(v, self.lat.device) for v in self.sc]
        cnt = self.counter[None, None, :, None, None]
        eu, ec = self.ps[0:1] / cnt, self.ps[1:2] / cnt
        v = eu + g * (ec - eu)
        x0 = sa_t * self.lat - sb_t * v
        e = sa_t * v + sb_t * self.lat
        return sa_p * x0 + sb_p * e

    def mutants(self):
        ref, _ = self.reference()
        _, C, F, H, W = self.lat.shape
        hw, n = H * W, self.lat.numel()
        ps0, ps1 = self.ps[0:1].double(), self.ps[1:2].double()
        cnt = self._cnt()
        i = torch.arange(n, device=self.lat.device)
        hw_wrong = max(1, (H // 2) * (W // 2))                   # the level below
        cw = self._cnt((i // hw_wrong) % F)
        c0 = self.counter.double()[0]
        m = {"counter read at (i / hw) % F with the hw of the wrong level": self._step(ps0 / cw, ps1 / cw),
             "counter of frame 0 for all frames": self._step(ps0 / c0, ps1 / c0),
             "eu and ec exchanged": self._step(ps1 / cnt, ps0 / cnt),
             "sb_p applied to x0": self._step(ps0 / cnt, ps1 / cnt, x0_sb=True),
             "division by the counter dropped": self._step(ps0, ps1)}
        if n > self.sweep:
            m["second sweep not written"] = unswept(ref, 1, self.sweep)
        return m


# ---- window accumulation ---------------------------------------------------------------------------------------------------------------------------

SNAN_BITS = 0x7FA00000           # a signalling NaN: `acc + 0` would quiet it (0x7FE00000), an untouched frame keeps it


def bits(t):
    return t.contiguous().view(torch.int32)


def fill_unwritten(ps, frames):
    """frames[0] of pred_sum becomes a signalling NaN throughout, frames[1] likewise except channel 0 = -0.0 (`-0.0 + 0` is +0.0): a kernel that
    rewrites a frame in no window changes the bits of both"""
    pat = torch.full((), SNAN_BITS, dtype=torch.int32, device=ps.device).view(F32)
    for n, f in enumerate(frames):
        ps[:, :, f] = pat
        if n == 1:
            ps[:, 0, f] = -0.0
    return ps


class Acc(_Exact):
    """pred ((rows B Fw), H, W, cpad) in CFG row major order [row][window][j], windows (B, Fw) int, pred_sum (2, C, F, H, W) and counter (F,) as
    they stand BEFORE the call.  expected() -> (pred_sum, counter) after it: the windows added in list order, bit for bit."""

    def __init__(self, what, pred, ps0, cnt0, windows, C, rows=2, row0=0, bump=True, sweep=SWEEP, unwritten=()):
        self.unwritten = tuple(unwritten)              # frames in no window that `fill_unwritten` prepared
        self.what, self.pred, self.ps0, self.cnt0, self.C, self.rows, self.row0, self.bump, self.sweep = what, pred, ps0, cnt0, C, rows, row0, bump, sweep
        self.windows = [list(map(int, w)) for w in windows]
        self.dt = F32

    def window_pred(self, k):
        """the slice of pred that a sequential `accumulate_window` call takes for window k: ((rows Fw), H, W, cpad)"""
        nw, Fw = len(self.windows), len(self.windows[0])
        p = self.pred.reshape((self.rows, nw, Fw) + tuple(self.pred.shape[1:]))
        return p[:, k].reshape((self.rows * Fw,) + tuple(self.pred.shape[1:])).contiguous()

    def expected(self, order=None, idx_of=None, bump_below=None, rewrite=False):
        """(pred_sum, counter).  order: the windows' order; idx_of(window) -> the frames its slices go to; bump_below: only positions j below it
        bump the counter; rewrite: every frame is rewritten with `acc + 0`."""
        ps, cnt = self.ps0.clone(), self.cnt0.clone()
        H, W = self.pred.shape[1:3]
        Fw = len(self.windows[0])
        for k in (range(len(self.windows)) if order is None else order):
            win = self.windows[k]
            tgt = torch.tensor(win if idx_of is None else idx_of(win), device=ps.device)
            p5 = self.window_pred(k)[..., :self.C].float().reshape(self.rows, Fw, H, W, self.C).permute(0, 4, 1, 2, 3)
            ps[self.row0:self.row0 + self.rows, :, tgt] += p5                # distinct frames in a window: one fp32 add per target
            if self.bump:
                b = torch.tensor(win[:Fw if bump_below is None else bump_below], device=ps.device)
                cnt[b] += 1.0
        if rewrite:
            ps = ps + 0.0
        return ps, cnt

    def reference(self):
        ps, cnt = self.expected()
        return (ps.double(), cnt.double()), (torch.zeros_like(ps, dtype=F64), torch.zeros_like(cnt, dtype=F64))

    def mutants(self):
        """{name: (pred_sum, counter)} fp32: compared through `bits`"""
        Fw, nw = len(self.windows[0]), len(self.windows)
        m = {"the idx[j] of the previous j": self.expected(idx_of=lambda w: w[-1:] + w[:-1])}
        if Fw > 64 and self.bump:
            m["counter bumped only for j < 64"] = self.expected(bump_below=64)
        if nw > 1:
            m["windows added in reverse list order"] = self.expected(order=range(nw - 1, -1, -1))
        if self.unwritten:              # (x + 0 keeps the bits of every other value: only the prepared frames can tell)
            assert not {f for w in self.windows for f in w} & set(self.unwritten)
            m["a frame in no window rewritten with acc + 0"] = self.expected(rewrite=True)
        total = self.rows * self.C * Fw * self.pred.shape[1] * self.pred.shape[2]
        if nw == 1 and total > self.sweep:                        # (accumulate_windows has no grid-stride loop: one thread per target)
            H, W = self.pred.shape[1:3]
            p5 = self.window_pred(0)[..., :self.C].float().reshape(self.rows, Fw, H, W, self.C).permute(0, 4, 1, 2, 3).contiguous()
            p5.reshape(-1)[self.sweep:] = 0.0                      # thread index = ((b C + c) Fw + j) hw + p: p5's own order
            ps, cnt = self.ps0.clone(), self.expected()[1]
            ps[self.row0:self.row0 + self.rows, :, torch.tensor(self.windows[0], device=ps.device)] += p5
            m["second sweep not added"] = (ps, cnt)
        return m


def same_bits(got, want):
    return torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))


# ---- softmax ---------------------------------------------------------------------------------------------------------------------------------------

class Softmax(_Case):
    """x (rows, cols) fp32 / bf16 (a view of any row stride) -> softmax(x * scale) rows in out_dt; drop: the width of the kernel's last vector (4:
    softmax_rows_f32_bf16, 1: softmax_rows)"""

    def __init__(self, what, x, scale, out_dt, drop=1):
        self.what, self.x, self.scale, self.dt, self.drop = what, x, scale, out_dt, drop
        self._ref = None

    def z(self):
        return self.x.double() * f32c(self.scale, self.x.device).double()

    def reference(self):
        if self._ref is None:
            z = self.z()
            m = z.amax(1, keepdim=True)
            p = torch.softmax(z, 1)
            eps = U32 * (z.abs() + 3 * (z - m).abs() + 2)
            D = -(-z.shape[1] // 64) + 6
            rel = torch.expm1(eps + (p * eps).sum(1, keepdim=True) + (D + 3) * U32)
            self._ref = (p, p * rel + (U * p if self.dt == BF16 else 0.0) + TINY)
        return self._ref

    def simulate(self):
        z = self.x.float() * f32c(self.scale, self.x.device)
        e = torch.exp(z - z.amax(1, keepdim=True))
        return (e * (1.0 / e.sum(1, keepdim=True))).to(self.dt)

    def _overflowing(self, z, m):
        """softmax with the reference m in fp32 range: an exponential beyond FLT_MAX is inf, inf * 0 and inf / inf are NaN"""
        e = torch.exp(z - m)
        e = torch.where(e > FLT_MAX, torch.full_like(e, float("inf")), e)
        return e * (1.0 / e.sum(1, keepdim=True))

    def mutants(self):
        z = self.z()
        cols = z.shape[1]
        m = {}
        if cols > 64 and (z.amax(1) - z[:, :64].amax(1)).max().item() > 89.0:
            m["the maximum over the first 64-column slice only"] = self._overflowing(z, z[:, :64].amax(1, keepdim=True))
        if self.dt == F32 and cols > 1:          # (a relative 2^-9 on the sum is below what a bf16 output can show)
            e = torch.exp(z - z.amax(1, keepdim=True))
            m["the sum over bf16-rounded exponentials"] = e / e.float().to(BF16).double().sum(1, keepdim=True)
        if cols > self.drop:
            zz = z[:, :cols - self.drop]
            mm = zz.amax(1, keepdim=True)
            m["the last vector of a row dropped"] = self._overflowing(z, mm) * torch.exp(z - mm).sum(1, keepdim=True) / torch.exp(zz - mm).sum(1, keepdim=True)
        return m


# ---- the split-operand GEMM path --------------------------------------------------------------------------------------------------------------------

def hi_lo(x):
    """fp32 -> (hi, lo) bf16, hi = bf16(x), lo = bf16(x - hi) (vae.py:195-197, elementwise.hip:253-258)"""
    hi = x.to(BF16)
    return hi, (x - hi.float()).to(BF16)


class Split3(_Exact):
    """qk (rows, 4 C) fp32, bias_q, bias_k (C,) fp32 -> (Qp, Kp) bf16 (rows, 3 C)"""

    def __init__(self, what, qk, bq, bk):
        self.what, self.qk, self.bq, self.bk, self.dt = what, qk, bq, bk, BF16

    def sums(self):
        C = self.bq.shape[0]
        qk = self.qk
        return (qk[:, :C] + qk[:, C:2 * C]) + self.bq, (qk[:, 2 * C:3 * C] + qk[:, 3 * C:]) + self.bk

    def expected(self, lo_truncated=False, k_in_q_order=False):
        def pieces(x):
            hi = x.to(BF16)
            d = x - hi.float()
            lo = (d.view(torch.int32) & -65536).view(F32).to(BF16) if lo_truncated else d.to(BF16)
            return hi, lo
        (qh, ql), (kh, kl) = [pieces(s) for s in self.sums()]
        return torch.cat([qh, qh, ql], 1), torch.cat([kh, kh, kl] if k_in_q_order else [kh, kl, kh], 1)

    def reference(self):
        q, k = self.expected()
        return (q.double(), k.double()), (torch.zeros_like(q, dtype=F64), torch.zeros_like(k, dtype=F64))

    def mutants(self):
        return {"lo from the unrounded difference, truncated": self.expected(lo_truncated=True),
                "Kp in Qp's order": self.expected(k_in_q_order=True)}


class GemmF32(_Case):
    """a (M, K), w (N, K) bf16 views -> fp32 (M, N) raw accumulators.  exact: integer operands in {-2 .. 2}, B = 0.  tile / resident: the
    persistent loop's tile edge and workgroup count for the second-tile mutant (gemm16.hip:574-577: 256 x 256 tiles on the CUs of the device)."""

    def __init__(self, what, a, w, exact=False, tile=256, resident=256):
        self.what, self.a, self.w, self.exact, self.tile, self.resident, self.dt = what, a, w, exact, tile, resident, F32
        self._ref = None

    def reference(self):
        if self._ref is None:
            a, w = self.a.double(), self.w.double()
            ref = a @ w.t()
            if self.exact:
                assert a.abs().max() <= 2 and w.abs().max() <= 2 and (a == a.round()).all() and (w == w.round()).all()
                B = torch.zeros_like(ref)
            else:
                B = (self.a.shape[1] + 2) * U32 * (a.abs() @ w.abs().t())
            self._ref = (ref, B)
        return self._ref

    def simulate(self):
        return self.a.float() @ self.w.float().t()

    def mutants(self):
        ref, _ = self.reference()
        a, w = self.a.double(), self.w.double()
        M, K = a.shape
        N, T = w.shape[0], self.tile
        m = {"last 64-wide K chunk dropped": a[:, :K - 64] @ w[:, :K - 64].t()} if K > 64 else {"last 64-wide K chunk dropped": torch.zeros_like(ref)}
        tm, tn = -(-M // T), -(-N // T)
        if tm * tn > self.resident and tm > 1:
            t = ref.clone()
            shifted = ref.roll(-T, 0)
            for tile in range(self.resident, tm * tn):
                r, c = divmod(tile, tn)
                t[r * T:(r + 1) * T, c * T:(c + 1) * T] = shifted[r * T:(r + 1) * T, c * T:(c + 1) * T]
            m["rows offset by one tile on a workgroup's second tile"] = t
        return m


class Logits(_Case):
    """t (n, C) bf16, Wq, Wk (C, C), bq, bk (C,) fp32 -> fp32 (n, n) logits through the operand pieces (vae.py:267-275).  B carries the WORST case
    of the first GEMM's accumulation, (C + 2) u32 A_q with A_q = sum |t||W| about sqrt(C) |q|: at C = 512 that is more than rounding q and k to bf16
    costs on AVERAGE, so the end-to-end gate tells the mutants below at small C only; the GPU test holds every stage to its own contract as well
    (GemmF32 on the operands handed to each GEMM, Split3 bit for bit), which does tell them at any C."""

    def __init__(self, what, t, wq, wk, bq, bk):
        self.what, self.t, self.wq, self.wk, self.bq, self.bk, self.dt = what, t, wq, wk, bq, bk, F32
        self._ref = None

    def w4(self):
        qh, ql = hi_lo(self.wq)
        kh, kl = hi_lo(self.wk)
        return torch.cat([qh, ql, kh, kl], 0).contiguous()

    def reference(self):
        if self._ref is None:
            t = self.t.double()
            C = t.shape[1]
            q, k = t @ self.wq.double().t() + self.bq.double(), t @ self.wk.double().t() + self.bk.double()
            dq, dk = [(2.0 ** -16 + (C + 2) * U32) * (t.abs() @ w.double().abs().t()) + 2 * U32 * (t.abs() @ w.double().abs().t() + b.double().abs())
                      + 2.0 ** -16 * x.abs() for w, b, x in ((self.wq, self.bq, q), (self.wk, self.bk, k))]
            B = dq @ k.abs().t() + q.abs() @ dk.t() + (2.0 ** -16 + (3 * C + 2) * U32 * (1 + 2.0 ** -7)) * (q.abs() @ k.abs().t())
            self._ref = (q @ k.t(), B)
        return self._ref

    def simulate(self):
        qk = self.t.float() @ self.w4().float().t()
        Qp, Kp = Split3("", qk, self.bq, self.bk).expected()
        return Qp.float() @ Kp.float().t()

    def mutants(self):
        t = self.t.double()
        q, k = t @ self.wq.double().t() + self.bq.double(), t @ self.wk.double().t() + self.bk.double()
        b = lambda x: x.float().to(BF16).double()
        return {"q and k rounded to bf16 (no lo pieces)": b(q) @ b(k).t(),
                "the weights' lo pieces dropped": (t @ b(self.wq).t() + self.bq.double()) @ (t @ b(self.wk).t() + self.bk.double()).t(),
                "Kp in Qp's order": b(q) @ b(k).t() + b(q) @ b(k).t() + (q - b(q)) @ (k - b(k)).t(),
                "the key bias dropped": q @ (k - self.bk.double()).t()}


# ---- operands (values depend on (tag, shape) alone: the CPU tests and the GPU tests of one family draw from the same recipe) -------------------------

def softmax_input(tag, rows, cols, scale, dt, device="cpu"):
    """(rows, cols) logits x with x * scale of five kinds, row r of kind r % 5: 0 random in +-3 / scale; 1 flat (all 2.0); 2 peaked (one logit
    60 above a +-1 background, in the LAST column for the first such row); 3 wide (|x scale| up to 100); 4 a step (the first 64 columns at -95, the
    rest wide: the maximum lies far above anything in the first slice)"""
    x = rnd(f"{tag}.x", (rows, cols), 1.0, device=device)
    z = torch.empty_like(x)
    for r in range(rows):
        kind = r % 5
        if kind == 0:
            z[r] = 3.0 * x[r]
        elif kind == 1:
            z[r] = 2.0
        elif kind == 2:
            z[r] = x[r]
            z[r, cols - 1 if r == 2 else (r * 37) % cols] += 60.0
        elif kind == 3:
            z[r] = 100.0 * x[r]
        else:
            z[r] = 100.0 * x[r]
            z[r, :64] = -95.0
            if cols > 64:
                z[r, 64 + (r * 37) % (cols - 64)] = 99.0
    return (z / scale).to(dt)


def ddim_scalars(step, steps=20):
    """(sa_t, sb_t, sa_p, sb_p) of step `step` (0 = the first, steps - 1 = the last) of a `steps`-step schedule"""
    from mmgt_amd.scheduler import DDIMScheduler
    s = DDIMScheduler()
    s.set_timesteps(steps)
    return s.step_coefficients(int(s.timesteps[step]))


def cfg_case(tag, C, F, H, W, guidance, step, device="cpu", sweep=SWEEP, equal_counter=None):
    """pred_sum = counter x hash_uniform (a sum of `counter` predictions), counter = 1 .. F (or `equal_counter` everywhere), latents hash_uniform"""
    cnt = torch.arange(1, F + 1, dtype=F32, device=device) if equal_counter is None else torch.full((F,), float(equal_counter), device=device)
    ps = guarded(rnd(f"{tag}.ps", (2, C, F, H, W), 1.0, device=device) * cnt[None, None, :, None, None])
    lat = guarded(rnd(f"{tag}.lat", (1, C, F, H, W), 1.0, device=device))
    return CfgDdim(f"{tag} cfg_ddim {C} x {F} x {H} x {W} g {guidance} step {step}", ps, cnt, lat, guidance, *ddim_scalars(step), sweep=sweep)


def acc_case(tag, windows, F, C, cpad, H, W, dt, device="cpu", rows=2, row0=0, bump=True, sweep=SWEEP, unwritten=()):
    """pred hash_uniform with NaN in the channels >= C, pred_sum hash_uniform x 3 and counter hash_uniform + 2 prefilled; `unwritten`: two frames in
    no window, filled by `fill_unwritten`"""
    nw, Fw = len(windows), len(windows[0])
    pred = rnd(f"{tag}.pred", (rows * nw * Fw, H, W, cpad), 1.0, dt, device)
    pred[..., C:] = NAN
    ps = fill_unwritten(rnd(f"{tag}.ps", (2, C, F, H, W), 3.0, device=device), unwritten)
    cnt = rnd(f"{tag}.cnt", (F,), 1.0, device=device) + 2.0
    return Acc(f"{tag} accumulate {nw} x {Fw} of {F}, C {C} / {cpad}, {H} x {W}, rows {rows} @ {row0}, {str(dt)[6:]}", guarded(pred), ps, cnt, windows, C,
               rows, row0, bump, sweep, unwritten)


def shuffled(n, F):
    """n distinct frames of F in a non-monotonic order"""
    return [(7 * i + 3) % F for i in range(F)][:n] if math.gcd(7, F) == 1 else list(range(n))[::-1]


def int_operand(tag, shape, device="cpu"):
    """integers in {-2 .. 2} as bf16"""
    return (rnd(tag, shape, 2.49, device=device)).round().to(BF16)


def logits_case(tag, n, C, gain, device="cpu"):
    t = guarded(rnd(f"{tag}.t", (n, C), 1.5, BF16, device))
    wq, wk = [rnd(f"{tag}.{x}", (C, C), gain / math.sqrt(C), device=device) for x in ("wq", "wk")]
    bq, bk = [rnd(f"{tag}.{x}", (C,), 0.5, device=device) for x in ("bq", "bk")]
    return Logits(f"{tag} logits n {n} C {C} gain {gain}", t, wq, wk, bq, bk)
