"""The numeric gate of the bf16 GEMM, conv and norm kernels (csrc/gemm.hip, gemm16.hip, elementwise.hip conv_taps_gather, norm.hip), torch only,
any device.  In the style of tests/attn_gate.py, whose U = 2^-8, `ratio` and `old_gate_accepts` are reused.

Every family is a case class (`Linear`, `Conv`, `Taps`, `Norm`) with `contract()` (the operation in fp64 on the operands AS STORED, only the
kernel's documented rounding points modelled), `bound()` (B per element; `reference()` returns both, computed once), `simulate()` (the kernel's
arithmetic in torch fp32 / bf16) and `mutants()` ({name: fp64 reference of what a subtly wrong kernel would compute}).  The gate is  |out - ref| <= 2 B  on EVERY element (`check`).  u32 = 2^-24 is the fp32 unit roundoff.  Nothing below is fitted to kernel
output; every term is read from the code it cites.

LINEAR  (gemm, gemm_post, batched, conv1x1_cat, GEGLU; the convs reduce to it over their gathered reduction)
  Order of the epilogue, the same in all three implementations -- the vectorised path of the 32x32 tiles (gemm.hip:474-505 bias as one more K-step,
  :552-560 GEGLU / :562-577 activation, :578 `v *= rs` with rs = row_scale[m] * alpha (:518), :592-598 bias_post, :600-606 residual, :609 one
  rounding), their element-wise FULL path (gemm.hip:681 bias, :686 GEGLU, :689 bias2, :690-694 activation, :695 scale, :696 bias_post, :698
  residual, :699 store) and the 16x16 core (gemm16.hip:193-196 the accumulators START from bias + bias2, :477-483 GEGLU, :502 fma(x, rs, bias_post),
  :510 residual, :514 one rounding; split-K: :609-626 slabs summed in slice order, bias, bias2, residual, one rounding):
      pre = acc + bias[n] + bias2[m / bias2_rows][n];   t = act(pre)  or  h * gelu(g) of the packed (h, g) pair;
      ref = t * (row_scale[m] * alpha) + bias_post[n] + residual[m][n],  rounded ONCE to the storage type.
  The activation comes BEFORE the scale (gemm.hip:562-578, :690-695); no caller combines the two, and `contract` follows the code.
  B = U |ref|                                                         the one output rounding (half an ulp) + half an ulp of slack
    + |s| L [ (K + 4) u32 (sum_k |a||w| + |bias| + |bias2|)           fp32 accumulation: every product is exact (bf16 x bf16 in fp32), each of the
                                                                      K + 4 additions of a chain (K products, bias, bias2, <= 2 split-K slab adds)
                                                                      rounds by at most u32 of a partial sum <= sum |a||w| + |bias| + |bias2|.
                                                                      Split-K and the tail split sum fp32 partials in a fixed order: the same K.
             + 2^-16 (|bias| + |bias2|) ]                             bf16 only: the 32x32 tiles feed bias + bias2 through the MFMA as a bf16 head
                                                                      + tail (gemm.hip:472-485; the tail's own rounding is 2^-18, the term as the
                                                                      issue states it)
    + activation                                                      L = 1.13 >= max |gelu'| (1.1290), 1.1 >= max |silu'| (1.0998), 1 without one;
        SiLU  (2^-21 + 2^-23 |pre|) |t|                               common.h:104 x / (1 + __expf(-x)): v_exp_f32 (1 ulp) behind one multiply by
                                                                      log2 e (an argument error of u32 |x| log2 e) and one division
        GEGLU |gelu(g)| d_h + |h| (1.13 d_g + 1e-6) + 2^-22 |t|       common.h:113-138 |gelu error| < 1e-6: `gelu_poly_error()` evaluates the same
                                                                      polynomial in torch fp32 against fp64 erf over [-12, 12] (measured 7.1e-7)
    + 4 u32 (|t s| + |bias_post| + |residual|)                        the epilogue's fp32 operations: rs * alpha, the scale, two additions
  with s = row_scale * alpha, d_h / d_g the bracket of the h / g column.

CONV  (conv3x3: stride 1, 2, -2 = pad-high-only, upsample True and 2, two sources; conv1x1_cat is LINEAR over [x0 | x1])
  gemm.hip:1008-1052 builds the implicit GEMM: rows (n, y, x), reduction (ky, kx, cin) over x0 | x1, zero padding by out-of-range DMA offsets
  (gemm_common.h:51-53), then the LINEAR epilogue with bias2_rows counted in output pixels.  Contract and bound are the LINEAR ones over the
  gathered reduction of 9 Cin (4 Cin for the four-phase form).
  Folded weights (packing.pack_conv3x3_up2: the taps that fall on one stored pixel summed in fp32 and rounded once; the [W_po W2 | W_po] image of
  unet3d `_ffpo_weights`): the CONTRACT multiplies the packed bf16 weights, as the kernel does.  `ideal` is the unfolded fp64 function; a relative
  error U on every folded weight moves it by at most  B_w = U sum |x||w_folded|,  gated as |out - ideal| <= 2 B + B_w  (B_s of attn_gate.py).
  Tap gather (conv_out as a 36-column GEMM + elementwise.hip:312-332): Y[pixel][4 tap + o] is stored in bf16, the gather sums nine of them and the
  bias in fp32 and rounds once.  The contract rounds the nine fp64 products to bf16; a product whose fp32 value lies across a rounding boundary from
  its fp64 value may round the other way, so B adds U sum_taps |y_tap| next to (320 + 4) u32 sum |x||w| and the ten fp32 additions.

NORM  (groupnorm normalise / affine tables, one or two sources; layernorm with pe, folded beta table, strides)
  Contract: exact fp64 mean and biased variance of the stored values, rstd = (var + eps)^-1/2, v = (x - mean) rstd gamma + beta, SiLU behind the
  affine (norm.hip:257-258, :361-362, :486-487, :613-614), pe row (row / pe_div) % pe_mod added last (norm.hip:700-717), one rounding; the tables
  entry (norm.hip:385-387, :469-475, :594-600: scale = rstd gamma, shift = beta - mean scale) is fp32 and has no output rounding.
  B = U |ref| + S, S the statistics term.  With D the number of fp32 additions on the longest path of a sum (below), n values per group,
      d_mean = D u32 mean|x - p| + u32 |mean|        p: the pivot of the shifted single-pass kernels (norm.hip:75-79), 0 for the two-pass ones
      d_var  = (D + 3) u32 (E[(x - p)^2] + (mean - p)^2) + 2 |mean - p| D u32 mean|x - p| + d_mean^2
      d_r    = d_var / (2 (var + eps)) + 3 u32       relative error of rstd: rsqrtf (1 ulp) and the division by n
      S = L (|gamma| (rstd d_mean + |z| d_r) + u32 (2 |gamma| rstd (|x| + |mean|) + |beta| + |pe| + 2 |v|))
  (the last bracket: x * scale + shift with shift = beta - mean * scale, norm.hip:240-242, each operation u32 of its result).  D per kernel:
      gn_slab / gn_small   ceil(HW / rp) + rp + C/G    a thread's rows (norm.hip:444-449, :568-574), the rp row slots in sequence (:427, :552), the
                                                       group's channels in sequence (:433, :558); rp = threads / (vectors per slab row)
      narrow               U ceil(HW / (chunks RS U)) + log2(64 / nvec) + 2 + C/G + ceil(chunks / 4) + 2     (norm.hip:290-298, :301-304, :312, :318, :199-206)
      general two-pass     ceil(HW / (chunks 4 rpw)) + log2(64 / lpr) + 3 + C/G + ceil(chunks / 4) + 2       (norm.hip:116-153, :156-161, :162-177, :181, :199-206)
      ln_kernel            vpl VEC + log2(lpr)                                                                (norm.hip:681-688, :692-697)
  `gn_form` mirrors the dispatchers (norm.hip:625-652, :736-748, :26-34, :765-829) to name the kernel a shape runs on and its D.
  `norm_check` asserts S < U/4 (|gamma| (|z| + 1) + |beta|) in every case: the gate stays dominated by the output rounding and no
  shape-dependent slack can grow to hide a mutant."""
import math

import torch
import torch.nn.functional as F

from mmgt_amd.synthetic import hash_uniform
from tests.attn_gate import NAN, SENT, U, old_gate_accepts, ratio  # noqa: F401  (re-exported: the tests take them from here)

U32 = 2.0 ** -24
GELU_ERR = 1e-6                    # common.h:114, verified by gelu_poly_error()
L_GELU, L_SILU = 1.13, 1.1
BF16 = torch.bfloat16


def dev():
    return torch.device("cuda:0")


def rnd(name, shape, scale=1.0, dt=torch.float32, device="cpu"):
    return hash_uniform(name, shape, scale, device).to(dt)


def guarded(t, extra_rows=8, cols=8):
    """`t` (2-D or more: rows first) as a view into an allocation with `extra_rows` NaN rows behind the last one and, for 2-D operands, `cols` NaN
    columns beside it (a strided view: what lies next to an operand must never be read)"""
    if t.dim() == 2:
        buf = torch.full((t.shape[0] + extra_rows, t.shape[1] + cols), NAN, device=t.device, dtype=t.dtype)
        view = buf[:t.shape[0], :t.shape[1]]
    else:
        buf = torch.full((t.shape[0] + extra_rows,) + tuple(t.shape[1:]), NAN, device=t.device, dtype=t.dtype)
        view = buf[:t.shape[0]]
    view.copy_(t)
    return view


def out_in_sentinels(shape, dt, device, ld=None, col0=0):
    """(buffer, view): an output block of `shape` (rows first) inside a sentinel-filled buffer with 3 more rows and, for 2-D blocks, a row
    stride of `ld` elements with the block at column col0"""
    if len(shape) == 2:
        ld = shape[1] if ld is None else ld
        buf = torch.full((shape[0] + 3, ld), SENT, device=device, dtype=dt)
        return buf, buf[:shape[0], col0:col0 + shape[1]]
    buf = torch.full((shape[0] + 1,) + tuple(shape[1:]), SENT, device=device, dtype=dt)
    return buf, buf[:shape[0]]


def assert_untouched(buf, view):
    """every element of `buf` outside `view` still holds the sentinel bit for bit"""
    chk = buf.clone()
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    if buf.dim() == 2:
        r0, c0 = divmod(off, buf.stride(0))
        chk[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = SENT
    else:
        assert off == 0
        chk[:view.shape[0]] = SENT
    bits = torch.int32 if buf.dtype == torch.float32 else torch.int16
    assert torch.equal(chk.view(bits), torch.full_like(chk, SENT).view(bits)), "the kernel wrote outside its output block"


def bf16_round(t):
    """fp64 -> nearest bf16 -> fp64 (through fp32: a double rounding only where the fp64 value lies within 2^-29 of a bf16 boundary)"""
    return t.float().to(BF16).double()


def to_storage(t, dt):
    return t.float().to(dt)


# ---- the gate ------------------------------------------------------------------------------------------------------------------------------

def check(out, ref, B, what, factor=2.0, ideal=None):
    """finite and |out - ref| <= factor * B on every element; ideal = (ideal reference, B_w): also |out - ideal| <= factor * B + B_w.
    Prints max and mean |d| / B; returns (max, mean)."""
    assert torch.isfinite(out.float()).all(), f"{what}: not finite"
    x = ratio(out, ref, B)
    mx, mean = x.max().item(), x.mean().item()
    msg = f"{what}: max |d| / B {mx:.3f}, mean |d| / B {mean:.3f}"
    if ideal is not None:
        msg += f"; max |out - ideal| / (2 B + B_w) {ratio(out, ideal[0], factor * B + ideal[1]).max().item():.3f}"
    print(msg)
    assert (x <= factor).all(), f"{what}: {(x > factor).sum().item()} elements beyond {factor} B, max {mx:.3f} B"
    if ideal is not None:
        assert ((out.double() - ideal[0]).abs() <= factor * B + ideal[1]).all(), f"{what}: beyond {factor} B + B_w of the ideal reference"
    return mx, mean


def check_fp32(out, ref, what):
    """the fp32 instantiations: rtol 1e-3 / atol 1e-4 against the same contract"""
    assert torch.isfinite(out).all(), f"{what}: not finite"
    torch.testing.assert_close(out.double(), ref, rtol=1e-3, atol=1e-4)


def rejects(mut, ref, B, factor=2.0):
    """max |bf16(mutant) - ref| / B if the gate rejects the mutant rounded to bf16 (what a wrong kernel would store), else 0"""
    x = ratio(bf16_round(mut), ref, B).max().item()
    return x if x > factor else 0.0


def gelu_poly(x):
    """common.h:127-138 in torch fp32 (separate multiply and add for the fmas, an exact reciprocal for v_rcp_f32)"""
    f = torch.float32
    k = torch.tensor(1.0442737824274138, dtype=f)
    c = [torch.tensor(v, dtype=f) * k for v in (0.04986734694, 0.02114100615, 0.003277626324, 0.000038003575, 0.000048890636, 0.00000538297500)]
    x = x.to(f)
    z = x.abs()
    p = c[5] * z + c[4]
    for i in (3, 2, 1, 0):
        p = p * z + c[i].to(x.device)
    p = p * z + k
    for _ in range(4):
        p = p * p
    return torch.clamp(x, min=0) - z * (1.0 / p)


def gelu_poly_error(n=2_400_001):
    """max |gelu_poly - x Phi(x)| over [-12, 12]"""
    x = torch.linspace(-12, 12, n, dtype=torch.float64).float()
    return (gelu_poly(x).double() - x.double() * 0.5 * (1 + torch.erf(x.double() / math.sqrt(2)))).abs().max().item()


def _gelu64(x):
    return x * 0.5 * (1 + torch.erf(x / math.sqrt(2)))


def _silu64(x):
    return x * torch.sigmoid(x)


class _Case:
    def contract(self):
        return self.reference()[0]

    def bound(self):
        return self.reference()[1]


# ---- LINEAR ----------------------------------------------------------------------------------------------------------------------------------

class Epi:
    """The epilogue operands of one problem: bias (N,), bias2 (blocks, N) with bias2_rows rows per block, row_scale (M,), alpha, bias_post (N,)
    fp32; act in ("none", "silu", "geglu"); residual (M, n_out) in the storage type.  GEGLU: N = 2 n_out columns in the UNPACKED order [h | g]
    (the kernel is handed packing.pack_geglu's image of the same weights)."""

    def __init__(self, bias=None, bias2=None, bias2_rows=0, row_scale=None, alpha=1.0, bias_post=None, act="none", residual=None):
        self.bias, self.bias2, self.bias2_rows, self.row_scale, self.alpha = bias, bias2, bias2_rows, row_scale, alpha
        self.bias_post, self.act, self.residual = bias_post, act, residual

    def but(self, **kw):
        e = Epi(self.bias, self.bias2, self.bias2_rows, self.row_scale, self.alpha, self.bias_post, self.act, self.residual)
        for k, v in kw.items():
            setattr(e, k, v)
        return e


def _b2(ep, M, early=0):
    """bias2 row of every output row -> (M, N) fp64; early = 1: the block boundary one row early (a mutant)"""
    idx = torch.clamp((torch.arange(M, device=ep.bias2.device) + early) // ep.bias2_rows, max=ep.bias2.shape[0] - 1)
    return ep.bias2.double()[idx]


def epilogue(acc, ep, absacc=None, K=0, dt=BF16, mut=None):
    """(ref, B): the epilogue of the module docstring on the fp64 accumulator `acc` (M, N).  B needs absacc = sum |a||w| and K; without absacc
    only ref is returned.  mut: a mutant's name (the wrong epilogues)."""
    M, N = acc.shape
    zero = torch.zeros((), dtype=torch.float64, device=acc.device)
    bias = ep.bias.double() if ep.bias is not None else zero
    bias2 = _b2(ep, M, 1 if mut == "bias2 early" else 0) if ep.bias2 is not None else zero
    s = (ep.row_scale.double()[:, None] if ep.row_scale is not None else 1.0) * float(ep.alpha)
    s = s if torch.is_tensor(s) else torch.full((1, 1), s, dtype=torch.float64, device=acc.device)
    if mut == "bias shifted":
        bias = bias.roll(1)
    if mut == "alpha before bias":
        pre = acc * s + bias + bias2
        s = torch.ones_like(s)
    else:
        pre = acc + bias + bias2
    if ep.act == "geglu":
        n = N // 2
        if mut == "geglu swapped":
            g, h = pre[:, :n], pre[:, n:]
        elif mut == "geglu unpacked":                  # the kernel's pairing (32 h | 32 gates) applied to the unpacked column order
            p4 = pre.reshape(M, N // 64, 2, 32)
            h, g = p4[:, :, 0].reshape(M, n), p4[:, :, 1].reshape(M, n)
        else:
            h, g = pre[:, :n], pre[:, n:]
        t = h * _gelu64(g)
    elif ep.act == "silu":
        t = _silu64(pre)
    else:
        t = pre
    post = ep.bias_post.double() if ep.bias_post is not None else zero
    if mut == "scale on bias_post":
        post = post * s
    res = ep.residual.double() if ep.residual is not None else zero
    if mut == "residual row":
        res = res.clone()
        res[-1] = res[-2]
    ref = t * s + post + res
    if absacc is None:
        return ref, None
    d = (K + 4) * U32 * (absacc + bias.abs() + bias2.abs()) + (2.0 ** -16 * (bias.abs() + bias2.abs()) if dt == BF16 else 0.0)
    if ep.act == "geglu":
        dtl = _gelu64(g).abs() * d[:, :n] + h.abs() * (L_GELU * d[:, n:] + GELU_ERR) + 2.0 ** -22 * t.abs()
    elif ep.act == "silu":
        dtl = L_SILU * d + (2.0 ** -21 + 2.0 ** -23 * pre.abs()) * t.abs()
    else:
        dtl = d
    B = (U if dt == BF16 else 0.0) * ref.abs() + s.abs() * dtl + 4 * U32 * ((t * s).abs() + post.abs() + res.abs())
    return ref, B


def epilogue_sim(acc32, ep):
    """the epilogue in fp32, in the kernels' order, the GELU by common.h's polynomial; acc32 fp32 (M, N) -> fp32 (M, n_out), not yet rounded"""
    M, N = acc32.shape
    pre = acc32
    if ep.bias is not None:
        pre = pre + ep.bias
    if ep.bias2 is not None:
        pre = pre + _b2(ep, M).float()
    if ep.act == "geglu":
        pre = pre[:, :N // 2] * gelu_poly(pre[:, N // 2:])
    elif ep.act == "silu":
        pre = pre / (1.0 + torch.exp(-pre))
    if ep.row_scale is not None or ep.alpha != 1.0:
        rs = (ep.row_scale if ep.row_scale is not None else torch.ones(M, device=acc32.device)) * torch.tensor(ep.alpha, dtype=torch.float32)
        pre = pre * rs[:, None]
    if ep.bias_post is not None:
        pre = pre + ep.bias_post
    if ep.residual is not None:
        pre = pre + ep.residual.float()
    return pre


class Linear(_Case):
    """a (M, K), w (N, K) in the storage type (views of any row stride), ep an Epi.  The fp64 accumulator and sum |a||w| are computed once."""

    def __init__(self, what, a, w, ep, dt=None):
        self.what, self.a, self.w, self.ep = what, a, w, ep
        self.dt = a.dtype if dt is None else dt
        self.K = a.shape[1]
        self._acc = self._abs = self._ref = None

    @property
    def acc(self):
        if self._acc is None:
            self._acc = self.a.double() @ self.w.double().t()
        return self._acc

    @property
    def absacc(self):
        if self._abs is None:
            self._abs = self.a.double().abs() @ self.w.double().abs().t()
        return self._abs

    def reference(self):
        """(ref, B), cached"""
        if self._ref is None:
            self._ref = epilogue(self.acc, self.ep, self.absacc, self.K, self.dt)
        return self._ref

    def simulate(self):
        """fp32 accumulation, the epilogue in fp32, one rounding"""
        return to_storage(epilogue_sim(self.a.float() @ self.w.float().t(), self.ep), self.dt)

    def mutants(self):
        """{name: fp64 mutant reference}; each only where the case has the ingredient it alters"""
        a, w, ep, acc = self.a.double(), self.w.double(), self.ep, self.acc
        run = lambda ac, **kw: epilogue(ac, ep, **kw)[0]
        m = {"last k dropped": run(acc - a[:, -1:] * w[:, -1][None, :]),
             "W columns k = 8, 9 swapped": run(acc + (a[:, 8:9] - a[:, 9:10]) * (w[:, 9] - w[:, 8])[None, :]),
             "accumulator x (1 + 2^-6)": run(acc * (1 + 2.0 ** -6))}
        if ep.bias is not None:
            m["bias shifted by one column"] = run(acc, mut="bias shifted")
        if ep.residual is not None and acc.shape[0] >= 2:
            m["residual of the last row from its neighbour"] = run(acc, mut="residual row")
        if ep.bias2 is not None and ep.bias2.shape[0] >= 2:
            m["bias2 block boundary one row early"] = run(acc, mut="bias2 early")
        scaled = ep.row_scale is not None or ep.alpha != 1.0
        if scaled and ep.bias_post is not None:
            m["alpha * row_scale applied to bias_post as well"] = run(acc, mut="scale on bias_post")
        if scaled and (ep.bias is not None or ep.bias2 is not None):
            m["alpha applied before the bias add"] = run(acc, mut="alpha before bias")
        if ep.act == "geglu":
            m["GEGLU halves swapped"] = run(acc, mut="geglu swapped")
            m["GEGLU columns paired in unpacked order"] = run(acc, mut="geglu unpacked")
        return m

    def assert_not_degenerate(self):
        """rms(ref) >= 0.15; without a residual sum |a||w| >= 4 |ref| on the median element (keeps `last k dropped` sharp)"""
        ref, _ = self.reference()
        rms = ref.pow(2).mean().sqrt().item()
        assert rms >= 0.15, (self.what, rms)
        if self.ep.residual is None:
            absacc = self.absacc
            if self.ep.act == "geglu":
                absacc = absacc[:, :absacc.shape[1] // 2]
            q = (absacc / ref.abs().clamp_min(1e-300)).median().item()
            assert q >= 4.0, (self.what, q)


def linear_case(tag, M, N, K, dt=BF16, device="cpu", wscale=1.0, bias=False, bias2_rows=0, row_scale=False, alpha=1.0, bias_post=False,
                act="none", residual=False, guard=False, a_scale=1.0, bias_scale=0.5):
    """The suite's operand recipe: a = hash_uniform * a_scale, w = hash_uniform * wscale / sqrt(K), bias / bias2 / bias_post 0.5, residual 1.0,
    row_scale in [0.5, 1) (a mask multiply).  guard: a, w and the residual are views with NaN rows and columns behind them.  Values depend on (tag, shape) alone."""
    g = guarded if guard else (lambda t: t)
    a = g(rnd(f"{tag}.a", (M, K), a_scale, dt, device))
    w = rnd(f"{tag}.w", (N, K), wscale / math.sqrt(K), dt, device)
    n_out = N // 2 if act == "geglu" else N
    ep = Epi(bias=rnd(f"{tag}.b", (N,), bias_scale, device=device) if bias else None,
             bias2=rnd(f"{tag}.b2", ((M + bias2_rows - 1) // bias2_rows, N), 0.5, device=device) if bias2_rows else None, bias2_rows=bias2_rows,
             row_scale=rnd(f"{tag}.rs", (M,), 0.25, device=device) + 0.75 if row_scale else None, alpha=alpha,
             bias_post=rnd(f"{tag}.bp", (N,), 0.5, device=device) if bias_post else None, act=act,
             residual=g(rnd(f"{tag}.r", (M, n_out), 1.0, dt, device)) if residual else None)
    return Linear(f"{tag} ({M}, {N}, {K}) {str(dt)[6:]}", a, w, ep)


# ---- CONV ------------------------------------------------------------------------------------------------------------------------------------

def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _conv2d(v, w, stride=1):
    """valid cross-correlation as im2col + one matrix product (fp64 / fp32 alike on any device): v (NB, C, H, W), w (Cout, C, kh, kw)"""
    kh, kw = w.shape[2:]
    oh, ow = (v.shape[2] - kh) // stride + 1, (v.shape[3] - kw) // stride + 1
    cols = F.unfold(v, (kh, kw), stride=stride)                          # (NB, C kh kw, oh ow)
    return (w.reshape(w.shape[0], -1) @ cols).reshape(v.shape[0], w.shape[0], oh, ow)


def conv_acc(x, w, stride, upsample, pad_mode="constant", pad_lo=None):
    """x (NB, H, W, Cin) channels-last, w (Cout, Cin, 3, 3) of one dtype -> the accumulator (NB, OH, OW, Cout).  stride -2: zero padding behind the
    last row / column only.  pad_lo overrides the padding in front (the sampling-shift mutant); the output size is the true geometry's."""
    v = _nchw(x)
    if upsample:
        v = F.interpolate(v, scale_factor=2.0, mode="nearest")
    vh, vw = v.shape[2:]
    st = abs(stride)
    lo = (0 if stride == -2 else 1) if pad_lo is None else pad_lo
    oh, ow = ((vh - 2) // 2 + 1, (vw - 2) // 2 + 1) if stride == -2 else ((vh - 1) // st + 1, (vw - 1) // st + 1)
    v = F.pad(v, (lo, 2, lo, 2), mode=pad_mode)            # (two rows / columns behind: enough for every geometry, cropped below)
    return _conv2d(v, w, st)[:, :, :oh, :ow].permute(0, 2, 3, 1)


def _up2_acc(x, wf):
    """the four-phase form: x (NB, H, W, Cin), wf (4, Cout, 2, 2, Cin) of one dtype (packing.pack_conv3x3_up2) -> (NB, 2 H, 2 W, Cout): output
    pixel (2 y + a, 2 x + b) = sum over (ty, tx) of wf[2 a + b][:, ty, tx] . x[y + a - 1 + ty][x + b - 1 + tx], zero outside the image"""
    NB, H, W, _ = x.shape
    v = F.pad(_nchw(x), (1, 1, 1, 1))
    out = torch.zeros((NB, 2 * H, 2 * W, wf.shape[1]), dtype=x.dtype, device=x.device)
    for a in range(2):
        for b in range(2):
            o = _conv2d(v[:, :, a:a + H + 1, b:b + W + 1], wf[2 * a + b].permute(0, 3, 1, 2))
            out[:, a::2, b::2] = o.permute(0, 2, 3, 1)
    return out


class Conv(_Case):
    """x0 (NB, H, W, C0) [+ x1 (NB, H, W, C1)] channels-last, w (Cout, C0 + C1, 3, 3) in the storage type; stride 1 / 2 / -2; upsample False /
    True / 2 (then the kernel multiplies wf = pack_conv3x3_up2(w), and so does the contract); ep: an Epi over the output pixels as rows."""

    def __init__(self, what, x0, w, ep, stride=1, upsample=False, x1=None):
        self.what, self.x0, self.x1, self.w, self.ep, self.stride, self.upsample = what, x0, x1, w, ep, stride, upsample
        self.dt = x0.dtype
        self.up2 = upsample is not True and upsample == 2
        self.cin = x0.shape[3] + (0 if x1 is None else x1.shape[3])
        self.K = (4 if self.up2 else 9) * self.cin
        self._ref = None
        if self.up2:
            from mmgt_amd.packing import pack_conv3x3_up2
            self.wf = pack_conv3x3_up2(w)

    def x(self):
        return (self.x0 if self.x1 is None else torch.cat([self.x0, self.x1], 3)).double()

    def _acc(self, x, w, **kw):
        if self.up2:
            return _up2_acc(x, w)
        return conv_acc(x, w, self.stride, bool(self.upsample), **kw)

    def _weights(self):
        return (self.wf if self.up2 else self.w).double()

    def _epi(self, acc, absacc=None, mut=None):
        shp = acc.shape
        ref, B = epilogue(acc.reshape(-1, shp[-1]), self.ep, None if absacc is None else absacc.reshape(-1, shp[-1]), self.K, self.dt, mut)
        return ref.reshape(shp), None if B is None else B.reshape(shp)

    def reference(self):
        if self._ref is None:
            x, w = self.x(), self._weights()
            self.acc, self.absacc = self._acc(x, w), self._acc(x.abs(), w.abs())
            self._ref = self._epi(self.acc, self.absacc)
        return self._ref

    def ideal(self):
        """(the unfolded fp64 function: conv3x3 of the upsampled image with the weights as given, B_w = U sum |x||w_folded|); up2 only"""
        assert self.up2
        self.reference()
        return self._epi(conv_acc(self.x(), self.w.double(), 1, True))[0], U * self.absacc

    def simulate(self):
        """fp32 accumulation over the same gather, the epilogue in fp32, one rounding"""
        acc = self._acc(self.x().float(), self._weights().float())
        shp = acc.shape
        return to_storage(epilogue_sim(acc.reshape(-1, shp[-1]), self.ep).reshape(shp), self.dt)

    def mutants(self):
        x, w = self.x(), self._weights()
        self.reference()
        m = {}
        NB, H, W, _ = x.shape
        vh, vw = (2 * H, 2 * W) if self.upsample else (H, W)
        if not self.up2:
            if vh >= 2 and vw >= 2:
                wt = w.clone()
                wt[:, :, 0, 1], wt[:, :, 1, 0] = w[:, :, 1, 0], w[:, :, 0, 1]
                m["the weights of one tap transposed (ky <-> kx)"] = self._epi(self._acc(x, wt))[0]
            m["zero padding replaced by edge clamp"] = self._epi(self._acc(x, w, pad_mode="replicate"))[0]
            if abs(self.stride) == 2 and vh >= 2 and vw >= 2:
                m["stride-2 sampling shifted by one pixel"] = self._epi(self._acc(x, w, pad_lo=1 if self.stride == -2 else 0))[0]
        if self.x1 is not None:
            c0 = self.x0.shape[3]
            xs = x.clone()
            xs[..., c0 - 1], xs[..., c0] = x[..., c0], x[..., c0 - 1]
            m["channels c0 - 1 and c0 swapped across the seam"] = self._epi(self._acc(xs, w))[0]
        if self.upsample:
            ref = self._ref[0]
            t = torch.empty_like(ref)
            for a in range(2):
                for b in range(2):
                    t[:, a::2, b::2] = ref[:, b::2, a::2]
            m["up-sampling phase (a, b) transposed"] = t
        if self.ep.bias is not None:
            m["bias shifted by one column"] = self._epi(self.acc, mut="bias shifted")[0]
        m["accumulator x (1 + 2^-6)"] = self._epi(self.acc * (1 + 2.0 ** -6))[0]
        if self.ep.bias2 is not None and self.ep.bias2.shape[0] >= 2:
            m["bias2 block boundary one row early"] = self._epi(self.acc, mut="bias2 early")[0]
        return m

    def assert_not_degenerate(self):
        ref, _ = self.reference()
        rms = ref.pow(2).mean().sqrt().item()
        assert rms >= 0.15, (self.what, rms)
        if self.ep.residual is None:
            q = (self.absacc / ref.abs().clamp_min(1e-300)).median().item()
            assert q >= 4.0, (self.what, q)


def conv_case(tag, NB, H, W, c0, cout, c1=0, stride=1, upsample=False, dt=BF16, device="cpu", bias=True, bias2_rows=0, residual=False, guard=False):
    """a = hash_uniform, w = hash_uniform / sqrt(9 Cin), bias / bias2 0.5, residual 1.0 (the suite's recipe); bias2_rows in output pixels"""
    g = guarded if guard else (lambda t: t)
    cin = c0 + c1
    x0 = g(rnd(f"{tag}.x0", (NB, H, W, c0), 1.0, dt, device))
    x1 = g(rnd(f"{tag}.x1", (NB, H, W, c1), 1.0, dt, device)) if c1 else None
    w = rnd(f"{tag}.w", (cout, cin, 3, 3), 1.0 / math.sqrt(9 * cin), dt, device)
    vh, vw = (2 * H, 2 * W) if upsample else (H, W)
    oh, ow = ((vh - 2) // 2 + 1, (vw - 2) // 2 + 1) if stride == -2 else ((vh - 1) // abs(stride) + 1, (vw - 1) // abs(stride) + 1)
    M = NB * oh * ow
    ep = Epi(bias=rnd(f"{tag}.b", (cout,), 0.5, device=device) if bias else None,
             bias2=rnd(f"{tag}.b2", ((M + bias2_rows - 1) // bias2_rows, cout), 0.5, device=device) if bias2_rows else None, bias2_rows=bias2_rows,
             residual=g(rnd(f"{tag}.r", (NB, oh, ow, cout), 1.0, dt, device)).reshape(M, cout) if residual else None)
    return Conv(f"{tag} {NB} x {H} x {W}, {c0} | {c1} -> {cout}, stride {stride}, up {upsample}, {str(dt)[6:]}", x0, w, ep, stride, upsample, x1)


# ---- the tap gather ----------------------------------------------------------------------------------------------------------------------------

class Taps(_Case):
    """conv_out as a GEMM over the taps + gather: x (NB, H, W, 320), w (4, 320, 3, 3) bf16, bias (4,) fp32 -> (NB, H, W, 4).  The nine products
    per output are rounded to bf16 (the stored Y) before their fp32 sum."""

    def __init__(self, what, x, w, bias):
        self.what, self.x, self.w, self.bias = what, x, w, bias
        self._ref = None

    def _gather(self, y, clamp=False, transpose=False):
        """y (NB, H, W, 3, 3, 4): products of every pixel for every tap -> sum over the taps of the neighbours' products"""
        NB, H, W = y.shape[:3]
        out = torch.zeros((NB, H, W, 4), dtype=y.dtype, device=y.device)
        for ky in range(3):
            for kx in range(3):
                src = y[:, :, :, kx, ky] if transpose and (ky, kx) in ((0, 1), (1, 0)) else y[:, :, :, ky, kx]
                if clamp:                               # the neighbour's index clamped to the image
                    iy = torch.clamp(torch.arange(H, device=y.device) + ky - 1, 0, H - 1)
                    ix = torch.clamp(torch.arange(W, device=y.device) + kx - 1, 0, W - 1)
                    out += src[:, iy][:, :, ix]
                else:
                    sp = F.pad(src.permute(0, 3, 1, 2), (1, 1, 1, 1))
                    out += sp[:, :, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1)
        return out

    def products(self, dtype=torch.float64):
        return torch.einsum("nhwc,ockl->nhwklo", self.x.to(dtype), self.w.to(dtype))

    def reference(self):
        if self._ref is None:
            y = bf16_round(self.products())
            ref = self._gather(y) + self.bias.double()
            absy = self._gather(y.abs())
            absxw = self._gather(torch.einsum("nhwc,ockl->nhwklo", self.x.double().abs(), self.w.double().abs()))
            B = U * ref.abs() + U * absy + (320 + 4) * U32 * absxw + 10 * U32 * (absy + self.bias.double().abs())
            self._ref = (ref, B)
        return self._ref

    def simulate(self):
        y = self.products(torch.float32).to(BF16).float()
        return (self._gather(y) + self.bias).to(BF16)

    def mutants(self):
        y = bf16_round(self.products())
        b = self.bias.double()
        return {"the weights of one tap transposed (ky <-> kx)": self._gather(y, transpose=True) + b,
                "zero padding replaced by edge clamp": self._gather(y, clamp=True) + b,
                "bias shifted by one column": self._gather(y) + b.roll(1)}


def taps_case(tag, NB, H, W, device="cpu", guard=False):
    x = rnd(f"{tag}.x", (NB, H, W, 320), 1.0, BF16, device)
    if guard:
        x = guarded(x)
    return Taps(f"{tag} taps {NB} x {H} x {W}", x, rnd(f"{tag}.w", (4, 320, 3, 3), 1.0 / math.sqrt(9 * 320), BF16, device),
                rnd(f"{tag}.b", (4,), 0.5, device=device))


# ---- NORM ------------------------------------------------------------------------------------------------------------------------------------

def _log2(v):
    return int(math.log2(v)) if v > 1 else 0


def _slab_gpw(C, G, HW, vec):
    """norm.hip:625-652 -> (groups per workgroup, threads) or (0, 0)"""
    cg = C // G

    def need(gpw, threads):
        cw = gpw * cg
        if G % gpw or cw % vec or cw > 320 or cw // vec > 256:
            return 1 << 30
        return -(-HW // (threads // (cw // vec)))
    for gpw in (4, 2, 1):
        if need(gpw, 256) <= 6:
            return gpw, 256
    for gpw in (1, 2, 4):
        if need(gpw, 256) <= 22:
            return gpw, 256
    for gpw in (1, 2, 4):
        if need(gpw, 1024) <= 16:
            return gpw, 1024
    return 0, 0


def _gn_chunks_cap(HW):
    c = (HW + 127) // 128 if HW >= 2048 else (HW + 31) // 32
    return max(1, min(256, c))


def gn_form(C0, C1, G, HW, vec, NB=1, slab=True):
    """(form, D): the kernel `mmgt_groupnorm_nhwc` / `mmgt_groupnorm_affine2` run this shape on (norm.hip:765-829, :845-899; slab: the
    `gn_slab` switch) and the number of fp32 additions on the longest path of its sums (module docstring).  form in ("slab", "slab1024",
    "small", "narrow", "general")."""
    C = C0 + C1
    cg, nvec = C // G, C // vec
    gpw, thr = _slab_gpw(C, G, HW, vec) if slab else (0, 0)
    if gpw:
        rp = thr // (gpw * cg // vec)
        return ("slab" if thr == 256 else "slab1024"), -(-HW // rp) + rp + cg
    gpw = 2 if (HW > 64 and G % 2 == 0 and (2 * cg) % vec == 0) else 4
    cw = gpw * cg
    if HW <= 256 and G % gpw == 0 and cw % vec == 0 and cw <= 320 and cw // vec <= 256:
        rp = 256 // (cw // vec)
        return "small", -(-HW // rp) + rp + cg
    if C1 == 0 and 8 <= nvec <= 64 and (64 % nvec == 0 or nvec > 32) and HW % (4 * (64 // nvec) * 4) == 0:
        step = 4 * (64 // nvec) * 4
        rows = max(64, (HW * NB + 2047) // 2048)
        rows = -(-rows // step) * step
        chunks = max(1, min(_gn_chunks_cap(HW), -(-HW // rows)))
        return "narrow", 4 * -(-HW // (chunks * step)) + _log2(64 // nvec) + 2 + cg + -(-chunks // 4) + 2
    rows = (256 if C <= 320 else 128) if HW >= 2048 else 64
    if HW >= 65536:
        rows = max(rows, (HW * NB + 1023) // 1024)
    chunks = max(1, min(_gn_chunks_cap(HW), -(-HW // rows)))
    maxs, lpr = 2560 // (vec * 64), 8
    while lpr < 64 and (lpr * maxs < nvec or nvec % lpr):
        lpr *= 2
    return "general", -(-HW // (chunks * 4 * (64 // lpr))) + _log2(64 // lpr) + 3 + cg + -(-chunks // 4) + 2


def ln_depth(C, vec):
    """norm.hip:919-923 -> D of ln_kernel and its rows per workgroup"""
    nvec, lpr = C // vec, 8
    while lpr < 64 and (nvec % lpr or nvec // lpr > 5):
        lpr *= 2
    return (nvec // lpr) * vec + _log2(lpr), 4 * (64 // lpr)


def _stats(x, gid, G, sel=None, denom_less=0):
    """x (NB, R, C) fp64, gid (C,) the group of every channel -> per-channel (mean, var, E|x|, n) each (NB, 1, C); sel (C,) bool: the channels
    the MEAN is taken over (a mutant); denom_less: the variance divides by n - denom_less"""
    NB, R, C = x.shape
    one = F.one_hot(gid, G).double()                                    # (C, G)
    cnt = one.sum(0) * R
    msel = one if sel is None else one * sel.double()[:, None]
    mcnt = torch.where(msel.sum(0) > 0, msel.sum(0), one.sum(0)) * R
    muse = torch.where((msel.sum(0) > 0)[None, :], msel, one)
    mean_g = (x.sum(1) @ muse) / mcnt                                   # (NB, G)
    mean = mean_g[:, gid][:, None, :]
    var_g = ((x - mean).pow(2).sum(1) @ one) / (cnt - denom_less)
    absm_g = (x.abs().sum(1) @ one) / cnt
    return mean, var_g[:, gid][:, None, :], absm_g[:, gid][:, None, :], cnt[gid][None, None, :]


class Norm(_Case):
    """GroupNorm over (x0 | x1) (NB, HW, C), groups of C / G channels, or LayerNorm (G = 0: x (rows, C) taken as (rows, 1, C) with one group);
    gamma (C,), beta (C,) or the folded (pe_mod, C) table, pe (pe_mod, C) or None.  D: the fp32 additions on the longest path of a sum; pivot:
    the single-pass kernels shift by the group's first value of pixel 0."""

    def __init__(self, what, x0, gamma, beta, eps, D, G=0, x1=None, silu=False, pe=None, pe_div=1, pe_mod=1, pivot=False, tables=False):
        self.what, self.x0, self.x1, self.gamma, self.beta, self.eps, self.D, self.G = what, x0, x1, gamma, beta, eps, D, G
        self.silu, self.pe, self.pe_div, self.pe_mod, self.pivot, self.tables = silu, pe, pe_div, pe_mod, pivot, tables
        self.dt = x0.dtype
        self._ref = None

    def x(self):
        x = (self.x0 if self.x1 is None else torch.cat([self.x0, self.x1], -1)).double()
        return x[:, None, :] if self.G == 0 else x

    def gid(self, shift=0):
        C = self.x().shape[-1]
        if self.G == 0:
            return torch.zeros(C, dtype=torch.long, device=self.x0.device)
        return torch.clamp((torch.arange(C, device=self.x0.device) + shift) // (C // self.G), max=self.G - 1)

    def _beta_pe(self, rows, mut=None):
        """(beta per element, pe per element) broadcastable to (rows, 1, C) for the LayerNorm forms"""
        if self.G or self.pe_mod <= 1:
            return self.beta.double(), 0.0
        idx = torch.arange(rows, device=self.x0.device)
        idx = (idx % self.pe_mod) if mut == "pe row" else (idx // self.pe_div) % self.pe_mod
        if self.pe is None:
            return self.beta.double()[idx][:, None, :], 0.0
        return self.beta.double(), self.pe.double()[idx][:, None, :]

    def compute(self, mut=None):
        """(ref, z, rstd, mean, var, absmean, n, beta, pe) in fp64; mut names a mutant"""
        x, G = self.x(), max(self.G, 1)
        sel = None
        if mut == "first source" and self.x1 is not None:
            sel = torch.arange(x.shape[-1], device=x.device) < self.x0.shape[-1]
        gid = self.gid(1 if mut == "group shift" else 0)
        mean, var, absm, n = _stats(x, gid, G, sel, 1 if mut == "n - 1" else 0)
        rstd = (var + (0.0 if mut == "no eps" else self.eps)).rsqrt()
        z = (x - mean) * rstd
        beta, pe = self._beta_pe(x.shape[0], mut)
        g = self.gamma.double()
        if self.tables:
            sc = rstd * g
            return (sc.expand(x.shape[0], 1, -1)[:, 0], (beta - mean * sc)[:, 0]), z, rstd, mean, var, absm, n, beta, pe
        v = g * _silu64(z) + beta if (mut == "silu first" and self.silu) else z * g + beta
        if self.silu and mut != "silu first":
            v = _silu64(v)
        v = v + pe
        return (v[:, 0] if self.G == 0 else v), z, rstd, mean, var, absm, n, beta, pe

    def reference(self):
        """(ref, B, S, cap): S the statistics term, cap = U/4 (|gamma| (|z| + 1) + |beta|) that it must stay below.  Tables: ref = (scale,
        shift) with their own bounds (B_scale, B_shift), no output rounding."""
        if self._ref is not None:
            return self._ref
        ref, z, rstd, mean, var, absm, n, beta, pe = self.compute()
        x, g, D = self.x(), self.gamma.double().abs(), self.D
        if self.pivot:                                       # the group's first channel at pixel 0 (norm.hip:92-95, :286)
            gid = self.gid()
            first = torch.arange(max(self.G, 1), device=x.device) * (x.shape[-1] // max(self.G, 1))
            p = x[:, :1, first][:, :, gid]
            m1 = _stats((x - p).abs(), gid, max(self.G, 1))[0]
            dm = (mean - p).abs()
            d_mean = D * U32 * m1 + U32 * mean.abs()
            d_var = (D + 3) * U32 * (var + 2 * dm * dm) + 2 * dm * D * U32 * m1 + d_mean ** 2
        else:
            d_mean = D * U32 * absm + U32 * mean.abs()
            d_var = (D + 3) * U32 * var + d_mean ** 2
        d_r = d_var / (2 * (var + self.eps)) + 3 * U32
        if self.tables:
            sc, sh = ref
            b_sc = (g * rstd * (d_r + U32))[:, 0].expand_as(sc)
            b_sh = (U32 * (beta.abs() + 2 * (mean * rstd).abs() * g) + g * rstd * d_mean + (mean * rstd).abs() * g * d_r)[:, 0].expand_as(sh)
            self._ref = ((sc, sh), (b_sc, b_sh), None, None)
            return self._ref
        pre = z * self.gamma.double() + beta
        pea = pe.abs() if torch.is_tensor(pe) else 0.0
        S = g * (rstd * d_mean + z.abs() * d_r) + U32 * (2 * g * rstd * (x.abs() + mean.abs()) + beta.abs() + pea + 2 * pre.abs())
        if self.silu:
            S = L_SILU * S + (2.0 ** -21 + 2.0 ** -23 * pre.abs()) * _silu64(pre).abs()
        cap = U / 4 * (g * (z.abs() + 1) + beta.abs())
        if self.G == 0:
            S, cap = S[:, 0], cap[:, 0]
        B = (U if self.dt == BF16 else 0.0) * ref.abs() + S
        self._ref = (ref, B, S, cap)
        return self._ref

    def simulate(self):
        """fp32 statistics (exact mean and centred variance in fp32), the affine as x * scale + shift in fp32, one rounding"""
        x = self.x().float()
        gid, G = self.gid(), max(self.G, 1)
        one = F.one_hot(gid, G).float()
        cnt = one.sum(0) * x.shape[1]
        mean = ((x.sum(1) @ one) / cnt)[:, gid][:, None, :]
        var = (((x - mean).pow(2).sum(1) @ one) / cnt)[:, gid][:, None, :]
        rstd = (var + self.eps).rsqrt()
        beta, pe = self._beta_pe(x.shape[0])
        sc = rstd * self.gamma
        sh = (beta.float() if torch.is_tensor(beta) else beta) - mean * sc
        if self.tables:
            return sc.expand(x.shape[0], 1, -1)[:, 0].contiguous(), sh[:, 0].contiguous()
        v = x * sc + sh
        if self.silu:
            v = v / (1.0 + torch.exp(-v))
        if torch.is_tensor(pe):
            v = v + pe.float()
        v = to_storage(v, self.dt)
        return v[:, 0] if self.G == 0 else v

    def mutants(self):
        run = lambda name: self.compute(name)[0]
        m = {"variance divided by n - 1": run("n - 1")}
        if self.G:
            m["group boundary shifted one channel across the seam"] = run("group shift")
            if self.x1 is not None:
                m["mean of the first source only"] = run("first source")
        if self.silu:
            m["SiLU applied before the affine"] = run("silu first")
        if self.pe_mod > 1 and self.pe_div > 1:
            m["pe row row % pe_mod instead of (row / pe_div) % pe_mod"] = run("pe row")
        if self.compute()[4].median().item() <= 20 * self.eps:          # a case scaled so that var is about 10 eps: eps matters
            m["eps omitted"] = run("no eps")
        return m

    def n_per_group(self):
        x = self.x()
        return x.shape[1] * x.shape[2] // max(self.G, 1)


def norm_check(out, case, what=None, factor=2.0):
    """`check` + the assertion that the statistics term stays below U/4 (|gamma| (|z| + 1) + |beta|)"""
    ref, B, S, cap = case.reference()
    assert (S < cap).all(), f"{case.what}: the statistics term reaches {(S / cap).max().item():.3f} of its cap"
    return check(out, ref, B, what or case.what, factor)


def gn_case(tag, NB, HW, c0, c1=0, G=32, eps=1e-5, silu=False, dt=BF16, device="cpu", x_scale=1.5, mean=0.3, tables=False, slab=True, guard=False):
    """x0 = hash_uniform * x_scale + mean, x1 = hash_uniform * 0.7 x_scale / 1.5, gamma = 1 + hash_uniform * 0.2, beta = hash_uniform * 0.2 (the
    suite's recipe)"""
    g = guarded if guard else (lambda t: t)
    x0 = g((rnd(f"{tag}.x0", (NB, HW, c0), x_scale, device=device) + mean).to(dt))
    x1 = g(rnd(f"{tag}.x1", (NB, HW, c1), 0.7 * x_scale / 1.5, dt, device)) if c1 else None
    C = c0 + c1
    form, D = gn_form(c0, c1, G, HW, 8 if dt == BF16 else 4, NB, slab)
    case = Norm(f"{tag} groupnorm {NB} x {HW} x ({c0} | {c1}) {form} {'tables ' if tables else ''}{str(dt)[6:]}", x0, rnd(f"{tag}.g", (C,), 0.2, device=device) + 1.0,
                rnd(f"{tag}.be", (C,), 0.2, device=device), eps, D, G, x1, silu, pivot=form in ("narrow", "general"), tables=tables)
    case.form = form
    return case


def ln_case(tag, rows, C, dt=BF16, device="cpu", pe_div=1, pe_mod=1, folded=False, eps=1e-5, x_scale=2.0, ldx=None, guard=False):
    """x = hash_uniform * x_scale + 0.5 (a view of row stride ldx), gamma = 1 + hash_uniform * 0.2, beta = hash_uniform * 0.2, pe = hash_uniform
    (pe_mod, C); folded: beta is the (pe_mod, C) table beta + pe"""
    ldx = C if ldx is None else ldx
    buf = torch.full((rows + (8 if guard else 0), ldx), NAN, device=device, dtype=dt)
    x = buf[:rows, :C]
    x.copy_((rnd(f"{tag}.x", (rows, C), x_scale, device=device) + 0.5).to(dt))
    gamma, beta = rnd(f"{tag}.g", (C,), 0.2, device=device) + 1.0, rnd(f"{tag}.be", (C,), 0.2, device=device)
    pe = rnd(f"{tag}.pe", (pe_mod, C), 1.0, device=device) if pe_mod > 1 else None
    if folded:
        beta, pe = (beta[None, :] + pe).contiguous(), None
    D, _ = ln_depth(C, 8 if dt == BF16 else 4)
    return Norm(f"{tag} layernorm {rows} x {C} pe ({pe_div}, {pe_mod}){' folded' if folded else ''} {str(dt)[6:]}", x, gamma, beta, eps, D, 0,
                pe=pe, pe_div=pe_div, pe_mod=pe_mod)
