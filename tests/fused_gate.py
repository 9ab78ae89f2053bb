"""The numeric gate of the CHAINED bf16 kernels (csrc/ffn.hip, rowgemm.hip, tleg.hip, gnconv.hip, rconv.hip), torch only, any device: every stage
of a chain observed BY ITSELF.  In the style of tests/mm_gate.py and tests/attn_gate.py, whose contracts, U = 2^-8, `check`, `rejects`, `guarded`
and sentinel helpers are reused; nothing here is fitted to kernel output.

Why.  The chains round to bf16 between their stages, so a whole-chain fp64 reference needs a flat absolute term for the one-ulp flips of the
intermediates (2e-3 .. 8e-3 in tests/test_rowgemm_gpu.py, test_ffn_gpu.py, test_gnconv_gpu.py, test_tleg_gpu.py), and that term hides a tanh
GELU, a variance over n - 1 and a missing eps (tests/test_fused_gate.py asserts all three).  Here the NEIGHBOURS of the observed stage get operands
for which they are exact -- one-hot and power-of-two weights, zero rows, a gate bias of 16 (gelu(16) == 16 in fp32: 16 Phi(-16) < 2^-24 16) -- so the
output is ONE stage's result rounded ONCE and the single-stage contract applies at 2 B.

A case is a `Stage`: `ops` (the kernel's operands as stored), `ref` / `B` (fp64 contract of the observed stage and its bound per element), for
the norm stages also `S` / `cap` (the statistics term and the stated fraction of U (|gamma| (|z| + 1) + |beta|) it must stay below), and
`mutants()` ({name: fp64 reference of what a subtly wrong kernel would store}).  `ff_sim` / `rowgemm_sim` play the WHOLE kernel's arithmetic on
`ops` in torch (fp32 accumulation, bf16 at the rounding points the sources state) and must land within 1 B.

STAGE CONTRACTS
  observed LayerNorm (ln_frag.h, `OnePassNorm`): mm_gate's norm contract -- exact fp64 mean and biased variance of the stored values, rstd =
    (var + eps)^-1/2, affine, beta (+ pe) row, one rounding -- with the statistics term of the ONE-PASS form.  ln_frag.h:25-39: per lane (half a
    row) four accumulators of 20 v_dot2 steps for sum x and four for sum x^2 (a step adds two exact products: at most 2 roundings), the tree
    (s0 + s1) + (s2 + s3) (:37), the partner lane (:38-39): D = 2 * 20 + 2 + 1 = 43 additions on the longest path.  mean = sum * fp32(1 / 320)
    (:40: two roundings), var = max(fma(-mean, mean, sq * fp32(1 / 320)), 0) (:41), rstd = rsqrtf(var + eps) (:42).  So
        d_mean = D u32 E|x| + 2 u32 |mean|
        d_var  = (D + 2) u32 E[x^2] + 2 |mean| d_mean + d_mean^2 + u32 var,    E[x^2] = var + mean^2:  d_var / var ~ (D + 2) u32 (1 + 3 mean^2 / var)
        d_r    = d_var / (2 (var + eps)) + 3 u32
        S      = |gamma| (rstd d_mean + |z| d_r) + u32 (2 |gamma| rstd (|x| + |mean|) + |beta| + 2 |v|)          (:44, :57, :60: -mean rstd, two FMAs)
    and S < frac U (|gamma| (|z| + 1) + |beta|) is asserted with the case's stated frac (1/4 as in mm_gate; the |mean| = 15 and 30 std cases state
    theirs: there the term IS the variance error the one-pass form is allowed).
  observed table apply (ln_frag.h STATS = false, `TableApply`): v = fma(x, scale, shift) (one rounding, u32 |v|; stated as 2 u32 (|x scale| +
    |shift|)), optional SiLU with mm_gate's SiLU term, one rounding.
  observed GELU (ffn.hip:61-89): B = U |ref| + |h| 1e-6 + 2^-22 |ref|: the class ffn.hip:63 and common.h:114 state, and the fp32 product.
  observed GEMM: mm_gate's LINEAR contract over that stage's K with the operands the transparent stages deliver exactly.

ISOLATION (ff_fused; C = 320, inner = 1280).  W2 is one-hot: output channel c observes hidden channel 4 PI(c) + s, PI(c) = (37 c + 11) % 320, in
selection set s = 0 .. 3: every set touches all 40 sub-blocks, the four sets every position of a sub-block.
  GELU sweep   h rows of W1 zero with b1 = h0[j], gate row j one-hot on x channel j / 4 -> out[c] = bf16(h0 gelu(x[PI(c)]))
  LayerNorm    h row j one-hot on channel j / 4, gate rows zero with bias 16, W2 weight 2^-4 -> hidden = 16 xn exactly, out[c] = xn[PI(c)]
  ff1 + GEGLU  random W1 / b1 (gates over [-4, 4]), W2 one-hot -> the LINEAR contract with act = geglu, K = 320
  ff2          h row j = +-2^k on one channel, gate bias 16 -> hidden = 16 2^k x exactly; random W2 / b2 / residual: LINEAR, K = 1280
  po 1         ff2 with Wpo a permutation, bias_po = residual2 = 0: the same contract, permuted;   po 2   W2 = 0, b2 = 0 -> hidden == residual:
               proj_out is LINEAR with K = 320, bias and residual2.
ISOLATION (rowgemm320).  W one-hot (column n observes channel (37 n + 11) % 320) -> the prologue alone, through normal and transposed tiles;
no norm -> LINEAR with bias, bias2 (row groups of 128) and residual."""
import math

import torch

from tests import mm_gate as G
from tests.mm_gate import BF16, U, U32, L_SILU, rnd

C, INNER = 320, 1280
LN_D = 2 * 20 + 2 + 1            # ln_frag.h:25-39, module docstring
GELU_FFN_ERR = 1e-6              # ffn.hip:63 (7.7e-7 stated for the fit), common.h:114: the class the issue's bound names
FF_G = (-1.000055242e+00, -1.150636504e+00, -4.603651887e-01, -5.145699537e-02, 6.927462962e-03, -4.497945628e-04)     # ffn.hip:66-71
H0 = (1.0, -1.0, 0.75, -2.5, 3.0)


def perm320(n, device="cpu"):
    """(37 i + 11) % 320 for i < n: a fixed map onto the 320 channels (a permutation of them when n == 320)"""
    return (37 * torch.arange(n, device=device) + 11) % C


def sel_hidden(s, device="cpu"):
    """the hidden channel output channel c observes in selection set s"""
    return 4 * perm320(C, device) + s


class Stage:
    def __init__(self, what, kernel, ops, ref, B, S=None, cap=None, mutants=None, floor=0.15, **extra):
        self.what, self.kernel, self.ops, self.ref, self.B, self.S, self.cap, self._mut, self.floor = what, kernel, ops, ref, B, S, cap, mutants, floor
        self.weak = ()             # mutants this case cannot reject (their ratio is printed and recorded in DESIGN.md; another case rejects them)
        self.__dict__.update(extra)

    def mutants(self):
        return self._mut() if self._mut else {}

    def assert_not_degenerate(self):
        rms = self.ref.pow(2).mean().sqrt().item()
        assert rms >= self.floor, (self.what, rms)
        return rms


def stage_check(out, st, factor=2.0):
    """mm_gate.check on a stage + the assertion that a statistics term stays below its stated cap"""
    if st.S is not None:
        assert stats_share(st) < 1.0, f"{st.what}: the statistics term reaches {stats_share(st):.3f} of its cap"
    return G.check(out, st.ref, st.B, st.what, factor)


def stats_share(st):
    """max S / cap (0 where both are exactly 0: gamma == 0 and beta == 0, the output is an exact zero)"""
    return torch.where(st.S == 0, torch.zeros_like(st.S), st.S / st.cap).max().item()


# ---- fp32 arithmetic of the kernels in torch ---------------------------------------------------------------------------------------------------

def fma32(a, b, c):
    """fmaf on fp32 tensors (the product is exact in fp64; the double rounding of the sum differs from fmaf only within 2^-29 of a tie)"""
    return (a.double() * b.double() + c.double()).float()


def gelu_ffn(x):
    """ffn.hip:77-89 in torch fp32: x Phi(x) = max(x, 0) - |x| exp2(p(min(|x|, 7)))"""
    x = x.float()
    g = [torch.tensor(v, dtype=torch.float32, device=x.device) for v in FF_G]
    z = x.abs().clamp(max=7.0)
    a = fma32(g[5].expand_as(z), z, g[4])
    for i in (3, 2, 1, 0):
        a = fma32(a, z, g[i])
    return fma32(-x.abs(), torch.exp2(a), x.clamp(min=0))


def gelu_ffn_error(n=1_600_001):
    """max |gelu_ffn - x Phi(x)| over [-8, 8] (beyond, Phi(-|x|) < 1e-15)"""
    x = torch.linspace(-8, 8, n, dtype=torch.float64).float()
    return (gelu_ffn(x).double() - G._gelu64(x.double())).abs().max().item()


def _gelu_tanh64(x):
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def _gelu_sigmoid64(x):
    return x * torch.sigmoid(1.702 * x)


def onepass_stats_sim(x):
    """ln_frag.h:25-41 on bf16 rows (M, 320) in the kernel's accumulation order -> (mean, E[x^2] - mean^2 unclamped) fp32 (M,)"""
    M = x.shape[0]
    xf = x.float().reshape(M, C // 16, 2, 4, 2)                    # (row, ks, hh, accumulator j, element of the pair)
    s = torch.zeros((M, 2, 4), dtype=torch.float32, device=x.device)
    q = torch.zeros_like(s)
    for ks in range(C // 16):
        p = xf[:, ks]
        s = s + (p[..., 0] + p[..., 1])
        q = q + (p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1])
    tree = lambda a: (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])
    sm, sq = tree(s), tree(q)
    sm, sq = sm[:, 0] + sm[:, 1], sq[:, 0] + sq[:, 1]
    inv = torch.tensor(1.0, dtype=torch.float32, device=x.device) / C
    mean = sm * inv
    return mean, fma32(-mean, mean, sq * inv)


def ln_onepass_sim(x, gamma, beta, eps, ddof=0, eps_on=True):
    """layernorm_fragments<20, true> in torch: beta (320,) or one row per x row (M, 320).  ddof / eps_on: the two wrong kernels of the flat-gate
    demonstration."""
    mean, var = onepass_stats_sim(x)
    var = var.clamp(min=0) * (C / (C - ddof))
    rstd = torch.rsqrt(var + (eps if eps_on else 0.0))
    z = fma32(x.float(), rstd[:, None], (-mean * rstd)[:, None])
    return fma32(z, gamma.float(), beta.float()).to(BF16)


def table_apply_sim(x, scale, shift, silu):
    v = fma32(x.float(), scale, shift)
    if silu:
        v = v / (1.0 + torch.exp(-v))
    return v.to(BF16)


def ff_sim(o, gelu="poly", ddof=0, eps_on=True):
    """mmgt_ff_fused / _po on the operands `o` in torch: LayerNorm (one pass) -> bf16 | ff1 in fp32 + b1, h * gelu(g) -> bf16 (ffn.hip:240-254) | ff2
    in fp32 + b2 + residual (:495) [-> bf16 | proj_out + bias_po + residual2 (:425, :495)] -> bf16"""
    xn = o["x"] if o.get("gamma") is None else ln_onepass_sim(o["x"], o["gamma"], o["beta"], o.get("eps", 1e-5), ddof, eps_on)
    hg = xn.float() @ o["w1"].float().t() + o["b1"]
    inner = hg.shape[1] // 2
    h, g = hg[:, :inner], hg[:, inner:]
    act = {"poly": gelu_ffn, "erf": lambda t: G._gelu64(t.double()).float(), "tanh": lambda t: _gelu_tanh64(t.double()).float()}[gelu](g)
    hid = (h * act).to(BF16)
    out = hid.float() @ o["w2"].float().t() + o["b2"] + o["res"].float()
    if o.get("wpo") is not None:
        out = out.to(BF16).float() @ o["wpo"].float().t() + o["bpo"] + o["res2"].float()
    return out.to(BF16)


def _row_groups(M, rows, mod, device):
    idx = torch.arange(M, device=device) // rows
    return idx % mod if mod > 1 else torch.zeros_like(idx)


def rowgemm_sim(o):
    """mmgt_rowgemm320 on `o`: prologue (rowgemm.hip:100-127) -> bf16 | accumulators start from bias + bias2 (:121, :186-197), 20 MFMAs, + residual
    (:235), one rounding -> (M, N), normal and transposed columns alike"""
    x, M = o["x"], o["x"].shape[0]
    if o["norm"]:
        grp = _row_groups(M, o["pe_div"], o["pe_mod"], x.device)
        beta = o["beta"].reshape(-1, C)[grp]
        if o["norm"] == 1:
            x = ln_onepass_sim(x, o["gamma"], beta, o["eps"])
        else:
            x = table_apply_sim(x, o["gamma"].reshape(-1, C)[grp], beta, o["norm"] == 3)
    b = torch.zeros(o["w"].shape[0], dtype=torch.float32, device=x.device) if o["bias"] is None else o["bias"]
    b = b[None, :].expand(M, -1)
    if o["bias2"] is not None:
        b = b + o["bias2"][_row_groups(M, o["bias2_rows"], 1 << 30, x.device)]
    out = b + x.float() @ o["w"].float().t()
    if o["res"] is not None:
        out = out + o["res"].float()
    return out.to(BF16)


# ---- the observed norm stages --------------------------------------------------------------------------------------------------------------------

class OnePassNorm(G.Norm):
    """mm_gate's LayerNorm contract (G = 0) with the statistics term of the one-pass form (module docstring).  frac: the stated fraction of
    U (|gamma| (|z| + 1) + |beta|) the term must stay below."""

    def __init__(self, what, x, gamma, beta, eps, D=LN_D, pe_div=1, pe_mod=1, frac=0.25):
        super().__init__(what, x, gamma, beta, eps, D, 0, pe_div=pe_div, pe_mod=pe_mod)
        self.frac = frac

    def reference(self):
        if self._ref is not None:
            return self._ref
        ref, z, rstd, mean, var, absm, n, beta, pe = self.compute()
        x, g, D = self.x(), self.gamma.double().abs(), self.D
        d_mean = D * U32 * absm + 2 * U32 * mean.abs()
        d_var = (D + 2) * U32 * (var + mean * mean) + 2 * mean.abs() * d_mean + d_mean ** 2 + U32 * var
        d_r = d_var / (2 * (var + self.eps)) + 3 * U32
        pre = z * self.gamma.double() + beta
        S = (g * (rstd * d_mean + z.abs() * d_r) + U32 * (2 * g * rstd * (x.abs() + mean.abs()) + beta.abs() + 2 * pre.abs()))[:, 0]
        cap = (self.frac * U * (g * (z.abs() + 1) + beta.abs()))[:, 0]
        self.rel_var = (d_var / (var + self.eps))[:, 0, 0]
        self._ref = (ref, U * ref.abs() + S, S, cap)
        return self._ref

    def compute(self, mut=None):
        if mut == "row + 1":                                   # the beta (+ pe) row of the NEXT row group
            idx = (torch.arange(self.x().shape[0], device=self.x0.device) // self.pe_div + 1) % self.pe_mod
            r = list(super().compute())
            r[0] = r[0] - self.beta.double()[(idx - 1) % self.pe_mod] + self.beta.double()[idx]
            return tuple(r)
        if mut == "gamma beta swap":                           # channels 2 and 5 of the eight a lane holds (ln_frag.h:51-59), of lane group 3
            g, b = self.gamma.clone(), self.beta.clone()
            for t in (g, b):
                t[..., 26], t[..., 29] = t[..., 29].clone(), t[..., 26].clone()
            return OnePassNorm(self.what, self.x0, g, b, self.eps, self.D, self.pe_div, self.pe_mod).compute()
        return super().compute(mut)


LN_KINDS = {                     # x = hash_uniform * scale + offset  ->  frac (the stated cap fraction)
    "plain": dict(scale=2.0, offset=0.5, frac=0.25),
    "smallvar": dict(scale=0.017, offset=0.0, frac=0.25),     # var ~ 1e-4 = 10 eps: eps matters
    "mean8": dict(scale=1.0, offset=8 / math.sqrt(3), frac=0.25),
    "mean15": dict(scale=1.0, offset=15 / math.sqrt(3), frac=0.5, weak=("variance divided by n - 1",)),      # the allowed one-pass variance error
    "mean30": dict(scale=1.0, offset=30 / math.sqrt(3), frac=1.5, weak=("variance divided by n - 1",)),      # exceeds 1 / 320 there
    "const": dict(scale=0.0, offset=0.0, frac=0.25),         # constant rows: the variance clamps at 0, z == 0, ref == beta
    "outlier": dict(scale=1.0, offset=0.0, frac=0.25),       # one value of 40 per row
}


def ln_input(tag, M, kind, device="cpu"):
    k = LN_KINDS[kind]
    m = torch.arange(M, device=device)
    if kind == "const":
        vals = torch.tensor([0.25, -0.5, 0.375], device=device)
        return vals[m % 3][:, None].expand(M, C).to(BF16).contiguous()
    x = rnd(f"{tag}.x", (M, C), k["scale"], device=device)
    if k["offset"]:
        x = x + k["offset"] * (1 - 2 * (m % 2).float())[:, None]          # the sign of the mean alternates with the row
    if kind == "outlier":
        x[m, (7 * m) % C] = 40.0
    return x.to(BF16)


def _ln_affine(tag, rows, device):
    gamma = rnd(f"{tag}.g", (C,), 0.2, device=device) + 1.0
    beta = rnd(f"{tag}.be", (rows, C), 0.2 if rows == 1 else 1.0, device=device)
    return gamma, (beta[0].contiguous() if rows == 1 else beta)


def _norm_mutants(norm, cols, kind, pe_mod):
    def m():
        run = lambda name: norm.compute(name)[0][:, cols]
        out = {"gamma / beta of two channels of one lane's eight swapped": run("gamma beta swap")}
        if kind != "const":                                    # (constant rows: z == 0, the variance does not reach the output)
            out["variance divided by n - 1"] = run("n - 1")
        if kind == "smallvar":
            out["eps omitted"] = run("no eps")
        if pe_mod > 1:
            out["beta + pe row off by one"] = run("row + 1")
        return out
    return m


class TableApply:
    """x (M, 320) bf16, scale / shift (groups, 320) fp32 of row groups of `rows` rows, SiLU or not -> (ref, B) (module docstring)"""

    def __init__(self, x, scale, shift, rows, silu):
        self.x, self.scale, self.shift, self.rows, self.silu = x, scale, shift, rows, silu

    def compute(self, mut=None):
        x, M = self.x.double(), self.x.shape[0]
        grp = _row_groups(M, self.rows, self.scale.shape[0], x.device)
        if mut == "row + 1":
            grp = (grp + 1) % self.scale.shape[0]
        sc, sh = self.scale.double()[grp], self.shift.double()[grp]
        if mut == "swap":
            sc, sh = sc.clone(), sh.clone()
            for t in (sc, sh):
                t[:, 26], t[:, 29] = t[:, 29].clone(), t[:, 26].clone()
        if mut == "silu first":
            return G._silu64(x) * sc + sh, None
        if mut == "shift first":
            v = (x + sh) * sc
        else:
            v = x * sc + sh
        ref = G._silu64(v) if self.silu else v
        B = 2 * U32 * ((x * sc).abs() + sh.abs())
        if self.silu:
            B = L_SILU * B + (2.0 ** -21 + 2.0 ** -23 * v.abs()) * ref.abs()
        return ref, U * ref.abs() + B

    def mutants(self, cols):
        def m():
            out = {"scale / shift of two channels of one lane's eight swapped": self.compute("swap")[0][:, cols],
                   "shift added before the scale": self.compute("shift first")[0][:, cols]}
            if self.scale.shape[0] > 1:
                out["table row off by one"] = self.compute("row + 1")[0][:, cols]
            if self.silu:
                out["SiLU applied before the affine"] = self.compute("silu first")[0][:, cols]
            return out
        return m


# ---- ff_fused -----------------------------------------------------------------------------------------------------------------------------------

def gelu_sweep_values(device="cpu"):
    """every bf16 value with 2^-10 <= |x| <= 8 (3330), +-0, +-16, +-64, padded to 11 rows of 320 by repeating from the start"""
    bits = torch.arange(0x3A80, 0x4100 + 1, dtype=torch.int32, device=device)              # 2^-10 = 0x3A80 .. 8.0 = 0x4100
    pos = bits.to(torch.int16).view(BF16)
    assert pos[0].item() == 2.0 ** -10 and pos[-1].item() == 8.0 and pos.numel() == 1665
    v = torch.cat([pos, -pos, torch.tensor([0.0, -0.0, 16.0, -16.0, 64.0, -64.0], dtype=BF16, device=device)])
    return torch.cat([v, v[:11 * C - v.numel()]])


def _zeros_ff(M, device):
    return dict(gamma=None, beta=None, w1=torch.zeros((2 * INNER, C), dtype=BF16, device=device),
                b1=torch.zeros(2 * INNER, dtype=torch.float32, device=device), w2=torch.zeros((C, INNER), dtype=BF16, device=device),
                b2=torch.zeros(C, dtype=torch.float32, device=device), res=torch.zeros((M, C), dtype=BF16, device=device))


def _drop_subblock(ref, sel, sb=1):
    """the observed outputs of hidden channels 32 sb .. 32 sb + 31 lost"""
    m = ref.clone()
    m[:, (sel // 32) == sb] = 0
    return m


def ff_gelu_sweep(M, s, device="cpu"):
    """out[m][c] = bf16(h0[j] gelu(x[m][PI(c)])), j = 4 PI(c) + s"""
    vals = gelu_sweep_values(device)
    m, ch = torch.arange(M, device=device)[:, None], torch.arange(C, device=device)[None, :]
    x = vals[((m % 11) * C + ch + 53 * (m // 11)) % vals.numel()]
    o = _zeros_ff(M, device)
    j = torch.arange(INNER, device=device)
    o["w1"][INNER + j, j // 4] = 1.0
    h0 = torch.tensor(H0, dtype=torch.float32, device=device)[(7 * j + j // 32) % len(H0)]
    o["b1"][:INNER] = h0
    sel, pi = sel_hidden(s, device), perm320(C, device)
    o["w2"][torch.arange(C, device=device), sel] = 1.0
    o["x"] = x
    xs, hs = x.double()[:, pi], h0.double()[sel][None, :]
    ref = hs * G._gelu64(xs)
    B = U * ref.abs() + hs.abs() * GELU_FFN_ERR + 2.0 ** -22 * ref.abs()

    def mut():
        return {"tanh GELU": hs * _gelu_tanh64(xs), "x sigmoid(1.702 x)": hs * _gelu_sigmoid64(xs), "a 32-channel sub-block dropped": _drop_subblock(ref, sel)}
    return Stage(f"ff_fused GELU sweep M = {M} set {s}", "ff", o, ref, B, mutants=mut, xs=xs)


def ff_ln_observed(M, s, kind, device="cpu"):
    """out[m][c] = LayerNorm(x)[m][PI(c)]"""
    tag = f"fg.ffln.{kind}"
    o = _zeros_ff(M, device)
    o["x"] = ln_input(tag, M, kind, device)
    o["gamma"], o["beta"] = _ln_affine(tag, 1, device)
    o["eps"] = 1e-5
    j = torch.arange(INNER, device=device)
    o["w1"][j, j // 4] = 1.0
    o["b1"][INNER:] = 16.0
    sel, pi = sel_hidden(s, device), perm320(C, device)
    o["w2"][torch.arange(C, device=device), sel] = 2.0 ** -4
    norm = OnePassNorm(f"ff_fused LayerNorm {kind} M = {M} set {s}", o["x"], o["gamma"], o["beta"], 1e-5, frac=LN_KINDS[kind]["frac"])
    ref, B, S, cap = norm.reference()
    base = _norm_mutants(norm, pi, kind, 1)

    def mut():
        d = base()
        d["a 32-channel sub-block dropped"] = _drop_subblock(ref[:, pi], sel)
        return d
    return Stage(norm.what, "ff", o, ref[:, pi], B[:, pi], S[:, pi], cap[:, pi], mut, floor=0.05 if kind == "const" else 0.15, norm=norm,
                 weak=LN_KINDS[kind].get("weak", ()))


def ff_ff1_geglu(M, s, device="cpu"):
    """out[m][c] = bf16(h gelu(g)) of hidden channel 4 PI(c) + s: mm_gate's LINEAR contract with act = geglu over K = 320"""
    tag = "fg.ff1"
    o = _zeros_ff(M, device)
    o["x"] = rnd(f"{tag}.x", (M, C), 1.0, BF16, device)
    o["w1"] = torch.cat([rnd(f"{tag}.wh", (INNER, C), 1.0 / math.sqrt(C), BF16, device), rnd(f"{tag}.wg", (INNER, C), 6.0 / math.sqrt(C), BF16, device)])
    o["b1"] = torch.cat([rnd(f"{tag}.bh", (INNER,), 0.5, device=device), rnd(f"{tag}.bg", (INNER,), 1.0, device=device)])
    sel = sel_hidden(s, device)
    o["w2"][torch.arange(C, device=device), sel] = 1.0
    rows = torch.cat([sel, INNER + sel])
    lin = G.Linear(f"ff_fused ff1 + GEGLU M = {M} set {s}", o["x"], o["w1"][rows], G.Epi(bias=o["b1"][rows], act="geglu"))
    ref, B = lin.reference()

    def mut():
        d = lin.mutants()
        acc, b = lin.acc, o["b1"][rows].double()
        h, g = acc[:, :C] + b[:C], acc[:, C:]
        d["b1 of the gate added after the GELU"] = h * (G._gelu64(g) + b[C:])
        d["tanh GELU"] = h * _gelu_tanh64(g + b[C:])
        d["a 32-channel sub-block dropped"] = _drop_subblock(ref, sel)
        return d
    # (a tanh GELU under random operands stays inside the accumulation term of the gates: the sweep is the case that rejects it)
    return Stage(lin.what, "ff", o, ref, B, mutants=mut, lin=lin, gates=lin.acc[:, C:] + o["b1"][rows].double()[C:], weak=("tanh GELU",))


def ff_ff2(M, po=0, device="cpu"):
    """hidden = 16 2^k x exactly -> out = bf16(W2 . hidden + b2 + residual): LINEAR over K = 1280.  po = 1: through proj_out as a permutation
    (bias_po = residual2 = 0); po = 2: W2 = 0 and b2 = 0, hidden == residual, proj_out is LINEAR over K = 320 with bias_po and residual2."""
    tag = "fg.ff2"
    o = _zeros_ff(M, device)
    o["x"] = rnd(f"{tag}.x", (M, C), 1.0, BF16, device)
    j = torch.arange(INNER, device=device)
    src = (3 * j + 1) % C
    wj = (1 - 2 * ((j // 3) % 2).float()) * 2.0 ** (-5 + (j % 3).float())            # +-2^-5, 2^-4, 2^-3
    o["w1"][j, src] = wj.to(BF16)
    o["b1"][INNER:] = 16.0
    o["res"] = rnd(f"{tag}.r", (M, C), 1.0, BF16, device)
    what = f"ff_fused{'_po' if po else ''} " + ("ff2", "ff2 through a permuting proj_out", "proj_out")[po] + f" M = {M}"
    if po < 2:
        o["w2"] = rnd(f"{tag}.w2", (C, INNER), 1.0 / math.sqrt(INNER), BF16, device)
        o["b2"] = rnd(f"{tag}.b2", (C,), 0.5, device=device)
        hidden = (16.0 * wj[None, :] * o["x"].float()[:, src]).to(BF16)
        assert torch.equal(hidden.double(), 16.0 * wj.double()[None, :] * o["x"].double()[:, src])
        lin = G.Linear(what, hidden, o["w2"], G.Epi(bias=o["b2"], residual=o["res"]))
    cols = torch.arange(C, device=device)
    if po:
        o["bpo"] = torch.zeros(C, dtype=torch.float32, device=device)
        o["res2"] = torch.zeros((M, C), dtype=BF16, device=device)
        if po == 1:
            cols = (C - 1 - perm320(C, device))
            o["wpo"] = torch.zeros((C, C), dtype=BF16, device=device)
            o["wpo"][torch.arange(C, device=device), cols] = 1.0
        else:
            o["wpo"] = rnd(f"{tag}.wpo", (C, C), 1.0 / math.sqrt(C), BF16, device)
            o["bpo"] = rnd(f"{tag}.bpo", (C,), 0.5, device=device)
            o["res2"] = rnd(f"{tag}.r2", (M, C), 1.0, BF16, device)
            o["w1"][INNER:] = rnd(f"{tag}.wg", (INNER, C), 1.0 / math.sqrt(C), BF16, device)      # W2 == 0: whatever ff1 computes must not matter
            lin = G.Linear(what, o["res"], o["wpo"], G.Epi(bias=o["bpo"], residual=o["res2"]))
    ref, B = lin.reference()

    def mut():
        d = {k: v[:, cols] for k, v in lin.mutants().items()}
        if po < 2:
            a = lin.a.double().clone()
            a[:, 32:64] = 0
            d["a 32-channel sub-block dropped"] = G.epilogue(a @ lin.w.double().t(), lin.ep)[0][:, cols]
        return d
    return Stage(what, "ffpo" if po else "ff", o, ref[:, cols], B[:, cols], mutants=mut, lin=lin)


def ffn_test_operands(M=512, device="cpu"):
    """the operands of tests/test_ffn_gpu.py::test_ff_fused_random_against_fp64 (ln = True) at M rows, and its reference and gate"""
    from mmgt_amd.synthetic import hash_uniform as hu
    bf = lambda t: t.to(BF16)
    x = bf(hu(f"ffn.x{M}", (M, C), 1.5, device) + 0.3)
    o = dict(x=x, gamma=1 + 0.2 * hu("ffn.g", (C,), 1.0, device), beta=0.1 * hu("ffn.b", (C,), 1.0, device), eps=1e-5,
             w1=bf(hu("ffn.w1", (2 * INNER, C), 1.0, device) * C ** -0.5), b1=0.1 * hu("ffn.b1", (2 * INNER,), 1.0, device),
             w2=bf(hu("ffn.w2", (C, INNER), 1.0, device) * INNER ** -0.5), b2=0.1 * hu("ffn.b2", (C,), 1.0, device), res=x)
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    xn = bf(((xd - mu) / torch.sqrt(var + 1e-5) * o["gamma"].double() + o["beta"].double()).float()).double()
    hg = xn @ o["w1"].double().t() + o["b1"].double()
    act = bf((hg[:, :INNER] * torch.nn.functional.gelu(hg[:, INNER:])).float()).double()
    ref = act @ o["w2"].double().t() + o["b2"].double() + x.double()
    return o, ref


def ffn_flat_gate(out, ref):
    """(both asserts of test_ff_fused_random_against_fp64 hold, max |d| / tol)"""
    d = (out.double() - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 4e-3
    return bool((d <= tol).all() and d.mean() <= 2.0 ** -9 * ref.abs().mean()), (d / tol).max().item()


# ---- rowgemm320 ---------------------------------------------------------------------------------------------------------------------------------

def _rg_ops(x, w, **kw):
    o = dict(x=x, w=w, norm=0, gamma=None, beta=None, pe_div=0, pe_mod=0, eps=1e-5, bias=None, bias2=None, bias2_rows=0, res=None)
    o.update(kw)
    return o


def rg_linear(M, N, n1=None, device="cpu"):
    """no prologue: LINEAR over K = 320 with bias, bias2 (row groups of 128) and, on normal tiles only (rowgemm.hip:293), a residual"""
    n1 = N if n1 is None else n1
    tag = f"fg.rg.lin{N}"
    x = rnd(f"{tag}.x", (M, C), 1.0, BF16, device)
    w = rnd(f"{tag}.w", (N, C), 1.0 / math.sqrt(C), BF16, device)
    ep = G.Epi(bias=rnd(f"{tag}.b", (N,), 0.5, device=device), bias2=rnd(f"{tag}.b2", ((M + 127) // 128, N), 0.5, device=device), bias2_rows=128,
               residual=rnd(f"{tag}.r", (M, N), 1.0, BF16, device) if n1 == N else None)
    lin = G.Linear(f"rowgemm320 linear M = {M} N = {N} n1 = {n1}", x, w, ep)
    ref, B = lin.reference()
    o = _rg_ops(x, w, bias=ep.bias, bias2=ep.bias2, bias2_rows=128, res=ep.residual)
    return Stage(lin.what, "rowgemm", o, ref, B, mutants=lin.mutants, lin=lin, n1=n1)


def rg_norm_observed(M, N, norm, kind="plain", n1=None, device="cpu"):
    """W one-hot: column n observes channel (37 n + 11) % 320 of the prologue's output.  norm 1: LayerNorm with beta + pe rows (pe_div 128, pe_mod
    3); 2 / 3: scale / shift tables per 128 rows (+ SiLU)."""
    n1 = N if n1 is None else n1
    tag = f"fg.rg.n{norm}.{kind}"
    cols = perm320(N, device)
    w = torch.zeros((N, C), dtype=BF16, device=device)
    w[torch.arange(N, device=device), cols] = 1.0
    groups = (M + 127) // 128
    if norm == 1:
        x = ln_input(tag, M, kind, device)
        gamma, beta = _ln_affine(tag, 3, device)
        nc = OnePassNorm(f"rowgemm320 LayerNorm {kind} M = {M} N = {N} n1 = {n1}", x, gamma, beta, 1e-5, pe_div=128, pe_mod=3, frac=LN_KINDS[kind]["frac"])
        ref, B, S, cap = nc.reference()
        o = _rg_ops(x, w, norm=1, gamma=gamma, beta=beta, pe_div=128, pe_mod=3)
        return Stage(nc.what, "rowgemm", o, ref[:, cols], B[:, cols], S[:, cols], cap[:, cols], _norm_mutants(nc, cols, kind, 3 if M > 128 else 1),
                     floor=0.05 if kind == "const" else 0.15, norm=nc, n1=n1, weak=LN_KINDS[kind].get("weak", ()))
    x = (rnd(f"{tag}.x", (M, C), 1.5, device=device) + 0.3).to(BF16)
    scale = rnd(f"{tag}.sc", (groups, C), 0.4, device=device) + 1.0
    shift = rnd(f"{tag}.sh", (groups, C), 1.0, device=device)
    ta = TableApply(x, scale, shift, 128, norm == 3)
    ref, B = ta.compute()
    o = _rg_ops(x, w, norm=norm, gamma=scale, beta=shift, pe_div=128, pe_mod=groups)
    return Stage(f"rowgemm320 tables{' + SiLU' if norm == 3 else ''} M = {M} N = {N} n1 = {n1}", "rowgemm", o, ref[:, cols], B[:, cols],
                 mutants=ta.mutants(cols), n1=n1)


# ---- temporal_leg320 ----------------------------------------------------------------------------------------------------------------------------
# tleg.hip: rows (b, f, pixel); xn = bf16(LayerNorm(x) gamma + bpe[f]) (:222-273, its OWN one-pass LayerNorm: a lane holds a quarter row, four
# accumulators of 10 v_dot2 steps, the tree, two exchanges in quad_sum: D = 2 * 10 + 2 + 2 = 24); q | k | v = bf16(W xn) (:333-358); per pixel and
# head s = k q^T in fp32 over the 40 channels (:382-383), p = exp2(fma(s, scale log2 e, -max scale log2 e)) (:404), the denominator sums the
# UNROUNDED p (:405), p -> bf16 (:407), O = bf16(V^T P^T / sum) (:420); out = bf16(bias + Wo O + x) (:464-489).
#
# Frame code.  gamma = 0 on F code channels cc[i] whose bpe rows hold 4 [f == i]: xn carries an exact one-hot frame code.  Wk copies it to head
# channel slot(i) of every head, Wq a per-head PERMUTED copy: the score is 16 [perm_h(f) == f'], times scale 8 the softmax is exactly one-hot
# (exp2(-184) == 0) and head h of frame f receives v_h[perm_h(f)] (tests/test_tleg_gpu.py::test_temporal_leg_routes_every_pixel_frame_head).
#   LayerNorm    gamma != 0 on the other channels, Wv = I, Wo = 64 I: out = bf16(64 xn[perm_h(f)] + x): the norm contract times 64 + one more rounding
#   V GEMM       gamma = 0 (xn = bpe[f] exactly), Wv random, Wo = I: out = bf16(v[perm_h(f)] + x); x == 0 on half of the elements, where the second
#                rounding is exact.  to_out GEMM: Wv one-hot, Wo random + bias + residual: LINEAR over K = 320, one rounding
#   q (k) GEMM   k (q) and v are the code: score[f][f'] = 4 q_h[f][slot(f')] (4 k_h[f'][slot(f)]), v = [f' == slot]: channel slot(f') of head h is
#                the probability of key f'.  Contract: the softmax of the UNROUNDED fp64 projection, B = U (sum P |v| + 2 |ref|) (attn_gate) and
#                B_s = sum_j P_j expm1(2 d_j) |v_j - ref| with d_j = 4 scale B_q the projection's LINEAR bound (its bf16 rounding included), gated as
#                |out - ref| <= 2 B + B_s.  Code offsets put slot() on head channels 0 .. F - 1, 40 - F .. 39 (and 14 .. 25 for F = 12).
#   attention    gamma = 0, Wq = Wk = Wv = Wo = I on a random bf16 table: attn_gate's contract with tleg's roundings; d_j = 43 u32 scale sum |q k|.
TL_H, TL_HD, TL_D = 8, 40, 2 * 10 + 2 + 2


def onepass_stats_quarter_sim(x):
    """tleg.hip:229-244 -> (mean, E[x^2] - mean^2 unclamped) fp32 (M,)"""
    M = x.shape[0]
    xf = x.float().reshape(M, C // 32, 4, 4, 2)                    # (row, ks, lq, accumulator j, element of the pair)
    s = torch.zeros((M, 4, 4), dtype=torch.float32, device=x.device)
    q = torch.zeros_like(s)
    for ks in range(C // 32):
        p = xf[:, ks]
        s = s + (p[..., 0] + p[..., 1])
        q = q + (p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1])
    tree = lambda a: (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])
    sm, sq = tree(tree(s)), tree(tree(q))
    inv = torch.tensor(1.0, dtype=torch.float32, device=x.device) / C
    mean = sm * inv
    return mean, fma32(-mean, mean, sq * inv)


def tleg_frames(o):
    return (torch.arange(o["x"].shape[0], device=o["x"].device) // o["n"]) % o["F"]


def tleg_sim(o):
    """mmgt_temporal_leg320 on `o` in torch with the roundings listed above"""
    x, Bn, F, n = o["x"], o["B"], o["F"], o["n"]
    M = x.shape[0]
    mean, var = onepass_stats_quarter_sim(x)
    rstd = torch.rsqrt(var.clamp(min=0) + o["eps"])
    z = fma32(x.float(), rstd[:, None], (-mean * rstd)[:, None])
    xn = fma32(z, o["g"], o["bpe"][tleg_frames(o)]).to(BF16)
    q, k, v = ((xn.float() @ o[t].float().t()).to(BF16).float() for t in ("wq", "wk", "wv"))
    sp = lambda t: t.view(Bn, F, n, TL_H, TL_HD).permute(0, 2, 3, 1, 4)                  # (B, n, H, F, HD)
    s = sp(q) @ sp(k).transpose(-1, -2)
    c = torch.tensor(o["scale"], dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    e = torch.exp2(fma32(s, c.to(x.device), -s.max(-1, keepdim=True).values * c.to(x.device)))
    att = (e.to(BF16).float() @ sp(v)) * (1.0 / e.sum(-1, keepdim=True))
    att = att.to(BF16).float().permute(0, 3, 1, 2, 4).reshape(M, C)
    return (o["bo"] + att @ o["wo"].float().t() + x.float()).to(BF16)


def _tleg_code(F):
    """(code channels cc (F,), their frame i)"""
    return (C // F) * torch.arange(F) + 3


def _tleg_perms(F):
    gen = torch.Generator().manual_seed(100 + F)
    return torch.stack([torch.randperm(F, generator=gen) for _ in range(TL_H)])          # (H, F): perm_h(f)


def _tleg_base(tag, B, F, n, device, x_scale=1.0, mask=True):
    """operands with the frame code in bpe and every weight zero; x = hash_uniform, zero where (channel + pixel) is even if `mask`"""
    M = B * F * n
    x = rnd(f"{tag}.x", (M, C), x_scale, device=device)
    if mask:
        pix = torch.arange(M, device=device) % n
        x = x * ((pix[:, None] + torch.arange(C, device=device)[None, :]) % 2).float()
    z = lambda *s: torch.zeros(s, dtype=BF16, device=device)
    bpe = torch.zeros((F, C), device=device)
    cc = _tleg_code(F).to(device)
    bpe[torch.arange(F, device=device), cc] = 4.0
    return dict(x=x.to(BF16), g=torch.zeros(C, device=device), bpe=bpe, wq=z(C, C), wk=z(C, C), wv=z(C, C), wo=z(C, C),
                bo=torch.zeros(C, device=device), B=B, F=F, n=n, scale=8.0, eps=1e-5), cc


def _tleg_route(o, cc, off=0, permuted=True):
    """Wk / Wq copy the code to head channels off + i (the key of frame i) / off + perm_h(i): returns src (M, 320), the row whose head-h value
    output row m receives on the channels of head h"""
    F, n, dev = o["F"], o["n"], o["x"].device
    perms = _tleg_perms(F).to(dev) if permuted else torch.arange(F, device=dev)[None, :].expand(TL_H, -1)
    i = torch.arange(F, device=dev)
    for h in range(TL_H):
        o["wk"][TL_HD * h + off + i, cc] = 1.0
        o["wq"][TL_HD * h + off + perms[h], cc] = 1.0
    m = torch.arange(o["x"].shape[0], device=dev)
    f = (m // n) % F
    src = m[:, None] + (perms[:, f].t() - f[:, None]) * n                                   # (M, H)
    return src.repeat_interleave(TL_HD, 1)


def _second_rounding(ref, B, x):
    """out = bf16(ref + x) behind a stage already rounded to bf16: exact where x == 0 (the sum is the stored bf16 value), one more U |ref| elsewhere"""
    r = ref + x.double()
    return r, B + torch.where(x == 0, 0.0, 1.0) * U * r.abs() + 2 * U32 * r.abs()


def _nbr_residual(ref, x):
    """the residual of the NEXT row (the last row: of the previous one)"""
    xd = x.double()
    return ref - xd + torch.cat([xd[1:], xd[-2:-1]])


def tleg_ln_observed(B, F, n, kind, device="cpu"):
    tag = f"fg.tl.ln.{kind}"
    o, cc = _tleg_base(tag, B, F, n, device, mask=False)
    o["x"] = ln_input(tag, B * F * n, kind, device)
    o["g"] = rnd(f"{tag}.g", (C,), 0.2, device=device) + 1.0
    o["g"][cc] = 0.0
    code = o["bpe"].clone()
    o["bpe"] = rnd(f"{tag}.bpe", (F, C), 1.0, device=device)
    o["bpe"][:, cc] = code[:, cc]
    src = _tleg_route(o, cc)
    eye = torch.eye(C, device=device)
    o["wv"], o["wo"] = eye.to(BF16), (64.0 * eye).to(BF16)
    nc = OnePassNorm(f"temporal_leg320 LayerNorm + pe {kind} B = {B} F = {F} n = {n}", o["x"], o["g"], o["bpe"], 1e-5, D=TL_D, pe_div=n, pe_mod=F,
                     frac=LN_KINDS[kind]["frac"])
    rl, Bl, S, cap = nc.reference()
    gather = lambda t: 64.0 * torch.gather(t, 0, src)
    ref, Bt = _second_rounding(gather(rl), gather(Bl), o["x"])
    base = _norm_mutants(nc, slice(None), kind, F)

    def mut():
        d = {k: gather(v) + o["x"].double() for k, v in base().items()}
        d["the neighbouring row's residual"] = _nbr_residual(ref, o["x"])
        return d
    return Stage(nc.what, "tleg", o, ref, Bt, gather(S) / 64.0, gather(cap) / 64.0, mut, norm=nc, weak=LN_KINDS[kind].get("weak", ()))


def _swap_3239(t):
    """channels 32 .. 39 exchanged between the two heads of every pair (the tile tleg.hip shares between them)"""
    t = t.clone()
    for g in range(TL_H // 2):
        a, b = TL_HD * 2 * g + 32, TL_HD * (2 * g + 1) + 32
        t[..., a:a + 8], t[..., b:b + 8] = t[..., b:b + 8].clone(), t[..., a:a + 8].clone()
    return t


def tleg_v_gemm(B, F, n, device="cpu"):
    tag = "fg.tl.v"
    o, cc = _tleg_base(tag, B, F, n, device)
    code = o["bpe"].clone()
    o["bpe"] = rnd(f"{tag}.bpe", (F, C), 1.0, BF16, device).float()
    o["bpe"][:, cc] = code[:, cc]
    src = _tleg_route(o, cc)
    o["wv"] = rnd(f"{tag}.wv", (C, C), 1.0 / math.sqrt(C), BF16, device)
    o["wo"] = torch.eye(C, device=device).to(BF16)
    lin = G.Linear(f"temporal_leg320 V GEMM B = {B} F = {F} n = {n}", o["bpe"].to(BF16), o["wv"], G.Epi())
    rv, Bv = lin.reference()
    fr = tleg_frames(o)
    gather = lambda t: torch.gather(t[fr], 0, src)
    ref, Bt = _second_rounding(gather(rv), gather(Bv), o["x"])

    def mut():
        d = {k: gather(v) + o["x"].double() for k, v in lin.mutants().items()}
        d["channels 32 .. 39 swapped between the two heads of a pair"] = gather(_swap_3239(rv)) + o["x"].double()
        d["the neighbouring row's residual"] = _nbr_residual(ref, o["x"])
        return d
    return Stage(lin.what, "tleg", o, ref, Bt, mutants=mut, lin=lin)


def tleg_out_gemm(B, F, n, device="cpu"):
    tag = "fg.tl.o"
    o, cc = _tleg_base(tag, B, F, n, device, mask=False)
    code = o["bpe"].clone()
    o["bpe"] = rnd(f"{tag}.bpe", (F, C), 1.0, BF16, device).float()
    o["bpe"][:, cc] = code[:, cc]
    src = _tleg_route(o, cc)
    srcv = (C - 1 - perm320(C, device))
    o["wv"][torch.arange(C, device=device), srcv] = 1.0
    o["wo"] = rnd(f"{tag}.wo", (C, C), 1.0 / math.sqrt(C), BF16, device)
    o["bo"] = rnd(f"{tag}.bo", (C,), 0.5, device=device)
    att = torch.gather(o["bpe"][:, srcv][tleg_frames(o)], 0, src).to(BF16)
    lin = G.Linear(f"temporal_leg320 to_out GEMM B = {B} F = {F} n = {n}", att, o["wo"], G.Epi(bias=o["bo"], residual=o["x"]))
    ref, Bt = lin.reference()

    def mut():
        d = lin.mutants()
        d["channels 32 .. 39 swapped between the two heads of a pair"] = G.epilogue(_swap_3239(att).double() @ o["wo"].double().t(), lin.ep)[0]
        d["the neighbouring row's residual"] = _nbr_residual(ref, o["x"])
        return d
    return Stage(lin.what, "tleg", o, ref, Bt, mutants=mut, lin=lin)


def _softmax_stage(s, dlt):
    """s (..., F keys) fp64 scores (scale applied), dlt their absolute error bound -> (P, B_attn + B_s / 2) for v = one-hot on the key axis"""
    P = torch.softmax(s, -1)
    w = P * torch.expm1(2 * dlt)
    tot = w.sum(-1, keepdim=True)
    Bs = w * (1 - P) + (tot - w) * P
    return P, 3 * U * P + Bs / 2


def tleg_qk_scores(B, F, n, which, off, device="cpu", scale=1.5):
    """which = "q": q random, k and v the code; "k": k random, q and v the code.  Head channel off + j of the output is the probability of key j."""
    tag = f"fg.tl.{which}"
    o, cc = _tleg_base(tag, B, F, n, device)
    code = o["bpe"].clone()
    o["bpe"] = rnd(f"{tag}.bpe", (F, C), 1.0, BF16, device).float()
    o["bpe"][:, cc] = code[:, cc]
    _tleg_route(o, cc, off, permuted=False)
    o["wv"] = 0.25 * o["wk"]                                                                 # v_h[f'] = [channel == off + f']
    o["w" + which] = rnd(f"{tag}.w", (C, C), 2.0 / math.sqrt(C), BF16, device)
    o["wo"] = torch.eye(C, device=device).to(BF16)
    o["scale"] = scale
    lin = G.Linear(f"temporal_leg320 {which} GEMM through the scores B = {B} F = {F} n = {n} code at {off}", o["bpe"].to(BF16), o["w" + which], G.Epi())
    acc, Bq = lin.reference()
    slots = (TL_HD * torch.arange(TL_H, device=device)[:, None] + off + torch.arange(F, device=device)[None, :])     # (H, F)

    def scores(a, sc=scale, drop_last=False):
        t = a[:, slots]                                                                     # (F rows, H, F slots)
        s = 4 * sc * (t.permute(1, 0, 2) if which == "q" else t.permute(1, 2, 0))           # (H, query f, key f')
        if drop_last:
            s = s.clone()
            s[..., -1] = -1e30
        return s

    def spread(P):
        """(H, F, F) -> (F, 320): head channel off + f' of frame f"""
        r = torch.zeros((F, C), dtype=torch.float64, device=device)
        r[:, slots.flatten()] = P.permute(1, 0, 2).reshape(F, -1)
        return r
    P, Bp = _softmax_stage(scores(acc), scores(Bq))
    fr = tleg_frames(o)
    ref, Bt = _second_rounding(spread(P)[fr], spread(Bp)[fr], o["x"])
    xd = o["x"].double()

    def mut():
        sm = lambda s: spread(torch.softmax(s, -1))[fr] + xd
        return {"channels 32 .. 39 swapped between the two heads of a pair": sm(scores(_swap_3239(acc))),
                "last frame dropped as a key": sm(scores(acc, drop_last=True)), "scale (1 + 2^-5)": sm(scores(acc, scale * (1 + 2.0 ** -5))),
                "last k dropped": sm(scores(lin.mutants()["last k dropped"])), "the neighbouring row's residual": _nbr_residual(ref, o["x"])}
    weak = () if off + F > 32 else ("channels 32 .. 39 swapped between the two heads of a pair",)       # (the code does not reach the shared tile)
    return Stage(lin.what, "tleg", o, ref, Bt, mutants=mut, lin=lin, P=P, weak=weak)


def tleg_attention(B, F, n, device="cpu", scale=0.3):
    tag = "fg.tl.att"
    o, _ = _tleg_base(tag, B, F, n, device)
    o["bpe"] = rnd(f"{tag}.bpe", (F, C), 1.0, BF16, device).float()
    eye = torch.eye(C, device=device).to(BF16)
    o["wq"], o["wk"], o["wv"], o["wo"] = eye, eye.clone(), eye.clone(), eye.clone()
    o["scale"] = scale
    t = o["bpe"].double().view(F, TL_H, TL_HD).permute(1, 0, 2)                             # (H, F, HD): q = k = v

    def att(k, sc=scale, drop_last=False):
        s = sc * (t @ k.transpose(-1, -2))
        if drop_last:
            s[..., -1] = -1e30
        P = torch.softmax(s, -1)
        return P, (P @ t).permute(1, 0, 2).reshape(F, C)
    P, r = att(t)
    dlt = 43 * U32 * scale * (t.abs() @ t.abs().transpose(-1, -2))
    w = P * torch.expm1(2 * dlt)
    Bs = (w[..., None] * (t[:, None, :, :] - (P @ t)[:, :, None, :]).abs()).sum(2)          # (H, F, HD)
    Ba = U * ((P @ t.abs()) + 2 * (P @ t).abs()) + Bs / 2
    fr = tleg_frames(o)
    ref, Bt = _second_rounding(r[fr], Ba.permute(1, 0, 2).reshape(F, C)[fr], o["x"])
    xd = o["x"].double()

    def mut():
        ts = _swap_3239(o["bpe"].double()).view(F, TL_H, TL_HD).permute(1, 0, 2)
        return {"channels 32 .. 39 of k swapped between the two heads of a pair": att(ts)[1][fr] + xd,
                "last frame dropped as a key": att(t, drop_last=True)[1][fr] + xd, "scale (1 + 2^-5)": att(t, scale * (1 + 2.0 ** -5))[1][fr] + xd,
                "the neighbouring row's residual": _nbr_residual(ref, o["x"])}
    return Stage(f"temporal_leg320 attention B = {B} F = {F} n = {n}", "tleg", o, ref, Bt, mutants=mut, P=P)


# ---- gn_silu_conv3x3 (gnconv.hip) and gn_silu_conv3x3_unet (rconv.hip) --------------------------------------------------------------------------
# Both: act = bf16(silu(fma(x, scale[n, c], shift[n, c]))) written to the LDS halo, ZEROS outside the image (gnconv.hip:144-161, rconv.hip:259-293:
# t * v_rcp_f32(1 + v_exp_f32(t * -log2 e)), the mask applied to the packed result), then the implicit GEMM over (ky, kx, cin) in fp32, bias
# (+ bias2[n / b2_imgs]) (+ residual), one rounding.
#   activation, tap by tap   w[co][ci][ky][kx] = 1 for ONE tap and ci = (37 co + 11 + s Cout) % Cin (selection sets s < Cin / Cout cover every input
#                            channel), no bias: out[n][y][x][co] = act[n][y + ky - 1][x + kx - 1][ci], an exact 0 outside the image -> the table
#                            apply + SiLU contract (`TableApply`), one rounding
#   conv alone               x and shift integers with x + shift in [18, 64], scale = 1: fma and SiLU are exact in fp32 (e^-18 < 2^-25: 1 + e == 1,
#                            rcp(1) == 1), bit for bit as the tap cases with the same inputs show -> mm_gate's CONV contract over K = 9 Cin with
#                            random zero-mean weights.
LOG2E = 1.4426950408889634


def conv_act_sim(x, scale, shift):
    t = fma32(x.float(), scale[:, None, None, :], shift[:, None, None, :])
    e = torch.exp2(t * torch.tensor(-LOG2E, dtype=torch.float32, device=x.device))
    return (t * (1.0 / (1.0 + e))).to(BF16)


def conv_sim(o):
    x = o["x0"] if o["x1"] is None else torch.cat([o["x0"], o["x1"]], 3)
    return G.Conv("sim", conv_act_sim(x, o["scale"], o["shift"]), o["w"], o["ep"]).simulate()


def _conv_inputs(tag, NB, H, W, cin, exact, device):
    """(x (NB, H, W, cin) bf16, scale, shift (NB, cin) fp32)"""
    if exact:
        x = torch.floor(rnd(f"{tag}.x", (NB, H, W, cin), 15.0, device=device) + 33.0)                # integers 18 .. 47
        shift = torch.floor(rnd(f"{tag}.sh", (NB, cin), 8.0, device=device) + 8.5)                    # integers 0 .. 16
        return x.to(BF16), torch.ones((NB, cin), device=device), shift
    x = (rnd(f"{tag}.x", (NB, H, W, cin), 1.5, device=device) + 0.3).to(BF16)
    return x, rnd(f"{tag}.sc", (NB, cin), 0.4, device=device) + 1.0, rnd(f"{tag}.sh", (NB, cin), 1.0, device=device)


def _act_contract(x, scale, shift):
    """(ref, B) of the table apply + SiLU on (NB, H, W, C)"""
    xd, sc, sh = x.double(), scale.double()[:, None, None, :], shift.double()[:, None, None, :]
    v = xd * sc + sh
    ref = G._silu64(v)
    B = L_SILU * 2 * U32 * ((xd * sc).abs() + sh.abs()) + (2.0 ** -21 + 2.0 ** -23 * v.abs()) * ref.abs()
    return ref, U * ref.abs() + B


def _shift_tap(t, ky, kx, fill=None):
    """out[n][y][x] = t[n][y + ky - 1][x + kx - 1], `fill` (NB, 1, 1, C) or zeros outside the image"""
    NB, H, W, Cc = t.shape
    p = torch.zeros((NB, H + 2, W + 2, Cc), dtype=t.dtype, device=t.device) if fill is None else fill.expand(NB, H + 2, W + 2, Cc).clone()
    p[:, 1:H + 1, 1:W + 1] = t
    return p[:, ky:ky + H, kx:kx + W]


def conv_sets(cin, cout):
    return max(1, cin // cout)


def conv_tap(kernel, c0, c1, cout, NB, H, W, tap, s, exact=False, device="cpu"):
    cin, (ky, kx) = c0 + c1, divmod(tap, 3)
    tag = f"fg.cv.{kernel}.{cin}.{int(exact)}"
    x, scale, shift = _conv_inputs(tag, NB, H, W, cin, exact, device)
    co = torch.arange(cout, device=device)
    ci = (37 * co + 11 + s * cout) % cin
    w = torch.zeros((cout, cin, 3, 3), dtype=BF16, device=device)
    w[co, ci, ky, kx] = 1.0
    ra, Ba = _act_contract(x, scale, shift)
    ref, B = _shift_tap(ra, ky, kx)[..., ci], _shift_tap(Ba, ky, kx)[..., ci]
    o = dict(x0=x[..., :c0].contiguous(), x1=x[..., c0:].contiguous() if c1 else None, scale=scale, shift=shift, w=w, ep=G.Epi(), b2_imgs=0)

    def mut():
        d = {"the next tap of the row": _shift_tap(ra, ky, (kx + 1) % 3)[..., ci]}
        if ky != kx:
            d["transposed tap"] = _shift_tap(ra, kx, ky)[..., ci]
        if tap != 4:
            d["padding before the activation"] = _shift_tap(ra, ky, kx, G._silu64(shift.double())[:, None, None, :])[..., ci]
        if kx == 0 and W > 16:
            m = ref.clone()
            m[:, :, 16] = _shift_tap(ra, ky, kx)[:, :, 15, ci]
            d["tile-seam column off by one"] = m
        if c1:
            rs = ra.clone()
            rs[..., c0 - 1], rs[..., c0] = ra[..., c0], ra[..., c0 - 1]
            d["x | x1 seam channels swapped"] = _shift_tap(rs, ky, kx)[..., ci]
        return d
    seam = bool(c1) and bool(((ci == c0 - 1) | (ci == c0)).any())
    return Stage(f"{kernel} activation {c0} | {c1} -> {cout} {NB} x {H} x {W} tap ({ky}, {kx}) set {s}{' exact inputs' if exact else ''}", kernel, o, ref, B,
                 mutants=mut, weak=() if (not c1 or seam) else ("x | x1 seam channels swapped",),
                 exact_ref=_shift_tap(x.double() + shift.double()[:, None, None, :], ky, kx)[..., ci] if exact else None)


def conv_alone(kernel, c0, c1, cout, NB, H, W, device="cpu"):
    cin = c0 + c1
    tag = f"fg.cv.{kernel}.{cin}.1"
    x, scale, shift = _conv_inputs(tag, NB, H, W, cin, True, device)
    act = (x.float() + shift[:, None, None, :]).to(BF16)
    assert torch.equal(act.double(), x.double() + shift.double()[:, None, None, :]) and act.min() >= 18
    w = rnd(f"{tag}.w{cout}", (cout, cin, 3, 3), 1.0 / math.sqrt(9 * cin), BF16, device)
    M = NB * H * W
    unet = kernel == "rconv"
    res = None if (cin, cout) == (128, 64) else rnd(f"{tag}.r{cout}", (M, cout), 1.0, BF16, device)
    ep = G.Epi(bias=rnd(f"{tag}.b{cout}", (cout,), 0.5, device=device), bias2=rnd(f"{tag}.b2{cout}", (NB, cout), 0.5, device=device) if unet else None,
               bias2_rows=H * W if unet else 0, residual=res)
    cv = G.Conv(f"{kernel} conv alone {c0} | {c1} -> {cout} {NB} x {H} x {W}", act[..., :c0].contiguous(), w, ep, x1=act[..., c0:].contiguous() if c1 else None)
    ref, B = cv.reference()
    o = dict(x0=x[..., :c0].contiguous(), x1=x[..., c0:].contiguous() if c1 else None, scale=scale, shift=shift, w=w, ep=ep, b2_imgs=1 if unet else 0)

    def mut():
        d = cv.mutants()
        v = G._silu64(shift.double())                                                      # what a padding pixel holds if the padding comes first
        const = v[:, None, None, :].expand(NB, H, W, cin).contiguous()
        extra = (v @ w.double().sum((2, 3)).t())[:, None, None, :] - G.conv_acc(const, w.double(), 1, False)
        d["padding before the activation"] = cv._epi(cv.acc + extra)[0]
        return d
    return Stage(cv.what, kernel, o, ref, B, mutants=mut, conv=cv)


# ---- the one-pass variance, measured through a kernel --------------------------------------------------------------------------------------------
# The bf16 output rounding (2^-9 relative) hides a relative rstd error of 1e-5 .. 1e-4 on a single element.  The probe cancels most of the
# normalised value before the rounding: gamma = 1 and a beta ROW per row group (rowgemm320 takes one per 128 rows) with
# beta[g][c] = fp32(-(1 - 2^-10) z_g[c]), z_g the exact normalised row g, so the kernel stores y = z' - (1 - 2^-10) z with z' = z (1 + e) + const:
# |y| ~ 2^-10 |z|, its rounding is 2^-19 |z|, and the least-squares slope of (out - ref) on z over the 320 channels is e (z has zero mean: a mean
# error, a constant, does not enter).  At a large mean x sits on a coarse bf16 grid, a row holds few distinct z and the roundings do not average
# out as 320 independent ones would: the estimate is good to 3e-6 (tests/test_fused_gate.py), 2^-6 instead of 2^-10 gave 5e-5.  The variance
# error is -2 e.

def variance_probe(kind, groups, device="cpu"):
    """(x (groups, 320) bf16 rows, beta rows (groups, 320) fp32, z fp64, ref fp64 of fma(z, 1, beta), the variance's derived relative bound, |mean| / std)"""
    x = ln_input(f"fg.probe.{kind}", groups, kind, device)
    xd = x.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    z = (xd - mean) * (var + 1e-5).rsqrt()
    beta = (-(1 - 2.0 ** -10) * z).float()
    nc = OnePassNorm(kind, x, torch.ones(C, device=device), torch.zeros(C, device=device), 1e-5)
    nc.reference()
    return x, beta, z, z + beta.double(), nc.rel_var, (mean.abs() / var.sqrt())[:, 0]


def variance_probe_estimate(out, z, ref):
    """out (groups, 320): the stored rows -> relative error of the variance per row"""
    e = ((out.double() - ref) * z).sum(1) / (z * z).sum(1)
    return -2 * e
