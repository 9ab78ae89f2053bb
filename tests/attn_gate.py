"""The numeric gate of the bf16 attention kernels (csrc/attention.hip, attn64.hip, attn80.hip, tattn.hip), torch only, any device.

The arithmetic contract of those kernels: Q' = bf16(fp32(q) * fp32(scale * log2 e)) is the operand of the score MFMA, the scores and the
accumulators are fp32, P = exp2(score - reference) is rounded to bf16 for the P.V MFMA, the denominator is the sum of the probabilities, the
output is rounded to bf16; the softmax reference (running maximum, lagging maximum, maximum of the first 32 keys) cancels in the quotient.

`contract(...)` is that computation in fp64 with only the Q' rounding modelled; the gate is  |out - ref| <= 2 B  on EVERY element with
    B[i][d] = u * (sum_j P[i][j] |v[j][d]| + 2 |ref[i][d]|),   u = 2^-8  (bf16 unit roundoff):
rounding P costs at most u sum P |v| in the numerator, the denominator is a sum of the same rounded values (at most u |ref|) and the output is
rounded once more (u |ref|); fp32 accumulation and the hardware exp2 are orders of magnitude below.  `simulate(...)` plays the kernels'
arithmetic in torch (fp32 exp2 against the maximum of the first 32 keys, bf16 P, denominator of the rounded P, bf16 output) and stays near B / 2,
so 2 B leaves a factor of about 4 for what the kernels do beyond the simulation (lazy rescale, accumulation order, v_exp_f32).

`ideal(...)` is the fp64 attention of the unrounded q * scale, and  B_s[i][d] = sum_j P[i][j] expm1(2 u A[i][j]) |v[j][d] - ideal[i][d]|,
A[i][j] = scale * sum_d |q[i][d] k[j][d]|,  the first-order worst case of a relative error u on every element of Q': what the Q rounding may
cost is gated by  |out - ideal| <= 2 B + B_s  and printed per case.

Operands: `build(..., q_scale)` -- Q = hash_uniform * 8 (PEAKED: a handful of keys carry a row, the output is far from the mean of V; asserted
by `assert_peaked`) or * 1 (FLAT: the product's logits are nearer to this), K and V = hash_uniform * 1, all rounded to the tested dtype.

Layout of every tensor here: (batch, tokens, heads * hd) views of any stride, as the kernels' C ABI takes them.  A bank is
(k_bank, v_bank, rows): batch entry b also attends the keys of bank row rows[b] (None: own keys only).

Also here: the guards of tests/test_attention_hd64_gpu.py (NaN rows / columns behind the last key, the output inside a sentinel-filled buffer)."""
import torch

from mmgt_amd.synthetic import hash_uniform

U = 2.0 ** -8                      # bf16 unit roundoff (8 significand bits, round to nearest even)
LOG2E = 1.4426950408889634
PEAKED, FLAT = 8.0, 1.0            # scale of Q
SENT = 7.0
NAN = float("nan")


# ---- operands and guards -------------------------------------------------------------------------------------------------------------------

def dev():
    return torch.device("cuda:0")


def rnd(name, shape, scale=1.0, dt=torch.float32, device=None):
    return hash_uniform(name, shape, scale).to(dev() if device is None else device).to(dt)


def in_wide(name, B, n, cols, dt, ld=None, col0=0, extra_rows=64, scale=1.0, device=None):
    """A (B, n, cols) operand as a view into a NaN-filled (B, n + extra_rows, ld) allocation at column col0: the rows behind the last
    token and the neighbouring columns are NaN."""
    ld = cols if ld is None else ld
    device = dev() if device is None else device
    buf = torch.full((B, n + extra_rows, ld), NAN, device=device, dtype=dt)
    view = buf[:, :n, col0:col0 + cols]
    view.copy_(rnd(name, (B, n, cols), scale, dt, device))
    return view


def v_transposed(v, pad_cols=64):
    """(B, nk, inner) -> V^T (B, inner, nk) as a view into rows of round_up(nk, 8) + pad_cols columns, NaN behind key nk"""
    B, nk, inner = v.shape
    buf = torch.full((B, inner, (nk + 7) // 8 * 8 + pad_cols), NAN, device=v.device, dtype=v.dtype)
    buf[:, :, :nk] = v.transpose(1, 2)
    return buf[:, :, :nk]


def out_view(B, nq, cols, dt, ld=None, extra_rows=3):
    """(buffer, view): the (B, nq, cols) output block inside a sentinel-filled (B + 1, nq + extra_rows, ld) buffer"""
    ld = cols if ld is None else ld
    buf = torch.full((B + 1, nq + extra_rows, ld), SENT, device=dev(), dtype=dt)
    return buf, buf[:B, :nq, :cols]


def assert_rest_untouched(buf, view):
    """every element of `buf` outside `view` still holds the sentinel bit for bit (7.0 has one encoding)"""
    chk = buf.clone()
    chk[:view.shape[0], :view.shape[1], :view.shape[2]] = SENT
    bits = torch.int32 if buf.dtype == torch.float32 else torch.int16
    assert torch.equal(chk.view(bits), torch.full_like(chk, SENT).view(bits)), "the kernel wrote outside its output block"


def st(t):
    return (t.stride(0), 0, t.stride(1))


def st2(t):
    return (t.stride(0), t.stride(1))


# ---- references ----------------------------------------------------------------------------------------------------------------------------

def _split(t, heads, hd):
    """(B, n, heads * hd) -> (B, heads, n, hd)"""
    return t.reshape(t.shape[0], t.shape[1], heads, hd).permute(0, 2, 1, 3)


def _merge(t):
    """(B, heads, n, hd) -> (B, n, heads * hd)"""
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)


def groups(q, k, v, heads, hd, bank=None):
    """[(batch indices, Q, K, V, own keys)] with Q (b, heads, nq, hd), K / V (b, heads, own [+ bank] keys, hd) in the storage type: the batch
    entries without a bank row and those with one."""
    B = q.shape[0]
    rows = [None] * B if bank is None else list(bank[2])
    out = []
    plain = [b for b in range(B) if rows[b] is None]
    if plain:
        out.append((plain, _split(q[plain], heads, hd), _split(k[plain], heads, hd), _split(v[plain], heads, hd), k.shape[1]))
    banked = [b for b in range(B) if rows[b] is not None]
    if banked:
        r = [rows[b] for b in banked]
        kk = torch.cat([k[banked], bank[0][r]], 1)
        vv = torch.cat([v[banked], bank[1][r]], 1)
        out.append((banked, _split(q[banked], heads, hd), _split(kk, heads, hd), _split(vv, heads, hd), k.shape[1]))
    return out


def scale_log2e(scale):
    """fp32(fp32(scale) * fp32(log2 e)): attention_entry's `scale * 1.4426950408889634f` on its float argument"""
    return torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)


def q_prime(Q, scale):
    """the score MFMA's Q operand: fp32(q) * fp32(scale * log2 e), rounded to bf16 by the bf16 kernels, as it is by the fp32 ones"""
    qp = Q.float() * scale_log2e(scale).to(Q.device)
    return qp.to(torch.bfloat16) if Q.dtype == torch.bfloat16 else qp


def _attend2(Qp, K, V):
    """base-2 softmax attention in fp64 -> (ref, P, sum_j P |v|)"""
    s = torch.einsum("bhqd,bhkd->bhqk", Qp.double(), K.double())
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    return torch.einsum("bhqk,bhkd->bhqd", p, V.double()), p, torch.einsum("bhqk,bhkd->bhqd", p, V.double().abs())


class Ref:
    """ref, absv (sum_j P |v|) and bound (B) as (batch, nq, heads * hd) fp64; P: [(batch indices, (b, heads, nq, keys))]"""

    def __init__(self, shape, device):
        self.ref = torch.zeros(shape, dtype=torch.float64, device=device)
        self.absv = torch.zeros(shape, dtype=torch.float64, device=device)
        self.P = []

    @property
    def bound(self):
        return U * (self.absv + 2 * self.ref.abs())

    def n_eff(self):
        """the effective key count 1 / sum_j P^2 of every (batch, head, query)"""
        return torch.cat([(1.0 / (p * p).sum(-1)).flatten() for _, p in self.P])


def contract(q, k, v, heads, hd, scale, bank=None, mutate=None):
    """The contract reference.  `mutate(Q, K, V, own) -> (Q, K, V)` alters a group's operands (the mutant references)."""
    r = Ref(q.shape, q.device)
    for idx, Q, K, V, own in groups(q, k, v, heads, hd, bank):
        if mutate is not None:
            Q, K, V = mutate(Q, K, V, own)
        o, p, a = _attend2(q_prime(Q, scale), K, V)
        r.ref[idx], r.absv[idx] = _merge(o), _merge(a)
        r.P.append((idx, p))
    return r


def ideal(q, k, v, heads, hd, scale, bank=None):
    """(ideal, B_s): fp64 softmax attention of the unrounded q * scale, and the first-order worst case of a relative error u on every element
    of Q' = q * scale * log2 e"""
    out = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    bs = torch.zeros_like(out)
    for idx, Q, K, V, _ in groups(q, k, v, heads, hd, bank):
        Q, K, V = Q.double(), K.double(), V.double()
        p = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", Q, K) * scale, -1)
        o = torch.einsum("bhqk,bhkd->bhqd", p, V)
        w = p * torch.expm1(2 * U * scale * torch.einsum("bhqd,bhkd->bhqk", Q.abs(), K.abs()))
        s = torch.empty_like(o)
        step = max(1, (1 << 24) // max(w.numel(), 1))
        for d0 in range(0, hd, step):           # sum_j w[i][j] |v[j][d] - o[i][d]| in slices of d (the (q, k, d) tensor is not built whole)
            dv = (V[:, :, None, :, d0:d0 + step] - o[:, :, :, None, d0:d0 + step]).abs()
            s[..., d0:d0 + step] = (w[..., None] * dv).sum(-2)
        out[idx], bs[idx] = _merge(o), _merge(s)
    return out, bs


def simulate(q, k, v, heads, hd, scale, bank=None):
    """The bf16 kernels' arithmetic in torch: scores of Q' in fp32, p = exp2(s - max of the first 32 keys) in fp32, P rounded to bf16, numerator
    and denominator from the rounded P accumulated in fp32, the quotient rounded to bf16."""
    assert q.dtype == torch.bfloat16
    out = torch.empty_like(q)
    for idx, Q, K, V, _ in groups(q, k, v, heads, hd, bank):
        s = torch.einsum("bhqd,bhkd->bhqk", q_prime(Q, scale).double(), K.double()).float()
        p = torch.exp2(s - s[..., :32].amax(-1, keepdim=True)).to(torch.bfloat16).float()
        o = torch.einsum("bhqk,bhkd->bhqd", p, V.float()) / p.sum(-1, keepdim=True)
        out[idx] = _merge(o.to(torch.bfloat16))
    return out


# ---- mutant references: what a subtly wrong kernel would compute -----------------------------------------------------------------------------

def _drop_last(Q, K, V, own):
    return Q, K[:, :, :-1], V[:, :, :-1]


def _drop_last_own(Q, K, V, own):
    keep = [j for j in range(K.shape[2]) if j != own - 1]
    return Q, K[:, :, keep], V[:, :, keep]


def _swap_v(Q, K, V, own):
    j = own // 3
    V = V.clone()
    V[:, :, [j, j + 1]] = V[:, :, [j + 1, j]]
    return Q, K, V


def _k_channels(Q, K, V, own):
    j = own // 3
    K = K.clone()
    K[:, :, j, 8:16] = K[:, :, j + 1, 8:16]
    return Q, K, V


def mutants(q, k, v, heads, hd, scale, bank=None):
    """{name: fp64 mutant reference (batch, nq, heads * hd)} from the same operands.  The mutants that need a bank (a second bank row)
    exist only where the case has one; the swap / channel mutants need two keys."""
    m = {"last key dropped": contract(q, k, v, heads, hd, scale, bank, _drop_last).ref} if k.shape[1] > 1 or bank is not None else {}
    if bank is not None:
        m["last own key dropped, bank kept"] = contract(q, k, v, heads, hd, scale, bank, _drop_last_own).ref
        if bank[0].shape[0] == 2:
            other = (bank[0], bank[1], [None if r is None else 1 - r for r in bank[2]])
            m["bank of the other CFG row"] = contract(q, k, v, heads, hd, scale, other).ref
    if k.shape[1] >= 4:
        m["V rows of keys j, j + 1 swapped"] = contract(q, k, v, heads, hd, scale, bank, _swap_v).ref
        m["channels 8..15 of key j from key j + 1"] = contract(q, k, v, heads, hd, scale, bank, _k_channels).ref
    if k.shape[1] > 1 or bank is not None:
        m["scale * (1 + 2^-5)"] = contract(q, k, v, heads, hd, scale * (1 + 2.0 ** -5), bank).ref
    return m


# ---- the gate ------------------------------------------------------------------------------------------------------------------------------

def assert_peaked(r, what):
    """A peaked case really is one: the median effective key count lies in [2, 32] (at most 32 with fewer than 16 keys, where 2 cannot be
    asked: a row of f keys has n_eff <= f) and the reference's rms is at least 0.15, so a flat case cannot slip back in."""
    ne = r.n_eff().median().item()
    rms = r.ref.pow(2).mean().sqrt().item()
    keys = min(p.shape[-1] for _, p in r.P)
    print(f"{what}: median n_eff {ne:.2f} ({keys} keys), rms(ref) {rms:.3f}")
    assert (2.0 if keys >= 16 else 1.0) <= ne <= 32.0, (what, ne)
    assert rms >= 0.15, (what, rms)


def ratio(out, ref, bound):
    """|out - ref| / B per element (0 / 0 = 0: an exact zero of the reference with a zero bound must be met exactly)"""
    d = (out.double() - ref).abs()
    return torch.where(d == 0, torch.zeros_like(d), d / bound)


def check(out, r, what, dt=torch.bfloat16, ideal_ref=None, factor=2.0, out_scale=None):
    """bf16: finite and |out - ref| <= factor * B on every element; with ideal_ref = (ideal, B_s) also |out - ideal| <= factor * B + B_s.
    fp32: rtol 1e-3 / atol 1e-4 against the contract reference.  out_scale (broadcastable to out): the reference times it, B times its
    magnitude plus u |ref * out_scale| for the multiply.  Prints max and mean |d| / B and the ideal-reference figures."""
    ref, bound = r.ref, r.bound
    if out_scale is not None:
        ref = ref * out_scale
        bound = bound * out_scale.abs() + U * ref.abs()
    assert torch.isfinite(out.float()).all(), f"{what}: not finite"
    x = ratio(out, ref, bound)
    msg = f"{what}: max |d| / B {x.max().item():.3f}, mean |d| / B {x.mean().item():.3f}"
    if ideal_ref is not None:
        idl, bs = ideal_ref
        if out_scale is not None:
            idl, bs = idl * out_scale, bs * out_scale.abs()
        di, dr = out.double() - idl, ref - idl
        msg += (f"; out - ideal: max {di.abs().max().item():.3e} rms {di.pow(2).mean().sqrt().item():.3e}"
                f"; ref - ideal: max {dr.abs().max().item():.3e} rms {dr.pow(2).mean().sqrt().item():.3e}"
                f" (max |ref - ideal| / B_s {ratio(ref, idl, bs).max().item():.3f})")
    print(msg)
    if dt == torch.float32:
        torch.testing.assert_close(out.double(), ref, rtol=1e-3, atol=1e-4)
        return x.max().item()
    assert (x <= factor).all(), f"{what}: {(x > factor).sum().item()} elements beyond {factor} B, max {x.max().item():.3f} B"
    if ideal_ref is not None:
        assert ((out.double() - idl).abs() <= factor * bound + bs).all(), f"{what}: beyond {factor} B + B_s of the ideal reference"
    return x.max().item()


def old_gate_accepts(out, ref, rtol=2e-2, atol=2e-2):
    """tests/test_hip_kernels.py `tol(bf16)`, as torch.testing.assert_close applies it"""
    return bool(((out.double() - ref).abs() <= atol + rtol * ref.abs()).all())


# ---- a case: operands + cached references ---------------------------------------------------------------------------------------------------

class Case:
    """q (B, nq, heads * hd), k / v (B, nk, heads * hd) views in the tested dtype, bank = (k_bank, v_bank, rows) or None.  peaked: Q was drawn at
    8 x -- the input conditions are then asserted when the reference is first built."""

    def __init__(self, what, q, k, v, heads, hd, bank=None, peaked=True, scale=None):
        self.what, self.q, self.k, self.v, self.heads, self.hd, self.bank, self.peaked = what, q, k, v, heads, hd, bank, peaked
        self.scale = hd ** -0.5 if scale is None else scale
        self.dt = q.dtype
        self._ref = self._ideal = None

    @property
    def args(self):
        return (self.q, self.k, self.v, self.heads, self.hd, self.scale, self.bank)

    def reference(self):
        if self._ref is None:
            self._ref = contract(*self.args)
            if self.peaked:
                assert_peaked(self._ref, self.what)
        return self._ref

    def ideal(self):
        if self._ideal is None:
            self._ideal = ideal(*self.args)
        return self._ideal

    def simulate(self):
        return simulate(*self.args)

    def mutants(self):
        return mutants(*self.args)

    def check(self, out, what=None, **kw):
        return check(out, self.reference(), what or self.what, self.dt, self.ideal(), **kw)


def build(tag, hd, heads, B, nq, nk, nk2=0, rows=None, dt=torch.bfloat16, q_scale=PEAKED, device="cpu", guarded=False):
    """The case `tag`: Q = hash_uniform * q_scale, K, V (and nk2 bank keys per bank row, rows[b] = the row of batch entry b or None) =
    hash_uniform * 1, rounded to dt.  guarded: K, V and the bank sit in allocations with 64 NaN rows behind the last key.  The values depend on
    (tag, shape) alone: the CPU tests and the GPU tests of one family see the same numbers."""
    inner = heads * hd
    mk = (lambda n, b, t: in_wide(n, b, t, inner, dt, device=device)) if guarded else (lambda n, b, t: rnd(n, (b, t, inner), 1.0, dt, device))
    q = rnd(f"{tag}.q", (B, nq, inner), q_scale, dt, device)
    k, v = mk(f"{tag}.k", B, nk), mk(f"{tag}.v", B, nk)
    bank = None
    if nk2:
        nrows = max(r for r in rows if r is not None) + 1
        bank = (mk(f"{tag}.kb", nrows, nk2), mk(f"{tag}.vb", nrows, nk2), list(rows))
    kind = "peaked" if q_scale == PEAKED else "flat"
    return Case(f"{tag} hd {hd} ({nq}, {nk} + {nk2}) {kind} {str(dt)[6:]}", q, k, v, heads, hd, bank, q_scale == PEAKED)
