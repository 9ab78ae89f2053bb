"""The audio-side kernels (SMGA glue: csrc/smga.hip; wav2vec2 glue: csrc/wav2vec.hip; mmgt_window_stack; LayerNorm and the GEMM at the
widths of wav2vec2 / WavLM / SMGA / CLIP) one by one through the C ABI (mmgt_amd.hip) against torch fp64 on the device, operands rounded to
the storage type first.

Gates:
  * fp32 mode: rtol 1e-3 / atol 1e-4 (tests/test_hip_kernels.py `tol`);
  * bf16 GEMM: rtol 2e-2 / atol 2e-2;
  * bf16 element-wise kernels and LayerNorm: ONE output ulp, as tests/test_step_shapes_gpu.py `check`: per element |d| <= 2^-8 |ref| + acc,
    mean |d| <= 2^-9 mean|ref| + acc -- round-to-nearest meets the first with equality at the bottom of a binade and the second with a third
    to spare, a truncating store or a second rounding misses both.  acc, the absolute error of the kernel's own fp32 arithmetic, is MEASURED
    in the test: the fp32 instantiation of the same kernel on the same (bf16-representable) inputs against the same fp64 reference, times 4,
    never above 1e-4 (`acc_from_fp32` prints each measured value);
  * pure data movement: bitwise.
The last tests of the file check the fp64 references themselves on the CPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from mmgt_amd.synthetic import hash_uniform

gpu = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
ULP = 2.0 ** -8
U32 = 2.0 ** -24
NAN = float("nan")
SENT = 7.0
GRID_CAP = 8192 * 256          # elements one trip of smga.hip's grid-stride loops covers (`grid_for`: at most 8192 workgroups of 256)


def tol(dt):
    return dict(rtol=1e-3, atol=1e-4) if dt == torch.float32 else dict(rtol=2e-2, atol=2e-2)


def dev():
    return torch.device("cuda:0")


def rnd(name, shape, scale=1.0, dt=torch.float32):
    return hash_uniform(name, shape, scale).to(dev()).to(dt)


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def check_ulp(out, ref, acc, what):
    """tests/test_step_shapes_gpu.py `check`"""
    d = (out.double() - ref).abs()
    gate = ULP * ref.abs() + acc
    worst = (d / gate).max().item()
    print(f"{what}: acc {acc:.3e}; max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e} on mean|ref| {ref.abs().mean().item():.3e}; worst d / gate {worst:.2f}")
    assert torch.isfinite(out.float()).all() and worst <= 1.0, what
    assert d.mean() <= 2.0 ** -9 * ref.abs().mean() + acc, what


def acc_from_fp32(out32, ref, what):
    """4 x the largest error of the kernel's fp32 instantiation on these (bf16-representable) inputs; the ceiling is 1e-4"""
    e = (out32.double() - ref).abs().max().item()
    print(f"{what}: fp32 instantiation max|d| {e:.3e}")
    assert e <= 1e-4, f"{what}: the fp32 arithmetic is {e:.3e} off fp64"
    return min(4.0 * e, 1e-4)


def check_both(fn, ref_fn, typed, side, dt, what):
    """fn(*typed in dt, *side) against ref_fn(the same in fp64) at the gate of dt.  `typed`: the tensors (or None) that live in the storage
    type, given in fp32 and rounded to dt here; `side`: the fp32 inputs (tables, affine vectors)."""
    cast = [None if a is None else a.to(dt) for a in typed]
    ref = ref_fn(*[None if a is None else a.double() for a in cast], *[a.double() for a in side])
    out = fn(*cast, *side)
    assert out.dtype == dt and out.shape == ref.shape
    if dt == torch.float32:
        d = (out.double() - ref).abs()
        print(f"{what}: fp32 max|d| {d.max().item():.3e}")
        assert torch.isfinite(out).all()
        torch.testing.assert_close(out.double(), ref, **tol(dt))
    else:
        out32 = fn(*[None if a is None else a.float() for a in cast], *side)
        check_ulp(out, ref, acc_from_fp32(out32, ref, what), what)
    return out


# ------------------------------------------------------------------------------------------------------------ rotary

def rotary_ref(x, cs, seq):
    """csrc/smga.hip rotary_kernel: pairs (x0, x1) -> (x0 c - x1 s, x1 c + x0 s), (c, s) = table[row % seq]"""
    rows, dim = x.shape
    t = cs.double()[torch.arange(rows, device=x.device) % seq]            # (rows, dim / 2, 2)
    x0, x1 = x.double()[:, 0::2], x.double()[:, 1::2]
    c, s = t[..., 0], t[..., 1]
    return torch.stack((x0 * c - x1 * s, x1 * c + x0 * s), dim=-1).reshape(rows, dim)


def rotary_table(seq, dim, rows):
    """angles as mmgt_amd/smga.py builds them in a table of `rows` rows: NaN behind row seq - 1 (a kernel that forgets the wrap reads NaN,
    not another allocation)"""
    freqs = 1.0 / (10000 ** (torch.arange(0, dim, 2)[: dim // 2].float() / dim))
    ang = torch.arange(seq).float()[:, None] * freqs[None]
    tab = torch.full((max(rows, seq + 3), dim // 2, 2), NAN)
    tab[:seq] = torch.stack((ang.cos(), ang.sin()), dim=-1)
    return tab.to(dev())


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("dim,seq,rows", [(64, 1, 8), (64, 82, 251), (512, 1, 8), (512, 82, 251), (1024, 82, 4100)])
def test_rotary(dt, dim, seq, rows):
    """rows = 3 seq + 5: row % seq wraps three times and ends inside a period; the table has as many rows as x, NaN behind row seq - 1.  4100 x 1024 is
    2 099 200 pairs: past the 8192-workgroup cap, the grid-stride loop takes a second trip.  An angle table of (1, 0) must return x bit for
    bit.  (fp32 instantiation's error on an MI355X: printed by the test, not yet recorded -- no GPU run of this file has been possible.)"""
    from mmgt_amd import hip
    assert rows == 3 * seq + 5 or rows * (dim // 2) > GRID_CAP
    x = rnd("rot.x", (rows, dim), 2.0)
    cs = rotary_table(seq, dim, rows)
    check_both(lambda x_, cs_: hip.rotary(x_, cs_, seq), lambda x_, cs_: rotary_ref(x_, cs_, seq), (x,), (cs,), dt, f"rotary {dim} {seq} {rows} {dt}")
    ident = torch.zeros_like(cs)
    ident[..., 0] = 1.0
    ident[seq:] = NAN
    xd = x.to(dt)
    assert same_bits(hip.rotary(xd, ident, seq), xd)


# ------------------------------------------------------------------------------------------------------------ FiLM + residual

def film_ref(x, ss, rpb, res, res2):
    rows, dim = x.shape
    s = ss.double()[torch.arange(rows, device=x.device) // rpb]
    out = (s[:, :dim] + 1.0) * x.double() + s[:, dim:2 * dim]
    for r in (res, res2):
        if r is not None:
            out = out + r.double()
    return out


def film_tables(nb, dim, slot=2, slots=5):
    """(nb, 2 dim) [scale | shift] as mmgt_amd/smga.py `film` slices it out of the fp32 GEMM output `film_all`: a column slice at a
    non-zero offset of rows of slots * 2 dim floats; every other column is NaN"""
    wide = torch.full((nb, slots * 2 * dim), NAN, device=dev())
    view = wide[:, slot * 2 * dim:(slot + 1) * 2 * dim]
    view.copy_(rnd("film.ss", (nb, 2 * dim), 0.5))
    return view


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("use_res,use_res2", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("dim,rpb,rows,nb", [(64, 1, 5, 6), (64, 80, 233, 3), (512, 1, 5, 6), (512, 80, 233, 3)])
def test_film_residual(dt, dim, rpb, rows, nb, use_res, use_res2):
    """res + res2 + (scale + 1) x + shift with the table row r // rows_per_batch; 233 rows = 3 batches of 80 less 7 (the wrapper asks for
    table rows * rows_per_batch >= rows only).  `res2` has no caller in the models: this is its only test.
    (fp32 instantiation's error on an MI355X: printed by the test, not yet recorded -- no GPU run of this file has been possible.)"""
    from mmgt_amd import hip
    x = rnd("film.x", (rows, dim), 1.0)
    res = rnd("film.r", (rows, dim), 1.0) if use_res else None
    res2 = rnd("film.r2", (rows, dim), 1.0) if use_res2 else None
    ss = film_tables(nb, dim)
    assert ss.stride(0) > 2 * dim and ss.storage_offset() > 0
    check_both(lambda x_, r_, r2_, ss_: hip.film_residual(x_, ss_, rpb, res=r_, res2=r2_), lambda x_, r_, r2_, ss_: film_ref(x_, ss_, rpb, r_, r2_),
               (x, res, res2), (ss,), dt, f"film {dim} {rpb} res={use_res} res2={use_res2} {dt}")


@gpu
@pytest.mark.parametrize("dt", DT)
def test_film_residual_above_the_grid_cap_and_identity(dt):
    """4100 x 512 = 2 099 200 elements: a second trip of the grid-stride loop, both residuals; zero scale / shift without a residual returns
    x bit for bit.  (fp32 instantiation's error on an MI355X: printed by the test, not yet recorded -- no GPU run of this file has been possible.)"""
    from mmgt_amd import hip
    rows, dim, rpb = 4100, 512, 80
    assert rows * dim > GRID_CAP
    x, res, res2 = (rnd(f"filmb.{n}", (rows, dim), 1.0) for n in ("x", "r", "r2"))
    ss = film_tables((rows + rpb - 1) // rpb, dim)
    check_both(lambda x_, r_, r2_, ss_: hip.film_residual(x_, ss_, rpb, res=r_, res2=r2_), lambda x_, r_, r2_, ss_: film_ref(x_, ss_, rpb, r_, r2_),
               (x, res, res2), (ss,), dt, f"film above the cap {dt}")
    xd = x.to(dt)
    zero = torch.zeros(((rows + rpb - 1) // rpb, 2 * dim), device=dev())
    assert same_bits(hip.film_residual(xd, zero, rpb), xd)


# ------------------------------------------------------------------------------------------------------------ token mean

@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("B,T,C", [(1, 1, 8), (3, 82, 512), (2, 1500, 1024)])
def test_mean_tokens(dt, B, T, C):
    """fp32 output for both storage types.  The values sit at 30 +- 1, so a wrong divisor or a dropped token moves the mean by 30 / T: 0.37
    at T = 82, seen by the north-star gate; 0.02 at T = 1500, which rtol 1e-3 on 30 would let through -- so the result must ALSO meet the
    worst-case bound of a length-T fp32 sum in any order, |d| <= (T + 1) 2^-24 mean_t|x| (Higham, gamma_(T-1) on the sum, one more rounding
    for the division): 2.7e-3 at T = 1500."""
    from mmgt_amd import hip
    x = (rnd("mean.x", (B, T, C), 1.0) + 30.0).to(dt)
    out = hip.mean_tokens(x)
    ref = x.double().mean(1)
    assert out.dtype == torch.float32 and out.shape == (B, C)
    d = (out.double() - ref).abs()
    bound = (T + 1) * U32 * x.double().abs().mean(1)
    print(f"mean_tokens {(B, T, C)} {dt}: max|d| {d.max().item():.3e}, bound {bound.min().item():.3e}")
    torch.testing.assert_close(out.double(), ref, rtol=1e-3, atol=1e-4)
    assert (d <= bound).all()


# ------------------------------------------------------------------------------------------------------------ SMGA's DDIM update

def ddim_coeffs(ac, time, time_next, eta=1.0):
    """(sqrt_recip, sqrt_recipm1, sqrt_next, c, sigma, last) of one DDIM pair from the cumulative alphas, in Python floats: the lines of
    oracle/smga_ref.py `ddim_sample` (diffusion.py:257-273)"""
    a = float(ac[time])
    if time_next < 0:
        return math.sqrt(1.0 / a), math.sqrt(1.0 / a - 1.0), 0.0, 0.0, 0.0, True
    an = float(ac[time_next])
    sigma = eta * math.sqrt((1 - a / an) * (1 - an) / (1 - a))
    return math.sqrt(1.0 / a), math.sqrt(1.0 / a - 1.0), math.sqrt(an), math.sqrt(1 - an - sigma ** 2), sigma, False


def ddim_ref(unc, cond, x, noise, w, recip, recipm1, a_next_sqrt, c, sigma, last):
    """the three lines of smga_ddim_kernel's comment, in the precision of the arguments"""
    x0 = (unc + (cond - unc) * w).clamp(-1.0, 1.0)
    eps = (recip * x - x0) / recipm1
    return x0 if last else x0 * a_next_sqrt + c * eps + sigma * noise


def clamp_edges():
    one = torch.tensor(1.0)
    up, down = torch.nextafter(one, torch.tensor(2.0)), torch.nextafter(one, torch.tensor(0.0))
    pos = torch.stack([one, up, down, torch.tensor(1.5), torch.tensor(50.0), torch.tensor(1e6), torch.tensor(0.0)])
    return torch.cat([pos, -pos[:-1]])             # (one zero: 0 + (-0 - 0) * 1 is +0)


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", [80 * 402, GRID_CAP + 77])
@pytest.mark.parametrize("pair", [0, 25, 49])
def test_smga_ddim_step(dt, n, pair):
    """x0 = clamp(unc + w (cond - unc)), eps = (x sqrt(1/a) - x0) / sqrt(1/a - 1), x' = x0 sqrt(a') + c eps + sigma noise, with the
    coefficients of the cosine schedule (oracle/smga_ref.py) at the first DDIM pair (999 -> 979: sqrt(1/a - 1) = 20291, the largest), a
    middle one (499 -> 479) and the last (19 -> -1, which returns x0 and takes no noise); guidance 2 on predictions of +-1.5, so about a
    sixth of the values clamp; the head of the tensor holds guided values of exactly +-1, one ulp either side, 1.5, 50, 1e6 and 0 (unc = 0,
    guidance 1 below).  The sampler state is fp32 whatever the predictions' type: north-star gate for both; n = 8192 * 256 + 77 runs the
    grid-stride loop twice."""
    from mmgt_amd import hip
    from oracle import smga_ref as R
    cfg = R.SMGAConfig()
    time, time_next = R.ddim_time_pairs(cfg)[pair]
    co = ddim_coeffs(R.cosine_alphas_cumprod(cfg.n_timestep), time, time_next, cfg.eta)
    assert co[5] == (pair == 49)
    unc, cond = rnd("ddim.u", (n,), 1.5, dt), rnd("ddim.c", (n,), 1.5, dt)
    x, noise = rnd("ddim.x", (n,), 2.0), rnd("ddim.n", (n,), 2.0)
    out = hip.smga_ddim_step(unc, cond, x, None if co[5] else noise, cfg.guidance_weight, *co)
    ref = ddim_ref(unc.double(), cond.double(), x.double(), noise.double(), cfg.guidance_weight, *co)
    d = (out.double() - ref).abs()
    print(f"ddim pair {pair} n {n} {dt}: max|d| {d.max().item():.3e}")
    assert out.dtype == torch.float32 and torch.isfinite(out).all()
    torch.testing.assert_close(out.double(), ref, rtol=1e-3, atol=1e-4)
    # the clamp edges through the whole update (guidance 1, unc = 0: the guided value is cond exactly)
    edges = clamp_edges().to(dev()).to(dt)
    m = edges.numel()
    zero = torch.zeros_like(edges)
    out = hip.smga_ddim_step(zero, edges, x[:m].contiguous(), None if co[5] else noise[:m].contiguous(), 1.0, *co)
    ref = ddim_ref(zero.double(), edges.double(), x[:m].double(), noise[:m].double(), 1.0, *co)
    torch.testing.assert_close(out.double(), ref, rtol=1e-3, atol=1e-4)
    with pytest.raises(RuntimeError, match="smga_ddim_step"):
        hip.smga_ddim_step(unc, cond, x, None, cfg.guidance_weight, *co[:5], False)           # noise = None is for the last step only


@gpu
@pytest.mark.parametrize("dt", DT)
def test_smga_ddim_last_step_is_the_clamped_prediction_bit_for_bit(dt):
    """last = 1 with guidance 1 and unc = 0 (0 + (cond - 0) * 1 is cond exactly): out == clamp(cond, -1, 1) bitwise, on random values and
    on the clamp edges: exactly +-1, one ulp inside and outside, far outside"""
    from mmgt_amd import hip
    cond = torch.cat([clamp_edges().to(dev()), rnd("ddimb.c", (80 * 402,), 1.5)]).to(dt)
    x = rnd("ddimb.x", (cond.numel(),), 2.0)
    out = hip.smga_ddim_step(torch.zeros_like(cond), cond, x, None, 1.0, 1.0008749, 0.0418402, 0.0, 0.0, 0.0, True)
    assert same_bits(out, cond.float().clamp(-1.0, 1.0))


# ------------------------------------------------------------------------------------------------------------ activations

MISH_CUT = 20.0        # common.h mish_f: x > 20 returns x


def gelu_ref(x):
    return F.gelu(x)                       # erf form


def mish_ref(x):
    return x * torch.tanh(torch.logaddexp(x, torch.zeros_like(x)))


ACT_REF = {"silu": F.silu, "gelu": gelu_ref, "mish": mish_ref}


def sweep(dt):
    """a dense grid over [-30, 30]; +-0, +-1e-30, +-20 and its neighbours (Mish's cut-over), +-88, +-100, +-1e4; for bf16 every finite
    bit pattern in [-100, 100]"""
    t20 = torch.tensor(MISH_CUT)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4])
    if dt == torch.float32:
        near = torch.stack([torch.nextafter(t20, torch.tensor(100.0)), torch.nextafter(t20, torch.tensor(0.0))])
        return torch.cat([torch.linspace(-30.0, 30.0, 60001), special, near]).to(dev())
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    every = every[torch.isfinite(every.float()) & (every.float().abs() <= 100.0)]
    assert every.numel() > 34000 and (every.float() == 20.125).any() and (every.float() == 19.875).any()      # 20 +- 1 ulp
    return torch.cat([every, torch.linspace(-30.0, 30.0, 60001).to(dt), special.to(dt)]).to(dev())


# fp32 SiLU / Mish gate as a fraction f of the north-star tolerance: |d| <= f (1e-4 + 1e-3 |ref|), never more than the whole of it.
# DERIVED, not yet measured on a GPU: __expf(x) is v_exp_f32 of the fp32 product x log2(e), so e = exp(-+x) carries (|x| + 2) 2^-24 relative.
# SiLU x / (1 + e): for x > 0 the weight e / (1 + e) <= e^-x leaves |x| e^-x 2^-24 + three roundings <= 3.4 x 2^-24 relative; for x < 0 the
# result |x| e^-|x| is small where |x| is large ((|x| + 5) |x|^2 e^-|x| 2^-24 <= 2e-7 absolute).  Mish x n / (n + 2), n = e (e + 2): the
# sensitivity 2 / (n + 2) to n's 2 (|x| + 3) 2^-24 peaks near x = 0 at under 8 x 2^-24.  Both stay below 1e-6 |ref| + 1e-7, i.e. f = 1e-3;
# the gate is 4 x that.  (A run on an MI355X prints the fraction it sees; replace this by 4 x that value.)
FP32_GATE_FRACTION = {"silu": 4e-3, "mish": 4e-3}
TAIL = -17.0           # below this gelu(x) underflows in float arithmetic: absolute gate only


def act_call(name):
    from mmgt_amd import hip
    if name == "hip.silu":
        return hip.silu
    code = {"silu": hip.ACT_SILU, "gelu": hip.ACT_GELU, "mish": hip.ACT_MISH}[name]
    return lambda x: hip.activation(x, code)


@gpu
@pytest.mark.parametrize("name", ["silu", "hip.silu", "gelu", "mish"])
def test_activation_fp32_sweep(name):
    """mmgt_activation (SiLU, erf-GELU, Mish) and mmgt_silu, fp32, against fp64 on the sweep; finite everywhere.
    GELU: |d| <= 2e-6 + 2^-22 |ref| (common.h documents |error| < 1e-6 for gelu_erf_f; the relative term is fp32 rounding of the result).
    SiLU / Mish: |d| <= f (1e-4 + 1e-3 |ref|), f = FP32_GATE_FRACTION (see there), never above 1.
    For x < -17 (where gelu(x) is below float's range) the gates lose their relative term.
    The largest fraction seen is printed."""
    kind = "silu" if name == "hip.silu" else name
    x = sweep(torch.float32)
    out = act_call(name)(x)
    ref = ACT_REF[kind](x.double())
    d = (out.double() - ref).abs()
    assert torch.isfinite(out).all()
    tail = x < TAIL
    if kind == "gelu":
        a, r = 2e-6, 2.0 ** -22
    else:
        frac = (d / (1e-4 + 1e-3 * ref.abs())).max().item()
        print(f"{name} fp32: max|d| {d.max().item():.3e}, largest fraction of the north-star gate {frac:.3e}")
        f = FP32_GATE_FRACTION[kind]
        assert f is not None and f <= 1.0
        a, r = f * 1e-4, f * 1e-3
    gate = a + torch.where(tail, torch.zeros_like(ref), r * ref.abs())
    worst = (d / gate).max().item()
    print(f"{name} fp32: max|d| {d.max().item():.3e} (tail {d[tail].max().item():.3e}); worst d / gate {worst:.3f}")
    assert worst <= 1.0


@gpu
@pytest.mark.parametrize("name", ["silu", "hip.silu", "gelu", "mish"])
def test_activation_bf16_every_value(name):
    """every finite bf16 value in [-100, 100] (and the fp32 sweep rounded to bf16): one output ulp, acc from the fp32 instantiation on the
    same values; finite everywhere; below x = -17 the gate is acc alone.  (fp32 instantiation's error on an MI355X: printed by the test, not yet recorded -- no GPU run of this file has been possible.)"""
    kind = "silu" if name == "hip.silu" else name
    x = sweep(torch.bfloat16)
    fn = act_call(name)
    out = fn(x)
    ref = ACT_REF[kind](x.double())
    acc = acc_from_fp32(fn(x.float()), ref, f"{name} bf16 sweep")
    check_ulp(out, ref, acc, f"{name} bf16 sweep")
    tail = x.float() < TAIL
    assert ((out.double() - ref).abs()[tail] <= acc).all()


@gpu
def test_activation_refuses_other_codes():
    from mmgt_amd import hip
    x = rnd("act.x", (64,), 1.0)
    for code in (hip.ACT_NONE, hip.ACT_GEGLU, hip.ACT_RELU, hip.ACT_QUICK_GELU, 7):
        with pytest.raises(RuntimeError, match="unsupported"):
            hip.activation(x, code)


# ------------------------------------------------------------------------------------------------------------ wav2vec2 glue

def channel_norm_gelu_ref(x, g, b, eps=1e-5):
    """GroupNorm(num_groups = C) over the rows of the channels-last (rows, C) tensor, then erf-GELU.  One row: F.group_norm refuses a
    single value per channel; the normalised value is 0 there, so the result is gelu(beta)."""
    rows, C = x.shape
    if rows == 1:
        return F.gelu(b.double()).expand(1, C).clone()
    return F.gelu(F.group_norm(x.double().t()[None], C, g.double(), b.double(), eps))[0].t()


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("rows,C", [(1, 8), (2, 512), (255, 512), (256, 512), (257, 512), (3071, 512)])
def test_channel_norm_gelu(dt, rows, C):
    """One workgroup of 256 threads strides the rows of its channels: fewer rows than threads, exactly 256, one more, and wav2vec2's 3071.
    rows = 1 has zero variance: gelu(beta), finite.  (fp32 instantiation's error on an MI355X: printed by the test, not yet recorded -- no GPU run of this file has been possible.)"""
    from mmgt_amd import hip
    x = rnd("cn.x", (rows, C), 2.0) + 0.5
    g, b = rnd("cn.g", (C,), 0.2) + 1.0, rnd("cn.b", (C,), 0.5)
    check_both(lambda x_, g_, b_: hip.channel_norm_gelu(x_, g_, b_, 1e-5), channel_norm_gelu_ref, (x,), (g, b), dt, f"channel_norm_gelu {rows} x {C} {dt}")


@gpu
def test_channel_norm_gelu_mean_much_larger_than_std_fp32():
    """channel means up to +-90 over unit spread (as test_layernorm_mean_much_larger_than_std_fp32): the kernel's statistics are two-pass"""
    from mmgt_amd import hip
    rows, C = 517, 512
    x = rnd("cnm.x", (rows, C), 1.0) + 30.0 * rnd("cnm.mean", (1, C), 3.0)
    g, b = rnd("cnm.g", (C,), 0.2) + 1.0, rnd("cnm.b", (C,), 0.2)
    torch.testing.assert_close(hip.channel_norm_gelu(x, g, b, 1e-5).double(), channel_norm_gelu_ref(x, g, b), rtol=1e-3, atol=1e-4)


@gpu
@pytest.mark.parametrize("dt,C", [(torch.float32, 6), (torch.bfloat16, 12)])
def test_wav2vec_glue_refuses_ragged_channel_counts(dt, C):
    from mmgt_amd import hip
    x = rnd("cnr.x", (16, C), 1.0, dt)
    with pytest.raises(RuntimeError, match="!= 0 or unaligned"):
        hip.channel_norm_gelu(x, rnd("cnr.g", (C,)), rnd("cnr.b", (C,)))
    with pytest.raises(RuntimeError, match="!= 0 or unaligned"):
        hip.lerp_rows(x, 5)


LERP_PAIRS = [(1, 5), (5, 1), (2, 2), (7, 7), (3071, 24), (149, 75), (24, 3071), (80, 81)]


def lerp_index_difference(rows_in, rows_out):
    """Largest |fp32 - fp64| source position of lerp_rows_kernel over the output rows: the kernel (as ATen's upsample_linear1d on the
    device) computes scale = (float)(rows_in - 1) / (float)(rows_out - 1) and src = scale * (float)i in fp32, the reference in fp64."""
    i = torch.arange(rows_out)
    if rows_out == 1:
        return 0.0
    scale32 = torch.tensor(float(rows_in - 1), dtype=torch.float32) / torch.tensor(float(rows_out - 1), dtype=torch.float32)
    src32 = scale32 * i.to(torch.float32)
    src64 = i.to(torch.float64) * (rows_in - 1) / (rows_out - 1)
    return (src32.double() - src64).abs().max().item()


# lerp_index_difference of LERP_PAIRS, computed on the CPU (test_lerp_index_difference_of_the_pairs pins them)
LERP_INDEX_DIFF = {(1, 5): 0.0, (5, 1): 0.0, (2, 2): 0.0, (7, 7): 0.0, (3071, 24): 1.1677e-4, (149, 75): 0.0, (24, 3071): 1.3669e-6, (80, 81): 4.5777e-6}


def lerp_ref(x, rows_out):
    return F.interpolate(x.double().t()[None], size=rows_out, mode="linear", align_corners=True)[0].t()


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("C", [8, 512])
@pytest.mark.parametrize("rows_in,rows_out", LERP_PAIRS)
def test_lerp_rows(dt, rows_in, rows_out, C):
    """F.interpolate(mode="linear", align_corners=True) along the rows.  The kernel's source position is fp32, the reference's fp64; they
    differ by at most LERP_INDEX_DIFF (1.17e-4 at 3071 -> 24, where positions reach 3070 and an fp32 ulp is 2.4e-4; 4.6e-6 at 80 -> 81;
    1.4e-6 at 24 -> 3071; exactly 0 for the other pairs), and the result is piecewise linear in the position, so the fp32 gate is
    that difference x max|x[i + 1] - x[i]| plus the rounding of w0 = 1 - w1, two products and a sum, 4 x 2^-24 max|x|.  bf16: one output
    ulp over that bound as acc.  The last output row is the last input row; rows_in == rows_out copies bit for bit."""
    from mmgt_amd import hip
    x = rnd("lerp.x", (rows_in, C), 1.0, dt)
    out = hip.lerp_rows(x, rows_out)
    ref = lerp_ref(x, rows_out)
    assert out.shape == (rows_out, C) and out.dtype == dt and torch.isfinite(out.float()).all()
    step = (x.double()[1:] - x.double()[:-1]).abs().max().item() if rows_in > 1 else 0.0
    bound = LERP_INDEX_DIFF[(rows_in, rows_out)] * step + 4 * U32 * x.double().abs().max().item()
    d = (out.double() - ref).abs()
    print(f"lerp {rows_in} -> {rows_out} x {C} {dt}: max|d| {d.max().item():.3e}, fp32 bound {bound:.3e}")
    if dt == torch.float32:
        assert d.max().item() <= bound
        assert (out[-1].double() - x[-1 if rows_out > 1 else 0].double()).abs().max().item() <= bound
    else:
        check_ulp(out, ref, bound, f"lerp {rows_in} -> {rows_out} x {C} bf16")
        check_ulp(out[-1], x[-1 if rows_out > 1 else 0].double(), bound, "lerp: last row")
    if rows_in == rows_out:
        assert same_bits(out, x)


# ------------------------------------------------------------------------------------------------------------ window stack

@gpu
@pytest.mark.parametrize("L,D,half", [(1, 8, 2), (3, 12 * 768, 2), (9, 12 * 768, 2), (5, 16, 1)])
def test_window_stack(L, D, half):
    """process_audio_emb (scripts/pose2vid.py:72-91): out[i, j] = x[clamp(i + j - half, 0, L - 1)], a copy: bitwise; L < half replicates
    the only frames there are"""
    from mmgt_amd import hip
    x = rnd("ws.x", (L, D), 1.0)
    idx = (torch.arange(L, device=dev())[:, None] + torch.arange(2 * half + 1, device=dev())[None] - half).clamp(0, L - 1)
    out = hip.window_stack(x, half)
    assert out.shape == (L, 2 * half + 1, D) and same_bits(out, x[idx])


# ------------------------------------------------------------------------------------------------------------ LayerNorm at the audio widths

LN_WIDTHS = [512, 1024]        # hip.layernorm( in wav2vec.py (512, 768), wavlm.py (512, 1024), smga.py (512), clip_vision.py (1024) less test_layernorm's 320, 640, 768, 1280


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("rows", [1, 3, 80, 4 * 6 * 5 + 3])
@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layernorm_audio_widths(dt, C, rows):
    """eps 1e-5 as every caller passes it.  (lanes per row, vectors per lane) = (16, 4) / (32, 4) at 512 / 1024 in bf16, (32, 4) / (64, 4)
    in fp32; 1 and 3 rows leave most of a workgroup's rows past the end.  (fp32 instantiation's error on an MI355X: printed by the test, not yet recorded -- no GPU run of this file has been possible.)"""
    from mmgt_amd import hip
    x = rnd("lna.x", (rows, C), 2.0) + 0.5
    g, b = rnd("lna.g", (C,), 0.2) + 1.0, rnd("lna.b", (C,), 0.2)
    check_both(lambda x_, g_, b_: hip.layernorm(x_, g_, b_, 1e-5), lambda x_, g_, b_: F.layer_norm(x_, (C,), g_, b_, 1e-5), (x,), (g, b), dt,
               f"layernorm {rows} x {C} {dt}")


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layernorm_strided_in_and_out(dt, C):
    """x and out= are column slices of wider tensors (ldx, ldo > C): x's neighbours are NaN, out's keep their sentinel"""
    from mmgt_amd import hip
    rows = 83
    xw = torch.full((rows, C + 72), NAN, device=dev(), dtype=dt)
    x = xw[:, 8:8 + C]
    x.copy_(rnd("lns.x", (rows, C), 2.0, dt) + 0.5)
    g, b = rnd("lns.g", (C,), 0.2) + 1.0, rnd("lns.b", (C,), 0.2)
    ow = torch.full((rows + 1, C + 40), SENT, device=dev(), dtype=dt)
    o = ow[:rows, 16:16 + C]
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)
    assert hip.layernorm(x, g, b, 1e-5, out=o).data_ptr() == o.data_ptr()
    if dt == torch.float32:
        torch.testing.assert_close(o.double(), ref, **tol(dt))
    else:
        o32 = hip.layernorm(x.float(), g, b, 1e-5)
        check_ulp(o, ref, acc_from_fp32(o32, ref, f"strided layernorm {C}"), f"strided layernorm {C}")
    chk = ow.clone()
    chk[:rows, 16:16 + C] = SENT
    assert same_bits(chk, torch.full_like(ow, SENT))


@gpu
@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layernorm_audio_widths_mean_much_larger_than_std_fp32(C):
    """test_hip_kernels.py::test_layernorm_mean_much_larger_than_std_fp32 at 512 and 1024 channels"""
    from mmgt_amd import hip
    rows = 517
    x = rnd("ln.x", (rows, C), 1.0) + 30.0 * rnd("ln.mean", (rows, 1), 3.0)
    g, b = rnd("g", (C,), 0.2) + 1.0, rnd("b", (C,), 0.2)
    ref = F.layer_norm(x.double(), (C,), g.double(), b.double(), 1e-5)
    torch.testing.assert_close(hip.layernorm(x, g, b).double(), ref, rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------------------------------------------------ GEMM at the audio-side shapes

def quick_gelu_ref(x):
    return x * torch.sigmoid(1.702 * x)


# (N, K, activation, residual, bias2 row group) that smga.py / wav2vec.py / wavlm.py / clip_vision.py pass to hip.gemm and no other test lists
GEMM_CASES = [
    (402, 512, "none", False, 0),        # smga final_layer: N is no multiple of 16, output rows are not 16-byte aligned
    (512, 1088, "none", False, 0),       # smga cond_projection: K = 1059 padded to 64
    (512, 448, "none", False, 82),       # smga in_face / in_body: K = 402 padded, per-batch bias rows, no bias
    (1024, 512, "none", False, 0),       # smga qk, wavlm proj
    (1024, 512, "gelu", False, 0),       # smga linear1
    (1024, 512, "mish", False, 0),       # (smga time_mlp.1 is 2048 x 512 with Mish)
    (1024, 512, "silu", False, 0),       # (smga non_attn_cond_projection.1 is 512 x 512 with SiLU)
    (1024, 512, "quick_gelu", False, 0),  # (clip fc1 is 4096 x 1024 with quick-GELU)
    (512, 1024, "none", True, 0),        # smga linear2 / encoder out-projection + residual
    (2048, 512, "mish", False, 0),       # smga time_mlp.1
    (512, 2048, "none", True, 0),        # smga to_time_cond.0 + residual
    (768, 512, "none", False, 0),        # wav2vec feature projection
    (3072, 768, "gelu", False, 0),       # wav2vec fc1
    (768, 3072, "none", True, 0),        # wav2vec fc2 + residual
    (512, 1536, "gelu", False, 0),       # wav2vec / wavlm conv layers as GEMMs over patches (kernel 3), no bias
    (4096, 1024, "quick_gelu", False, 0),  # clip fc1
]
GEMM_ACT = {"none": lambda x: x, "gelu": F.gelu, "mish": mish_ref, "silu": F.silu, "quick_gelu": quick_gelu_ref}


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M", [1, 2, 82, 160 + 4])
@pytest.mark.parametrize("N,K,act,use_res,b2_rows", GEMM_CASES)
def test_gemm_audio_side_shapes(dt, M, N, K, act, use_res, b2_rows):
    """fp64 GEMM + bias (+ per-row-group bias) + activation (+ residual), gates of test_gemm_plain_and_epilogue.  The output is the head of a
    sentinel-filled buffer one row longer: the extra row stays untouched (at N = 402 a row is 804 / 1608 bytes, no multiple of 16)."""
    from mmgt_amd import hip
    code = {"none": hip.ACT_NONE, "gelu": hip.ACT_GELU, "mish": hip.ACT_MISH, "silu": hip.ACT_SILU, "quick_gelu": hip.ACT_QUICK_GELU}[act]
    a = rnd("ag.a", (M, K), 1.0, dt)
    w = rnd("ag.w", (N, K), 1.0 / math.sqrt(K), dt)
    bias = None if b2_rows or (act == "gelu" and K == 1536) else rnd("ag.b", (N,), 0.5)
    b2 = rnd("ag.b2", ((M + b2_rows - 1) // b2_rows, N), 0.5) if b2_rows else None
    res = rnd("ag.r", (M, N), 1.0, dt) if use_res else None
    buf = torch.full((M + 1, N), SENT, device=dev(), dtype=dt)
    out = hip.gemm(a, w, bias, out=buf[:M], residual=res, bias2=b2, bias2_rows=b2_rows, act=code)
    ref = a.double() @ w.double().t()
    if bias is not None:
        ref = ref + bias.double()
    if b2 is not None:
        ref = ref + b2.double().repeat_interleave(b2_rows, 0)[:M]
    ref = GEMM_ACT[act](ref)
    if res is not None:
        ref = ref + res.double()
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), ref, **tol(dt))
    assert same_bits(buf[M:], torch.full_like(buf[M:], SENT))


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M", [2, 160 + 4])
@pytest.mark.parametrize("N,K,H", [(48, 128 * 48, 768), (64, 128 * 64, 1024)])
def test_gemm_positional_conv_group(dt, M, N, K, H):
    """One group of the positional conv embedding of wav2vec2 (16 groups of 48 channels, kernel 128) / WavLM (16 x 64): GELU(a W^T + b) +
    x[:, group] written into out[:, group], residual and output being column slices of (M, H) tensors; the other columns keep the sentinel."""
    from mmgt_amd import hip
    a = rnd("pc.a", (M, K), 1.0, dt)
    w = rnd("pc.w", (N, K), 1.0 / math.sqrt(K), dt)
    bias = rnd("pc.b", (N,), 0.5)
    x = rnd("pc.x", (M, H), 1.0, dt)
    xs = torch.full((M, H), SENT, device=dev(), dtype=dt)
    sl = slice(3 * N, 4 * N)
    hip.gemm(a, w, bias, act=hip.ACT_GELU, residual=x[:, sl], out=xs[:, sl])
    ref = F.gelu(a.double() @ w.double().t() + bias.double()) + x[:, sl].double()
    torch.testing.assert_close(xs[:, sl].double(), ref, **tol(dt))
    chk = xs.clone()
    chk[:, sl] = SENT
    assert same_bits(chk, torch.full_like(xs, SENT))


# ------------------------------------------------------------------------------------------------------------ the references themselves (CPU)

def test_lerp_index_difference_of_the_pairs():
    """the table test_lerp_rows gates with IS the fp32 / fp64 difference of the source positions, pair by pair (zero where it says zero)"""
    for pair in LERP_PAIRS:
        d = lerp_index_difference(*pair)
        want = LERP_INDEX_DIFF[pair]
        assert (d == 0.0) if want == 0.0 else (0.999 * want <= d <= want), (pair, d, want)
    # and the reference interpolates at those fp64 positions
    x = hash_uniform("lerp.cpu", (24, 8), 1.0)
    pos = torch.arange(3071, dtype=torch.float64) * 23 / 3070
    lo = pos.floor().long().clamp(max=22)
    w1 = (pos - lo)[:, None]
    torch.testing.assert_close(lerp_ref(x, 3071), x.double()[lo] * (1 - w1) + x.double()[lo + 1] * w1, rtol=0, atol=1e-14)


def test_ddim_restatement_matches_the_oracle(monkeypatch):
    """`ddim_coeffs` + `ddim_ref` against oracle/smga_ref.py `ddim_sample`, whose model call is replaced by a fixed guided prediction: the
    first DDIM step, and all 50 to the end (the last one returns the clamped prediction).  The oracle works in fp32, and at the first pair
    c^2 = 1 - a' - sigma^2 cancels to 2.5e-6 of its terms: its c = 1.6e-3 carries ~1 % of fp32 rounding, 4e-5 on x' for |eps| <= 2 -- the
    atol; everything else agrees to 1e-5."""
    from oracle import smga_ref as R
    cfg = R.SMGAConfig()
    shape = (1, 4, 6)
    pred = hash_uniform("ddim.cpu.pred", shape, 1.5)
    noises = [hash_uniform(f"ddim.cpu.n{i}", shape, 2.0) for i in range(cfg.sampling_timesteps)]
    monkeypatch.setattr(R, "guided_forward", lambda sd, cfg_, x, cf, ce, tc, w: pred)
    traj = []
    R.ddim_sample(None, cfg, None, None, noises, trajectory=traj)
    ac = R.cosine_alphas_cumprod(cfg.n_timestep)
    x = noises[0].double()
    for i, (time, time_next) in enumerate(R.ddim_time_pairs(cfg)):
        co = ddim_coeffs(ac, time, time_next, cfg.eta)
        noise = noises[1 + i].double() if not co[5] else None
        # unc = cond = the guided prediction: unc + (cond - unc) w is that prediction for any w
        x = ddim_ref(pred.double(), pred.double(), x, noise, cfg.guidance_weight, *co)
        torch.testing.assert_close(x, traj[i].double(), rtol=1e-5, atol=5e-5)
    assert torch.equal(traj[-1], pred.clamp(-1.0, 1.0))


def test_activation_references_match_torch():
    x = torch.cat([torch.linspace(-30.0, 30.0, 6001, dtype=torch.float64), torch.tensor([0.0, -0.0, 1e-30, 20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4],
                                                                                         dtype=torch.float64)])
    torch.testing.assert_close(mish_ref(x), F.mish(x), rtol=1e-12, atol=1e-300)
    erf = torch.tensor([math.erf(v / math.sqrt(2.0)) for v in x.tolist()], dtype=torch.float64)
    torch.testing.assert_close(gelu_ref(x), 0.5 * x * (1.0 + erf), rtol=1e-12, atol=1e-14)        # (1 + erf cancels in the negative tail: an ulp of erf is 3e-15 on x = -30)
    torch.testing.assert_close(quick_gelu_ref(x), x / (1.0 + torch.exp(-1.702 * x)), rtol=1e-12, atol=1e-300)
    torch.testing.assert_close(ACT_REF["silu"](x), x / (1.0 + torch.exp(-x)), rtol=1e-12, atol=1e-300)
    # one row per channel: what channel_norm_gelu_ref returns where F.group_norm refuses
    b = hash_uniform("cn.cpu.b", (8,), 0.5)
    torch.testing.assert_close(channel_norm_gelu_ref(torch.ones(1, 8), torch.ones(8), b), F.gelu(b.double())[None])
    x2 = hash_uniform("cn.cpu.x", (5, 8), 1.0)
    m, v = x2.double().mean(0), x2.double().var(0, unbiased=False)
    torch.testing.assert_close(channel_norm_gelu_ref(x2, torch.ones(8), b), F.gelu((x2.double() - m) / (v + 1e-5).sqrt() + b.double()))
