"""The bf16 attention kernels held to a derived bound on peaked inputs (tests/attn_gate.py: the arithmetic contract, the fp64 contract
reference, B = u (sum P |v| + 2 |ref|) and the gate |out - ref| <= 2 B on every element).

CPU tests (no mark): on every shape family the torch simulation of the kernels' bf16 arithmetic passes the gate and EVERY mutant reference
(a key dropped, two V rows swapped, eight K channels of the neighbouring key, the scale off by 2^-5, the other CFG row's bank) violates it
by reaching 4 B somewhere -- the standing evidence that the gate can fail; and the flat operands with the old rtol 2e-2 / atol 2e-2 gate
accept two of those mutants.

GPU tests (`gpu` mark), through mmgt_amd.hip.attention, the smallest shapes that reach each dispatch branch of launch_hd / attention_entry
(csrc/attention.hip): attn64.hip with and without the running maximum, the twin output, attn80.hip, the register-staged kernel with V^T (whole
and ragged tiles) and row-major V (64- and 32-key tiles, heads-inner order, out_scale), the one-wave forms, tattn.hip.  bf16 at 2 B on peaked
(Q = 8 x hash_uniform) and flat operands, fp32 -- where the kernel has an fp32 instantiation -- at rtol 1e-3 / atol 1e-4 on the peaked ones.
K and V lie in front of NaN rows (NaN columns for V^T), the output inside a sentinel-filled buffer.  Each case prints max and mean |d| / B
and its distance from the ideal (unrounded q * scale) reference."""
import pytest
import torch

from tests import attn_gate as G
from tests.attn_gate import FLAT, PEAKED

gpu = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
KINDS = [(BF, PEAKED), (BF, FLAT), (F32, PEAKED)]
KIND_IDS = ["bf16-peaked", "bf16-flat", "fp32-peaked"]


def bank_rows(B, first, bdiv):
    """rows[b] of attn_gate's bank triple as the kernel reads them: batch entry b >= seg2_first_batch attends bank row b // k2_bdiv"""
    return [b // bdiv if b >= first else None for b in range(B)]


# ---- CPU: the gate passes the simulated arithmetic and fails every mutant ---------------------------------------------------------------------
# (tag, hd, heads, B, nq, nk, nk2, seg2_first_batch, k2_bdiv): the GPU families below at one or two (batch, head) pairs per bank row
FAMILIES = [
    ("a64", 40, 2, 4, 256, 256, 128, 2, 2), ("a64", 40, 2, 4, 256, 256, 128, 0, 2), ("a64", 40, 2, 3, 512, 512, 0, 0, 1),
    ("a80", 80, 2, 4, 256, 256, 64, 2, 2), ("a80", 80, 2, 3, 256, 256, 0, 0, 1),
    ("vt", 40, 2, 4, 200, 200, 72, 2, 2), ("vt", 80, 2, 4, 200, 200, 72, 2, 2), ("vt", 160, 2, 4, 200, 200, 72, 2, 2),
    ("vt", 160, 2, 4, 64, 64, 64, 2, 2),
    ("rm", 40, 3, 3, 80, 77, 0, 0, 1), ("rm", 80, 3, 3, 80, 77, 0, 0, 1), ("rm", 160, 3, 3, 80, 77, 0, 0, 1),
    ("k32", 40, 24, 3, 200, 32, 0, 0, 1),
    ("w1vt", 40, 4, 4, 24, 24, 64, 2, 2), ("w1rm", 40, 4, 4, 17, 17, 32, 2, 2), ("w1vt", 80, 4, 4, 24, 24, 64, 2, 2),
    ("w1rm", 80, 4, 4, 17, 17, 32, 2, 2),
    ("h64", 64, 4, 2, 17, 17, 0, 0, 1), ("h64", 64, 4, 2, 80, 80, 0, 0, 1), ("h64", 64, 4, 2, 257, 257, 0, 0, 1),
    ("h64x", 64, 8, 3, 80, 82, 0, 0, 1),
] + [("ta", hd, 320 // hd, 10, f, f, 0, 0, 1) for hd in (40, 80, 160) for f in (1, 3, 16, 17, 24, 32)]


def family_case(fam, dt=BF, q_scale=PEAKED, device="cpu", guarded=False):
    tag, hd, heads, B, nq, nk, nk2, first, bdiv = fam
    return G.build(tag, hd, heads, B, nq, nk, nk2, bank_rows(B, first, bdiv) if nk2 else None, dt, q_scale, device, guarded)


def fam_id(f):
    return f"{f[0]}-hd{f[1]}-{f[4]}x{f[5]}+{f[6]}-first{f[7]}-B{f[3]}"


@pytest.mark.parametrize("fam", FAMILIES, ids=fam_id)
def test_simulated_bf16_arithmetic_passes_and_every_mutant_fails(fam):
    """Peaked operands (median n_eff and rms asserted when the reference is built).  The simulation stays inside 2 B (it measures <= 0.63 B);
    every mutant reaches at least 4 B on some element (measured: scale * (1 + 2^-5) is the weakest at 10 B, the others 80 B and more); the
    contract reference lies inside B_s (and inside 2 B + B_s) of the ideal one.  One frame (temporal attention of a single frame) has one key: the
    output is V, nothing can be mutated and the gate asks for V to within 3 u |v|."""
    c = family_case(fam)
    r = c.reference()
    x = G.ratio(c.simulate(), r.ref, r.bound)
    idl, bs = c.ideal()
    print(f"{c.what}: simulation max |d| / B {x.max().item():.3f} mean {x.mean().item():.3f}; ref - ideal: max "
          f"{(r.ref - idl).abs().max().item():.3e} rms {(r.ref - idl).pow(2).mean().sqrt().item():.3e}, max / B_s "
          f"{G.ratio(r.ref, idl, bs).max().item():.3f}, max / B {G.ratio(r.ref, idl, r.bound).max().item():.3f}")
    G.check(c.simulate(), r, c.what + " simulated", BF, (idl, bs))
    assert ((r.ref - idl).abs() <= bs).all()
    muts = c.mutants()
    assert len(muts) >= (4 if fam[5] >= 4 else 2 if fam[5] > 1 else 0), list(muts)
    if fam[6]:
        assert "last own key dropped, bank kept" in muts and "bank of the other CFG row" in muts
    for name, m in muts.items():
        reach = G.ratio(m, r.ref, r.bound).max().item()
        print(f"    mutant '{name}': reaches {reach:.1f} B")
        assert reach >= 4.0, (name, reach)


def test_old_gate_accepts_a_dropped_key_and_swapped_v_rows_on_flat_operands():
    """The motivation, on the operands of test_hip_kernels.py::test_attention_spatial_with_bank[...-40-256-0-bfloat16] (hash_uniform * 1: a
    nearly flat softmax over 256 keys, output rms ~ 0.04): rtol 2e-2 / atol 2e-2 against the plain fp64 reference accepts the reference with the
    last key dropped and the one with two V rows swapped -- as fp64 values and rounded to bf16 as a kernel would store them --, while the
    derived gate rejects both."""
    heads, hd, B, nq = 8, 40, 6, 256
    q, k, v = (G.rnd(n, (B, nq, heads * hd), 1.0, BF, "cpu") for n in "qkv")
    c = G.Case("flat spatial hd 40 (256, 256)", q, k, v, heads, hd, peaked=False)
    r = c.reference()
    idl, _ = c.ideal()
    print(f"rms(ref) {r.ref.pow(2).mean().sqrt().item():.4f}, median n_eff {r.n_eff().median().item():.1f}")
    muts = c.mutants()
    for name in ("last key dropped", "V rows of keys j, j + 1 swapped"):
        m = muts[name]
        reach = G.ratio(m, r.ref, r.bound).max().item()
        print(f"'{name}': max |mutant - ideal| {(m - idl).abs().max().item():.3e}, reaches {reach:.1f} B")
        assert G.old_gate_accepts(m, idl) and G.old_gate_accepts(m.to(BF), idl)
        assert reach >= 4.0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------

def launch(c, vt, first=0, bdiv=1, twin=False, out_scale=None, out_scale_heads=0, o_ld=None):
    """hip.attention on the case's operands: V (and the bank's V) transposed into NaN-padded rows if vt, the output (and the twin output) a
    view inside a sentinel buffer whose rest must stay untouched."""
    from mmgt_amd import hip
    B, nq, inner = c.q.shape
    nk = c.k.shape[1]
    v = G.v_transposed(c.v) if vt else c.v
    kw = {}
    if c.bank is not None:
        kb, vb = c.bank[0], c.bank[1]
        v2 = G.v_transposed(vb) if vt else vb
        kw = dict(k2=kb, v2=v2, k2_str=G.st2(kb), v2_str=G.st2(v2), k2_bdiv=bdiv, nk2=kb.shape[1], seg2_first_batch=first)
    if out_scale is not None:
        kw.update(out_scale=out_scale, out_scale_heads=out_scale_heads)
    buf, o = G.out_view(B, nq, inner, c.dt, ld=o_ld)
    tbuf, tw = G.out_view(B, nq, inner, c.dt, ld=o_ld) if twin else (None, None)
    if twin:
        kw.update(twin_out=tw)
    hip.attention(c.q, c.k, v, o, batch=B, heads=c.heads, hd=c.hd, nq=nq, nk=nk, scale=c.scale, q_str=G.st(c.q), k_str=G.st(c.k), v_str=G.st(v),
                  o_str=G.st(o), v_transposed=vt, **kw)
    G.assert_rest_untouched(buf, o)
    if twin:
        G.assert_rest_untouched(tbuf, tw)
        return o, tw
    return o


def tuned(settings, defaults, fn):
    """fn() under hip.tune(key, value) for every setting, the defaults restored whatever happens"""
    from mmgt_amd import hip
    try:
        for k_, v_ in settings.items():
            hip.tune(k_, v_)
        return fn()
    finally:
        for k_, v_ in defaults.items():
            hip.tune(k_, v_)


A64_DEFAULT = {"attn64": 1, "attn_nomax": 1}
A64_MODES = [{"attn64": 1, "attn_nomax": 1}, {"attn64": 1, "attn_nomax": 0}, {"attn64": 0}]


def gpu_case(tag, hd, heads, B, nq, nk, nk2, first, bdiv, dt, q_scale):
    return G.build(tag, hd, heads, B, nq, nk, nk2, bank_rows(B, first, bdiv) if nk2 else None, dt, q_scale, G.dev(), True)


@gpu
@pytest.mark.parametrize("dt,q_scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("B,heads", [(4, 2), (3, 2)])
@pytest.mark.parametrize("nq,nk2,first_half", [(256, 0, 0), (256, 128, 0), (256, 128, 1), (512, 0, 0), (512, 128, 0), (512, 128, 1)])
def test_attn64_and_its_register_staged_twin(nq, nk2, first_half, B, heads, dt, q_scale):
    """head_dim 40, V^T, whole 64-key tiles, nq % 256 == 0: attn64d_kernel<FAST> (attn_nomax 1), attn64d_kernel<!FAST> (attn_nomax 0) and, with
    attn64 0, attn_kernel<bf16, 40, 4, true, 64, false> on the same operands; 8 pairs (XCD-dealt) and 6; the bank read by every batch entry or
    by the second half.  fp32 has only the register-staged kernel."""
    first, bdiv = (B // 2 if first_half else 0), (B + 1) // 2
    c = gpu_case("a64", 40, heads, B, nq, nq, nk2, first, bdiv, dt, q_scale)
    for mode in (A64_MODES if dt == BF else A64_MODES[2:]):
        out = tuned(mode, A64_DEFAULT, lambda: launch(c, True, first, bdiv))
        c.check(out, f"{c.what} B {B} first {first} {mode}")


@gpu
@pytest.mark.parametrize("nomax", [1, 0])
def test_attn64_a_key_far_above_the_first_keys(nomax):
    """The spike of test_hip_kernels.py::test_attention_without_running_maximum_and_its_overflow_guard on the flat operands (512 queries and keys,
    256 bank keys): key 337 of batch entry 1 is 60 x query row 130, 2^(~180) above what the first 32 keys set -- attn_nomax 1 overflows, its
    guard re-runs the workgroup with the running maximum, and the re-run meets 2 B like everything else."""
    B, heads, nq, nk2 = 4, 2, 512, 256
    c = gpu_case("a64s", 40, heads, B, nq, nq, nk2, 2, 2, BF, FLAT)
    c.k[1, 64 * 5 + 17] = (c.q[1, 130].float() * 60).to(BF)
    out = tuned({"attn_nomax": nomax}, A64_DEFAULT, lambda: launch(c, True, 2, 2))
    c.check(out, f"{c.what} spiked, attn_nomax {nomax}")


@gpu
@pytest.mark.parametrize("q_scale", [PEAKED, FLAT], ids=["peaked", "flat"])
@pytest.mark.parametrize("frames", [2, 3])
def test_twin_output(frames, q_scale):
    """mmgt_attention_twin, nq 256, 128 bank keys: `out` against the contract reference over [own | bank], `twin_out` against the one over the own
    keys (the bitwise comparisons with separate launches stay in test_hip_kernels.py)."""
    heads = 8
    c = gpu_case("tw", 40, heads, frames, 256, 256, 128, 0, frames, BF, q_scale)
    own = G.Case(c.what + " own keys", c.q, c.k, c.v, heads, 40, None, q_scale == PEAKED)
    out, tw = launch(c, True, 0, frames, twin=True)
    c.check(out, c.what + " out")
    own.check(tw, c.what + " twin_out")


@gpu
@pytest.mark.parametrize("dt,q_scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("B,heads", [(4, 2), (3, 2)])
@pytest.mark.parametrize("nk2", [0, 64])
def test_attn80_and_its_register_staged_twin(nk2, B, heads, dt, q_scale):
    """head_dim 80, V^T, nq 256: attn80.hip (DMA staged, no running maximum in the fast pass) and, with attn80 0, attention.hip's
    attn_kernel<bf16, 80, 4, true, 64, false>; fp32 has only the latter."""
    first, bdiv = B // 2, (B + 1) // 2
    c = gpu_case("a80", 80, heads, B, 256, 256, nk2, first, bdiv, dt, q_scale)
    for a80 in ((1, 0) if dt == BF else (0,)):
        out = tuned({"attn80": a80}, {"attn80": 1}, lambda: launch(c, True, first, bdiv))
        c.check(out, f"{c.what} B {B} attn80 {a80}")


@gpu
@pytest.mark.parametrize("a80", [1, 0])
def test_attn80_a_key_far_above_the_first_keys(a80):
    """the overflow case of test_hip_kernels.py::test_attention_head_dim_80_dma_staged on the flat operands: key 209 of batch entry 1 is 40 x
    query row 130; the guard's re-run with the running maximum meets 2 B"""
    c = gpu_case("a80s", 80, 2, 4, 256, 256, 64, 2, 2, BF, FLAT)
    c.k[1, 64 * 3 + 17] = (c.q[1, 130].float() * 40).to(BF)
    out = tuned({"attn80": a80}, {"attn80": 1}, lambda: launch(c, True, 2, 2))
    c.check(out, f"{c.what} spiked, attn80 {a80}")


@gpu
@pytest.mark.parametrize("dt,q_scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("hd,n,nk2", [(40, 200, 72), (80, 200, 72), (160, 200, 72), (160, 64, 64)])
def test_generic_kernel_v_transposed(hd, n, nk2, dt, q_scale):
    """attn_kernel<T, hd, 4, true, 64> with ragged last tiles in both key segments (200 + 72), and <..., false> (whole tiles) at head_dim 160"""
    c = gpu_case("vt", hd, 2, 4, n, n, nk2, 2, 2, dt, q_scale)
    c.check(launch(c, True, 2, 2))


@gpu
@pytest.mark.parametrize("dt,q_scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("hd", [40, 80, 160])
def test_row_major_v_64_key_tiles(hd, dt, q_scale):
    """attn_kernel<T, hd, 4, false, 64>: 80 queries (three waves of the workgroup carry rows), 77 keys (one whole tile + 13 keys)"""
    c = gpu_case("rm", hd, 3, 3, 80, 77, 0, 0, 1, dt, q_scale)
    c.check(launch(c, False))


@gpu
@pytest.mark.parametrize("dt,q_scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "out_scale"])
@pytest.mark.parametrize("B", [3, 8])
def test_row_major_v_32_key_tiles(B, scaled, dt, q_scale):
    """attn_kernel<T, 40, 4, false, 32>, 24 heads, (200, 32): batch 3 keeps the plain workgroup order, batch 8 runs the heads-inner order
    (attn_heads_inner 1) and the plain one (0); with out_scale (three head groups, fp32 row multipliers in (0, 1), the output in rows of
    3 inner + 64 columns) the reference is multiplied, B scaled by |out_scale| plus u |ref out_scale| for the multiply."""
    heads, hd, nq = 24, 40, 200
    c = gpu_case("k32", hd, heads, B, nq, 32, 0, 0, 1, dt, q_scale)
    rs = (G.rnd("k32.rs", (3, B * nq), 0.5) + 0.5) if scaled else None
    mult = rs.double().reshape(3, B, nq).permute(1, 2, 0).repeat_interleave(8 * hd, dim=2) if scaled else None
    kw = dict(out_scale=rs, out_scale_heads=8, o_ld=heads * hd + 64) if scaled else {}
    outs = []
    for hi in ((1, 0) if B == 8 else (1,)):
        outs.append(tuned({"attn_heads_inner": hi}, {"attn_heads_inner": 1}, lambda: launch(c, False, **kw)))
        c.check(outs[-1], f"{c.what} B {B} heads_inner {hi} out_scale {scaled}", out_scale=mult)
    assert all(torch.equal(outs[0], o) for o in outs[1:])


@gpu
@pytest.mark.parametrize("dt,q_scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("hd", [40, 80])
@pytest.mark.parametrize("vt,nq,nk2", [(True, 24, 64), (False, 17, 32)])
def test_one_wave_forms(vt, nq, nk2, hd, dt, q_scale):
    """nq <= 32: attn_kernel<T, hd, 1, true, 64> on (24, 24 + 64 bank keys) and, row-major with a second segment so that tattn.hip declines,
    attn_kernel<T, hd, 1, false, 32> on (17, 17 + 32)"""
    c = gpu_case("w1vt" if vt else "w1rm", hd, 4, 4, nq, nq, nk2, 2, 2, dt, q_scale)
    c.check(launch(c, vt, 2, 2))


@gpu
@pytest.mark.parametrize("dt,q_scale", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("frames", [1, 3, 16, 17, 24, 32])
@pytest.mark.parametrize("hd,heads", [(40, 8), (40, 16), (80, 4), (80, 8), (160, 2), (160, 8)])
def test_tattn(hd, heads, frames, dt, q_scale):
    """tattn_kernel<T, hd> in the ((b f), hw, 3 C) token layout of test_hip_kernels.py::test_attention_temporal_layout, b = 2, hw = 5: one
    and several 320-column head groups per pixel, one head and two heads per wave, 1 .. 32 frames (one frame: one key, the output is V).
    The qkv tensor has a NaN (frame) row block behind it, the output lies in a sentinel buffer."""
    from mmgt_amd import hip
    b, hw = 2, 5
    C = heads * hd
    c = G.build("ta", hd, heads, b * hw, frames, frames, 0, None, dt, q_scale, G.dev())       # sequences: (pixel, frame, C)
    qkv_buf = torch.full((b * frames + 1, hw, 3 * C), G.NAN, device=G.dev(), dtype=dt)
    qkv = qkv_buf[:b * frames]
    tok = lambda t: t.reshape(b, hw, frames, C).permute(0, 2, 1, 3).reshape(b * frames, hw, C)
    qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:] = tok(c.q), tok(c.k), tok(c.v)
    buf, o = G.out_view(b * frames, hw, C, dt)
    s_in = (frames * qkv.stride(0), qkv.stride(1), qkv.stride(0))
    hip.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], o, batch=b * hw, heads=heads, hd=hd, nq=frames, nk=frames, scale=hd ** -0.5,
                  q_str=s_in, k_str=s_in, v_str=s_in, o_str=(frames * o.stride(0), o.stride(1), o.stride(0)), bdiv=hw)
    G.assert_rest_untouched(buf, o)
    c.check(o.reshape(b, frames, hw, C).permute(0, 2, 1, 3).reshape(b * hw, frames, C))
