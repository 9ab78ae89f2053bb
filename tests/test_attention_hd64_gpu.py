"""The flash-attention kernel at head_dim 64 (`launch_hd<T, 64>` in csrc/attention.hip: CLIP vision, wav2vec2, SMGA) against fp64 softmax
attention of the same storage-rounded operands, through the C ABI (mmgt_amd.hip).  head_dim 64 is the one instantiation without spare
reduction slots (the running maximum is the MFMA's initial accumulator, not folded into Q), without a spare V row (the denominator is a
per-lane sum) and with the register-batched K fragments / branch-free full-tile staging of the hd <= 80 path; tattn.hip declines it, so its
short sequences run the one-wave and 32-key forms of the generic kernel.

fp32 mode: rtol 1e-3 / atol 1e-4; bf16: 2e-2 / 2e-2 (tests/test_hip_kernels.py `tol`).  Guards on every case: K and V sit in allocations
with 64 NaN rows (columns, for V^T) behind the last key -- one key read past the end and the output is NaN --, and `out` is a view into a
sentinel-filled buffer of which nothing outside the (batch, nq, heads * 64) block may change (the guards live in tests/attn_gate.py).

The `peaked` tests run the row-major, cross-attention and packed-qkv shapes on Q = 8 x hash_uniform against the contract reference of
tests/attn_gate.py: bf16 within 2 B = 2 u (sum P |v| + 2 |ref|) on every element, fp32 at rtol 1e-3 / atol 1e-4."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attn_gate as G  # noqa: E402
from tests.attn_gate import assert_rest_untouched, dev, in_wide, out_view, rnd, st, v_transposed  # noqa: E402, F401

DT = [torch.float32, torch.bfloat16]
HD = 64


def tol(dt):
    return dict(rtol=1e-3, atol=1e-4) if dt == torch.float32 else dict(rtol=2e-2, atol=2e-2)


def _ref_attn(q, k, v, scale):
    # q (B, H, Nq, d), k/v (B, H, Nk, d) doubles
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    return torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, -1), v)


def ref_rows(q, k, v, heads):
    """(B, n, heads * 64) row-major views -> (B, nq, heads * 64) fp64"""
    sp = lambda t: t.double().reshape(t.shape[0], t.shape[1], heads, HD).permute(0, 2, 1, 3)
    o = _ref_attn(sp(q), sp(k), sp(v), HD ** -0.5)
    return o.permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[1], heads * HD)


def attn(q, k, v, o, heads, nq, nk, **kw):
    from mmgt_amd import hip
    hip.attention(q, k, v, o, batch=q.shape[0], heads=heads, hd=HD, nq=nq, nk=nk, scale=HD ** -0.5, q_str=st(q), k_str=st(k), v_str=st(v),
                  o_str=st(o), **kw)


def check(out, ref, dt, what, **gate):
    d = (out.double() - ref).abs()
    print(f"{what}: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e}")
    assert torch.isfinite(out.float()).all(), what
    torch.testing.assert_close(out.double(), ref, **(gate or tol(dt)))


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", [1, 17, 32, 33, 64, 80, 129, 257])
def test_self_attention_row_major_v(dt, n):
    """nq = nk = n: one wave with 32-key tiles (1, 17, 32: the shapes tattn.hip takes at head_dim 40 / 80 / 160), four waves with a ragged
    64-key tile (33, 80), whole tiles (64), a ragged last query block AND key tile (129), one 128-query block plus one row whose last key
    tile holds a single key (257).  Batch x heads = 15, 18, 12, 21, 16, 8, 24, 18 pairs: both the XCD-dealt (pairs % 8 == 0) and the plain
    workgroup order."""
    B, heads = 2 + n % 2, 4 + n % 5
    inner = heads * HD
    q = rnd("h64.q", (B, n, inner), 1.0, dt)
    k = in_wide("h64.k", B, n, inner, dt)
    v = in_wide("h64.v", B, n, inner, dt)
    buf, o = out_view(B, n, inner, dt)
    attn(q, k, v, o, heads, n, n)
    check(o, ref_rows(q, k, v, heads), dt, f"self n={n} {dt}")
    assert_rest_untouched(buf, o)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("n", [17, 80, 257])
def test_self_attention_row_major_v_peaked(dt, n):
    """test_self_attention_row_major_v's one-wave, ragged four-wave and 128 + 1 query shapes on peaked operands at the derived gate"""
    B, heads = 2 + n % 2, 4 + n % 5
    c = G.build("h64", HD, heads, B, n, n, 0, None, dt, G.PEAKED, dev(), guarded=True)
    buf, o = out_view(B, n, heads * HD, dt)
    attn(c.q, c.k, c.v, o, heads, n, n)
    c.check(o)
    assert_rest_untouched(buf, o)


@pytest.mark.parametrize("dt", DT)
def test_cross_attention_peaked(dt):
    """(80, 82) of test_cross_attention_unequal_lengths_and_strides, its three token strides and NaN neighbour columns, on peaked operands"""
    B, heads, nq, nk = 3, 8, 80, 82
    d = heads * HD
    q = in_wide("h64x.q", B, nq, d, dt, ld=2 * d, col0=0, extra_rows=0, scale=G.PEAKED)
    k = in_wide("h64x.k", B, nk, d, dt, ld=3 * d, col0=d)
    v = in_wide("h64x.v", B, nk, d, dt, ld=d + 8)
    c = G.Case(f"cross (80, 82) peaked {dt}", q, k, v, heads, HD)
    buf, o = out_view(B, nq, d, dt)
    attn(q, k, v, o, heads, nq, nk)
    c.check(o)
    assert_rest_untouched(buf, o)


@pytest.mark.parametrize("dt", DT)
def test_packed_qkv_peaked(dt):
    """test_packed_qkv_at_the_wav2vec_layout with the q columns of the packed tensor drawn at 8 x"""
    heads, S = 12, 149
    H = heads * HD
    qkv = in_wide("w2vp.qkv", 1, S, 3 * H, dt)
    qkv[..., :H] = rnd("w2vp.q", (1, S, H), G.PEAKED, dt)
    q, k, v = qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:]
    c = G.Case(f"packed qkv peaked {dt}", q, k, v, heads, HD)
    buf, o = out_view(1, S, H, dt)
    from mmgt_amd import hip
    hip.attention(q, k, v, o, batch=1, heads=heads, hd=HD, nq=S, nk=S, scale=HD ** -0.5, q_str=(S * 3 * H, 0, 3 * H), k_str=(S * 3 * H, 0, 3 * H),
                  v_str=(S * 3 * H, 0, 3 * H), o_str=st(o))
    c.check(o)
    assert_rest_untouched(buf, o)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("nq,nk,B", [(80, 82, 3), (17, 82, 2), (80, 24, 3), (80, 24, 8), (200, 32, 3), (200, 32, 8)])
def test_cross_attention_unequal_lengths_and_strides(dt, nq, nk, B):
    """Cross-attention as mmgt_amd/smga.py `_attn` lays it out, with three different token strides: q = columns [0, d) of a (B, nq, 2 d)
    tensor, k = columns [d, 2 d) of a (B, nk, 3 d) tensor, v alone in rows of d + 8; the other columns are NaN.  (17, 82) is the one-wave form
    with a 64-key tile.  nk <= 32 takes the 32-key tile (`short_keys`) and, with zero inner batch strides and several heads, sets
    `heads_inner`: run with mmgt_tune("attn_heads_inner") 0 and 1 -- at B = 3 the kernel's own condition (batch % 8 == 0) keeps the plain
    order, at B = 8 the heads-inner order really runs.  The order is a permutation of the grid: each result meets the gate and they are
    bitwise equal."""
    from mmgt_amd import hip
    heads = 8
    d = heads * HD
    q = in_wide("x64.q", B, nq, d, dt, ld=2 * d, col0=0, extra_rows=0)
    k = in_wide("x64.k", B, nk, d, dt, ld=3 * d, col0=d)
    v = in_wide("x64.v", B, nk, d, dt, ld=d + 8)
    assert len({q.stride(1), k.stride(1), v.stride(1)}) == 3
    ref = ref_rows(q, k, v, heads)
    outs = []
    try:
        for hi in ((0, 1) if nk <= 32 else (1,)):
            hip.tune("attn_heads_inner", hi)
            buf, o = out_view(B, nq, d, dt)
            attn(q, k, v, o, heads, nq, nk)
            check(o, ref, dt, f"cross ({nq}, {nk}) B={B} heads_inner={hi} {dt}")
            assert_rest_untouched(buf, o)
            outs.append(o)
    finally:
        hip.tune("attn_heads_inner", 1)
    assert all(torch.equal(outs[0], x) for x in outs[1:])


@pytest.mark.parametrize("dt", DT)
def test_packed_qkv_at_the_wav2vec_layout(dt):
    """mmgt_amd/wav2vec.py: one (S, 3 H) qkv tensor, batch 1, 12 heads, S = 149 tokens, strides (S * 3 H, 0, 3 H)"""
    heads, S = 12, 149
    H = heads * HD
    qkv = in_wide("w2v.qkv", 1, S, 3 * H, dt)
    q, k, v = qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:]
    buf, o = out_view(1, S, H, dt)
    from mmgt_amd import hip
    hip.attention(q, k, v, o, batch=1, heads=heads, hd=HD, nq=S, nk=S, scale=HD ** -0.5, q_str=(S * 3 * H, 0, 3 * H), k_str=(S * 3 * H, 0, 3 * H),
                  v_str=(S * 3 * H, 0, 3 * H), o_str=st(o))
    check(o, ref_rows(q, k, v, heads), dt, f"packed qkv {dt}")
    assert_rest_untouched(buf, o)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("nq,nk", [(256, 128), (200, 200)])
def test_v_transposed(dt, nq, nk):
    """V^T operand at head_dim 64 (the ABI admits it; no model passes it): whole 64-key tiles (the instantiation without the ragged-tail
    code) and a ragged case; the V^T rows carry 64 NaN columns behind key nk."""
    B, heads = 3, 4
    inner = heads * HD
    q = rnd("vt64.q", (B, nq, inner), 1.0, dt)
    k = in_wide("vt64.k", B, nk, inner, dt)
    v = rnd("vt64.v", (B, nk, inner), 1.0, dt)
    vT = v_transposed(v)
    buf, o = out_view(B, nq, inner, dt)
    attn(q, k, vT, o, heads, nq, nk, v_transposed=True)
    check(o, ref_rows(q, k, v, heads), dt, f"V^T ({nq}, {nk}) {dt}")
    assert_rest_untouched(buf, o)


@pytest.mark.parametrize("dt", DT)
def test_second_key_segment(dt):
    """[own keys | k2 / v2 of 82 keys] from batch entry 1 of 3 on (bank row b // 2), row-major V, both segments ending in a ragged tile"""
    B, heads, n, nk2 = 3, 5, 129, 82
    inner = heads * HD
    q = rnd("s2.q", (B, n, inner), 1.0, dt)
    k = in_wide("s2.k", B, n, inner, dt)
    v = in_wide("s2.v", B, n, inner, dt)
    k2 = in_wide("s2.k2", 2, nk2, inner, dt)
    v2 = in_wide("s2.v2", 2, nk2, inner, dt)
    buf, o = out_view(B, n, inner, dt)
    attn(q, k, v, o, heads, n, n, k2=k2, v2=v2, k2_str=(k2.stride(0), k2.stride(1)), v2_str=(v2.stride(0), v2.stride(1)), k2_bdiv=2, nk2=nk2,
         seg2_first_batch=1)
    refs = [ref_rows(q[:1], k[:1], v[:1], heads)]
    for b in (1, 2):
        refs.append(ref_rows(q[b:b + 1], torch.cat([k[b:b + 1], k2[b // 2][None]], 1), torch.cat([v[b:b + 1], v2[b // 2][None]], 1), heads))
    check(o, torch.cat(refs), dt, f"second segment {dt}")
    assert_rest_untouched(buf, o)


@pytest.mark.parametrize("dt", DT)
def test_scaled_rows_into_a_padded_operand(dt):
    """mmgt_attention_scaled at head_dim 64, shaped like test_hip_kernels.py::test_attention_scaled_rows_into_a_padded_operand with
    (nq, bf) = (200, 3): 24 heads in three groups of 8, 32 keys, the output rows of a group times its fp32 row multiplier, written into
    rows of 3 inner + 64 columns whose pad keeps the sentinel."""
    nq, bf, heads, nk = 200, 3, 24, 32
    k3 = heads * HD
    q3 = rnd("os.q3", (bf, nq, k3), 1.0, dt)
    kv = in_wide("os.kv", bf, nk, 2 * k3, dt)
    rs = rnd("os.rs", (3, bf * nq), 0.5) + 0.5
    buf, o = out_view(bf, nq, k3, dt, ld=k3 + 64)
    attn(q3, kv[..., :k3], kv[..., k3:], o, heads, nq, nk, out_scale=rs, out_scale_heads=8)
    ref = ref_rows(q3, kv[..., :k3], kv[..., k3:], heads).reshape(bf, nq, heads, HD)
    ref = ref * rs.double().reshape(3, bf, nq).permute(1, 2, 0).repeat_interleave(8, dim=2)[..., None]
    check(o, ref.reshape(bf, nq, k3), dt, f"out_scale {dt}")
    assert_rest_untouched(buf, o)


@pytest.mark.parametrize("dt", DT)
def test_online_softmax_rescale_branch_is_forced(dt):
    """nq = nk = 257, row-major V: keys 73 (tile 1), 201 (tile 3) and 256 (the single key of the ragged last tile) are 6 x the query rows 5,
    77 and 200 (test_hip_kernels.py's recipe), so those rows' running maximum jumps by ~20 octaves mid-sequence and the tile takes the
    rescale pass (M moves, O and the per-lane denominator are multiplied down: at head_dim 64 the denominator is NOT a row of O).  Full
    tensor against fp64; bf16 at rtol 2e-2 / atol 3e-2 as the other spiked-row tests (nearly one-hot rows: P and the output are bf16)."""
    B, heads, n = 2, 4, 257
    inner = heads * HD
    q = rnd("rs.q", (B, n, inner), 1.0, dt)
    k = in_wide("rs.k", B, n, inner, dt)
    v = in_wide("rs.v", B, n, inner, dt)
    for key, qrow in ((64 + 9, 5), (3 * 64 + 9, 77), (256, 200)):
        k[:, key] = (q[:, qrow].float() * 6).to(dt)
    buf, o = out_view(B, n, inner, dt)
    attn(q, k, v, o, heads, n, n)
    gate = dict(rtol=1e-3, atol=1e-4) if dt == torch.float32 else dict(rtol=2e-2, atol=3e-2)
    check(o, ref_rows(q, k, v, heads), dt, f"forced rescale {dt}", **gate)
    assert_rest_untouched(buf, o)


@pytest.mark.parametrize("dt", DT)
def test_run_to_run_deterministic(dt):
    """two launches on the same operands are bitwise equal (ragged query block and key tile, four waves)"""
    B, heads, n = 3, 8, 129
    inner = heads * HD
    q, k, v = rnd("det64.q", (B, n, inner), 1.0, dt), in_wide("det64.k", B, n, inner, dt), in_wide("det64.v", B, n, inner, dt)
    outs = []
    for _ in range(2):
        _, o = out_view(B, n, inner, dt)
        attn(q, k, v, o, heads, n, n)
        outs.append(o)
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


def test_unsupported_head_dim_is_refused():
    heads, n = 4, 40
    q, k, v = (rnd(f"hd48.{i}", (2, n, heads * 48), 1.0, torch.bfloat16) for i in "qkv")
    o = torch.empty_like(q)
    from mmgt_amd import hip
    with pytest.raises(RuntimeError, match="head_dim 48 unsupported"):
        hip.attention(q, k, v, o, batch=2, heads=heads, hd=48, nq=n, nk=n, scale=48 ** -0.5, q_str=st(q), k_str=st(k), v_str=st(v), o_str=st(o))
