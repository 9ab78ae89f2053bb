"""The kernels of csrc/elementwise.hip and `mmgt_gemm_bf16_f32` (through mmgt_amd.hip) against the contracts of tests/step_gate.py: bit for bit
where the operation is exact, |out - ref| <= 2 B on every element otherwise.  The fp64 references are computed with torch on the device.  Every
operand is a view with NaN behind it, every output sits inside a sentinel-filled buffer that must come back untouched.  The shapes are the smallest
that reach the branch in question: the second sweep of the grid-stride loops (more than 8192 x 256 thread indices), the ragged channel vector, a
counter bump across two waves, every instantiation of the register softmax, the persistent GEMM walking more tiles than the device has CUs.
tests/test_step_gate.py proves on the CPU that this gate rejects subtly wrong kernels which the flat tolerances accept.  No model-level forward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import step_gate as G  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
DT = [BF16, F32]
IDS = ["bf16", "f32"]


def guard_rows(t):
    """a CONTIGUOUS view with 8 NaN rows behind it (for the entry points that take no row stride); frame indices: 8 zeros behind them (an index
    read past the end then adds to frame 0, which the bit-for-bit comparison sees, and stays inside pred_sum)"""
    buf = torch.full((t.shape[0] + 8,) + tuple(t.shape[1:]), G.NAN if t.is_floating_point() else 0, device=t.device, dtype=t.dtype)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def sentinels(shape, dt):
    return G.out_in_sentinels(tuple(shape), dt, DEV)


def gate(out, case):
    ref, B = case.reference()
    return G.check(out, ref, B, case.what)


# ---- layout ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B,C,F,H,W,cpad,scale", [(2, 316, 7, 61, 67, 320, 1.0), (2, 4, 3, 5, 7, 64, 1 / 0.18215), (1, 3, 2, 9, 9, 8, 1.0)])
def test_ncfhw_to_nhwc_bit_for_bit(B, C, F, H, W, cpad, scale, dt):
    """(2, 316, 7, 61, 67) -> 320: 2 288 720 vectors, a second sweep with a ragged end, a last channel vector of 4 + 4 zeros, HW not a power of two"""
    from mmgt_amd import hip
    c = G.ToNhwc(f"to_nhwc {(B, C, F, H, W)} -> {cpad} {dt}", guard_rows(G.rnd("gpu.to.x", (B, C, F, H, W), 2.0, device=DEV)), cpad, dt, scale)
    if C == 316:
        assert B * F * H * W * (cpad // 8) > G.SWEEP
    buf, out = sentinels((B * F, H, W, cpad), dt)
    hip.ncfhw_to_nhwc(c.x, cpad, dt, scale, out=out)
    G.assert_untouched(buf, out)
    assert torch.equal(out, c.expected())
    bits = torch.int16 if dt == BF16 else torch.int32
    assert (out[..., C:].contiguous().view(bits) == 0).all()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B,C,F,H,W,cpad,kw", [(1, 3, 3, 512, 512, 64, dict(scale=0.5, shift=0.5, clamp01=True)), (2, 4, 5, 6, 7, 64, {}), (2, 4, 5, 6, 7, 8, {})],
                         ids=["vae-out", "cpad64", "cpad8"])
def test_nhwc_to_ncfhw(B, C, F, H, W, cpad, kw, dt):
    """3 x 3 x 512 x 512: 2 359 296 elements (a second sweep), scale, shift and the clamp acting on both sides; NaN in the channels >= C"""
    from mmgt_amd import hip
    x = (G.rnd("gpu.from.x", (B * F, H, W, cpad), 1.0, device=DEV) * 3.0173).to(dt)        # (off hash_uniform's 2^-24 grid: x * 0.5 + 0.5 rounds)
    x[..., C:] = G.NAN
    c = G.FromNhwc(f"from_nhwc {(B, C, F, H, W)} <- {cpad} {dt} {kw}", guard_rows(x), B, C, **kw)
    buf, out = sentinels((B, C, F, H, W), F32)
    hip.nhwc_to_ncfhw(c.x, B, C, out=out, **kw)
    G.assert_untouched(buf, out)
    ref, _ = c.reference()
    if kw:
        assert out.numel() > G.SWEEP and (ref == 0).any() and (ref == 1).any() and ((ref > 0) & (ref < 1)).any()
    else:
        assert torch.equal(out.double(), ref)                      # x * 1 + 0 is exact
    gate(out, c)


# ---- timestep features, SiLU -------------------------------------------------------------------------------------------------------------------

def _ts(kind):
    if kind == "all":
        return torch.arange(1000, dtype=F32, device=DEV)
    if kind == "twin":
        return torch.tensor([949.0, 949.0], device=DEV)
    return 999.0 * torch.arange(6600, dtype=F32, device=DEV) / 6599


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("kind", ["all", "twin", "ramp"])
def test_timestep_features(kind, dt):
    """every integer timestep in one call; the sampler's call (two equal timesteps); 6600 x 320 = 2 112 000 elements: a second sweep"""
    from mmgt_amd import hip
    c = G.Timestep(f"timestep_features {kind} {dt}", guard_rows(_ts(kind)), 320, dt)
    if kind == "ramp":
        assert c.ts.numel() * 320 > G.SWEEP
    buf, out = sentinels((c.ts.numel(), 320), dt)
    hip.timestep_features(c.ts, 320, dt, out=out)
    G.assert_untouched(buf, out)
    gate(out, c)


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_silu(dt):
    """2 100 001 values in [-100, 100] with +-0 and the range below -88.7 where __expf(-x) overflows: a second sweep with a ragged end"""
    from mmgt_amd import hip
    x = torch.linspace(-100, 100, 2_100_001, device=DEV)
    x[7], x[8] = 0.0, -0.0
    c = G.Silu(f"silu {dt}", guard_rows(x.to(dt)))
    assert x.numel() > G.SWEEP and (c.x.double() < -89).any()
    buf, out = sentinels((x.numel(),), dt)
    hip.silu(c.x, out=out)
    G.assert_untouched(buf, out)
    gate(out, c)


# ---- CFG + DDIM ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("guidance", [3.5, 1.0])
@pytest.mark.parametrize("step", [0, 10, 19], ids=["first", "middle", "last"])
@pytest.mark.parametrize("C,F,H,W", [(4, 7, 5, 9), (4, 24, 160, 160)])
def test_cfg_ddim_step(C, F, H, W, step, guidance):
    """counter = 1 .. F (a counter read at the wrong frame shows); 4 x 24 x 160 x 160 = 2 457 600 elements: a second sweep; the first (sa_t = 0),
    a middle and the last (sa_p = 1, sb_p = 0) step pair of a 20-step schedule"""
    from mmgt_amd import hip
    c = G.cfg_case("gpu.cfg", C, F, H, W, guidance, step, device=DEV)
    buf, out = sentinels((1, C, F, H, W), F32)
    hip.cfg_ddim_step(c.ps, guard_rows(c.counter), c.lat, *c.sc, out=out)
    G.assert_untouched(buf, out)
    gate(out, c)


def test_cfg_ddim_step_refusals():
    from mmgt_amd import hip
    c = G.cfg_case("gpu.cfg.ref", 4, 7, 5, 9, 3.5, 10, device=DEV)
    ps, cnt, lat = c.ps.contiguous(), c.counter, c.lat.contiguous()
    before = hip.call_count("mmgt_cfg_ddim_step")
    with pytest.raises(RuntimeError, match="latents must be"):
        hip.cfg_ddim_step(ps, cnt, torch.cat([lat, lat]), *c.sc)
    with pytest.raises(RuntimeError, match="pred_sum must be"):
        hip.cfg_ddim_step(ps[:, :3].contiguous(), cnt, lat, *c.sc)
    with pytest.raises(RuntimeError, match="pred_sum must be"):
        hip.cfg_ddim_step(ps.double(), cnt, lat, *c.sc)
    with pytest.raises(RuntimeError, match="counter has"):
        hip.cfg_ddim_step(ps, cnt[:6].contiguous(), lat, *c.sc)
    assert hip.call_count("mmgt_cfg_ddim_step") == before            # a refused call launches nothing


# ---- window accumulation ---------------------------------------------------------------------------------------------------------------------------

def _run_window(c, k=0, ps=None, cnt=None):
    """one `accumulate_window` call for window k of the case on (ps, cnt), in place"""
    from mmgt_amd import hip
    idx = torch.tensor(c.windows[k], device=DEV, dtype=torch.int32)
    hip.accumulate_window(guard_rows(c.window_pred(k)), ps, cnt, guard_rows(idx), c.C, rows=c.rows, row0=c.row0, bump_counter=c.bump)


def _state(c):
    """pred_sum and counter of the case as guarded, writable copies"""
    return guard_rows(c.ps0.clone()), guard_rows(c.cnt0.clone())


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("cpad", [8, 64])
@pytest.mark.parametrize("rows,row0,bump", [(2, 0, True), (1, 1, False)], ids=["both-rows", "row1-no-bump"])
def test_accumulate_window_bit_for_bit(rows, row0, bump, cpad, dt):
    """Fw = 100 of F = 130 frames in a non-monotonic order: the counter bump runs across two waves; Cpad 8 and 64; prefilled sums and counters"""
    c = G.acc_case("gpu.acc", [G.shuffled(100, 130)], 130, 4, cpad, 5, 7, dt, DEV, rows=rows, row0=row0, bump=bump)
    assert sorted(c.windows[0]) != c.windows[0] and len(set(c.windows[0])) == 100
    ps, cnt = _state(c)
    _run_window(c, 0, ps, cnt)
    assert G.same_bits((ps, cnt), c.expected())
    if not bump:
        assert torch.equal(cnt, c.cnt0) and torch.equal(G.bits(ps[0]), G.bits(c.ps0[0]))


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_accumulate_window_second_sweep(dt):
    """(rows, C, Fw, hw) = (2, 4, 24, 112 x 112): 2 408 448 thread indices"""
    c = G.acc_case("gpu.acc.sweep", [list(range(24))], 24, 4, 8, 112, 112, dt, DEV)
    assert 2 * 4 * 24 * 112 * 112 > G.SWEEP
    ps, cnt = _state(c)
    _run_window(c, 0, ps, cnt)
    assert G.same_bits((ps, cnt), c.expected())


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("which", ["three", "two-hundred"])
def test_accumulate_windows_bit_for_bit_and_equal_to_sequential_calls(which, dt):
    """three windows of four over nine frames (two frames in no window: a signalling NaN and -0.0 that any rewrite would change; counts not
    uniform; 13 x 11 pixels: five x-blocks with a ragged tail) and 200 windows of two over 300 frames"""
    from mmgt_amd import hip
    if which == "three":
        c = G.acc_case("gpu.acc.win3", [[0, 1, 2, 3], [2, 3, 4, 5], [5, 6, 0, 1]], 9, 4, 8, 13, 11, dt, DEV, unwritten=(7, 8))
    else:
        c = G.acc_case("gpu.acc.win200", [[(3 * k) % 300, (3 * k + 7) % 300] for k in range(200)], 300, 4, 8, 3, 3, dt, DEV)
    ps, cnt = _state(c)
    idx = guard_rows(torch.tensor(c.windows, device=DEV, dtype=torch.int32))
    hip.accumulate_windows(c.pred, ps, cnt, idx, c.C)
    assert G.same_bits((ps, cnt), c.expected())
    ps2, cnt2 = _state(c)
    for k in range(len(c.windows)):
        _run_window(c, k, ps2, cnt2)
    assert G.same_bits((ps2, cnt2), (ps, cnt))
    if c.unwritten:
        u = list(c.unwritten)
        assert torch.equal(G.bits(ps[:, :, u]), G.bits(c.ps0[:, :, u])) and torch.equal(G.bits(cnt[u]), G.bits(c.cnt0[u]))
        assert (G.bits(ps[:, 1:, u[0]]) == G.SNAN_BITS).all() and (G.bits(ps[:, 0, u[1]]) == -2 ** 31).all()


def test_accumulate_window_refusals():
    from mmgt_amd import hip
    c = G.acc_case("gpu.acc.ref", [[0, 1, 2, 3]], 6, 4, 8, 3, 3, BF16, DEV)
    pred, idx = c.window_pred(0), torch.tensor(c.windows[0], device=DEV, dtype=torch.int32)
    ps, cnt = c.ps0.clone(), c.cnt0.clone()
    before = hip.call_count("mmgt_accumulate_window")
    with pytest.raises(RuntimeError, match="must be float32"):
        hip.accumulate_window(pred, ps.double(), cnt, idx, 4)
    with pytest.raises(RuntimeError, match="must be float32"):
        hip.accumulate_window(pred, ps, cnt.double(), idx, 4)
    with pytest.raises(RuntimeError, match="channels"):
        hip.accumulate_window(pred, ps, cnt, idx, 3)
    with pytest.raises(RuntimeError, match="counter has"):
        hip.accumulate_window(pred, ps, cnt[:5].contiguous(), idx, 4)
    assert hip.call_count("mmgt_accumulate_window") == before
    assert torch.equal(ps, c.ps0) and torch.equal(cnt, c.cnt0)


# ---- softmax ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("cols", [1, 5, 1000])
def test_softmax_rows_in_place_and_strided(cols, dt):
    """37 rows (a last workgroup of one wave) of random, flat, peaked, wide and step logits; in place on a buffer whose row stride exceeds cols, as
    vae.py:251 calls it, and out of place into a strided output"""
    from mmgt_amd import hip
    x = G.softmax_input(f"gpu.sm.{cols}", 37, cols, 0.3, dt, DEV)
    c = G.Softmax(f"softmax_rows 37 x {cols} {dt}", G.guarded(x), 0.3, dt, 1)
    buf, out = G.out_in_sentinels((37, cols), dt, DEV, ld=cols + 24, col0=8)
    hip.softmax_rows(c.x, 0.3, out=out)
    G.assert_untouched(buf, out)
    gate(out, c)
    buf, io = G.out_in_sentinels((37, cols), dt, DEV, ld=cols + 24, col0=8)
    io.copy_(x)
    hip.softmax_rows(io, 0.3, out=io)
    G.assert_untouched(buf, io)
    gate(io, c)
    assert torch.equal(io, out)


@pytest.mark.parametrize("nv", [1, 2, 3, 4, 6, 8, 12, 16, 24, 32])
def test_softmax_rows_f32_bf16_every_instantiation(nv):
    """nine rows (a last workgroup of one wave), ldx and ldo larger than cols with NaN / sentinels beside the rows; a flat row of a power-of-two width
    is 1 / cols exactly"""
    from mmgt_amd import hip
    cols, scale = 256 * nv, 0.044
    x = G.softmax_input(f"gpu.smv.{nv}", 9, cols, scale, F32, DEV)
    c = G.Softmax(f"softmax_rows_f32_bf16 9 x {cols}", G.guarded(x), scale, BF16, 4)
    assert c.x.stride(0) == cols + 8 and c.z().abs().max() > 99
    buf, out = G.out_in_sentinels((9, cols), BF16, DEV, ld=cols + 16, col0=4)
    hip.softmax_rows_f32_bf16(c.x, scale, out)
    G.assert_untouched(buf, out)
    gate(out, c)
    if nv & (nv - 1) == 0:
        assert (out[[1, 6]].double() == 1.0 / cols).all()


@pytest.mark.parametrize("cols", [1280, 8448, 100])
def test_softmax_rows_f32_bf16_refusals(cols):
    """cols / 256 = 5 has no instantiation; 8448 > 8192; 100 is no multiple of 256"""
    from mmgt_amd import hip
    x = torch.zeros((4, cols), device=DEV)
    out = torch.full((4, cols), G.SENT, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError, match="softmax_rows_f32_bf16"):
        hip.softmax_rows_f32_bf16(x, 1.0, out)
    assert (out == G.SENT).all()


# ---- the split-operand GEMM path --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,C", [(4096, 512), (5, 4)])
def test_qk_split3_bit_for_bit(rows, C):
    from mmgt_amd import hip
    c = G.Split3(f"qk_split3 {rows} x {C}", guard_rows(G.rnd("gpu.sp.qk", (rows, 4 * C), 3.0, device=DEV)), guard_rows(G.rnd("gpu.sp.bq", (C,), 1.0, device=DEV)),
                 guard_rows(G.rnd("gpu.sp.bk", (C,), 1.0, device=DEV)))
    (qbuf, Qp), (kbuf, Kp) = sentinels((rows, 3 * C), BF16), sentinels((rows, 3 * C), BF16)
    hip.qk_split3(c.qk, c.bq, c.bk, out=(Qp, Kp))
    G.assert_untouched(qbuf, Qp)
    G.assert_untouched(kbuf, Kp)
    eq, ek = c.expected()
    assert torch.equal(Qp, eq) and torch.equal(Kp, ek)
    assert torch.equal(Qp[:, :C], Qp[:, C:2 * C]) and torch.equal(Kp[:, :C], Kp[:, 2 * C:])


def _gemm_case(M, N, K, exact):
    mk = G.int_operand if exact else (lambda tag, shape, device: G.rnd(tag, shape, 1.0, BF16, device))
    a, w = mk("gpu.g.a", (M, K + 64), device=DEV), mk("gpu.g.w", (N, K + 128), device=DEV)
    a, w = G.guarded(a)[:, 64:], G.guarded(w)[:, :K]                    # strided a and w: windows of wider matrices, NaN behind and beside
    return G.GemmF32(f"gemm_bf16_f32 ({M}, {N}, {K}) {'integers' if exact else 'random'}", a, w, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["integers", "random"])
@pytest.mark.parametrize("M,N,K", [(300, 264, 192), (1, 8, 64), (4352, 4104, 1536)])
def test_gemm_bf16_f32(M, N, K, exact):
    """(4352, 4104, 1536): 17 x 17 = 289 tiles of 256 x 256 for the persistent loop -- more than the device has CUs --, a ragged last column of
    tiles, 24 K chunks; a and w are column windows of wider matrices, the output a column window of a wider buffer"""
    from mmgt_amd import hip
    c = _gemm_case(M, N, K, exact)
    assert not c.a.is_contiguous() or M == 1
    if M == 4352:
        assert 17 * 17 > torch.cuda.get_device_properties(0).multi_processor_count
    buf, out = G.out_in_sentinels((M, N), F32, DEV, ld=N + 24, col0=8)
    hip.gemm_bf16_f32(c.a, c.w, out=out)
    G.assert_untouched(buf, out)
    ref, _ = c.reference()
    if exact:
        assert torch.equal(out.double(), ref)
        assert ref.abs().max() > 16
    gate(out, c)


@pytest.mark.parametrize("gain", [1.0, 400.0])
def test_logits_chain(gain):
    """vae.py:267-275 on 1024 tokens of 512 channels: t x weight pieces -> qk_split3 -> Qp . Kp^T against the fp64 logits of the fp32 weights; gain
    400 on to_q / to_k puts the logits where real VAE weights put them.  Every stage is also held to its own contract on the operands it was
    handed (the end-to-end bound carries the worst case of the first GEMM's accumulation and is loose at C = 512: see step_gate.Logits)."""
    from mmgt_amd import hip
    c = G.logits_case("gpu.lg", 1024, 512, gain, DEV)
    w4 = c.w4()
    qk = hip.gemm_bf16_f32(c.t, w4)
    gate(qk, G.GemmF32(f"logits stage 1 gain {gain}", c.t, w4))
    Qp, Kp = hip.qk_split3(qk, c.bq, c.bk)
    eq, ek = G.Split3("", qk, c.bq, c.bk).expected()
    assert torch.equal(Qp, eq) and torch.equal(Kp, ek)
    buf, out = G.out_in_sentinels((1024, 1024), F32, DEV)
    hip.gemm_bf16_f32(Qp, Kp, out=out)
    G.assert_untouched(buf, out)
    gate(out, G.GemmF32(f"logits stage 3 gain {gain}", Qp, Kp))
    ref, _ = c.reference()
    gate(out, c)
    plain = c.mutants()["q and k rounded to bf16 (no lo pieces)"]
    assert (plain - ref).abs().max() > 20 * (out.double() - ref).abs().max()            # what the pieces buy


# ---- the tap gather behind the noise prediction ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("NB,H,W", [(2, 6, 5), (3, 19, 23)])
def test_conv_taps_gather_into_a_guarded_output(NB, H, W):
    """mm_gate's `Taps` contract on products handed over as stored (a (pixels, 36 + 4) bf16 matrix with NaN beside and behind it); (3, 19, 23):
    1311 pixels, six workgroups with a ragged last one.  Channels 4 .. 7 of the output are +0."""
    from mmgt_amd import hip
    from tests import mm_gate as M
    c = M.taps_case("gpu.taps", NB, H, W, device=DEV)
    y = M.bf16_round(c.products()).reshape(NB * H * W, 36).to(BF16)
    ybuf = torch.full((NB * H * W + 8, 40), G.NAN, device=DEV, dtype=BF16)
    ybuf[:NB * H * W, :36] = y
    buf, out = sentinels((NB, H, W, 8), BF16)
    hip.conv_taps_gather(ybuf[:NB * H * W], guard_rows(c.bias), NB, H, W, out=out)
    G.assert_untouched(buf, out)
    ref, B = c.reference()
    G.check(out[..., :4], ref, B, c.what)
    assert (out[..., 4:].contiguous().view(torch.int16) == 0).all()
