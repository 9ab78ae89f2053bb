"""The GEMM, conv and norm kernels of libmmgt_hip.so (through mmgt_amd.hip) against the contracts of tests/mm_gate.py: bf16 to |out - ref| <= 2 B on
every element, fp32 (where the kernel has an fp32 instantiation) to rtol 1e-3 / atol 1e-4 against the same contract.  The fp64 references are
computed with torch on the device.  Operands are views with NaN rows (and columns) behind them, every output sits inside a sentinel-filled buffer
that must come back untouched, every `hip.tune` is restored in a `finally`.  tests/test_mm_gate.py proves on the CPU that this gate rejects subtly
wrong kernels which the flat tolerance of tests/test_hip_kernels.py accepts.

Which branch a case reaches is read from the dispatchers (csrc/gemm_plan.h `plan_gemm`, which tests/test_gemm_plan.py checks on the CPU; csrc/gemm.hip
`epi_fast`, `gemm_entry`; csrc/norm.hip): a forced `gemm_cfg`
runs that tile unless the epilogue needs another instantiation -- cfg 16 / 17 / 19 / 20 are bf16 only and take no activation (GEGLU: cfg 16) and
fall back to cfg 9 / 12 / 12 / 1; an activation other than GEGLU, a problem that is not `fast` (N % 8, 16-byte rows, bias2_rows >= 256) runs the
FULL 128 x 128 instantiation; row scale / alpha / bias_post run its EPI = 1 form (gemm16: its POST epilogue).  The entry points do not tell the
branches apart (`hip.call_count` counts `mmgt_gemm` for all of them), so the branch is stated per test; for the norms tests/mm_gate.gn_form mirrors
the shape rules and the test asserts the form it expects."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mm_gate as G  # noqa: E402

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
DT = [BF16, F32]
ALL_CFG = (0, 1, 3, 6, 9, 12, 16, 17, 19, 20)
F32_CFG = (0, 1, 3, 6, 9, 12)               # (the gemm16 numbers run the same five tiles in fp32)


def cfgs(dt):
    return ALL_CFG if dt == BF16 else F32_CFG


def gate(out, case, what, ideal=None):
    ref, B = case.reference()
    if case.dt == BF16:
        return G.check(out, ref, B, what, ideal=ideal)
    return G.check_fp32(out, ref, what)


def forced(cfg, f):
    from mmgt_amd import hip
    try:
        hip.tune("gemm_cfg", cfg)
        return f()
    finally:
        hip.tune("gemm_cfg", 0)


# ---- linear ----------------------------------------------------------------------------------------------------------------------------------

SHAPES = [(300, 320, 192), (515, 968, 64), (260, 1280, 1280)]      # (M crossing a 256-row tile; ragged N, one-chunk K; several chunks)
EPI = {
    "none": dict(),
    "bias+res": dict(bias=True, residual=True),
    "bias+bias2+res": dict(bias=True, bias2_rows=256, residual=True),      # 256 < M: the 192-row tile of cfg 19 crosses the block inside a tile
    "post": dict(bias=True, row_scale=True, alpha=0.75, bias_post=True, residual=True),
    "silu": dict(bias=True, act="silu", wscale=2.0),
    "geglu": dict(bias=True, act="geglu", bias_scale=1.0),
}


def linear(epi, M, N, K, dt):
    return G.linear_case(f"lin.{epi}", M, N, K, dt=dt, device=DEV, guard=True, **EPI[epi])


def run_linear(c, cfg=0, ld=None, col0=0):
    """one launch of `hip.gemm` / `hip.gemm_post` on the case's operands into a sentinel-guarded output; returns the output view"""
    from mmgt_amd import hip
    from mmgt_amd.packing import pack_geglu
    ep, M, N = c.ep, c.a.shape[0], c.w.shape[0]
    w, bias, act, n_out = c.w, ep.bias, hip.ACT_NONE, N
    if ep.act == "geglu":
        w, bias = pack_geglu(c.w, ep.bias)
        act, n_out = hip.ACT_GEGLU, N // 2
    elif ep.act == "silu":
        act = hip.ACT_SILU
    buf, out = G.out_in_sentinels((M, n_out), c.dt, DEV, ld, col0)

    def f():
        if ep.bias_post is not None:
            return hip.gemm_post(c.a, w, bias, ep.row_scale, ep.alpha, ep.bias_post, ep.residual, out=out)
        return hip.gemm(c.a, w, bias, out=out, residual=ep.residual, bias2=ep.bias2, bias2_rows=ep.bias2_rows, row_scale=ep.row_scale,
                        alpha=ep.alpha, act=act)
    forced(cfg, f)
    G.assert_untouched(buf, out)
    return out


@pytest.mark.parametrize("dt", DT, ids=["bf16", "f32"])
@pytest.mark.parametrize("epi", list(EPI))
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_every_tile_configuration(M, N, K, epi, dt):
    """Forced cfg 1, 3, 6, 9, 12 (32x32 MFMA tiles, both dtypes), 16, 17, 19, 20 (gemm16, bf16; others fall back as the module docstring says)
    and the heuristic's choice.  `post` is mmgt_gemm_post on a strided A view with alpha = 0.75; GEGLU takes pack_geglu's image (N = 2 x the
    output width, a multiple of 64) and reaches its own epilogue on cfg 1, 6, 9, 16 and through the planner's fallback (cfg 3, 12 -> 1; 17, 19 -> 1;
    20 -> 1: the GEGLU and gemm16 rules of gemm_plan.h `plan_gemm`) on the others."""
    if epi == "geglu":
        N = 2 * (N // 32 * 32)
    c = linear(epi, M, N, K, dt)
    for cfg in cfgs(dt):
        gate(run_linear(c, cfg), c, f"{c.what} {epi} cfg {cfg}")


@pytest.mark.parametrize("dt", DT, ids=["bf16", "f32"])
@pytest.mark.parametrize("how", ["bias2_rows = 7", "N = 1282", "8-byte rows"])
def test_gemm_full_instantiation_three_ways(how, dt):
    """`epi_fast` (gemm.hip:810-816) is false -- bias2 blocks shorter than a tile, N % 8 != 0, output rows 8-byte but not 16-byte aligned -- so
    every cfg runs the element-wise epilogue of the FULL 128 x 128 instantiation (gemm_plan.h `plan_gemm`: T128x128_FULL; gemm.hip:667-702)."""
    esz = 2 if dt == BF16 else 4
    if how == "bias2_rows = 7":
        c, ld = G.linear_case("full.b2", 300, 320, 192, dt=dt, device=DEV, guard=True, bias=True, bias2_rows=7, residual=True), None
    elif how == "N = 1282":
        c, ld = G.linear_case("full.n", 300, 1282, 192, dt=dt, device=DEV, guard=True, bias=True, residual=True), None
    else:
        c, ld = G.linear_case("full.ld", 300, 320, 192, dt=dt, device=DEV, guard=True, bias=True, residual=True), 320 + 8 // esz
        assert (ld * esz) % 16 == 8
    for cfg in (0, 1, 16):
        gate(run_linear(c, cfg, ld=ld), c, f"{c.what} FULL ({how}) cfg {cfg}")


@pytest.mark.parametrize("dt", DT, ids=["bf16", "f32"])
@pytest.mark.parametrize("M,N,K,act", [(1, 1280, 320, "silu"), (1, 1282, 320, "none"), (1, 1280, 1280, "none"), (2, 1282, 320, "none"), (4, 640, 64, "silu")])
def test_gemm_of_a_few_rows(M, N, K, act, dt):
    """M = 1 without bias2 / scale / residual runs gemv_kernel (gemm.hip:966), M = 2 and 4 stay on the tiles (SiLU, N % 8 != 0: FULL)."""
    c = G.linear_case("few", M, N, K, dt=dt, device=DEV, guard=True, bias=True, act=act, wscale=2.0 if act == "silu" else 1.0)
    gate(run_linear(c), c, f"{c.what} {act}")


@pytest.mark.parametrize("K,split", [(2560, True), (2496, False)])
def test_gemm_either_side_of_the_split_k_condition(K, split):
    """gemm_plan.h `plan_gemm` / `splitk_slices`: bf16, plain vectorised epilogue, K >= 2560, N % 256 == 0; one tile, K / 64 = 40 chunks -> S = 2 slices of 20 >= 16
    chunks; K = 2496 is below the condition and runs one launch.  As tests/test_step_shapes_gpu.py does, the `splitk` switch tells the two apart:
    with it off the split shape runs the unsplit kernel, whose result it must match to the gate, and the plain shape must not change at all."""
    from mmgt_amd import hip
    c = G.linear_case("splitk", 64, 256, K, dt=BF16, device=DEV, guard=True, bias=True, residual=True)
    try:
        hip.tune("splitk", 1)
        on = run_linear(c).clone()
        hip.tune("splitk", 0)
        off = run_linear(c).clone()
    finally:
        hip.tune("splitk", 1)
    gate(on, c, f"{c.what} splitk on")
    gate(off, c, f"{c.what} splitk off")
    if not split:
        assert torch.equal(on, off)


@pytest.mark.parametrize("dt", DT, ids=["bf16", "f32"])
def test_gemm_batched(dt):
    """grid.z = batch (gemm.hip `bz`): the V^T projection w . x[b]^T into rows of 104 columns for 100 tokens (the four columns behind them keep
    their sentinel) and dense 3-D operands; no epilogue: LINEAR with acc alone, per batch entry"""
    from mmgt_amd import hip
    B, ntok, C, inner = 3, 100, 320, 320
    x, w = G.guarded(G.rnd("bat.x", (B, ntok, C), 1.0, dt, DEV)), G.guarded(G.rnd("bat.w", (inner, C), C ** -0.5, dt, DEV), cols=0)
    out = torch.full((B, inner, 104), G.SENT, device=DEV, dtype=dt)
    hip.gemm_batched_wx(w, x, out=out)
    assert (out[:, :, ntok:] == G.SENT).all()
    w3 = G.guarded(G.rnd("bat.w3", (B, 200, C), C ** -0.5, dt, DEV))
    out3 = torch.full((B + 1, ntok, 200), G.SENT, device=DEV, dtype=dt)
    hip.gemm_batched(x, w3, out=out3[:B])
    assert (out3[B] == G.SENT).all()
    for b in range(B):
        c = G.Linear(f"batched w.x^T [{b}] {str(dt)[6:]}", w, x[b], G.Epi())
        gate(out[b, :, :ntok], c, c.what)
        c = G.Linear(f"batched a.w^T [{b}] {str(dt)[6:]}", x[b], w3[b], G.Epi())
        gate(out3[b], c, c.what)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("rows,c0,c1,cout", [(777, 64, 128, 256), (3072, 1280, 1280, 1280)])
def test_conv1x1_over_two_sources(rows, c0, c1, cout, res):
    """mmgt_conv1x1_cat_nhwc (gemm16's conv gather over two sources with one tap; 3072 x 2560: the split-K size); LINEAR over [x0 | x1]"""
    from mmgt_amd import hip
    K = c0 + c1
    x0, x1 = G.guarded(G.rnd("cat.x0", (rows, c0), 1.0, BF16, DEV), cols=0), G.guarded(G.rnd("cat.x1", (rows, c1), 1.0, BF16, DEV), cols=0)
    w = G.rnd("cat.w", (cout, K), K ** -0.5, BF16, DEV)
    r = G.guarded(G.rnd("cat.r", (rows, cout), 1.0, BF16, DEV), cols=0) if res else None
    c = G.Linear(f"conv1x1_cat {rows} x ({c0} | {c1}) -> {cout}", torch.cat([x0, x1], 1), w, G.Epi(bias=G.rnd("cat.b", (cout,), 0.5, device=DEV), residual=r))
    buf, out = G.out_in_sentinels((rows, cout), BF16, DEV)
    hip.conv1x1_cat(x0, x1, w, c.ep.bias, residual=r, out=out)
    G.assert_untouched(buf, out)
    gate(out, c, c.what + (" + residual" if res else ""))


def test_ff2_and_proj_out_folded_into_one_gemm():
    """The `ffpo` form (unet3d `_ffpo_weights`): proj_out(hid + b2 + W2 g) + x as one two-source GEMM with the host-multiplied weight
    [W_po W2 | W_po].  Contract on the packed bf16 weights; the unfolded fp64 function is held to 2 B + B_w."""
    from mmgt_amd import hip
    rows, C, inner = 520, 640, 2560
    g, hid, xres = (G.guarded(G.rnd(f"fp.{n}", (rows, k), 1.0, BF16, DEV), cols=0) for n, k in (("g", inner), ("h", C), ("x", C)))
    w2, b2 = G.rnd("fp.w2", (C, inner), inner ** -0.5, BF16, DEV), G.rnd("fp.b2", (C,), 0.3, device=DEV)
    wpo, bpo = G.rnd("fp.wpo", (C, C), C ** -0.5, BF16, DEV), G.rnd("fp.bpo", (C,), 0.3, device=DEV)
    wpf = wpo.float()
    wcat = torch.cat([wpf @ w2.float(), wpf], 1).to(BF16).contiguous()
    bcat = (bpo + wpf @ b2).contiguous()
    c = G.Linear(f"ffpo {rows} x ({inner} | {C}) -> {C}", torch.cat([g, hid], 1), wcat, G.Epi(bias=bcat, residual=xres))
    ideal = (hid.double() + b2.double() + g.double() @ w2.double().t()) @ wpo.double().t() + bpo.double() + xres.double()
    buf, out = G.out_in_sentinels((rows, C), BF16, DEV)
    hip.conv1x1_cat(g, hid, wcat, bcat, residual=xres, out=out)
    G.assert_untouched(buf, out)
    gate(out, c, c.what, ideal=(ideal, G.U * c.absacc))


# ---- conv ------------------------------------------------------------------------------------------------------------------------------------

def run_conv(c, cfg=0):
    from mmgt_amd import hip
    from mmgt_amd.packing import pack_conv3x3
    ref, _ = c.reference()
    buf, out = G.out_in_sentinels(tuple(ref.shape), c.dt, DEV)
    wp = c.wf if c.up2 else pack_conv3x3(c.w)
    res = None if c.ep.residual is None else c.ep.residual.view(ref.shape)
    forced(cfg, lambda: hip.conv3x3(c.x0, wp, c.ep.bias, stride=abs(c.stride), upsample=c.upsample, bias2=c.ep.bias2, bias2_rows=c.ep.bias2_rows,
                                    residual=res, x1=c.x1, out=out, pad_high_only=c.stride == -2))
    G.assert_untouched(buf, out)
    return out


CONV_CFG = (0, 1, 3, 12, 16, 17)
MODES = {"s1": dict(), "s2": dict(stride=2), "hi": dict(stride=-2), "up": dict(upsample=True), "up2": dict(upsample=2)}


# (the four-phase form is bf16 with one source; a 1 x 1 image has no output pixel with padding behind only)
CONV_CASES = [(c0, c1, cout, H, W, mode, dt) for c0, c1, cout in [(64, 0, 320), (320, 128, 320), (640, 0, 640)] for H, W in [(5, 7), (8, 8), (1, 1)]
              for mode in MODES for dt in DT if not (mode == "up2" and (dt == F32 or c1)) and not (mode == "hi" and H == 1)]


@pytest.mark.parametrize("c0,c1,cout,H,W,mode,dt", CONV_CASES, ids=[f"{c[0]}+{c[1]}-{c[2]}-{c[3]}x{c[4]}-{c[5]}-{str(c[6])[6:]}" for c in CONV_CASES])
def test_conv3x3_gather_modes(c0, c1, cout, H, W, mode, dt):
    """mmgt_conv3x3_nhwc: stride 1, 2, -2 (zero padding behind the last row / column only), the 3 x 3 conv on the nearest-2x view (`up`) and
    its four-phase form (`up2`: bf16, one source, gemm16 only -- gemm_plan.h `plan_gemm` sends every other cfg there), one and two sources (the seam inside a
    64-channel chunk run: 320 | 128), 8 images (280 / 512 / 8 output rows before striding: more than one row tile at 5 x 7 and 8 x 8), forced
    cfg 1, 3, 12, 16, 17 (fp32: 16 / 17 fall back to 9 / 12) and the heuristic's."""
    c = G.conv_case(f"cv.{mode}", 8, H, W, c0, cout, c1, dt=dt, device=DEV, guard=True, **MODES[mode])
    for cfg in CONV_CFG:
        out = run_conv(c, cfg)
        gate(out, c, f"{c.what} cfg {cfg}", ideal=c.ideal() if c.up2 else None)


@pytest.mark.parametrize("dt", DT, ids=["bf16", "f32"])
@pytest.mark.parametrize("b2rows", [256, 64])
def test_conv3x3_bias2_and_residual_on_both_epilogues(b2rows, dt):
    """bias2 + residual on the conv path: bias2_rows = 256 (four 8 x 8 images per row) keeps `epi_fast` and runs the vectorised epilogue of
    every tile, 64 (one image per row) is below a tile's rows and runs the FULL instantiation (gemm.hip:813; gemm_plan.h `plan_gemm`)."""
    c = G.conv_case("cv.b2", 8, 8, 8, 64, 320, dt=dt, device=DEV, guard=True, bias2_rows=b2rows, residual=True)
    for cfg in CONV_CFG:
        gate(run_conv(c, cfg), c, f"{c.what} bias2_rows {b2rows} cfg {cfg}")


def test_conv_out_as_gemm_over_the_taps_and_gather():
    """rowgemm320 over all nine taps (36 of 64 columns) + mmgt_conv_taps_gather at (2, 16, 8): the nine bf16 products are part of the contract"""
    from mmgt_amd import hip
    from mmgt_amd.packing import pack_conv_taps
    c = G.taps_case("taps", 2, 16, 8, device=DEV, guard=True)
    y, _ = hip.rowgemm320(c.x.view(-1, 320), pack_conv_taps(c.w), 64)
    out = hip.conv_taps_gather(y, c.bias, 2, 16, 8)
    assert (out[..., 4:] == 0).all()
    ref, B = c.reference()
    G.check(out[..., :4], ref, B, c.what)


# ---- norms -----------------------------------------------------------------------------------------------------------------------------------

GN_CASES = [   # tag, NB, HW, c0, c1, silu, slab switch, the form expected (bf16, fp32)
    ("gn.slab", 3, 64, 320, 0, True, True, ("slab", "slab")),
    ("gn.hw1", 3, 1, 1280, 0, True, True, ("slab", "slab")),
    ("gn.slab.two", 2, 16, 1280, 640, True, True, ("slab", "slab")),
    ("gn.slab1024", 2, 1000, 1920, 0, False, True, ("slab1024", "slab1024")),
    ("gn.slab1024.two", 2, 1000, 1280, 640, True, True, ("slab1024", "slab1024")),
    ("gn.small", 2, 37, 320, 0, False, False, ("small", "small")),
    ("gn.small.two", 2, 16, 1280, 640, True, False, ("small", "small")),
    ("gn.narrow", 1, 16448, 128, 0, True, True, ("narrow", "narrow")),
    ("gn.general", 1, 4100, 320, 0, False, True, ("general", "general")),
    ("gn.general.two", 1, 1100, 1280, 640, True, True, ("general", "general")),
]


@pytest.mark.parametrize("dt", DT, ids=["bf16", "f32"])
@pytest.mark.parametrize("tag,NB,HW,c0,c1,silu,slab,forms", GN_CASES, ids=[c[0] for c in GN_CASES])
def test_groupnorm_every_dispatch_form(tag, NB, HW, c0, c1, silu, slab, forms, dt):
    """mmgt_groupnorm_nhwc and mmgt_groupnorm_affine2 (norm.hip:752-902) on the slab in registers (256 and 1024 threads), the small-image kernel
    (its shapes all fit a slab: reached with the `gn_slab` switch off), the narrow and the general two-pass kernels; one source, and two sources
    whose groups of 60 channels straddle the seam (1280 | 640) on every form that takes two; HW = 1 and ragged HW (37, 1000, 1100, 4100).  The form
    is asserted from tests/mm_gate.gn_form, the mirror of the shape rules."""
    from mmgt_amd import hip
    c = G.gn_case(tag, NB, HW, c0, c1, silu=silu, dt=dt, device=DEV, slab=slab, guard=True)
    t = G.gn_case(tag, NB, HW, c0, c1, dt=dt, device=DEV, slab=slab, guard=True, tables=True)
    assert c.form == forms[0 if dt == BF16 else 1], c.form
    buf, out = G.out_in_sentinels((NB, HW, c0 + c1), dt, DEV)
    try:
        hip.tune("gn_slab", int(slab))
        n0 = hip.call_count("mmgt_groupnorm_nhwc")
        hip.groupnorm(c.x0, c.gamma, c.beta, 32, c.eps, silu=silu, x1=c.x1, out=out)
        assert hip.call_count("mmgt_groupnorm_nhwc") == n0 + 1
        sc, sh = hip.groupnorm_affine(t.x0, t.gamma, t.beta, 32, t.eps, x1=t.x1)
    finally:
        hip.tune("gn_slab", 1)
    G.assert_untouched(buf, out)
    ref, B, S, cap = c.reference()
    assert (S < cap).all()
    if dt == BF16:
        G.norm_check(out, c)
    else:
        G.check_fp32(out, ref, c.what)
    (rsc, rsh), (bsc, bsh), _, _ = t.reference()
    G.check(sc, rsc, bsc, t.what + " scale")
    G.check(sh, rsh, bsh, t.what + " shift")


@pytest.mark.parametrize("dt", DT, ids=["bf16", "f32"])
@pytest.mark.parametrize("C", [320, 640, 768, 1280])
def test_layernorm(C, dt):
    """mmgt_layernorm (norm.hip:909-934): 123 rows (no multiple of the 4 .. 32 rows of a workgroup), plain, with `pe`, with the folded
    (pe_mod, C) beta table, strided input and strided output"""
    from mmgt_amd import hip
    rows = 123
    assert rows % G.ln_depth(C, 8 if dt == BF16 else 4)[1]
    for kw in (dict(), dict(pe_div=5, pe_mod=6), dict(pe_div=5, pe_mod=6, folded=True)):
        c = G.ln_case("ln", rows, C, dt=dt, device=DEV, ldx=C + 16, guard=True, **kw)
        buf, out = G.out_in_sentinels((rows, C), dt, DEV, ld=C + 24, col0=8)
        hip.layernorm(c.x0, c.gamma, c.beta, c.eps, pe=c.pe, pe_div=c.pe_div, pe_mod=c.pe_mod, out=out)
        G.assert_untouched(buf, out)
        if dt == BF16:
            G.norm_check(out, c)
        else:
            G.check_fp32(out, c.reference()[0], c.what)


# ---- exact integers on the 32x32-MFMA tiles ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DT, ids=["bf16", "f32"])
@pytest.mark.parametrize("cfg", [1, 3, 6, 9, 12])
def test_gemm32_tiles_exact_integers(cfg, dt):
    """The tiles of gemm.hip (the ones the fp32 parity mode runs on; their bias travels as a head + tail through the MFMA), as
    test_gemm16_core_exact_integers_and_geglu does for gemm16: an asymmetric W, a row-dependent column of A, ragged M and N, integer bias and
    residual -- every product and sum is exact, so any row / column / k mix-up in the fragment maps, the quad transposes of the epilogue or the
    bias step shows as a wrong integer -- and one conv with sparse -1 / 0 / 1 operands on a 7 x 9 image."""
    from mmgt_amd import hip
    from mmgt_amd.packing import pack_conv3x3
    gen = torch.Generator(device=DEV).manual_seed(100 + cfg)
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=gen, device=DEV).float()

    def runs():
        for M, N, K in [(256, 256, 64), (300, 264, 128), (1000, 320, 192), (515, 968, 64)]:
            a, w = ri((M, K), -1, 1).to(dt), ri((N, K), -1, 1).to(dt)
            w[:, 0] = (torch.arange(N, device=DEV) % 5 - 2).to(dt)
            a[:, 1] = (torch.arange(M, device=DEV) % 7 - 3).to(dt)
            bias, res = ri((N,), -3, 3), ri((M, N), -3, 3).to(dt)
            for b, r in ((None, None), (bias, res)):
                ref = a.double() @ w.double().t() + (0 if b is None else b.double() + r.double())
                assert ref.abs().max() < 256
                buf, out = G.out_in_sentinels((M, N), dt, DEV)
                hip.gemm(a, w, b, residual=r, out=out)
                G.assert_untouched(buf, out)
                assert torch.equal(out.double(), ref), (cfg, M, N, K, b is not None, (out.double() - ref).abs().max().item())
        x = (ri((3, 7, 9, 64), -1, 1) * (torch.rand((3, 7, 9, 64), generator=gen, device=DEV) < 0.5)).to(dt)
        wc = ri((320, 64, 3, 3), -1, 1) * (torch.rand((320, 64, 3, 3), generator=gen, device=DEV) < 0.5)
        bias, res = ri((320,), -3, 3), ri((3, 7, 9, 320), -3, 3).to(dt)
        ref = G.conv_acc(x.double(), wc.double(), 1, False) + bias.double() + res.double()
        assert ref.abs().max() < 256
        out = hip.conv3x3(x, pack_conv3x3(wc).to(dt), bias, residual=res)
        assert torch.equal(out.double(), ref), (cfg, "conv", int((out.double() != ref).sum()))
    forced(cfg, runs)
