"""The chained bf16 kernels held to the contract of EACH of their stages (tests/fused_gate.py): mmgt_ff_fused / mmgt_ff_fused_po (csrc/ffn.hip),
mmgt_rowgemm320 (csrc/rowgemm.hip), mmgt_temporal_leg320 (csrc/tleg.hip), mmgt_gn_silu_conv3x3 (csrc/gnconv.hip) and mmgt_gn_silu_conv3x3_unet
(csrc/rconv.hip) through `mmgt_amd.hip` and the C ABI.  The neighbours of the observed stage get operands for which they are exact, the output is
that stage's result rounded once (temporal_leg320: once more where its residual is not zero), and the gate is |out - ref| <= 2 B on EVERY element
against the fp64 contract reference computed with torch on the device.  Operands are views with NaN rows (and, where the ABI takes a row stride,
NaN columns) behind them, outputs sit inside sentinel buffers; the shapes cover a single row, row-group and workgroup tails, both tile kinds, both
window lengths, a tile seam and two-source inputs.  tests/test_fused_gate.py proves on the CPU that the same gates reject the listed mutants."""
import pytest
import torch

from tests import fused_gate as FG
from tests import mm_gate as G

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FF_M = (1, 33, 333)


def run_ff(st):
    from mmgt_amd import hip
    from mmgt_amd.packing import pack_ff_fused, pack_ff_proj_out
    o = st.ops
    M = o["x"].shape[0]
    x, res = G.guarded(o["x"]), G.guarded(o["res"])
    img = pack_ff_fused(o["w1"], o["b1"], o["w2"])
    buf, view = G.out_in_sentinels((M, FG.C), BF16, x.device, ld=FG.C + 16, col0=8)
    if st.kernel == "ffpo":
        hip.ff_fused_po(x, o["gamma"], o["beta"], img, o["b2"], res, FG.INNER, pack_ff_proj_out(o["wpo"]), o["bpo"], G.guarded(o["res2"]), out=view)
    else:
        hip.ff_fused(x, o["gamma"], o["beta"], img, o["b2"], res, FG.INNER, out=view)
    torch.cuda.synchronize()
    G.assert_untouched(buf, view)
    return FG.stage_check(view, st)


def run_rowgemm_raw(st):
    return run_rowgemm(st, check=False)


def run_rowgemm(st, n_tok=128, check=True):
    """through the C ABI (`hip.rowgemm320` asserts M % pre_rows == 0 for the tables; the kernel takes a ragged last group).  Transposed tiles go to
    out_t (M / n_tok, N - n1, npad) with npad = n_tok + 8: the padding columns and the batch behind the last must keep the sentinel."""
    from mmgt_amd import hip
    from mmgt_amd.packing import pack_rowgemm
    o, n1 = st.ops, st.n1
    M, N = o["x"].shape[0], o["w"].shape[0]
    dev = o["x"].device
    x = G.guarded(o["x"])
    res = None if o["res"] is None else G.guarded(o["res"])
    buf = view = tbuf = out_t = None
    if n1:
        buf, view = G.out_in_sentinels((M, n1), BF16, dev, ld=n1 + 16, col0=8)
    npad = n_tok + 8
    if n1 < N:
        assert M % n_tok == 0
        tbuf = torch.full((M // n_tok + 1, N - n1, npad), G.SENT, device=dev, dtype=BF16)
        out_t = tbuf[:M // n_tok]
    p, f = hip._ptr, hip._f32
    hip._check(hip.lib().mmgt_rowgemm320(p(x), x.stride(0), o["norm"], p(f(o["gamma"], "gamma")), p(f(o["beta"], "beta")), o["pe_div"], o["pe_mod"],
                                         o["eps"], p(pack_rowgemm(o["w"])), p(f(o["bias"], "bias")), p(f(o["bias2"], "bias2")), o["bias2_rows"],
                                         p(res), 0 if res is None else res.stride(0), p(view), 0 if view is None else view.stride(0), n1,
                                         p(out_t), n_tok if n1 < N else 0, npad if n1 < N else 0, M, N, hip.dtype_code(BF16), hip._stream()),
               "mmgt_rowgemm320")
    torch.cuda.synchronize()
    parts = []
    if n1:
        G.assert_untouched(buf, view)
        parts.append(view)
    if check is False:
        return view
    if n1 < N:
        chk = tbuf.clone()
        chk[:M // n_tok, :, :n_tok] = G.SENT
        assert torch.equal(chk.view(torch.int16), torch.full_like(chk, G.SENT).view(torch.int16)), "the kernel wrote into the npad padding of out_t"
        parts.append(out_t[:, :, :n_tok].permute(0, 2, 1).reshape(M, N - n1))
    return FG.stage_check(torch.cat(parts, 1), st)


# ---- ff_fused / ff_fused_po ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", FF_M)
def test_ff_fused_gelu_sweep(M):
    """every bf16 gate value with 2^-10 <= |g| <= 8 and +-0, +-16, +-64 (M = 1: the first 320 of them) through the kernel's own GELU polynomial"""
    for s in range(4):
        run_ff(FG.ff_gelu_sweep(M, s, G.dev()))


@pytest.mark.parametrize("kind", list(FG.LN_KINDS))
@pytest.mark.parametrize("M", FF_M)
def test_ff_fused_layernorm_observed(M, kind):
    for s in range(4):
        run_ff(FG.ff_ln_observed(M, s, kind, G.dev()))


@pytest.mark.parametrize("M", FF_M)
def test_ff_fused_ff1_geglu_is_a_linear_contract(M):
    for s in range(4):
        run_ff(FG.ff_ff1_geglu(M, s, G.dev()))


@pytest.mark.parametrize("po", [0, 1, 2])
@pytest.mark.parametrize("M", FF_M)
def test_ff_fused_ff2_and_proj_out_are_linear_contracts(M, po):
    run_ff(FG.ff_ff2(M, po, G.dev()))


# ---- rowgemm320 ---------------------------------------------------------------------------------------------------------------------------------
# Transposed tiles need M % n_tok == 0 with n_tok % 128 == 0 (rowgemm.hip:291): the N = 960 / n1 = 640 cases run at M = 256 and 384, the ragged
# M = 1, 129, 300 on normal tiles.

RG_SHAPES = [(M, N, None) for M in (1, 129, 300) for N in (32, 320, 1920)] + [(256, 960, 640), (384, 960, 640), (256, 320, 0)]


@pytest.mark.parametrize("M,N,n1", RG_SHAPES)
def test_rowgemm_linear(M, N, n1):
    run_rowgemm(FG.rg_linear(M, N, n1, G.dev()))


@pytest.mark.parametrize("M,N,n1", RG_SHAPES)
@pytest.mark.parametrize("norm", [1, 2, 3])
def test_rowgemm_prologue_observed(norm, M, N, n1):
    run_rowgemm(FG.rg_norm_observed(M, N, norm, "plain", n1, G.dev()))


@pytest.mark.parametrize("M,N,n1", [(300, 320, None), (384, 960, 640)])
@pytest.mark.parametrize("kind", [k for k in FG.LN_KINDS if k != "plain"])
def test_rowgemm_layernorm_inputs(kind, M, N, n1):
    run_rowgemm(FG.rg_norm_observed(M, N, 1, kind, n1, G.dev()))


# ---- temporal_leg320 ----------------------------------------------------------------------------------------------------------------------------

TL_SHAPES = [(2, 24, 8), (2, 24, 48), (2, 12, 16), (2, 12, 48)]        # (batch, frames, pixels): n is a multiple of 4 * 48 / F (tleg.hip:515)


def run_tleg(st):
    """x and out are contiguous (rows, 320) blocks (the C ABI takes no strides): NaN rows behind x, sentinel rows behind out"""
    from mmgt_amd import hip
    from mmgt_amd.packing import pack_tleg
    o = st.ops
    M = o["x"].shape[0]
    xbuf = torch.full((M + 8, FG.C), G.NAN, device=o["x"].device, dtype=BF16)
    xbuf[:M] = o["x"]
    buf, view = G.out_in_sentinels((M, FG.C), BF16, o["x"].device)
    hip.temporal_leg320(xbuf[:M], o["g"], o["bpe"], pack_tleg(o["wq"], o["wk"], o["wv"], o["wo"]), o["bo"], o["B"], o["F"], o["n"], o["scale"], out=view)
    torch.cuda.synchronize()
    G.assert_untouched(buf, view)
    return FG.stage_check(view, st)


@pytest.mark.parametrize("B,F,n", TL_SHAPES)
@pytest.mark.parametrize("kind", list(FG.LN_KINDS))
def test_temporal_leg_layernorm_and_pe_observed(kind, B, F, n):
    run_tleg(FG.tleg_ln_observed(B, F, n, kind, G.dev()))


@pytest.mark.parametrize("B,F,n", TL_SHAPES)
def test_temporal_leg_v_and_to_out_gemms(B, F, n):
    run_tleg(FG.tleg_v_gemm(B, F, n, G.dev()))
    run_tleg(FG.tleg_out_gemm(B, F, n, G.dev()))


@pytest.mark.parametrize("B,F,n", TL_SHAPES)
@pytest.mark.parametrize("which", ["q", "k"])
def test_temporal_leg_q_and_k_gemms_through_the_scores(which, B, F, n):
    """the code on head channels 0 .. F - 1, 40 - F .. 39 (F = 12: and 14 .. 25): every channel of q / k, the tile two heads share included"""
    for off in ((0, 16) if F == 24 else (0, 14, 28)):
        run_tleg(FG.tleg_qk_scores(B, F, n, which, off, G.dev()))


@pytest.mark.parametrize("B,F,n", TL_SHAPES)
def test_temporal_leg_attention_stage(B, F, n):
    run_tleg(FG.tleg_attention(B, F, n, G.dev()))


# ---- gn_silu_conv3x3 / gn_silu_conv3x3_unet -----------------------------------------------------------------------------------------------------

GNCONV = [(128, 0, 128), (256, 0, 128), (256, 0, 256), (128, 0, 64)]
RCONV = [(64, 64, 160), (320, 0, 320)]


def run_conv(st):
    """contiguous channels-last blocks (the C ABIs take no strides): NaN images behind the inputs, a sentinel image behind the output"""
    from mmgt_amd import hip
    from mmgt_amd.packing import pack_gnconv, pack_rconv
    o, ep = st.ops, st.ops["ep"]
    NB, H, W, _ = o["x0"].shape
    cout = o["w"].shape[0]
    x0 = G.guarded(o["x0"])
    x1 = None if o["x1"] is None else G.guarded(o["x1"])
    tab = torch.stack([o["scale"], o["shift"]])
    res = None if ep.residual is None else G.guarded(ep.residual.view(NB, H, W, cout))
    buf, view = G.out_in_sentinels((NB, H, W, cout), BF16, x0.device)
    if st.kernel == "gnconv":
        hip.gn_silu_conv3x3_tables(x0, tab[0], tab[1], pack_gnconv(o["w"]), cout, ep.bias, res, out=view)
    else:
        hip.gn_silu_conv3x3_unet(x0, tab[0], tab[1], pack_rconv(o["w"]), cout, ep.bias, ep.bias2, o["b2_imgs"], res, x1=x1, out=view)
    torch.cuda.synchronize()
    G.assert_untouched(buf, view)
    if getattr(st, "exact_ref", None) is not None:
        assert torch.equal(view.double(), st.exact_ref), f"{st.what}: the activation of the conv-alone inputs is not exact"
    return FG.stage_check(view, st)


def _conv_cases():
    for c0, c1, cout in GNCONV:
        yield "gnconv", c0, c1, cout, 16, 32                      # two tiles side by side: a tile seam
    for c0, c1, cout in RCONV:
        yield "rconv", c0, c1, cout, 16, 16
        yield "rconv", c0, c1, cout, 32, 16


@pytest.mark.parametrize("kernel,c0,c1,cout,H,W", list(_conv_cases()))
@pytest.mark.parametrize("exact", [False, True])
def test_conv_activation_tap_by_tap(exact, kernel, c0, c1, cout, H, W):
    """exact = True: the integer inputs of the conv-alone cases, whose activation must come out bit for bit"""
    for s in range(FG.conv_sets(c0 + c1, cout)):
        for tap in range(9):
            run_conv(FG.conv_tap(kernel, c0, c1, cout, 2, H, W, tap, s, exact, G.dev()))


@pytest.mark.parametrize("kernel,c0,c1,cout,H,W", list(_conv_cases()))
def test_conv_alone(kernel, c0, c1, cout, H, W):
    run_conv(FG.conv_alone(kernel, c0, c1, cout, 2, H, W, G.dev()))


# ---- the one-pass variance of the fused LayerNorms, measured ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mean8", "mean15", "mean30"])
def test_one_pass_variance_error_measured_through_the_kernels(kind):
    """ln_frag.h through rowgemm320: 96 row groups of 128 identical rows with a beta row each (tests/fused_gate.py `variance_probe`; the CPU suite
    shows that the estimator recovers a known error to 4e-6).  Prints the figures DESIGN.md section 2 records and asserts the contract's derived
    bound.  (tleg.hip's own LayerNorm cannot be probed this way: its residual x sets the ulp of the output.)"""
    dev = G.dev()
    groups = 96
    x, beta, z, ref, bound, ratio = FG.variance_probe(kind, groups, dev)
    st = FG.Stage("probe", "rowgemm", FG._rg_ops(x.repeat_interleave(128, 0), torch.eye(FG.C, device=dev).to(BF16), norm=1, gamma=torch.ones(FG.C, device=dev),
                                                 beta=beta.contiguous(), pe_div=128, pe_mod=groups), None, None, n1=FG.C)
    out = run_rowgemm_raw(st)
    assert torch.equal(out.view(groups, 128, FG.C)[:, 0], out.view(groups, 128, FG.C)[:, 127])
    est = FG.variance_probe_estimate(out.view(groups, 128, FG.C)[:, 0], z, ref)
    print(f"ln_frag.h (rowgemm320), |mean| / std {ratio.mean().item():.1f}: one-pass variance, relative error max {est.abs().max().item():.2e}, "
          f"mean {est.abs().mean().item():.2e}, signed mean {est.mean().item():+.2e}; derived bound {bound.max().item():.2e}")
    assert (est.abs() <= bound).all()
