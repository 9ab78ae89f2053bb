"""tests/fused_gate.py on the CPU: on small twins of the cases of tests/test_fused_contract_gpu.py a torch simulation of the WHOLE kernel's arithmetic
(fp32 accumulation, bf16 at the rounding points the sources state) passes the isolated stage's gate at HALF the slack (factor 1), every listed
mutant is rejected at factor 2, and the flat gates of today's whole-chain tests are shown to accept a tanh GELU, a variance over n - 1 and a
missing eps.  No case is degenerate: a floor on rms(ref) is asserted per case (0.15; 0.05 for the constant rows, whose reference is beta alone)."""
import functools

import pytest
import torch

from tests import fused_gate as FG
from tests import mm_gate as G

CASES = {}
for s in range(4):
    CASES[f"ff.gelu.{s}"] = lambda s=s: FG.ff_gelu_sweep(33, s)
for i, kind in enumerate(FG.LN_KINDS):
    CASES[f"ff.ln.{kind}"] = lambda i=i, kind=kind: FG.ff_ln_observed(33, i % 4, kind)
    CASES[f"rg.ln.{kind}"] = lambda kind=kind: FG.rg_norm_observed(300, 320, 1, kind)
for s in (0, 3):
    CASES[f"ff.ff1.{s}"] = lambda s=s: FG.ff_ff1_geglu(33, s)
for po in range(3):
    CASES[f"ff.ff2.po{po}"] = lambda po=po: FG.ff_ff2(33, po)
CASES["rg.lin.320"] = lambda: FG.rg_linear(129, 320)
CASES["rg.lin.1920"] = lambda: FG.rg_linear(40, 1920)
CASES["rg.lin.t"] = lambda: FG.rg_linear(256, 960, 640)
for norm in (2, 3):
    CASES[f"rg.tab{norm}.320"] = lambda norm=norm: FG.rg_norm_observed(300, 320, norm)
    CASES[f"rg.tab{norm}.1920"] = lambda norm=norm: FG.rg_norm_observed(129, 1920, norm)
for i, kind in enumerate(FG.LN_KINDS):
    CASES[f"tl.ln.{kind}"] = lambda i=i, kind=kind: FG.tleg_ln_observed(1, (24, 12)[i % 2], (8, 16)[i % 2], kind)
CASES["tl.v"] = lambda: FG.tleg_v_gemm(1, 12, 16)
CASES["tl.o"] = lambda: FG.tleg_out_gemm(1, 24, 8)
for which in "qk":
    for F, off in ((24, 0), (24, 16), (12, 0), (12, 14), (12, 28)):
        CASES[f"tl.{which}.{F}.{off}"] = lambda which=which, F=F, off=off: FG.tleg_qk_scores(1, F, 192 // F, which, off)
CASES["tl.att.24"] = lambda: FG.tleg_attention(1, 24, 8)
CASES["tl.att.12"] = lambda: FG.tleg_attention(1, 12, 16)
GNCONV = [(128, 0, 128), (256, 0, 128), (256, 0, 256), (128, 0, 64)]
RCONV = [(64, 64, 160), (320, 0, 320)]
for kernel, shapes, hw in (("gnconv", GNCONV, (16, 32)), ("rconv", RCONV, (32, 16))):
    for i, (c0, c1, cout) in enumerate(shapes):
        for tap in range(9):
            s = (tap + i) % FG.conv_sets(c0 + c1, cout)
            CASES[f"{kernel}.tap{tap}.{c0 + c1}.{cout}"] = lambda k=kernel, a=c0, b=c1, c=cout, t=tap, s=s, hw=hw: FG.conv_tap(k, a, b, c, 2, *hw, t, s, exact=t % 2 == 1)
        CASES[f"{kernel}.conv.{c0 + c1}.{cout}"] = lambda k=kernel, a=c0, b=c1, c=cout, hw=hw: FG.conv_alone(k, a, b, c, 2, *hw)


@functools.lru_cache(maxsize=None)
def case(tag):
    return CASES[tag]()


def simulate(st):
    return {"rowgemm": FG.rowgemm_sim, "tleg": FG.tleg_sim, "gnconv": FG.conv_sim, "rconv": FG.conv_sim}.get(st.kernel, FG.ff_sim)(st.ops)


def test_gelu_polynomial_error_is_what_ffn_hip_states():
    err = FG.gelu_ffn_error()
    print(f"max |ffn.hip gelu - x Phi(x)| over [-8, 8] in fp32: {err:.3e}")
    assert err < FG.GELU_FFN_ERR


@pytest.mark.parametrize("tag", list(CASES))
def test_simulation_passes_at_factor_one(tag):
    st = case(tag)
    sim = simulate(st)
    FG.stage_check(sim, st, factor=1.0)
    if getattr(st, "exact_ref", None) is not None:           # the inputs of the conv-alone cases: the activation is exact, bit for bit
        assert torch.equal(sim.double(), st.exact_ref)


@pytest.mark.parametrize("tag", list(CASES))
def test_every_mutant_is_rejected(tag):
    st = case(tag)
    muts = st.mutants()
    assert muts, tag
    for name, mut in muts.items():
        worst = G.ratio(G.bf16_round(mut), st.ref, st.B).max().item()
        print(f"{st.what}: {name}: {worst:.1f} B{' (not rejected by this case, as stated)' if name in st.weak else ''}")
        assert (worst <= 2.0) if name in st.weak else (worst > 2.0), (st.what, name, "accepted by the gate")


@pytest.mark.parametrize("tag", list(CASES))
def test_cases_are_not_degenerate_and_the_statistics_term_stays_below_its_cap(tag):
    st = case(tag)
    st.assert_not_degenerate()
    if st.S is not None:
        print(f"{st.what}: statistics term at most {FG.stats_share(st):.3f} of its cap ({st.norm.frac} U (|gamma| (|z| + 1) + |beta|))")
        assert FG.stats_share(st) < 1.0
    if tag.startswith("ff.ff1"):                       # the gates spread over [-4, 4]
        q = torch.quantile(st.gates.flatten(), torch.tensor([0.02, 0.98], dtype=torch.float64))
        assert q[0] < -3.0 and q[1] > 3.0 and st.gates.abs().max() < 8.0, q
        st.lin.assert_not_degenerate()


def test_the_sweep_holds_every_bf16_value_of_the_range():
    st = case("ff.gelu.0")
    seen = set(st.ops["x"][:11].flatten().view(torch.int16).tolist())
    assert len(seen) == 3336
    assert set(st.xs.flatten().float().to(torch.bfloat16).view(torch.int16).tolist()) == seen          # and every one of them is observed


@pytest.mark.parametrize("kind", list(FG.LN_KINDS))
def test_the_neighbours_of_an_observed_layernorm_are_transparent(kind):
    """the simulated chain's output IS the LayerNorm's bf16 output, bit for bit, for ff_fused and rowgemm320"""
    st = case(f"ff.ln.{kind}")
    o = st.ops
    xn = FG.ln_onepass_sim(o["x"], o["gamma"], o["beta"], 1e-5)
    assert torch.equal(simulate(st).view(torch.int16), xn[:, FG.perm320(320)].view(torch.int16))
    st = case(f"rg.ln.{kind}")
    o = st.ops
    xn = FG.ln_onepass_sim(o["x"], o["gamma"], o["beta"][FG._row_groups(300, 128, 3, "cpu")], 1e-5)
    assert torch.equal(simulate(st).view(torch.int16), xn[:, FG.perm320(320)].view(torch.int16))


@pytest.mark.parametrize("kind,std", [("mean8", 8), ("mean15", 15), ("mean30", 30)])
def test_one_pass_variance_error_of_the_simulation_stays_inside_the_derived_term(kind, std):
    x = FG.ln_input("fg.var", 333, kind)
    xd = x.double()
    mean, var = xd.mean(1), xd.var(1, unbiased=False)
    r = (mean.abs() / var.sqrt())
    assert (r > 0.9 * std).all() and (r < 1.1 * std).all()
    rel = ((FG.onepass_stats_sim(x)[1].double() - var).abs() / var)
    nc = FG.OnePassNorm(kind, x, torch.ones(320), torch.zeros(320), 0.0)
    nc.reference()
    print(f"|mean| = {std} std: one-pass variance, simulated: max relative error {rel.max().item():.2e}, mean {rel.mean().item():.2e}; "
          f"derived term {nc.rel_var.max().item():.2e}")
    assert (rel <= nc.rel_var).all()


@pytest.mark.parametrize("name,kw", [("tanh GELU", dict(gelu="tanh")), ("variance over n - 1", dict(ddof=1)), ("eps omitted", dict(eps_on=False))])
def test_flat_gate_of_test_ffn_gpu_accepts(name, kw):
    """tests/test_ffn_gpu.py::test_ff_fused_random_against_fp64 (2^-8 |ref| + 4e-3 and the mean assert) on its own operands at M = 512"""
    o, ref = ffn_operands()
    ok, worst = FG.ffn_flat_gate(FG.ff_sim(o), ref)
    ok_m, worst_m = FG.ffn_flat_gate(FG.ff_sim(o, **kw), ref)
    print(f"flat gate: honest simulation {worst:.2f} of tol, {name} {worst_m:.2f} of tol")
    assert ok and ok_m, "the flat gate was expected to accept this mutant"


@functools.lru_cache(maxsize=None)
def ffn_operands():
    return FG.ffn_test_operands(512)


@pytest.mark.parametrize("kind", ["mean8", "mean15", "mean30"])
def test_the_variance_probe_recovers_the_simulated_one_pass_error(kind):
    """the estimator of the GPU measurement on the simulation, whose variance error is known exactly: it must recover it to 4e-6"""
    x, beta, z, ref, bound, _ = FG.variance_probe(kind, 96)
    out = FG.ln_onepass_sim(x, torch.ones(320), beta, 1e-5)
    est = FG.variance_probe_estimate(out, z, ref)
    var = x.double().var(1, unbiased=False)
    true = (FG.onepass_stats_sim(x)[1].double() - var) / var
    print(f"{kind}: simulated variance error max {true.abs().max().item():.2e}; the probe's estimate differs by at most {(est - true).abs().max().item():.2e}")
    assert (est - true).abs().max() < 4e-6 and (est.abs() <= bound).all()
