"""tests/mm_gate.py on the CPU: the gate of the bf16 GEMM / conv / norm kernels accepts the kernels' arithmetic (`simulate`, at HALF the slack: factor
1) and rejects every mutant (factor 2) on small twins of the cases of tests/test_mm_contract_gpu.py (the same tags), while the flat rtol 2e-2 / atol
2e-2 of tests/test_hip_kernels.py accepts a scaled accumulator, a dropped last k at K = 5120 and a variance over n - 1.  No case is degenerate:
rms(ref) >= 0.15 and, without a residual, sum |a||w| >= 4 |ref| on the median element."""
import functools

import pytest
import torch

from tests import mm_gate as G

LIN = {
    "lin.plain": dict(M=200, N=320, K=640),
    "lin.bres": dict(M=333, N=960, K=320, bias=True, residual=True),
    "lin.b2": dict(M=300, N=320, K=192, bias=True, bias2_rows=128, residual=True),
    "lin.post": dict(M=150, N=320, K=192, bias=True, row_scale=True, alpha=0.75, bias_post=True, residual=True),
    "lin.silu": dict(M=130, N=320, K=192, bias=True, act="silu", wscale=2.0),
    "lin.geglu": dict(M=150, N=256, K=320, bias=True, act="geglu", bias_scale=1.0),
    "lin.k5120": dict(M=96, N=1280, K=5120, bias=True),
    "lin.cat": dict(M=77, N=256, K=192, bias=True, residual=True),
}
CONV = {
    "cv.s1": dict(NB=2, H=5, W=7, c0=16, cout=24),
    "cv.s2": dict(NB=2, H=5, W=7, c0=16, cout=24, stride=2),
    "cv.hi": dict(NB=2, H=8, W=8, c0=16, cout=24, stride=-2),
    "cv.up": dict(NB=2, H=5, W=7, c0=16, cout=24, upsample=True),
    "cv.up2": dict(NB=2, H=5, W=7, c0=16, cout=32, upsample=2),
    "cv.two": dict(NB=4, H=5, W=7, c0=16, c1=8, cout=24, bias2_rows=70, residual=True),
    "cv.two.s2": dict(NB=2, H=8, W=8, c0=16, c1=8, cout=24, stride=2),
    "cv.1x1": dict(NB=6, H=1, W=1, c0=16, cout=24, bias2_rows=3, residual=True),
}
GN = {
    "gn.1": dict(NB=3, HW=1, c0=1280, silu=True),
    "gn.4": dict(NB=3, HW=4, c0=1280),
    "gn.64": dict(NB=3, HW=64, c0=320, silu=True),
    "gn.two": dict(NB=2, HW=16, c0=1280, c1=640, silu=True),
    "gn.small": dict(NB=2, HW=37, c0=320, slab=False),
    "gn.general": dict(NB=1, HW=300, c0=320, slab=False),
    "gn.eps": dict(NB=2, HW=64, c0=320, x_scale=0.017, mean=0.0),
    "gn.tab": dict(NB=3, HW=64, c0=320, tables=True),
    "gn.tab.two": dict(NB=2, HW=16, c0=1280, c1=640, tables=True),
}
LN = {
    "ln.320": dict(rows=123, C=320, pe_div=5, pe_mod=6),
    "ln.640": dict(rows=61, C=640, pe_div=5, pe_mod=6, folded=True),
    "ln.768": dict(rows=50, C=768),
    "ln.1280": dict(rows=33, C=1280, ldx=1288),
}


@functools.lru_cache(maxsize=None)
def case(tag):
    """a case and its references, built once for every test that uses it"""
    if tag in LIN:
        return G.linear_case(tag, **LIN[tag])
    if tag in CONV:
        return G.conv_case(tag, **CONV[tag])
    if tag == "taps":
        return G.taps_case(tag, 2, 6, 5)
    if tag in GN:
        return G.gn_case(tag, **GN[tag])
    return G.ln_case(tag, **LN[tag])


def _pairs(c):
    """[(what, ref, B)] of a case: one entry, or (scale, shift) of the tables entry"""
    r = c.reference()
    if isinstance(r[0], tuple):
        return [(f"{c.what} scale", r[0][0], r[1][0]), (f"{c.what} shift", r[0][1], r[1][1])]
    return [(c.what, r[0], r[1])]


ALL = list(LIN) + list(CONV) + ["taps"] + list(GN) + list(LN)


def test_gelu_polynomial_error_is_what_common_h_states():
    err = G.gelu_poly_error()
    print(f"max |gelu_erf_f - x Phi(x)| over [-12, 12] in fp32: {err:.3e}")
    assert err < G.GELU_ERR


@pytest.mark.parametrize("tag", ALL)
def test_simulation_passes_at_factor_one(tag):
    c = case(tag)
    sim = c.simulate()
    sims = list(sim) if isinstance(sim, tuple) else [sim]
    for (what, ref, B), s in zip(_pairs(c), sims):
        G.check(s, ref, B, what, factor=1.0)
    if tag in GN or tag in LN:
        if not c.tables:
            G.norm_check(sim, c, factor=1.0)
    if tag == "cv.up2":
        ref, B = c.reference()
        G.check(sim, ref, B, c.what + " (ideal)", ideal=c.ideal())


@pytest.mark.parametrize("tag", ALL)
def test_every_mutant_is_rejected(tag):
    c = case(tag)
    muts = c.mutants()
    assert muts, tag
    pairs = _pairs(c)
    for name, mut in muts.items():
        ms = list(mut) if isinstance(mut, tuple) else [mut]
        if pairs[0][1].dtype == torch.float64 and len(pairs) == 2:      # the fp32 tables: no output rounding
            worst = max(G.ratio(m, ref, B).max().item() for (_, ref, B), m in zip(pairs, ms))
        else:
            worst = max(G.rejects(m, ref, B) for (_, ref, B), m in zip(pairs, ms))
        print(f"{c.what}: {name}: {worst:.1f} B")
        assert worst > 2.0, (c.what, name, "accepted by the gate")


@pytest.mark.parametrize("tag", list(LIN) + list(CONV))
def test_cases_are_not_degenerate(tag):
    case(tag).assert_not_degenerate()


@pytest.mark.parametrize("tag", list(GN) + list(LN))
def test_norm_cases_are_not_degenerate_and_the_statistics_term_stays_small(tag):
    c = case(tag)
    r = c.reference()
    if c.tables:
        return
    ref, B, S, cap = r
    assert ref.pow(2).mean().sqrt().item() >= 0.15
    assert (S < cap).all(), (S / cap).max().item()


@pytest.mark.parametrize("tag", list(LIN))
def test_flat_gate_accepts_a_scaled_accumulator(tag):
    c = case(tag)
    ref, B = c.reference()
    mut = G.bf16_round(c.mutants()["accumulator x (1 + 2^-6)"])
    assert G.old_gate_accepts(mut, ref), "the flat gate was expected to accept this mutant"
    assert G.rejects(mut, ref, B) > 2.0


def test_flat_gate_accepts_a_dropped_last_k_at_5120():
    c = case("lin.k5120")
    ref, B = c.reference()
    mut = G.bf16_round(c.mutants()["last k dropped"])
    assert G.old_gate_accepts(mut, ref)
    assert G.rejects(mut, ref, B) > 2.0


@pytest.mark.parametrize("tag", [t for t in GN if not GN[t].get("tables")])
def test_flat_gate_accepts_the_variance_over_n_minus_one(tag):
    c = case(tag)
    assert c.n_per_group() >= 40
    ref, B, _, _ = c.reference()
    mut = G.bf16_round(c.mutants()["variance divided by n - 1"])
    assert G.old_gate_accepts(mut, ref)
    assert G.rejects(mut, ref, B) > 2.0
