"""tests/step_gate.py on the CPU: the gate of the sampler-step and VAE-attention kernels accepts the kernels' arithmetic (`simulate`, at HALF the
slack: factor 1; the exact kernels bit for bit) and rejects every mutant (factor 2) on small twins of the cases of tests/test_step_contract_gpu.py,
while the flat tolerances of tests/test_hip_kernels.py and tests/test_vae.py accept a counter read at the wrong frame (every counter of the old test
is 2), a sum over bf16-rounded exponentials, and -- at a timestep below 100 -- a changed frequency constant and a native sine.  The twins take a
small `sweep` so that the grid-stride mutants exist at CPU sizes."""
import functools
import math

import pytest
import torch

from tests import step_gate as G

BF16, F32 = torch.bfloat16, torch.float32
DTS = {"bf16": BF16, "f32": F32}


def _to_nhwc(tag, B, C, F, H, W, cpad, dt, scale=1.0, sweep=G.SWEEP):
    return G.ToNhwc(f"{tag} {dt}", G.rnd(f"{tag}.x", (B, C, F, H, W), 2.0), cpad, dt, scale, sweep)


def _from_nhwc(tag, B, C, F, H, W, cpad, dt, sweep=G.SWEEP, **kw):
    x = (G.rnd(f"{tag}.x", (B * F, H, W, cpad), 1.0) * 3.0173).to(dt)          # (off hash_uniform's 2^-24 grid: x * 0.5 + 0.5 rounds)
    x[..., C:] = G.NAN
    return G.FromNhwc(f"{tag} {dt}", x, B, C, sweep=sweep, **kw)


def _softmax(tag, rows, cols, dt, out_dt, drop, scale=0.3):
    return G.Softmax(f"{tag} {rows} x {cols} {dt} -> {out_dt}", G.softmax_input(tag, rows, cols, scale, dt), scale, out_dt, drop)


WIN3 = [[0, 1, 2, 3], [2, 3, 4, 5], [5, 6, 0, 1]]          # of 9 frames: 7 and 8 in no window, counts not uniform

CASES = {}
for _n, _dt in DTS.items():
    CASES.update({
        f"to.sweep.{_n}": lambda dt=_dt: _to_nhwc("to.sweep", 2, 12, 3, 5, 7, 16, dt, sweep=300),
        f"to.scale.{_n}": lambda dt=_dt: _to_nhwc("to.scale", 2, 4, 3, 5, 7, 64, dt, scale=1 / 0.18215),
        f"to.small.{_n}": lambda dt=_dt: _to_nhwc("to.small", 1, 3, 2, 9, 9, 8, dt),
        f"from.clamp.{_n}": lambda dt=_dt: _from_nhwc("from.clamp", 1, 3, 3, 16, 16, 64, dt, scale=0.5, shift=0.5, clamp01=True, sweep=2000),
        f"from.64.{_n}": lambda dt=_dt: _from_nhwc("from.64", 2, 4, 5, 6, 7, 64, dt),
        f"from.8.{_n}": lambda dt=_dt: _from_nhwc("from.8", 2, 4, 5, 6, 7, 8, dt),
        f"ts.all.{_n}": lambda dt=_dt: G.Timestep(f"ts 0..999 {dt}", torch.arange(1000, dtype=F32), 320, dt),
        f"ts.prod.{_n}": lambda dt=_dt: G.Timestep(f"ts twin {dt}", torch.tensor([949.0, 949.0]), 320, dt),
        f"ts.sweep.{_n}": lambda dt=_dt: G.Timestep(f"ts ramp {dt}", 999.0 * torch.arange(66, dtype=F32) / 65, 320, dt, sweep=10000),
        f"silu.{_n}": lambda dt=_dt: G.Silu(f"silu {dt}", torch.cat([torch.linspace(-100, 100, 20001), torch.tensor([0.0, -0.0])]).to(dt), sweep=10000),
        f"acc.one.{_n}": lambda dt=_dt: G.acc_case("acc.one", [G.shuffled(100, 130)], 130, 4, 8, 5, 7, dt),
        f"acc.one64.{_n}": lambda dt=_dt: G.acc_case("acc.one64", [G.shuffled(100, 130)], 130, 4, 64, 5, 7, dt),
        f"acc.row.{_n}": lambda dt=_dt: G.acc_case("acc.row", [G.shuffled(100, 130)], 130, 4, 8, 5, 7, dt, rows=1, row0=1, bump=False),
        f"acc.sweep.{_n}": lambda dt=_dt: G.acc_case("acc.sweep", [G.shuffled(6, 9)], 9, 4, 8, 4, 4, dt, sweep=300),
        f"acc.win3.{_n}": lambda dt=_dt: G.acc_case("acc.win3", WIN3, 9, 4, 8, 13, 11, dt, unwritten=(7, 8)),
        f"acc.win200.{_n}": lambda dt=_dt: G.acc_case("acc.win200", [[(3 * k) % 300, (3 * k + 7) % 300] for k in range(200)], 300, 4, 8, 3, 3, dt),
    })
    for _cols in (1, 5, 1000):
        CASES[f"sm.{_cols}.{_n}"] = lambda dt=_dt, cols=_cols: _softmax(f"sm.{cols}", 37, cols, dt, dt, 1)
for _nv in (1, 3, 32):
    CASES[f"smv.{_nv}"] = lambda nv=_nv: _softmax(f"smv.{nv}", 9, 256 * nv, F32, BF16, 4, scale=0.044)
for _g in (3.5, 1.0):
    for _step in (0, 10, 19):
        CASES[f"cfg.{_g}.{_step}"] = lambda g=_g, step=_step: G.cfg_case("cfg", 4, 7, 5, 9, g, step)
CASES.update({
    "cfg.sweep": lambda: G.cfg_case("cfg.sweep", 4, 6, 8, 8, 3.5, 10, sweep=1000),
    "split.5": lambda: G.Split3("split 5 x 4", G.rnd("sp5.qk", (5, 16), 3.0), G.rnd("sp5.bq", (4,)), G.rnd("sp5.bk", (4,))),
    "split.64": lambda: G.Split3("split 64 x 16", G.rnd("sp64.qk", (64, 64), 3.0), G.rnd("sp64.bq", (16,)), G.rnd("sp64.bk", (16,))),
    "gemm.rnd": lambda: G.GemmF32("gemm 300 x 264 x 192", G.rnd("g.a", (300, 192), 1.0, BF16), G.rnd("g.w", (264, 192), 1.0, BF16)),
    "gemm.int": lambda: G.GemmF32("gemm int 300 x 264 x 192", G.int_operand("gi.a", (300, 192)), G.int_operand("gi.w", (264, 192)), exact=True),
    "gemm.one": lambda: G.GemmF32("gemm 1 x 8 x 64", G.rnd("g1.a", (1, 64), 1.0, BF16), G.rnd("g1.w", (8, 64), 1.0, BF16)),
    "gemm.tiles": lambda: G.GemmF32("gemm 70 x 72 x 128, 32-tiles", G.rnd("gt.a", (70, 128), 1.0, BF16), G.rnd("gt.w", (72, 128), 1.0, BF16), tile=32, resident=4),
    "gemm.tiles.int": lambda: G.GemmF32("gemm int 70 x 72 x 128, 32-tiles", G.int_operand("gti.a", (70, 128)), G.int_operand("gti.w", (72, 128)), exact=True,
                                        tile=32, resident=4),
    "logits.1": lambda: G.logits_case("lg", 64, 32, 1.0),
    "logits.400": lambda: G.logits_case("lg", 64, 32, 400.0),
})
ACC = [t for t in CASES if t.startswith("acc.")]
SPLIT = [t for t in CASES if t.startswith("split.")]
PLAIN = [t for t in CASES if t not in ACC and t not in SPLIT]


@functools.lru_cache(maxsize=None)
def case(tag):
    return CASES[tag]()


@pytest.mark.parametrize("tag", PLAIN)
def test_simulation_passes_at_factor_one(tag):
    c = case(tag)
    ref, B = c.reference()
    G.check(c.simulate(), ref, B, c.what, factor=1.0)


@pytest.mark.parametrize("tag", PLAIN)
def test_every_mutant_is_rejected(tag):
    c = case(tag)
    ref, B = c.reference()
    muts = c.mutants()
    assert muts or tag.startswith("sm.1."), tag                 # (one column: the probability is 1 whatever the kernel does with the row)
    for name, mut in muts.items():
        print(f"{c.what}: {name}: {G.worst(mut, ref, B, c.dt):.1f} B")
        assert G.rejected(mut, ref, B, c.dt), (c.what, name, "accepted by the gate")


EXPECTED_MUTANTS = {
    "to.sweep.bf16": {"second sweep not written", "channel tail compared against Cpad", "f and c exchanged"},
    "to.scale.bf16": {"scale applied after the rounding"},
    "from.clamp.f32": {"second sweep not written", "clamp before shift", "f and c exchanged"},
    "from.64.bf16": {"channel tail compared against Cpad", "f and c exchanged"},
    "ts.sweep.f32": {"denominator half - 1", "sin first", "ln(10000) replaced by 9.21", "argument with a 2^-12 relative error (a native sin)",
                     "second sweep not written"},
    "cfg.3.5.10": {"counter read at (i / hw) % F with the hw of the wrong level", "counter of frame 0 for all frames", "eu and ec exchanged",
                   "sb_p applied to x0", "division by the counter dropped"},
    "cfg.sweep": {"second sweep not written"},
    "acc.one.bf16": {"counter bumped only for j < 64", "the idx[j] of the previous j"},
    "acc.sweep.f32": {"second sweep not added"},
    "acc.win3.bf16": {"windows added in reverse list order", "a frame in no window rewritten with acc + 0", "the idx[j] of the previous j"},
    "sm.1000.f32": {"the maximum over the first 64-column slice only", "the sum over bf16-rounded exponentials", "the last vector of a row dropped"},
    "smv.32": {"the maximum over the first 64-column slice only", "the last vector of a row dropped"},
    "split.64": {"lo from the unrounded difference, truncated", "Kp in Qp's order"},
    "gemm.tiles": {"last 64-wide K chunk dropped", "rows offset by one tile on a workgroup's second tile"},
    "gemm.tiles.int": {"last 64-wide K chunk dropped", "rows offset by one tile on a workgroup's second tile"},
}


@pytest.mark.parametrize("tag", list(EXPECTED_MUTANTS))
def test_the_listed_mutants_exist_where_they_are_expected(tag):
    """a mutant is built only where the case has the ingredient it alters: these cases have it"""
    assert EXPECTED_MUTANTS[tag] <= set(case(tag).mutants()), EXPECTED_MUTANTS[tag] - set(case(tag).mutants())


@pytest.mark.parametrize("tag", ACC)
def test_window_accumulation_mutants_differ_bitwise(tag):
    c = case(tag)
    want = c.expected()
    assert G.same_bits(c.expected(), want)
    muts = c.mutants()
    assert muts, tag
    for name, mut in muts.items():
        assert not G.same_bits(mut, want), (c.what, name, "bit-equal to the contract")


def test_unwritten_frames_keep_their_bits_and_the_windows_equal_sequential_calls():
    c = case("acc.win3.bf16")
    ps, cnt = c.expected()
    assert torch.equal(G.bits(ps[:, :, 7:]), G.bits(c.ps0[:, :, 7:])) and torch.equal(G.bits(cnt[7:]), G.bits(c.cnt0[7:]))
    assert (G.bits(ps[:, 1:, 7]) == G.SNAN_BITS).all() and (G.bits(ps[:, 0, 8]) == -2 ** 31).all()
    # B sequential single-window cases on the same operands
    ps2, cnt2 = c.ps0, c.cnt0
    for k, win in enumerate(c.windows):
        ps2, cnt2 = G.Acc("", c.window_pred(k), ps2, cnt2, [win], c.C).expected()
    assert G.same_bits((ps2, cnt2), (ps, cnt))


@pytest.mark.parametrize("tag", SPLIT)
def test_split3_pieces_and_mutants(tag):
    c = case(tag)
    Qp, Kp = c.expected()
    C = c.bq.shape[0]
    q, k = c.sums()
    assert torch.equal(Qp[:, :C], Qp[:, C:2 * C]) and torch.equal(Kp[:, :C], Kp[:, 2 * C:])
    assert ((Qp[:, :C].double() + Qp[:, 2 * C:].double() - q.double()).abs() <= 2.0 ** -16 * q.double().abs()).all()
    assert ((Kp[:, :C].double() + Kp[:, C:2 * C].double() - k.double()).abs() <= 2.0 ** -16 * k.double().abs()).all()
    for name, (mq, mk) in c.mutants().items():
        assert not (torch.equal(mq, Qp) and torch.equal(mk, Kp)), (c.what, name)


# ---- what the flat tolerances let through ------------------------------------------------------------------------------------------------------

def test_flat_gate_accepts_a_counter_read_at_the_wrong_frame():
    """tests/test_hip_kernels.py::test_cfg_ddim_and_window_accumulate: every frame's counter is 2, rtol 1e-5 / atol 1e-6"""
    old = G.cfg_case("cfg.old", 4, 6, 3, 3, 3.5, 10, equal_counter=2)
    ref, _ = old.reference()
    new = case("cfg.3.5.10")
    nref, nB = new.reference()
    for name in ("counter read at (i / hw) % F with the hw of the wrong level", "counter of frame 0 for all frames"):
        assert G.flat_accepts(old.mutants()[name].float(), ref, 1e-5, 1e-6), name
        assert G.rejected(new.mutants()[name], nref, nB, F32), name


@pytest.mark.parametrize("dt,atol", [(F32, 2e-3), (BF16, 1e-2)])
def test_flat_gate_accepts_a_native_sine_and_a_changed_constant_below_timestep_100(dt, atol):
    """tests/test_hip_kernels.py::test_softmax_rows_and_plumbing holds timestep_features to rtol 1e-3 and atol 2e-3 (fp32) / 1e-2 (bf16): at
    t = 999 that does catch both mutants, at the t = 3 it also runs -- and at every t up to 99 for the constant -- it does not, while the derived
    bound catches them at t = 3 (fp32: B is a few u32 there)."""
    c = G.Timestep("ts old", torch.tensor([99.0, 3.0]), 320, dt)
    ref, B = c.reference()
    muts = c.mutants()
    assert G.flat_accepts(muts["ln(10000) replaced by 9.21"].float().to(dt), ref, 1e-3, atol)
    low = G.Timestep("ts 3", torch.tensor([3.0]), 320, dt)
    lref, lB = low.reference()
    name = "argument with a 2^-12 relative error (a native sin)"
    assert G.flat_accepts(low.mutants()[name].float().to(dt), lref, 1e-3, atol)
    for n in (name, "ln(10000) replaced by 9.21"):
        assert G.rejected(muts[n], ref, B, dt), n
    if dt == F32:
        for n in (name, "ln(10000) replaced by 9.21"):
            assert G.rejected(low.mutants()[n], lref, lB, dt), n


def test_flat_gate_accepts_a_sum_over_rounded_exponentials():
    """tests/test_hip_kernels.py `tol(fp32)`: rtol 1e-3 / atol 1e-4 on softmax_rows"""
    c = case("sm.1000.f32")
    ref, B = c.reference()
    mut = c.mutants()["the sum over bf16-rounded exponentials"]
    assert G.flat_accepts(mut.float(), ref, 1e-3, 1e-4)
    assert G.rejected(mut, ref, B, F32)


def test_flat_gate_accepts_a_truncated_lo_piece():
    """tests/test_vae.py::test_split_operand_kernels: hi + lo against the sum at rtol 2e-5 / atol 1e-6"""
    c = case("split.64")
    C = c.bq.shape[0]
    q, _ = c.sums()
    mq, _ = c.mutants()["lo from the unrounded difference, truncated"]
    assert G.flat_accepts(mq[:, :C].double() + mq[:, 2 * C:].double(), q.double(), 2e-5, 1e-6)
    assert not torch.equal(mq, c.expected()[0])


def test_reversed_windows_differ_only_because_fp32_adds_do_not_commute():
    c = case("acc.win3.f32")
    a, b = c.expected()[0], c.mutants()["windows added in reverse list order"][0]
    shared = [2, 3, 5, 0, 1]
    assert not torch.equal(G.bits(a[:, :, shared]), G.bits(b[:, :, shared]))
    assert torch.equal(G.bits(a[:, :, [4, 6, 7, 8]]), G.bits(b[:, :, [4, 6, 7, 8]]))          # one window or none: the order cannot matter
    assert ((a[:, :, shared].double() - b[:, :, shared].double()).abs() <= 4 * G.U32 * 8.0).all()


def test_silu_bound_admits_the_overflow_of_expf_and_nothing_else():
    c = case("silu.f32")
    ref, B = c.reference()
    x = c.x.double()
    over = -x >= 127 * math.log(2.0)
    assert over.any() and (B[over] < 2.0 ** -119).all() and (B[~over] <= (2.0 ** -20 + 2.0 ** -23 * x[~over].abs()) * ref[~over].abs()).all()
