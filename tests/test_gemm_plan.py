"""The GEMM / conv dispatch as data: mmgt_amd/csrc/gemm_plan.h (`plan_gemm`: shape + switches -> plan) through tools/gemm_plan_host_check.cpp, a
stand-alone program built under ASan + UBSan and run as a child process; nothing of it is loaded into Python.

* tests/golden/gemm_plans.json holds the plan of every case of tools/ab_cfg.py's SETS "step", "ctx12", "vae", "wx", "l3small" and "bm192" under the
  default switches, recorded from the dispatcher as it was BEFORE the planner existed (its `launch()` body with the launches replaced by recorders):
  the planner must give the same plan, field by field.  The case list is read from tools/ab_cfg.py's source, so a case added there needs its plan here.
* The contracts that csrc/gemm.hip's launch side and csrc/gemm16.hip rely on hold over a sweep of shapes x switches (the program's `contracts`; the
  test runs every 499-th shape of the sweep against all 96 switch settings, `gemm_plan_host_check contracts` without a step runs all of it).  A forced
  `gemm_cfg` 19 is the one way to the 192-row tile with the `bm192` switch off: the switch gates the heuristic, as `splitk` and `tailsplit` do.
* The shapes whose plan kind tests/test_mm_contract_gpu.py and tests/test_step_shapes_gpu.py state in their docstrings get that kind."""
import ast
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED_SETS = ("step", "ctx12", "vae", "wx", "l3small", "bm192")
SHAPE_FIELDS = ["bf16", "mode", "M", "N", "K", "batch", "act", "fast", "post", "residual", "bias_unaligned", "bias_post_unaligned", "up", "ksplit", "img"]
PLAN_FIELDS = ["kind", "BM", "BN", "WM", "WN", "NSTAGE", "EPI", "bm", "bn", "S", "rows_a"]


def shape(mode, M, N, K, *, batch=1, act=0, residual=0, up=0, img=1, bf16=1):
    """a launch whose operands are 16-byte aligned tensors with bias / bias2 / residual only (no row scale, alpha or post-scale bias), as
    mmgt_amd/hip.py's gemm, gemm_batched_wx and conv3x3 send it"""
    n_out = N // 2 if act == 1 else N
    return [bf16, mode, M, N, K, batch, act, int(N % 8 == 0 and n_out % 8 == 0), 0, int(residual), 0, 0, int(up), 0, img]


def case_shape(fn, args, kw):
    """the launch behind a case of tools/ab_cfg.py (its gemm_case / conv_case / wx_case)"""
    if fn == "gemm_case":
        M, N, K = args
        return shape(0, M, N, K, act=kw.get("act", 0), residual=kw.get("res", False))
    if fn == "conv_case":
        nb, h, cin, cout = args
        ho = 2 * h if kw.get("up", False) else h
        return shape(1, nb * ho * ho, cout, 9 * cin, up=kw.get("up", False), img=ho * ho)
    assert fn == "wx_case", fn
    B, R, ntok, K = args
    return shape(0, R, ntok, K, batch=B)


def ab_cfg_cases():
    """[(set, case text, shape)] of the recorded SETS, from the source of tools/ab_cfg.py (importing it would open the device)"""
    with open(os.path.join(ROOT, "tools", "ab_cfg.py")) as fh:
        tree = ast.parse(fh.read())
    sets = next(n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "SETS")
    by_name = {k.value: v.body.elts for k, v in zip(sets.keys, sets.values)}
    out = []
    for name in RECORDED_SETS:
        for call in by_name[name]:
            args = [ast.literal_eval(a) for a in call.args]
            kw = {k.arg: ast.literal_eval(k.value) for k in call.keywords}
            out.append((name, ast.unparse(call), case_shape(call.func.id, args, kw)))
    return out


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/gemm_plan_host_check.cpp with"
    exe = tmp_path_factory.mktemp("gemm_plan_host") / "gemm_plan_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "gemm_plan_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def plans(host_check, tmp_path, shapes, gemm_cfg=0, splitk=1, tailsplit=1, bm192=1):
    """[{field: value}] of PLAN_FIELDS, one per shape"""
    path = tmp_path / "shapes.txt"
    path.write_text("".join(" ".join(str(v) for v in s) + "\n" for s in shapes))
    r = subprocess.run([host_check, "plan", str(path), str(gemm_cfg), str(splitk), str(tailsplit), str(bm192)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(shapes)
    out = []
    for ln in lines:
        f = ln.split()
        out.append(dict(zip(PLAN_FIELDS, [f[0]] + [int(v) for v in f[1:]])))
    return out


def test_planner_gives_the_recorded_plans(host_check, tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "gemm_plans.json")) as fh:
        golden = json.load(fh)
    assert golden["shape_fields"] == SHAPE_FIELDS and golden["plan_fields"] == PLAN_FIELDS
    cases = ab_cfg_cases()
    assert [(c["set"], c["case"], c["shape"]) for c in golden["cases"]] == [(s, t, sh) for s, t, sh in cases], "tools/ab_cfg.py's SETS and the recorded cases differ"
    got = plans(host_check, tmp_path, [sh for _, _, sh in cases])
    for c, g in zip(golden["cases"], got):
        want = dict(zip(PLAN_FIELDS, c["plan"]))
        for f in PLAN_FIELDS:
            assert g[f] == want[f], (c["set"], c["case"], f, g, want)
    assert {c["plan"][0] for c in golden["cases"]} >= {"tile", "g16_tile", "g16_splitk", "g16_tail"}      # (the sets reach every kind that launches)


def test_contracts_hold_over_the_sweep(host_check):
    r = subprocess.run([host_check, "contracts", "499"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.rstrip().endswith("ok"), r.stdout
    assert int(r.stdout.split()[0]) > 10_000_000, r.stdout


def test_split_k_condition_of_the_mm_contract_test(host_check, tmp_path):
    """tests/test_mm_contract_gpu.py::test_gemm_either_side_of_the_split_k_condition: 64 x 256, bias + residual; K = 2560 splits in two with the
    switch on and runs one launch with it off; K = 2496 runs the same single launch either way."""
    sh = {K: shape(0, 64, 256, K, residual=1) for K in (2560, 2496)}
    on = plans(host_check, tmp_path, [sh[2560], sh[2496]], splitk=1)
    off = plans(host_check, tmp_path, [sh[2560], sh[2496]], splitk=0)
    assert (on[0]["kind"], on[0]["bn"], on[0]["S"]) == ("g16_splitk", 256, 2)
    assert off[0]["kind"] == "tile"
    assert on[1] == off[1] and on[1]["kind"] == "tile"


def test_split_shapes_of_the_step_shapes_test(host_check, tmp_path):
    """tests/test_step_shapes_gpu.py: its split-K shapes split with `splitk` on and run one launch with it off (but 3072 x 1280 x 5120: a dense
    shape of 60 tiles stays on the 128x64 tile either way); its tail-split convs (48 images of 32 x 32, 640 columns) run images [0, 32) as one launch
    and the rest split in two with `tailsplit` on, and one launch with it off."""
    convs = [shape(1, 48 * 64, 1280, 9 * 1280, residual=1, img=64), shape(1, 48 * 64, 1280, 9 * 2560, residual=1, img=64), shape(1, 6 * 64, 512, 9 * 640, residual=1, img=64)]
    dense = [shape(0, 1000, 640, 2560, residual=1), shape(0, 3072, 1280, 5120, residual=1)]
    on, off = plans(host_check, tmp_path, convs + dense, splitk=1), plans(host_check, tmp_path, convs + dense, splitk=0)
    assert [p["kind"] for p in on] == ["g16_splitk"] * 4 + ["tile"]
    assert all(2 <= p["S"] <= 8 for p in on[:4])
    assert all(p["kind"] in ("tile", "g16_tile") for p in off)
    assert on[4] == off[4] and (on[4]["BM"], on[4]["BN"]) == (128, 64)
    tails = [shape(1, 48 * 1024, 640, 9 * 640, residual=1, img=1024), shape(1, 48 * 1024, 640, 9 * 1920, residual=1, img=1024)]
    on, off = plans(host_check, tmp_path, tails, tailsplit=1), plans(host_check, tmp_path, tails, tailsplit=0)
    for p, q in zip(on, off):
        assert (p["kind"], p["bn"], p["S"], p["rows_a"]) == ("g16_tail", 320, 2, 32 * 1024)
        assert q["kind"] == "g16_tile" and q["bn"] == 320
