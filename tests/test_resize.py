"""The device image resize without a GPU: the numpy restatement tests/resize_ref.py is held to PIL.Image.resize byte for byte, the
coefficient tables of mmgt_amd.conditioning.pil_resample_tables to the restatement's, to pil_bilinear_tables and to the 32-bit accumulator bound, and
the product's own arithmetic and indexing -- csrc/resample_core.h, the code the kernels call -- runs in a stand-alone host program built with
AddressSanitizer and UBSan on buffers of exactly the size the C ABI asks for, against PIL on the same cases."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, f) for s in R.SHAPES for f in R.FILTERS]
CASE_IDS = [f"{R.shape_id(s)}-{f}" for s, f in CASES]


# ---- the restatement is PIL ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape,filt", CASES, ids=CASE_IDS)
def test_restatement_equals_pil(shape, filt, kind, c):
    (hs, ws), (hd, wd) = shape
    img = R.image(hs, ws, c, kind)
    got, want = R.resize(img, hd, wd, filt), R.pil_resize(img, hd, wd, filt)
    assert got.shape == want.shape == (hd, wd, c) and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} bytes differ, max |d| = {np.abs(got.astype(int) - want).max()}"


def test_images_hold_what_they_are_for():
    """The edge images are 0 / 255 only and have both; Lanczos and bicubic over- and undershoot on them, so both clamps of clip8 are reached."""
    img = R.image(135, 240, 3, "edges")
    assert set(np.unique(img)) == {0, 255}
    for filt in ("bicubic", "lanczos"):
        rows = R.coefficients(240, 64, filt)
        assert min(int(k.min()) for _, k in rows) < 0
    assert max(len(k) for _, k in R.coefficients(300, 8, "lanczos")) == 225                         # of ksize = 2 ceil(3 * 37.5) + 1 = 227


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------------------
def _sizes():
    return sorted({(a, b) for (hs, ws), (hd, wd) in R.SHAPES for a, b in ((hs, hd), (ws, wd))} | {(1080, 512), (1920, 512), (512, 256), (512, 192),
                                                                                                    (150, 224), (100, 224)})


def test_bilinear_tables_are_pil_bilinear_tables():
    from mmgt_amd import conditioning as C
    for a, b in _sizes() + [(64, 32), (64, 16), (64, 8), (512, 64)]:
        b0, k0 = C.pil_bilinear_tables(a, b)
        b1, k1 = C.pil_resample_tables(a, b, "bilinear")
        assert torch.equal(b0, b1) and torch.equal(k0, k1), (a, b)
        assert torch.equal(k1, C.pil_resample_tables(a, b)[1])                                      # bilinear is the default


@pytest.mark.parametrize("filt", R.FILTERS)
def test_tables_equal_the_restatement_and_meet_the_accumulator_bound(filt):
    from mmgt_amd import conditioning as C
    support = R.KERNELS[filt][1]
    for a, b in _sizes():
        bounds, kk = C.pil_resample_tables(a, b, filt)
        rows = R.coefficients(a, b, filt)
        assert bounds.dtype == kk.dtype == torch.int32 and tuple(bounds.shape) == (b, 2)
        assert kk.shape[1] == 2 * int(np.ceil(support * max(a / b, 1.0))) + 1
        for o, (lo, k) in enumerate(rows):
            first, cnt = (int(v) for v in bounds[o])
            assert (first, cnt) == (lo, len(k)) and 0 <= first and first + cnt <= a and 1 <= cnt <= kk.shape[1], (a, b, o)
            assert np.array_equal(kk[o, :cnt].numpy(), k) and not kk[o, cnt:].any(), (a, b, o)
            assert 255 * int(np.abs(k).sum()) + (1 << 21) <= 2 ** 31 - 1, (a, b, o)


def test_tables_refuse_what_they_cannot_do():
    from mmgt_amd import conditioning as C
    with pytest.raises(ValueError, match="filter"):
        C.pil_resample_tables(8, 4, "nearest")
    for a, b in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        with pytest.raises(ValueError, match="16384"):
            C.pil_resample_tables(a, b, "bilinear")
    assert tuple(C.pil_resample_tables(16384, 1, "lanczos")[1].shape) == (1, 2 * 3 * 16384 + 1)    # the largest tap count there is


def test_pose_tensor_device_still_raises_on_another_size():
    from mmgt_amd import inputs
    frames = torch.zeros((2, 48, 80, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="pose_tensor"):
        inputs.pose_tensor_device(frames, 64, 48)
    with pytest.raises(ValueError, match="pose_tensor"):
        inputs.pose_tensor_device(frames, 64, 48, resize=False)
    with pytest.raises(ValueError, match="uint8"):
        inputs.pose_tensor_device(frames.float(), 80, 48, resize=True)
    with pytest.raises(ValueError, match="resample"):
        inputs.resize_frames_device(frames, 64, 48, "nearest")


# ---- the product's arithmetic in a host program under ASan + UBSan ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/resize_host_check.cpp with"
    exe = tmp_path_factory.mktemp("resize_host") / "resize_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "resize_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def write_job(path, frames, hd, wd, filt, lut=None):
    from mmgt_amd import conditioning as C
    n, hs, ws, c = frames.shape
    tabs = [C.pil_resample_tables(s, d, filt) if s != d else None for s, d in ((ws, wd), (hs, hd))]
    ks = [t[1].shape[1] if t else 0 for t in tabs]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<10i", 0x314A5352, n, hs, ws, hd, wd, c, ks[0], ks[1], 0 if lut is None else 1))
        for t in tabs:
            if t:
                fh.write(t[0].numpy().astype("<i4").tobytes() + t[1].numpy().astype("<i4").tobytes())
        if lut is not None:
            fh.write(np.ascontiguousarray(lut, "<f4").tobytes())
        fh.write(np.ascontiguousarray(frames).tobytes())


def run_host(exe, job, out):
    r = subprocess.run([exe, str(job), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, f"{r.stdout[-500:]}{r.stderr[-4000:]}"


@pytest.mark.parametrize("shape,filt", CASES, ids=CASE_IDS)
def test_host_program_equals_pil(host_check, tmp_path, shape, filt):
    (hs, ws), (hd, wd) = shape
    for kind in R.KINDS:
        for c in (1, 3):
            for n in (1, 3):
                fr = R.frames(n, hs, ws, c, kind)
                write_job(tmp_path / "job.bin", fr, hd, wd, filt)
                run_host(host_check, tmp_path / "job.bin", tmp_path / "out.bin")
                got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(n, hd, wd, c)
                want = np.stack([R.pil_resize(f, hd, wd, filt) for f in fr])
                assert np.array_equal(got, want), (kind, c, n)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[1], R.SHAPES[2], R.SHAPES[7]], ids=R.shape_id)
def test_host_program_float_epilogue_is_the_planar_lookup(host_check, tmp_path, shape):
    """The fp32 epilogue in each place it can run (after the vertical pass, after the horizontal pass alone, after the vertical alone, as a plain
    lookup): (C, n, Hd, Wd) = lut[c][PIL's byte]."""
    (hs, ws), (hd, wd) = shape
    for c in (1, 3):
        fr = R.frames(2, hs, ws, c, "noise")
        lut = np.random.default_rng(c).standard_normal((c, 256)).astype(np.float32)
        write_job(tmp_path / "job.bin", fr, hd, wd, "bicubic", lut)
        run_host(host_check, tmp_path / "job.bin", tmp_path / "out.bin")
        got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(c, 2, hd, wd)
        want = np.stack([R.pil_resize(f, hd, wd, "bicubic") for f in fr])                           # (n, hd, wd, c)
        assert np.array_equal(got, np.stack([lut[ch][want[..., ch]] for ch in range(c)]))


def test_host_program_reports_a_tap_outside_the_image(host_check, tmp_path):
    """The buffers are exact: a table whose last row reaches one tap past the row ends in an AddressSanitizer report, not in a pass."""
    from mmgt_amd import conditioning as C
    fr = R.frames(1, 8, 12, 1, "noise")
    write_job(tmp_path / "job.bin", fr, 8, 5, "bilinear")
    bounds, kk = C.pil_resample_tables(12, 5, "bilinear")
    raw = bytearray((tmp_path / "job.bin").read_bytes())
    at = 40 + 4 * (2 * 4)                                                                             # bounds[4][0]: the last row's first tap
    first, cnt = int(bounds[4, 0]), int(bounds[4, 1])
    assert first + cnt == 12 and struct.unpack_from("<i", raw, at)[0] == first
    struct.pack_into("<i", raw, at, first + 1)
    (tmp_path / "bad.bin").write_bytes(bytes(raw))
    r = subprocess.run([host_check, str(tmp_path / "bad.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr, r.stderr[-2000:]
