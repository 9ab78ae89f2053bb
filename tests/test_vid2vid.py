"""Re-voicing an existing clip without a GPU: the strength rule of both schedulers, the integer rules of csrc/vid2vid_core.h in a host
program under ASan + UBSan against the numpy restatements of tests/vid2vid_ref.py (on the cases the GPU kernels are held to), and the pipeline's
refusals.  The program is stand-alone (its own main); nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import sampler_ref as R
from tests import vid2vid_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the strength rule ----------------------------------------------------------------------------------------------------------------------------------

NS, STRENGTHS = (1, 8, 25, 30), (0.04, 0.29, 0.5, 0.999, 1.0)


def _classes():
    from mmgt_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    return DDIMScheduler, DPMSolverMultistepScheduler


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("strength", STRENGTHS)
def test_strength_keeps_the_last_entries_of_the_trailing_list(n, strength):
    want = V.kept_timesteps(n, strength)
    for cls in _classes():
        s = cls()
        if not want:
            with pytest.raises(ValueError, match=f"num_inference_steps={n} at strength={strength}"):
                s.set_timesteps(n, strength=strength)
            continue
        s.set_timesteps(n, strength=strength)
        assert s.timesteps.tolist() == want and s.timesteps.dtype == torch.int64
        assert s.num_inference_steps == n
    if strength == 1.0:
        assert want == R.trailing_timesteps(n)
    assert len(want) == min(int(n * strength), n)


def test_the_cases_cover_the_float_truncation_and_the_empty_list():
    """int(25 * 0.29) is 7 (7.25); int(30 * 0.999) is 29; 8 * 0.04 leaves nothing, 25 * 0.04 exactly one step"""
    assert len(V.kept_timesteps(25, 0.29)) == 7 and len(V.kept_timesteps(30, 0.999)) == 29
    assert V.kept_timesteps(8, 0.04) == [] and len(V.kept_timesteps(25, 0.04)) == 1 and V.kept_timesteps(1, 0.999) == []


@pytest.mark.parametrize("bad", [-0.1, 1.0001, float("nan")])
def test_strength_outside_the_unit_interval_is_a_value_error(bad):
    for cls in _classes():
        with pytest.raises(ValueError, match="strength must lie in"):
            cls().set_timesteps(8, strength=bad)


def test_ddim_kept_steps_are_the_full_schedules_steps():
    DDIM, _ = _classes()
    full, part = DDIM(), DDIM()
    full.set_timesteps(30)
    part.set_timesteps(30, strength=0.5)
    assert part.timesteps.tolist() == full.timesteps.tolist()[15:]
    for t in part.timesteps:
        assert part.step_coefficients(t) == full.step_coefficients(t)
        assert part.update_coefficients(t, 0.5) == full.update_coefficients(t, 0.5)
        assert part.alpha_bar_after(t) == full._alpha_bar(int(t) - 1000 // 30)
    assert part.alpha_bar_after(part.timesteps[-1]) == part.final_alpha_cumprod == 1.0


def test_alpha_bar_after_the_last_step_is_one_where_ddim_itself_lands_on_timestep_zero():
    """N = 6: the last trailing timestep is 166 = 1000 // 6, so the update lands on alphas_cumprod[0] (the reference's quirk, unchanged); what is
    kept of a known clip still ends at alpha-bar 1"""
    DDIM, _ = _classes()
    s = DDIM()
    s.set_timesteps(6)
    ts = s.timesteps.tolist()
    assert ts[-1] - 1000 // 6 == 0 and s.step_coefficients(ts[-1])[2] == float(s.alphas_cumprod[0] ** 0.5) < 1.0
    assert s.alpha_bar_after(ts[-1]) == 1.0
    assert [s.alpha_bar_after(t) for t in ts[:-1]] == [float(s.alphas_cumprod[t - 166]) for t in ts[:-1]]


def test_solver_sees_the_shortened_list():
    _, DPM = _classes()
    full, part = DPM(), DPM()
    full.set_timesteps(8)
    part.set_timesteps(8, strength=0.5)
    ts = part.timesteps.tolist()
    assert ts == full.timesteps.tolist()[4:]
    co, _, r0 = part.step_details(ts[0])
    assert r0 is None and co[4] == 0.0 and part.update_coefficients(ts[0])[4] == 0.0
    assert full.step_details(ts[0])[2] is not None                      # in the full list the same timestep is a second-order step
    assert part.step_details(ts[1])[2] is not None and part.step_details(ts[1]) == full.step_details(ts[1])
    assert part.alpha_bar_after(ts[0]) == float(part.alphas_cumprod[ts[1]])
    assert part.alpha_bar_after(ts[-1]) == part.final_alpha_cumprod == 1.0


def test_known_scalars_at_the_ends_of_the_schedule():
    from mmgt_amd.scheduler import DDIMScheduler, known_scalars
    s = DDIMScheduler()
    assert float(s.alphas_cumprod[999]) == 0.0                          # zero terminal SNR: strength 1 starts from the noise itself
    assert known_scalars(s._alpha_bar(999)) == (0.0, 1.0) and known_scalars(s.final_alpha_cumprod) == (1.0, 0.0)
    assert known_scalars(0.25) == V.scalars(0.25)


# ---- the integer rules in a host program under ASan + UBSan ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/vid2vid_host_check.cpp with"
    exe = tmp_path_factory.mktemp("vid2vid_host") / "vid2vid_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "vid2vid_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def _host(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-4000:]


@pytest.mark.parametrize("shape", V.MASK_SHAPES, ids=str)
def test_host_mask_to_latent_equals_the_restatement(host_check, tmp_path, shape):
    L, H, W = shape
    for name, mask in V.mask_cases(L, H, W).items():
        mask.tofile(tmp_path / "in.u8")
        for grow in V.GROWS:
            _host(host_check, "mask", L, H, W, grow, tmp_path / "in.u8", tmp_path / "out.f32")
            got = np.fromfile(tmp_path / "out.f32", np.float32).reshape(L, H // 8, W // 8)
            assert np.array_equal(got, V.mask_to_latent_ref(mask, grow)), (name, grow)


def test_the_mask_restatement_on_cases_worked_by_hand():
    m = np.zeros((1, 24, 40), np.uint8)
    m[0, 8, 39] = 128                                                   # cell (1, 4), the right edge
    m[0, 0, 0] = 127                                                    # below the threshold
    want = np.zeros((1, 3, 5), np.float32)
    want[0, 1, 4] = 1
    assert np.array_equal(V.mask_to_latent_ref(m, 0), want)
    want[0, :, 3:] = 1
    assert np.array_equal(V.mask_to_latent_ref(m, 1), want)
    assert V.mask_to_latent_ref(m, 8).all()


@pytest.mark.parametrize("grid", V.FEATHER_GRIDS, ids=str)
def test_host_feather_alpha_equals_the_restatement(host_check, tmp_path, grid):
    L, h, w = grid
    cells = V.feather_cells(L, h, w)
    cells.tofile(tmp_path / "in.f32")
    for r in V.FEATHER_RADII:
        _host(host_check, "feather", L, h, w, r, tmp_path / "in.f32", tmp_path / "out.u8")
        got = np.fromfile(tmp_path / "out.u8", np.uint8).reshape(L, 8 * h, 8 * w)
        want = V.feather_ref(cells, r)
        assert np.array_equal(got, want), r
        if r == 0:
            assert set(np.unique(got)) == {0, 255} and np.array_equal(got[:, ::8, ::8] == 255, cells >= 0.5)
        else:
            assert len(np.unique(got)) > 2


def test_host_composite_equals_the_restatement_on_every_triple(host_check, tmp_path):
    gen, orig, alpha = V.composite_triples()
    for name, a in (("gen", gen), ("orig", orig), ("alpha", alpha)):
        a.tofile(tmp_path / f"{name}.u8")
    _host(host_check, "composite", alpha.size, tmp_path / "gen.u8", tmp_path / "orig.u8", tmp_path / "alpha.u8", tmp_path / "out.u8")
    got = np.fromfile(tmp_path / "out.u8", np.uint8).reshape(gen.shape)
    assert np.array_equal(got, V.composite_ref(gen, orig, alpha))
    assert np.array_equal(got[:, :, 0], orig[:, :, 0]) and np.array_equal(got[:, :, 255], gen[:, :, 255])


def test_host_program_refuses_a_short_input(host_check, tmp_path):
    np.zeros(63, np.uint8).tofile(tmp_path / "in.u8")
    r = subprocess.run([host_check, "mask", "1", "8", "8", "0", str(tmp_path / "in.u8"), str(tmp_path / "out.f32")], capture_output=True, text=True)
    assert r.returncode == 2 and "expected exactly 64" in r.stderr


# ---- the pipeline's refusals ------------------------------------------------------------------------------------------------------------------------------

L, STEPS = 8, 4


class _NoUNet:
    device = torch.device("cpu")
    in_channels = 4


def _pipe(scheduler=None):
    from mmgt_amd.pipeline import Pose2VideoPipeline
    from mmgt_amd.scheduler import DDIMScheduler
    return Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=_NoUNet(), pose_guider=None,
                              scheduler=scheduler or DDIMScheduler())


def _call(**kw):
    return _pipe()(None, None, None, [], [], [], 32, 32, L, STEPS, 3.5, **kw)


VIDEO = torch.zeros(L, 32, 32, 3, dtype=torch.uint8)
LATENTS = torch.zeros(1, 4, L, 4, 4)


@pytest.mark.parametrize("kw, parties", [
    (dict(strength=0.5), ("strength=0.5", "init_video or init_latents")),
    (dict(regen_mask=torch.zeros(L, 32, 32, dtype=torch.uint8)), ("regen_mask", "init_video or init_latents")),
    (dict(paste_back=True), ("paste_back", "init_video or init_latents")),
    (dict(init_video=VIDEO, init_latents=LATENTS), ("init_video", "init_latents")),
    (dict(init_video=VIDEO, window_group=True), ("init_video", "window_group")),
    (dict(init_latents=LATENTS, window_group=True), ("init_latents", "window_group")),
    (dict(init_latents=LATENTS, num_images_per_prompt=2), ("init_latents", "num_images_per_prompt=2")),
    (dict(init_video=VIDEO, interpolation_factor=2), ("init_video", "interpolation_factor=2")),
    (dict(init_video=VIDEO[:5]), ("init_video has 5 frames", f"video_length={L}")),
    (dict(init_latents=LATENTS[:, :, :7]), ("init_latents has 7 frames", f"video_length={L}")),
    (dict(init_latents=LATENTS, paste_back=True, output_type="uint8"), ("paste_back", "init_video")),
    (dict(init_video=VIDEO, paste_back=True), ("paste_back", 'output_type="uint8"')),
], ids=lambda v: "-".join(v) if isinstance(v, dict) else None)
def test_pipeline_refusals_name_both_parties(kw, parties):
    with pytest.raises(ValueError) as e:
        _call(**kw)
    for p in parties:
        assert p in str(e.value), (p, str(e.value))


def test_pipeline_hands_the_strength_errors_of_the_scheduler_on():
    with pytest.raises(ValueError, match="strength must lie in"):
        _call(init_latents=LATENTS, strength=1.5)
    with pytest.raises(ValueError, match=f"num_inference_steps={STEPS} at strength=0.2"):
        _call(init_latents=LATENTS, strength=0.2)


def test_denoise_refuses_a_kept_region_with_a_window_group():
    with pytest.raises(ValueError, match="window_group"):
        _pipe().denoise(LATENTS, [999], None, None, None, [], [], [], 3.5, None, 12, 1, 4, window_group=True, known=(LATENTS, LATENTS, None))
