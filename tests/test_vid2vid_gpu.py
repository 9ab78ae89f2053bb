"""Re-voicing an existing clip on the device: the four kernels of csrc/vid2vid.hip against tests/vid2vid_ref.py, AutoencoderKL.encode_video
against the oracle, and Pose2VideoPipeline's init arguments -- the loop without weights over the Gaussian stand-in of tests/test_sampler_gpu.py
(restated here), one run of the tiny model with paste-back, and scripts/pose2vid.py.

The integer kernels are held byte for byte.  `known_latents` is held to one fp32 ulp at the magnitude |sa x0| + |sb z| (vid2vid_ref.known_reference
says why the result's own ulp cannot serve), and bit for bit wherever the contract is a selection.  The loop is held to sampler_ref's closed-form
bound (tests/test_sampler_gpu.py's docstring derives it) from the start the kernel produced, which the fp64 loop takes as exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import sampler_ref as R  # noqa: E402
from tests import step_gate as G  # noqa: E402
from tests import vid2vid_ref as V  # noqa: E402

DEV = "cuda:0"
F32 = torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = "mmgt_known_latents"
NAMES = (KNOWN, "mmgt_mask_to_latent", "mmgt_feather_alpha", "mmgt_composite_u8")


def _bits_equal(a, b):
    return torch.equal(G.bits(a), G.bits(b))


# ---- known_latents ----------------------------------------------------------------------------------------------------------------------------------------

KNOWN_SHAPES = [(1,) + s for s in R.SHAPES] + [(1, 3, 2, 5, 7)]            # 210 elements: no multiple of 4, the scalar path


def _known_case(shape):
    tag = "v2v.known." + ".".join(map(str, shape))
    x0, z, x = (G.rnd(f"{tag}.{n}", shape, s, device=DEV).contiguous() for n, s in (("x0", 1.2), ("z", 1.7), ("x", 1.5)))
    _, _, F, h, w = shape
    frame = torch.arange(F, device=DEV).view(F, 1, 1)
    col = torch.arange(w, device=DEV).view(1, 1, w)
    mask = ((col + frame) % 2 == 0).expand(F, h, w).to(F32).contiguous()        # a checkerboard of columns that shifts with the frame
    return x0, z, x, mask


@pytest.mark.parametrize("shape", KNOWN_SHAPES, ids=str)
def test_known_latents(shape):
    from mmgt_amd import hip
    x0, z, x, mask = _known_case(shape)
    sa, sb = V.scalars(0.37)
    ref, B = V.known_reference(x0, z, sa, sb)
    out = torch.full(shape, G.NAN, device=DEV)
    before = hip.call_count(KNOWN)
    got = hip.known_latents(G.guarded(x0, 1), G.guarded(z, 1), sa, sb, out=out)
    assert got is out and hip.call_count(KNOWN) == before + 1
    G.check(out, ref, B, f"known_latents {shape}", factor=1.0)                  # NaN-filled out: every element written
    assert _bits_equal(hip.known_latents(x0, z, sa, sb), out)                   # two launches, the same bits
    assert _bits_equal(hip.known_latents(x0, z, 1.0, 0.0), x0) and _bits_equal(hip.known_latents(x0, z, 0.0, 1.0), z)
    # the blend: mask 1 -> x, mask 0 -> the unmasked call's bits; per frame (a wrong frame index takes the neighbouring frame's columns)
    blend = hip.known_latents(x0, z, sa, sb, x=G.guarded(x, 1), mask=G.guarded(mask, 1), out=torch.full(shape, G.NAN, device=DEV))
    assert _bits_equal(blend, torch.where(mask.bool()[None, None], x, out))
    assert _bits_equal(hip.known_latents(x0, z, sa, sb, x=x, mask=torch.ones_like(mask)), x)
    assert _bits_equal(hip.known_latents(x0, z, sa, sb, x=x, mask=torch.zeros_like(mask)), out)
    inplace = x.clone()
    assert hip.known_latents(x0, z, sa, sb, x=inplace, mask=mask, out=inplace) is inplace and _bits_equal(inplace, blend)


def test_known_latents_keeps_signed_zeros_and_ignores_the_dropped_operand():
    from mmgt_amd import hip
    x0, z, _, _ = _known_case((1, 3, 2, 5, 7))
    x0 = x0.clone()
    x0.view(-1)[:3] = torch.tensor([-0.0, 0.0, -1.5], device=DEV)
    nan = torch.full_like(z, G.NAN)
    assert _bits_equal(hip.known_latents(x0, nan, 1.0, 0.0), x0) and _bits_equal(hip.known_latents(nan, x0, 0.0, 1.0), x0)


def test_known_latents_between_zero_and_one():
    """m x + (1 - m) known with m = 0.25 (exact in fp32, as is 1 - m): the two products and the sum round once each at most, known carries its own
    ulp: B = 0.75 B_known + u (|m x| + |0.75 known| + |out|), the gate 2 B as for every bounded kernel (tests/step_gate.py)."""
    from mmgt_amd import hip
    x0, z, x, mask = _known_case((1, 4, 7, 5, 3))
    sa, sb = V.scalars(0.37)
    kn, Bk = V.known_reference(x0, z, sa, sb)
    ref = 0.25 * x.double() + 0.75 * kn
    B = 0.75 * Bk + R.U * ((0.25 * x.double()).abs() + (0.75 * kn).abs() + ref.abs())
    G.check(hip.known_latents(x0, z, sa, sb, x=x, mask=torch.full_like(mask, 0.25)), ref, B, "known_latents mask 0.25")


def test_known_latents_refusals_launch_nothing():
    from mmgt_amd import hip
    x0, z, x, mask = _known_case((1, 4, 7, 5, 3))
    before = dict(hip._calls)
    for bad, pat in ((dict(x0=x0[0]), "x0 must be"), (dict(z=z.double()), "z must be"), (dict(z=z[:, :3].contiguous()), "z must be"),
                     (dict(x=x), "come together"), (dict(mask=mask), "come together"), (dict(x=x, mask=mask[:6].contiguous()), "mask must be"),
                     (dict(x=x, mask=mask.double()), "mask must be"), (dict(x=x.permute(0, 1, 2, 4, 3), mask=mask), "x must be"),
                     (dict(out=x0), "not x0 or z"), (dict(out=torch.empty(1, 4, 7, 5, 4, device=DEV)), "out must be")):
        kw = dict(x0=x0, z=z)
        kw.update(bad)
        a, b = kw.pop("x0"), kw.pop("z")
        with pytest.raises(RuntimeError, match=pat):
            hip.known_latents(a, b, 0.5, 0.5, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        hip.known_latents(x0.cpu(), z, 0.5, 0.5)
    assert hip._calls == before


# ---- the integer kernels ----------------------------------------------------------------------------------------------------------------------------------

def _behind(t, value):
    """`t` on the device as a view with one more frame behind it that holds `value`: read as part of the operand, it would set cells that are clear"""
    buf = torch.full((t.shape[0] + 1,) + tuple(t.shape[1:]), value, device=DEV, dtype=t.dtype)
    buf[:t.shape[0]].copy_(t)
    return buf[:t.shape[0]]


@pytest.mark.parametrize("shape", V.MASK_SHAPES, ids=str)
def test_mask_to_latent(shape):
    from mmgt_amd import hip
    L, H, W = shape
    for name, mask in V.mask_cases(L, H, W).items():
        m = _behind(torch.from_numpy(mask), 255)
        for grow in V.GROWS:
            got = hip.mask_to_latent(m, grow)
            assert got.dtype == F32 and tuple(got.shape) == (L, H // 8, W // 8)
            assert np.array_equal(got.cpu().numpy(), V.mask_to_latent_ref(mask, grow)), (name, grow)
    assert torch.equal(hip.mask_to_latent(m, 1), hip.mask_to_latent(m, 1))


@pytest.mark.parametrize("grid", V.FEATHER_GRIDS, ids=str)
def test_feather_alpha(grid):
    from mmgt_amd import hip
    L, h, w = grid
    cells = V.feather_cells(L, h, w)
    c = _behind(torch.from_numpy(cells), 1.0)
    for r in V.FEATHER_RADII:
        got = hip.feather_alpha(c, r)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (L, 8 * h, 8 * w)
        assert np.array_equal(got.cpu().numpy(), V.feather_ref(cells, r)), r
    assert set(np.unique(hip.feather_alpha(c, 0).cpu().numpy())) == {0, 255}


def test_composite_u8_on_every_triple():
    from mmgt_amd import hip
    gen, orig, alpha = V.composite_triples()
    want = V.composite_ref(gen, orig, alpha)
    g, o, a = (torch.from_numpy(t).to(DEV) for t in (gen, orig, alpha))
    got = hip.composite_u8(g, o, a)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got[:, :, 0], o[:, :, 0]) and torch.equal(got[:, :, 255], g[:, :, 255])


def test_composite_u8_odd_sizes_and_unaligned_views():
    """7 x 5 x 3 = 105 pixels: a tail behind the groups of four; views one frame into an allocation of 105-byte frames start at an odd address, where
    the kernel goes pixel by pixel"""
    from mmgt_amd import hip
    rng = np.random.default_rng(5)
    gen, orig = (rng.integers(0, 256, (3, 7, 5, 3), dtype=np.uint8) for _ in range(2))
    alpha = rng.integers(0, 256, (3, 7, 5), dtype=np.uint8)
    alpha[0, 0] = 0
    alpha[0, 1] = 255
    g, o, a = (torch.from_numpy(t).to(DEV) for t in (gen, orig, alpha))
    assert np.array_equal(hip.composite_u8(g, o, a).cpu().numpy(), V.composite_ref(gen, orig, alpha))
    assert g[1:].data_ptr() % 4 and a[1:].data_ptr() % 4
    assert np.array_equal(hip.composite_u8(g[1:], o[1:], a[1:]).cpu().numpy(), V.composite_ref(gen[1:], orig[1:], alpha[1:]))


def test_integer_kernels_refusals_launch_nothing():
    from mmgt_amd import hip
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)
    before = dict(hip._calls)
    for fn, pat in ((lambda: hip.mask_to_latent(u8(2, 12, 16)), "multiples of 8"), (lambda: hip.mask_to_latent(u8(2, 16, 16).float()), "uint8"),
                    (lambda: hip.mask_to_latent(u8(2, 16, 16), 9), "grow"), (lambda: hip.mask_to_latent(u8(2, 16, 16), -1), "grow"),
                    (lambda: hip.mask_to_latent(u8(2, 16, 16, 1)), "uint8"),
                    (lambda: hip.feather_alpha(u8(2, 3, 5)), "float32"), (lambda: hip.feather_alpha(u8(2, 3, 5).float(), 33), "radius"),
                    (lambda: hip.feather_alpha(u8(2, 3, 5).float(), 1.5), "radius"),
                    (lambda: hip.composite_u8(u8(2, 8, 8, 3), u8(2, 8, 8, 3), u8(2, 8, 4)), "alpha must be"),
                    (lambda: hip.composite_u8(u8(2, 8, 8, 3), u8(2, 8, 4, 3), u8(2, 8, 8)), "orig must be"),
                    (lambda: hip.composite_u8(u8(2, 8, 8, 4), u8(2, 8, 8, 4), u8(2, 8, 8)), "gen must be"),
                    (lambda: hip.composite_u8(u8(2, 8, 8, 3).float(), u8(2, 8, 8, 3), u8(2, 8, 8)), "gen must be")):
        with pytest.raises(RuntimeError, match=pat):
            fn()
    g = u8(2, 8, 8, 3)
    with pytest.raises(RuntimeError, match="of its own"):
        hip.composite_u8(g, u8(2, 8, 8, 3), u8(2, 8, 8), out=g)
    assert hip._calls == before


# ---- encode_video -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tol", [(torch.float32, dict(rtol=1e-3, atol=1e-4)), (torch.bfloat16, dict(rtol=0, atol=6e-2))])
def test_encode_video_matches_the_oracle(dtype, tol):
    from mmgt_amd.synthetic import hash_uniform, synth_state_dict
    from mmgt_amd.vae import AutoencoderKL, vae_decoder_spec, vae_encoder_spec
    from oracle import vae_ref
    spec = vae_decoder_spec()
    spec.update(vae_encoder_spec())
    sd = synth_state_dict(spec, prefix="vae.", device="cpu")
    frames = ((hash_uniform("v2v.frames", (3, 128, 64, 3), 0.5) + 0.5) * 255).clamp(0, 255).to(torch.uint8)
    x = (torch.from_numpy(frames.numpy().astype(np.float32) / 255.0) * 2.0 - 1.0).permute(0, 3, 1, 2)       # _pil_to_tensor's float stage
    with torch.no_grad():
        ref = vae_ref.vae_encode_mean(sd, x) * 0.18215                                                      # (3, 4, 16, 8)
    vae = AutoencoderKL(device=DEV, dtype=dtype)
    vae.load_state_dict(sd)
    out = vae.encode_video(frames.to(DEV), frames_per_batch=2)
    assert tuple(out.shape) == (1, 4, 3, 16, 8) and out.dtype == F32 and out.is_cuda
    print(dtype, "max|d|", (out[0].permute(1, 0, 2, 3).cpu() - ref).abs().max().item(), "mean|ref|", ref.abs().mean().item())
    torch.testing.assert_close(out[0].permute(1, 0, 2, 3).cpu(), ref, **tol)
    with pytest.raises(ValueError, match="uint8"):
        vae.encode_video(frames.to(DEV).float())
    dec = AutoencoderKL(device=DEV, dtype=dtype)
    dec.load_state_dict(synth_state_dict(vae_decoder_spec(), prefix="vae.", device="cpu"))
    with pytest.raises(RuntimeError, match="encoder weights were not loaded"):
        dec.encode_video(frames.to(DEV))


# ---- the loop, end to end, without weights ------------------------------------------------------------------------------------------------------------------

L, CTX, OV, STEPS, HW, S_U, S_C = 20, 12, 4, 6, 8, 0.5, 2.0
TABLE = R.alphas_cumprod()


class _GaussianUNet:
    """tests/test_sampler_gpu.py's stand-in for the operator (no `boc`), restated: the exact v-prediction of data N(0, 0.5^2) for the unconditional
    rows and N(0, 2^2) for the conditional ones, v = fp32(c(t)) x in fp32 on the device, in the operator's layout ((rows Fw), h, w, 64) with garbage
    in the pad channels -- plus what Pose2VideoPipeline.__call__ asks of a denoising_unet besides the forward."""
    device = torch.device(DEV)
    in_channels = 4

    def __init__(self):
        self.calls = 0

    def set_banks(self, banks):
        pass

    def clear_banks(self):
        pass

    def denoise_window(self, latent_in, t, encoder_hidden_states, audio_embedding, pose_cond_fea, full_mask, face_mask, body_mask, motion_scale,
                       cfg_row=None):
        rows, c, f, h, w = latent_in.shape
        assert cfg_row is None and rows % 2 == 0 and latent_in.dtype == F32
        a_t = R.a_of(TABLE, int(t))
        gains = [R.f32(R.gaussian_v_gain(a_t, S_U))] * (rows // 2) + [R.f32(R.gaussian_v_gain(a_t, S_C))] * (rows // 2)
        v = latent_in * torch.tensor(gains, device=DEV, dtype=F32).view(rows, 1, 1, 1, 1)
        out = torch.full((rows * f, h, w, 64), 1e9, device=DEV, dtype=F32)
        out[..., :c] = v.permute(0, 2, 3, 4, 1).reshape(rows * f, h, w, c)
        self.calls += 1
        return out


def _z():
    return G.rnd("v2v.loop.z", (1, 4, L, HW, HW), 1.7, device=DEV).contiguous()


def _x0():
    return G.rnd("v2v.loop.x0", (1, 4, L, HW, HW), 1.1, device=DEV).contiguous()


def _pipe(scheduler):
    from mmgt_amd.pipeline import Pose2VideoPipeline
    unet = _GaussianUNet()
    return Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=unet, pose_guider=None, scheduler=scheduler), unet


def _run(scheduler, **kw):
    """the pipeline's __call__ over the stand-in: 64 x 64 px = 8 x 8 latents, L = 20, windows 12 / 4, six steps, the noise handed in"""
    pipe, unet = _pipe(scheduler)
    out = pipe(None, None, torch.zeros(1, L, 1, 1), [], [], [], 8 * HW, 8 * HW, L, STEPS, R.GUIDANCE, context_frames=CTX, context_overlap=OV,
               clip_image_embeds=torch.zeros(1, 8), reference_banks={}, pose_features=torch.zeros(1, 1, L, 1, 1), latents=_z(), decode=False, **kw)
    torch.cuda.synchronize()
    return out.videos, unet


def _windows():
    from mmgt_amd.context import get_context_scheduler
    return list(get_context_scheduler("uniform")(0, STEPS, L, CTX, 1, OV))


def _by_hand(scheduler, start, timesteps, **kw):
    pipe, _ = _pipe(scheduler)
    out = pipe.denoise(start, timesteps, torch.zeros(2, 1, 8, device=DEV), None, torch.zeros(2, L, 1, 1, device=DEV), [], [], [], R.GUIDANCE, None,
                       context_frames=CTX, context_stride=1, context_overlap=OV, num_inference_steps=STEPS, **kw)
    torch.cuda.synchronize()
    return out


def _counts(hip):
    return {n: hip.call_count(n) for n in (KNOWN, "mmgt_cfg_ddim_step", "mmgt_sampler_step")}


def test_strength_one_without_a_mask_is_the_plain_sample():
    from mmgt_amd import hip
    from mmgt_amd.scheduler import DDIMScheduler
    c0 = _counts(hip)
    plain, _ = _run(DDIMScheduler())
    c1 = _counts(hip)
    assert c1[KNOWN] == c0[KNOWN] and c1["mmgt_cfg_ddim_step"] - c0["mmgt_cfg_ddim_step"] == STEPS          # no init arguments: nothing new launched
    got, _ = _run(DDIMScheduler(), init_latents=_x0())
    c2 = _counts(hip)
    assert c2[KNOWN] - c1[KNOWN] == 1 and c2["mmgt_cfg_ddim_step"] - c1["mmgt_cfg_ddim_step"] == STEPS and c2["mmgt_sampler_step"] == c0["mmgt_sampler_step"]
    assert _bits_equal(got, plain) and plain.abs().max() > 0.1


@pytest.mark.parametrize("rule", ["ddim", "dpm"])
def test_strength_half_runs_the_last_three_steps(rule):
    from mmgt_amd import hip
    from mmgt_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    cls = DDIMScheduler if rule == "ddim" else DPMSolverMultistepScheduler
    got, unet = _run(cls(), init_latents=_x0(), strength=0.5)
    assert unet.calls == 3 * len(_windows())
    ts = R.trailing_timesteps(STEPS)[3:]
    start = hip.known_latents(_x0(), _z(), *V.scalars(R.a_of(TABLE, ts[0])))
    s = cls()
    if rule == "ddim":
        s.set_timesteps(STEPS)
        hand_ts = s.timesteps[3:]
    else:                                                       # the solver reads its neighbours from its own list
        s.set_timesteps(STEPS, strength=0.5)
        hand_ts = s.timesteps
    assert hand_ts.tolist() == ts
    assert _bits_equal(got, _by_hand(s, start.clone(), hand_ts))
    steps = V.ddim_pairs_of(TABLE, ts, STEPS) if rule == "ddim" else V.dpm_triples_of(TABLE, ts)
    ref, bound = V.loop_from(start, steps, rule, R.GUIDANCE, S_U, S_C)
    assert ref.abs().max() > 0.1 and (bound < 1e-3 * (ref.abs() + 1)).all()
    G.check(got, ref, bound, f"strength 0.5 {rule}")


def _half_mask():
    """the left half of every even frame and the right half of every odd one are regenerated"""
    m = torch.zeros(L, HW, HW, device=DEV)
    m[0::2, :, :HW // 2] = 1
    m[1::2, :, HW // 2:] = 1
    return m


@pytest.mark.parametrize("strength", [0.5, 1.0])
def test_mask_of_ones_is_the_unmasked_run_and_mask_of_zeros_returns_the_clip(strength):
    from mmgt_amd.scheduler import DDIMScheduler
    free, _ = _run(DDIMScheduler(), init_latents=_x0(), strength=strength)
    ones, _ = _run(DDIMScheduler(), init_latents=_x0(), strength=strength, regen_mask=torch.ones(L, HW, HW))
    zeros, _ = _run(DDIMScheduler(), init_latents=_x0(), strength=strength, regen_mask=torch.zeros(L, HW, HW))
    assert _bits_equal(ones, free) and _bits_equal(zeros, _x0()) and not torch.equal(free, _x0())


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_half_and_half_mask(eta):
    from mmgt_amd import hip
    from mmgt_amd.scheduler import DDIMScheduler
    mask, x0, z = _half_mask(), _x0(), _z()
    keep = (mask == 0)[None, None].expand(1, 4, L, HW, HW)
    gen = lambda: torch.Generator(device=DEV).manual_seed(11) if eta else None
    traj = []
    c0 = _counts(hip)
    got, _ = _run(DDIMScheduler(), init_latents=x0, regen_mask=mask, eta=eta, generator=gen(), callback=lambda i, t, lat: traj.append((int(t), lat.clone())))
    c1 = _counts(hip)
    assert c1[KNOWN] - c0[KNOWN] == 1 + STEPS and len(traj) == STEPS
    assert c1["mmgt_sampler_step" if eta else "mmgt_cfg_ddim_step"] - c0["mmgt_sampler_step" if eta else "mmgt_cfg_ddim_step"] == STEPS
    assert [t for t, _ in traj] == R.trailing_timesteps(STEPS)
    for i, (t, lat) in enumerate(traj):                         # after every step the kept cells are the clip noised to where the step landed;
        a_after = R.a_of(TABLE, t - 1000 // STEPS) if i + 1 < STEPS else 1.0      # behind the last one that is alpha-bar 1 (166 - 1000 // 6 is 0, not -1)
        want = hip.known_latents(x0, z, *V.scalars(a_after))
        assert _bits_equal(lat[keep], want[keep]), t
    assert _bits_equal(traj[-1][1], got) and _bits_equal(got[keep], x0[keep])
    # the regenerated cells: the stand-in is elementwise and the regions do not interact, so they follow the unmasked loop from z
    noises = None
    if eta:
        twin = gen()
        noises = [torch.randn((1, 4, L, HW, HW), generator=twin, device=DEV, dtype=F32) for _ in range(STEPS)]
    ref, bound = V.loop_from(z, R.ddim_pairs(TABLE, STEPS), "ddim", R.GUIDANCE, S_U, S_C, eta, noises)
    G.check(got[~keep], ref[~keep], bound[~keep], f"half mask eta {eta}: regenerated cells")
    two, unet2 = _run(DDIMScheduler(), init_latents=x0, regen_mask=mask, eta=eta, generator=gen(), context_batch_size=2)
    assert _bits_equal(two, got) and unet2.calls == STEPS * -(-len(_windows()) // 2)


# ---- the tiny model: init_video, a lips mask, paste-back ------------------------------------------------------------------------------------------------------

def test_tiny_model_revoices_the_masked_region_and_pastes_it_back():
    from mmgt_amd import hip
    from mmgt_amd.synthetic import hash_uniform, synth_state_dict
    from mmgt_amd.vae import vae_decoder_spec, vae_encoder_spec
    from tests.test_pipeline_gpu import _build, _inputs, build_weights
    sds = build_weights(DEV)
    spec = vae_decoder_spec()
    spec.update(vae_encoder_spec())
    sds["vae"] = synth_state_dict(spec, prefix="vae.", device=DEV)
    pipe = _build(sds, torch.float32)
    inp = _inputs(8, 8)
    video = ((hash_uniform("v2v.clip", (8, 64, 64, 3), 0.5) + 0.5) * 255).clamp(0, 255).to(torch.uint8)
    lips = np.zeros((8, 64, 64), np.uint8)
    for l in range(8):
        lips[l, 40:46, 30 + l % 3:38 + l % 3] = 255
    before = {n: hip.call_count(n) for n in NAMES}
    out = pipe(None, inp["pose"], inp["audio"], inp["full"], inp["face"], inp["lips"], 64, 64, 8, 4, 3.5, motion_scale=[1.0, 1.0, 2.0],
               latents=inp["latents"], clip_image_embeds=inp["clip"], ref_image_latents=inp["ref_lat"], output_type="uint8",
               init_video=video, regen_mask=torch.from_numpy(lips), paste_back=True).videos
    assert [hip.call_count(n) - before[n] for n in NAMES] == [1 + 4, 1, 1, 1]
    assert isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == (1, 8, 64, 64, 3)
    alpha = V.feather_ref(V.mask_to_latent_ref(lips, 1), 8)
    assert (alpha == 0).any() and (alpha == 255).any()
    got, clip = out[0].numpy(), video.numpy()
    assert np.array_equal(got[alpha == 0], clip[alpha == 0])
    assert (got[alpha == 255] != clip[alpha == 255]).any()


# ---- the script -----------------------------------------------------------------------------------------------------------------------------------------------

def test_pose2vid_script_revoices_a_clip(tmp_path):
    rng = np.random.default_rng(2)
    clip = rng.integers(0, 256, (8, 64, 64, 3), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", clip)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pose2vid.py"), "--synthetic", "-W", "64", "-H", "64", "-L", "8", "--steps", "4",
                        "--init_video", str(tmp_path / "clip.npy"), "--strength", "0.5", "--regen_mask", "lips", "--paste_back", "--out_dir",
                        str(tmp_path)], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["video"] == [1, 8, 64, 64, 3] and rec["finite"] and rec["init_video"] and rec["strength"] == 0.5 and rec["regen_mask"] == "lips"
    frames = torch.load(rec["saved"])
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (1, 8, 64, 64, 3)
