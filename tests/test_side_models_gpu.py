"""ReferenceNet (write mode + bank hand-off), PoseGuider and AudioProjModel on the HIP kernels vs the oracle / the
reference's golden outputs."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmgt_amd.synthetic import synth_state_dict  # noqa: E402
from oracle import unet3d_ref as R  # noqa: E402
from tests import geometry_cases as gx  # noqa: E402
from tests import golden_cases as gc  # noqa: E402

F32 = dict(rtol=1e-3, atol=1e-4)


def _g(golden_dir, name):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, name + ".npz")).items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_reference_net_banks(golden_dir, dtype):
    from mmgt_amd.reference_unet import UNet2DConditionModel
    from mmgt_amd.unet3d_spec import unet2d_reference_spec
    g = _g(golden_dir, "refnet_full")
    sd = synth_state_dict(unet2d_reference_spec(), prefix="refnet.", device="cuda:0")
    m = UNet2DConditionModel(device="cuda:0", dtype=dtype)
    m.load_state_dict(sd)
    inp = gc.refnet_inputs(gc.REFNET_CASES["full"])
    out = m(inp["latents"].cuda(), inp["timestep"], encoder_hidden_states=inp["ehs"].cuda(), return_dict=False)[0]
    assert list(m.bank) == [k[len("bank."):] for k in g if k.startswith("bank.")]
    for k, v in m.bank.items():
        if dtype == torch.float32:
            torch.testing.assert_close(v.cpu(), g["bank." + k], **F32)
        else:
            # bf16 product mode against the fp32 golden: banks are LayerNorm outputs of magnitude up to ~4, where one bf16
            # ulp is 7.8e-3..3.1e-2; the gate is the noise floor of that storage type (a few ulps at the maximum, about
            # one in the mean: measured max 4.4e-2..8.1e-2, mean 8.1e-3), not a parity claim -- parity is the fp32 branch above.
            d = (v.cpu() - g["bank." + k]).abs()
            assert d.max().item() <= 1.2e-1 and d.mean().item() <= 1.2e-2, \
                f"bank {k}: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e}"
    torch.testing.assert_close(out.float().cpu(), g["sample"], **(F32 if dtype == torch.float32 else dict(rtol=0, atol=1e-1)))


@pytest.fixture(scope="module")
def refnet_sd():
    from mmgt_amd.unet3d_spec import unet2d_reference_spec
    sd = synth_state_dict(unet2d_reference_spec(), prefix="refnet.", device="cuda:0")
    return sd, {k: v.cpu() for k, v in sd.items()}


_GEOMETRY_ORACLE = {}


def _refnet_geometry_oracle(sd_cpu, latent):
    """({bank: fp32 oracle}, {bank: (max, mean) of |oracle under CPU bf16 - fp32 oracle|}) at a latent x latent reference image; computed once
    per size and shared by the two dtypes (13-50 MB of banks: not a cache entry)."""
    if latent not in _GEOMETRY_ORACLE:
        inp = gc.refnet_inputs(dict(gc.REFNET_CASES["full"], latent=latent))
        lo = lambda t: t.bfloat16() if t.is_floating_point() else t
        with torch.no_grad():
            ref, _ = R.reference_net_banks(sd_cpu, R.UNet3DConfig(), inp["latents"], inp["timestep"], inp["ehs"])
            low, _ = R.reference_net_banks({k: lo(v) for k, v in sd_cpu.items()}, R.UNet3DConfig(), lo(inp["latents"]), inp["timestep"], lo(inp["ehs"]))
        floors = {k: ((low[k].float() - v).abs().max().item(), (low[k].float() - v).abs().mean().item()) for k, v in ref.items()}
        _GEOMETRY_ORACLE[latent] = (ref, floors)
    return _GEOMETRY_ORACLE[latent]


def _level_blocks(levels):
    """Block prefixes of the resnets at UNet levels `levels` (level l: side latent / 2^l)."""
    at = {0: ("down_blocks.0.", "up_blocks.3."), 1: ("down_blocks.1.", "up_blocks.2."), 2: ("down_blocks.2.", "up_blocks.1."),
          3: ("down_blocks.3.", "mid_block.", "up_blocks.0.")}
    return tuple(p for l in levels for p in at[l])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("latent", gx.REFNET_LATENTS)
def test_reference_net_banks_at_320_and_384_px(refnet_sd, latent, dtype):
    """`write_banks` at 40 x 40 and 48 x 48 reference latents (1600 / 400 / 100 / 25 and 2304 / 576 / 144 / 36 tokens per bank) against the
    oracle on the same inputs: fp32 mode at the parity tolerance with the banks in the oracle's key order, bf16 mode per bank within 1.5x
    the oracle's own CPU-bf16 error; the fused resnet legs that ran are exactly those of the levels whose sides tile into 16 x 16."""
    from mmgt_amd.reference_unet import UNet2DConditionModel
    sd, sd_cpu = refnet_sd
    ref, floors = _refnet_geometry_oracle(sd_cpu, latent)
    m = UNet2DConditionModel(device="cuda:0", dtype=dtype)
    m.load_state_dict(sd)
    inp = gc.refnet_inputs(dict(gc.REFNET_CASES["full"], latent=latent))
    bank = m.write_banks(inp["latents"].cuda(), inp["timestep"], inp["ehs"].cuda())
    assert list(bank) == list(ref) and len(bank) == 16
    for k, v in bank.items():
        d = (v.cpu() - ref[k]).abs()
        fmax, fmean = floors[k]
        print(f"latent {latent} {dtype} bank {k} {tuple(v.shape)}: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e} "
              f"(CPU-bf16 floor {fmax:.3e} / {fmean:.3e})")
    for k, v in bank.items():
        assert v.shape == ref[k].shape and torch.isfinite(v).all()
        if dtype == torch.float32:
            torch.testing.assert_close(v.cpu(), ref[k], **F32)
        else:
            d = (v.cpu() - ref[k]).abs()
            assert d.max().item() <= 1.5 * floors[k][0] and d.mean().item() <= 1.5 * floors[k][1], k
    # images of the fused legs are built by the forward that runs them: level 0 alone at 48 (five resnets, two legs each), none at 40, none in fp32 mode
    levels = gx.refnet_fused_levels(latent) if dtype == torch.bfloat16 else ()
    assert levels == ((0,) if latent == 48 and dtype == torch.bfloat16 else ())
    want = {r + cv + ".rimg" for r in m._resnets if r.startswith(_level_blocks(levels)) for cv in (".conv1", ".conv2")}
    assert len(want) == 10 * len(levels) and {k for k in m.w if k.endswith(".rimg")} == want


def test_reference_net_refuses_latent_side_20(refnet_sd):
    """The ReferenceNet shares the UNet's three stride-2 levels: a side that is no multiple of 8 is refused by name before any launch."""
    from mmgt_amd import hip
    from mmgt_amd.reference_unet import UNet2DConditionModel
    sd, _ = refnet_sd
    m = UNet2DConditionModel(device="cuda:0", dtype=torch.bfloat16)
    m.load_state_dict(sd)
    inp = gc.refnet_inputs(dict(gc.REFNET_CASES["full"], latent=20))
    before = dict(hip._calls)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        m.write_banks(inp["latents"].cuda(), inp["timestep"], inp["ehs"].cuda())
    assert dict(hip._calls) == before and not m.bank


def test_reference_attention_control_handoff(golden_dir):
    """writer.update -> reader banks: same pairing as the reference, fp16 round trip, then the denoiser runs with them."""
    from mmgt_amd.reference_unet import ReferenceAttentionControl, UNet2DConditionModel
    from mmgt_amd.unet3d import UNet3DConditionModel
    from mmgt_amd.unet3d_spec import unet2d_reference_spec, unet3d_spec
    ref = UNet2DConditionModel(device="cuda:0", dtype=torch.float32)
    ref.load_state_dict(synth_state_dict(unet2d_reference_spec(), prefix="refnet.", device="cuda:0"))
    den = UNet3DConditionModel(device="cuda:0", dtype=torch.float32)
    sd3 = synth_state_dict(unet3d_spec(), device="cuda:0")
    den.load_state_dict(sd3)
    den.enable_gradient_checkpointing()
    writer = ReferenceAttentionControl(ref, do_classifier_free_guidance=True, mode="write", batch_size=1, fusion_blocks="full")
    reader = ReferenceAttentionControl(den, do_classifier_free_guidance=True, mode="read", batch_size=1, fusion_blocks="full")
    rin = gc.refnet_inputs(gc.REFNET_CASES["full"])
    ref(rin["latents"].cuda(), torch.tensor(0), encoder_hidden_states=rin["ehs"].cuda(), return_dict=False)
    reader.update(writer)
    assert set(den._banks) == set(ref.bank) and len(den._banks) == 16
    case = dict(gc.UNET_CASES["full_cfg1"], frames=2)
    inp = gc.unet_inputs(case)
    mv = lambda t: t.cuda()
    out = den(mv(inp["sample"]), inp["timestep"], encoder_hidden_states=mv(inp["ehs"]), audio_embedding=mv(inp["audio"]),
              pose_cond_fea=mv(inp["pose"]), full_mask=[mv(x) for x in inp["full"]], face_mask=[mv(x) for x in inp["face"]],
              body_mask=[mv(x) for x in inp["lips"]], motion_scale=inp["motion_scale"], return_dict=False)[0].cpu()
    # oracle: same banks (the golden ones = what the reference's ReferenceNet wrote), fp16 round trip inside
    g = _g(golden_dir, "refnet_full")
    banks = {k[len("bank."):]: v for k, v in g.items() if k.startswith("bank.")}
    sd_cpu = {k: v.cpu() for k, v in sd3.items()}
    with torch.no_grad():
        want = R.unet3d_forward(sd_cpu, R.UNet3DConfig(), inp["sample"], inp["timestep"], inp["ehs"], inp["audio"],
                                inp["pose"], inp["full"], inp["face"], inp["lips"], inp["motion_scale"], banks)
    torch.testing.assert_close(out, want, **F32)
    reader.clear()
    writer.clear()
    assert not den._banks and not ref.bank


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pose_guider_and_audio_proj(golden_dir, dtype):
    from mmgt_amd.side_models import AudioProjModel, PoseGuider
    g = _g(golden_dir, "side_models")
    inp = gc.side_inputs()
    pg = PoseGuider(320, block_out_channels=(16, 32, 96, 256), device="cuda:0", dtype=dtype)
    pg.load_state_dict(synth_state_dict(pg.spec, prefix="pose_guider."))
    out = pg(inp["pose_rgb"].cuda()).cpu()
    tol = F32 if dtype == torch.float32 else dict(rtol=0, atol=5e-3)
    torch.testing.assert_close(out, g["pose_guider"], **tol)
    nhwc = pg.forward_nhwc(inp["pose_rgb"].cuda())
    assert nhwc.shape == (2, 8, 8, 320) and nhwc.dtype == dtype
    ap = AudioProjModel(device="cuda:0", dtype=dtype)
    ap.load_state_dict(synth_state_dict(ap.spec, prefix="audioproj."))
    out = ap(inp["audio_feats"].cuda()).cpu()
    torch.testing.assert_close(out, g["audio_proj"], **(F32 if dtype == torch.float32 else dict(rtol=0, atol=6e-2)))
