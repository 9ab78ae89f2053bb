"""VAE decode leg (decode_latents): HIP decoder through the C ABI vs the oracle restatement of diffusers' AutoencoderKL
decoder, plus analytic anchors for the oracle itself (the reference holds no fixture for this third-party piece)."""
import pytest
import torch

from mmgt_amd.synthetic import hash_uniform, synth_state_dict
from oracle import vae_ref


def _sd(device="cpu", encoder=False):
    from mmgt_amd.vae import vae_decoder_spec, vae_encoder_spec
    spec = vae_decoder_spec()
    if encoder:
        spec.update(vae_encoder_spec())
    return synth_state_dict(spec, prefix="vae.", device=device)


def test_oracle_vae_shapes_and_frame_independence():
    sd = _sd()
    lat = hash_uniform("vae.lat", (1, 4, 3, 8, 8), 1.0)
    with torch.no_grad():
        v = vae_ref.decode_latents(sd, lat)
        v1 = vae_ref.decode_latents(sd, lat[:, :, 1:2])
    assert v.shape == (1, 3, 3, 64, 64) and v.min() >= 0 and v.max() <= 1
    torch.testing.assert_close(v[:, :, 1:2], v1)                       # decoding is per frame


def test_oracle_vae_known_answer_zero_weights():
    """All conv / linear weights zero: every resnet is the identity on its (zero) input, so the output is conv_out.bias
    everywhere -> decode_latents == clamp(bias / 2 + 0.5)."""
    sd = {k: torch.zeros_like(v) for k, v in _sd().items()}
    sd["decoder.conv_out.bias"] = torch.tensor([-2.0, 0.2, 3.0])
    with torch.no_grad():
        v = vae_ref.decode_latents(sd, torch.randn(1, 4, 2, 8, 8))
    want = torch.tensor([0.0, 0.6, 1.0]).view(1, 3, 1, 1, 1).expand_as(v)
    torch.testing.assert_close(v, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float32, dict(rtol=1e-3, atol=1e-4)), (torch.bfloat16, dict(rtol=0, atol=4e-2))])
def test_hip_vae_matches_oracle(dtype, tol):
    from mmgt_amd.vae import AutoencoderKL
    sd = _sd()
    lat = hash_uniform("vae.lat", (1, 4, 3, 8, 8), 1.0)
    with torch.no_grad():
        ref = vae_ref.decode_latents(sd, lat)
    vae = AutoencoderKL(device="cuda:0", dtype=dtype)
    vae.load_state_dict(sd)
    out = vae.decode_video(lat.cuda(), frames_per_batch=2).cpu()
    assert out.shape == ref.shape
    print(dtype, "max|d|", (out - ref).abs().max().item())
    torch.testing.assert_close(out, ref, **tol)
    one = vae.decode((lat[0, :, 1:2] / 0.18215).permute(1, 0, 2, 3).cuda()).sample.cpu()    # diffusers-style call
    torch.testing.assert_close((one / 2 + 0.5).clamp(0, 1), ref[0, :, 1:2].permute(1, 0, 2, 3), **tol)


@pytest.mark.gpu
def test_hip_vae_gnconv_modes_agree():
    """The three forms of the decoder's GroupNorm -> SiLU -> conv legs (mmgt_tune "gnconv": 0 two launches, 1 fused launch behind a statistics
    pass, 2 statistics from the producing launch: the default) against the oracle at the bf16 gate, and against each other."""
    from mmgt_amd import hip
    from mmgt_amd.vae import AutoencoderKL
    sd = _sd()
    lat = hash_uniform("vae.lat", (1, 4, 3, 8, 8), 1.0)
    with torch.no_grad():
        ref = vae_ref.decode_latents(sd, lat)
    vae = AutoencoderKL(device="cuda:0", dtype=torch.bfloat16)
    vae.load_state_dict(sd)
    outs = []
    try:
        for mode in (0, 1, 2):
            hip.tune("gnconv", mode)
            outs.append(vae.decode_video(lat.cuda(), frames_per_batch=3).cpu())
            torch.testing.assert_close(outs[-1], ref, rtol=0, atol=4e-2)
    finally:
        hip.tune("gnconv", 2)
    assert (outs[1] - outs[0]).abs().max() < 3e-2 and (outs[2] - outs[1]).abs().max() < 3e-2


@pytest.mark.gpu
def test_split_operand_kernels():
    """The three entry points of the bf16 model's mid-block attention (include/mmgt_hip.h): bf16 x bf16 -> raw fp32 accumulators,
    the hi / lo split of q and k, fp32 logits -> bf16 probabilities."""
    from mmgt_amd import hip
    dev = "cuda:0"
    a = hash_uniform("sp.a", (300, 192), 1.0).to(dev).bfloat16()
    w = hash_uniform("sp.w", (264, 192), 1.0).to(dev).bfloat16()
    out = hip.gemm_bf16_f32(a, w)
    torch.testing.assert_close(out.double(), a.double() @ w.double().t(), rtol=1e-5, atol=1e-5)
    # strided operands (a row window of a wider matrix) and an output with a row stride
    big = hash_uniform("sp.big", (300, 448), 1.0).to(dev).bfloat16()
    dst = torch.zeros((300, 512), device=dev)
    hip.gemm_bf16_f32(big[:, 64:256], w, out=dst[:, 8:272])
    torch.testing.assert_close(dst[:, 8:272].double(), big[:, 64:256].double() @ w.double().t(), rtol=1e-5, atol=1e-5)
    assert dst[:, :8].abs().max() == 0 and dst[:, 272:].abs().max() == 0
    # q . k through the pieces: 17 bits, where bf16-rounded q and k keep 8
    C, rows = 512, 160
    qk = hash_uniform("sp.qk", (rows, 4 * C), 3.0).to(dev)
    bq, bk = hash_uniform("sp.bq", (C,), 1.0).to(dev), hash_uniform("sp.bk", (C,), 1.0).to(dev)
    Qp, Kp = hip.qk_split3(qk, bq, bk)
    q = (qk[:, :C] + qk[:, C:2 * C] + bq).double()
    k = (qk[:, 2 * C:3 * C] + qk[:, 3 * C:] + bk).double()
    assert torch.equal(Qp[:, :C], Qp[:, C:2 * C]) and torch.equal(Kp[:, :C], Kp[:, 2 * C:])
    torch.testing.assert_close(Qp[:, :C].double() + Qp[:, 2 * C:].double(), q, rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(Kp[:, :C].double() + Kp[:, C:2 * C].double(), k, rtol=2e-5, atol=1e-6)
    want = q @ k.t()
    got = hip.gemm_bf16_f32(Qp, Kp).double()
    scale = (q.norm(dim=1)[:, None] * k.norm(dim=1)[None, :])
    assert ((got - want).abs() / scale).max() < 3e-5, ((got - want).abs() / scale).max()
    plain = q.bfloat16().double() @ k.bfloat16().double().t()
    assert ((plain - want).abs() / scale).max() > 20 * ((got - want).abs() / scale).max()     # what the pieces buy
    # softmax
    for cols in (256, 1536, 4096):
        x = hash_uniform(f"sp.x{cols}", (37, cols), 300.0).to(dev)
        p = torch.empty((37, cols), device=dev, dtype=torch.bfloat16)
        hip.softmax_rows_f32_bf16(x, 0.044, p)
        ref = torch.softmax(x.double() * 0.044, dim=1)
        torch.testing.assert_close(p.double(), ref, rtol=1e-2, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("gain", [1.0, 400.0])
def test_hip_vae_split_attention(gain):
    """The bf16 model's mid-block attention through operand pieces (vae._mid_attention_split, 16 x 16 latents = 256 tokens) against
    the oracle and against the fp32 kernels on the same bf16 model; gain 400 scales to_q / to_k so that the logits reach the hundreds
    real sd-vae-ft-mse weights produce, where bf16-rounded q / k would move softmax weights by tens of percent."""
    from mmgt_amd.vae import AutoencoderKL
    sd = _sd()
    a = "decoder.mid_block.attentions.0"
    for n in ("to_q", "to_k"):
        sd[f"{a}.{n}.weight"] = sd[f"{a}.{n}.weight"] * gain
    lat = hash_uniform("vae.lat16", (1, 4, 2, 16, 16), 1.0)
    with torch.no_grad():
        ref = vae_ref.decode_latents(sd, lat)
    vae = AutoencoderKL(device="cuda:0", dtype=torch.bfloat16)
    vae.load_state_dict(sd)
    x = hash_uniform("vae.midx", (2, 16, 16, 512), 1.5).cuda().bfloat16()
    t = vae._gn(a + ".group_norm", x, False).view(-1, 512).float()
    logits = (t @ vae.w[a + ".q.w"].t() + vae.w[a + ".q.bias"]) @ (t @ vae.w[a + ".k.w"].t() + vae.w[a + ".k.bias"]).t() * 512 ** -0.5
    print("gain", gain, "max |logit|", logits.abs().max().item())
    if gain > 1:
        assert logits.abs().max() > 100
    split = vae._mid_attention(x)
    vae._split_attention = False
    full = vae._mid_attention(x)
    vae._split_attention = True
    d = (split.float() - full.float()).abs()
    print("split vs fp32 kernels: max", d.max().item(), "mean", d.mean().item())
    assert d.max() <= 6e-2 and d.mean() <= 3e-3, (d.max().item(), d.mean().item())
    out = vae.decode_video(lat.cuda(), frames_per_batch=2).cpu()
    print("decode vs oracle: max|d|", (out - ref).abs().max().item())
    torch.testing.assert_close(out, ref, rtol=0, atol=4e-2)


def oracle_full_resolution_frame():
    """The oracle's decode of frame 1 of the full-resolution test latent (64 x 64 latent -> one 512 x 512 frame, ~2.5 TFLOP of CPU work):
    tests/golden/oracle_cache/vae_decode_512x512_frame.pt (tests/oracle_cache.py)."""
    with torch.no_grad():
        return vae_ref.decode_latents(_sd(), hash_uniform("vae.lat512", (1, 4, 2, 64, 64), 1.0)[:, :, 1:2])


@pytest.mark.gpu
def test_hip_vae_full_resolution_frame():
    """One 512x512 frame (64x64 latent) in bf16: the size the sampler decodes (pipeline_pose2vid_long.py:112-125), against the ORACLE's decode of
    the same latent at the bf16 gate in all three forms of the GroupNorm -> SiLU -> conv legs -- only a full-resolution frame has `gnconv`
    tiles in the interior, on every edge and many tiles per workgroup, the statistics chain across its 12 launches and the two-launch
    256-wide split -- and through frame independence.  The 512-channel levels run as `groupnorm` + `conv3x3` in every form (csrc/rconv.hip
    serves the UNet's 320- and 1280-wide levels only)."""
    from tests.oracle_cache import cached
    from mmgt_amd.vae import AutoencoderKL
    vae = AutoencoderKL(device="cuda:0", dtype=torch.bfloat16)
    vae.load_state_dict(_sd("cuda:0"))
    lat = hash_uniform("vae.lat512", (1, 4, 2, 64, 64), 1.0).cuda()
    both = vae.decode_video(lat, frames_per_batch=2)
    single = vae.decode_video(lat[:, :, 1:2].contiguous(), frames_per_batch=1)
    assert both.shape == (1, 3, 2, 512, 512) and torch.isfinite(both).all()
    ref = cached("vae_decode_512x512_frame", oracle_full_resolution_frame)
    assert ref.shape == (1, 3, 1, 512, 512)
    for name, got in (("two frames", both[:, :, 1:2]), ("one frame", single)):
        d = (got.cpu() - ref).abs()
        print(f"512x512 VAE frame, {name}, vs oracle: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e}")
        torch.testing.assert_close(got.cpu(), ref, rtol=0, atol=4e-2)
        assert d.mean() <= 4e-3
    # A frame's pixels do not depend on its batch mates beyond bf16 rounding: the GEMM dispatcher may pick another tile for M = 1
    # frame than for 2 (gemm16 adds the bias in fp32 as the accumulator's start, the 32x32 tiles as a bf16 head + tail), so the
    # comparison is at the rounding level of a 30-layer bf16 decoder, not bitwise.  Measured: max 2.1e-2, mean 2.0e-3 (1.7e-3 with the
    # mid-block attention on the fp32 kernels, `_split_attention = False`: its P V and output projection are bf16 GEMMs now).
    d = (both[:, :, 1:2] - single).abs()
    assert d.max() <= 5e-2 and d.mean() <= 3e-3, (d.max().item(), d.mean().item())
    # ... and at this size the three forms of the GroupNorm -> SiLU -> conv legs (two launches / fused behind a statistics pass / statistics
    # from the producing launch, the default) agree at the same level: the fused launches work on 16 x 16 pixel tiles with halos, so only a
    # full-resolution frame exercises tiles in the interior, on every edge and many tiles per workgroup
    from mmgt_amd import hip
    try:
        hip.tune("gnconv", 0)
        two = vae.decode_video(lat, frames_per_batch=2)
        hip.tune("gnconv", 1)
        one = vae.decode_video(lat, frames_per_batch=2)
    finally:
        hip.tune("gnconv", 2)
    for other in (two, one):
        d = (both - other).abs()
        assert d.max() <= 5e-2 and d.mean() <= 3e-3, (d.max().item(), d.mean().item())
        torch.testing.assert_close(other[:, :, 1:2].cpu(), ref, rtol=0, atol=4e-2)          # each form against the oracle, not only against each other
    assert torch.equal(both, vae.decode_video(lat, frames_per_batch=2))                      # repeatable


def oracle_rectangular_frame():
    """The oracle's decode of one 40 x 24 latent (a 320 x 192 px frame) and the two scalars of its CPU-bf16 floor, max and mean of |decode with
    bf16 weights and activations - fp32 decode|: tests/golden/oracle_cache/vae_decode_320x192_frame.pt."""
    from tests import geometry_cases as gx
    sd = _sd()
    lat = hash_uniform("vae.lat_rect", (1, 4, 1) + gx.VAE_RECT, 1.0)
    with torch.no_grad():
        ref = vae_ref.decode_latents(sd, lat)
        low = vae_ref.decode_latents({k: v.bfloat16() for k, v in sd.items()}, lat.bfloat16()).float()
    floor = (low - ref).abs()
    return {"ref": ref, "floor_max": floor.max(), "floor_mean": floor.mean()}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_hip_vae_rectangular_frame_320x192(dtype):
    """A 40 x 24 latent -> 320 x 192 px: rows and columns differ at every level, the mid-block attention has 960 tokens (no multiple of 256: the
    fp32 kernels in both modes) and the fused GroupNorm -> SiLU -> conv legs are off at the 40 x 24 level's sides and on from 160 x 96 up.
    fp32 mode at the file's parity tolerance; bf16 mode within 1.5x the CPU-bf16 floor of the same oracle, with the fused launches counted."""
    from mmgt_amd import hip
    from mmgt_amd.vae import AutoencoderKL
    from tests import geometry_cases as gx
    from tests.oracle_cache import cached
    o = cached("vae_decode_320x192_frame", oracle_rectangular_frame)
    ref, fmax, fmean = o["ref"], o["floor_max"].item(), o["floor_mean"].item()
    h, w = gx.VAE_RECT
    assert ref.shape == (1, 3, 1, 8 * h, 8 * w)
    vae = AutoencoderKL(device="cuda:0", dtype=dtype)
    vae.load_state_dict(_sd("cuda:0"))
    lat = hash_uniform("vae.lat_rect", (1, 4, 1, h, w), 1.0).cuda()
    n0 = hip.call_count("mmgt_gn_silu_conv3x3")
    out = vae.decode_video(lat, frames_per_batch=1).cpu()
    launches = hip.call_count("mmgt_gn_silu_conv3x3") - n0
    d = (out - ref).abs()
    print(f"320x192 VAE frame, {dtype}: max|d| {d.max().item():.3e} mean|d| {d.mean().item():.3e} (CPU-bf16 floor {fmax:.3e} / {fmean:.3e}); "
          f"{launches} fused launches")
    assert out.shape == ref.shape and torch.isfinite(out).all()
    if dtype == torch.float32:
        assert launches == 0
        torch.testing.assert_close(out, ref, rtol=1e-3, atol=1e-4)
    else:
        assert launches == gx.vae_gnconv_launches(h, w) == 17
        assert d.max() <= 1.5 * fmax and d.mean() <= 1.5 * fmean


@pytest.mark.gpu
def test_hip_vae_never_runs_the_unet_fused_leg():
    """csrc/rconv.hip cuts its output into blocks of 320 / 256 / 160 channels of a multiple of 160: the decoder's 512- and 256-wide convs are
    not among them, so the VAE holds no image for that launch and a full-resolution decode never calls it."""
    from mmgt_amd import hip
    from mmgt_amd.vae import AutoencoderKL
    vae = AutoencoderKL(device="cuda:0", dtype=torch.bfloat16)
    vae.load_state_dict(_sd("cuda:0", encoder=True))
    assert not any(k.endswith(".rimg") for k in vae.w)
    n0 = hip.call_count("mmgt_gn_silu_conv3x3_unet")
    out = vae.decode_video(hash_uniform("vae.lat512", (1, 4, 2, 64, 64), 1.0).cuda()[:, :, 1:2].contiguous(), frames_per_batch=1)
    assert out.shape == (1, 3, 1, 512, 512) and torch.isfinite(out).all()
    assert hip.call_count("mmgt_gn_silu_conv3x3_unet") == n0


def test_oracle_vae_encoder_known_answers():
    """Shapes; the high-side-only padding of the downsamplers (an impulse in the LAST row/column reaches the output, one
    in front of the FIRST does not exist); zero weights -> mean == quant_conv.bias[:4]."""
    import torch.nn.functional as F
    sd = _sd(encoder=True)
    x = hash_uniform("vae.img", (2, 3, 32, 32), 1.0)
    with torch.no_grad():
        m = vae_ref.vae_encode_mean(sd, x)
    assert m.shape == (2, 4, 4, 4) and torch.isfinite(m).all()
    w = torch.zeros(1, 1, 3, 3)
    w[0, 0, 0, 0] = 1.0                                               # tap (ky, kx) = (0, 0) picks in[2y][2x]
    img = torch.arange(16.0).view(1, 1, 4, 4)
    out = F.conv2d(F.pad(img, (0, 1, 0, 1)), w, stride=2)
    torch.testing.assert_close(out, img[:, :, ::2, ::2])
    sdz = {k: torch.zeros_like(v) for k, v in sd.items()}
    sdz["quant_conv.bias"] = torch.arange(8.0)
    with torch.no_grad():
        mz = vae_ref.vae_encode_mean(sdz, x)
    torch.testing.assert_close(mz, torch.arange(4.0).view(1, 4, 1, 1).expand_as(mz))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol", [(torch.float32, dict(rtol=1e-3, atol=1e-4)), (torch.bfloat16, dict(rtol=0, atol=6e-2))])
def test_hip_vae_encoder_matches_oracle(dtype, tol):
    from mmgt_amd.vae import AutoencoderKL
    sd = _sd(encoder=True)
    x = hash_uniform("vae.img", (2, 3, 128, 64), 1.0)                 # non-square; 16 x 8 = 128 mid-block tokens
    with torch.no_grad():
        ref = vae_ref.vae_encode_mean(sd, x)
    vae = AutoencoderKL(device="cuda:0", dtype=dtype)
    vae.load_state_dict(sd)
    out = vae.encode_mean(x.cuda()).cpu()
    assert out.shape == ref.shape == (2, 4, 16, 8)
    print(dtype, "max|d|", (out - ref).abs().max().item(), "mean|ref|", ref.abs().mean().item())
    torch.testing.assert_close(out, ref, **tol)


@pytest.mark.gpu
def test_hip_conv_high_side_padding():
    """The stride-2 conv with padding after the last row / column only, against F.pad + conv2d, odd and even sizes."""
    import math
    import torch.nn.functional as F
    from mmgt_amd import hip
    from mmgt_amd.packing import pack_conv3x3
    for hw in (8, 6, 10):
        x = hash_uniform(f"dn.x{hw}", (3, 64, hw, hw + 2), 1.0)
        w = hash_uniform("dn.w", (128, 64, 3, 3), 1.0 / math.sqrt(9 * 64))
        b = hash_uniform("dn.b", (128,), 0.5)
        ref = F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), w.double(), b.double(), stride=2)
        out = hip.conv3x3(x.permute(0, 2, 3, 1).contiguous().cuda(), pack_conv3x3(w).cuda(), b.cuda(), stride=2,
                          pad_high_only=True)
        torch.testing.assert_close(out.double().cpu(), ref.permute(0, 2, 3, 1), rtol=1e-3, atol=1e-4)


def test_vae_without_encoder_weights_raises():
    from mmgt_amd.vae import AutoencoderKL
    vae = AutoencoderKL.__new__(AutoencoderKL)
    vae._has_encoder = False
    with pytest.raises(RuntimeError, match="encoder weights"):
        vae.encode_nhwc(None)
