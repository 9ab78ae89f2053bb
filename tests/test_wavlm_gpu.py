"""WavLM-Large on the MI355X (mmgt_amd/wavlm.py, csrc/wavlm.hip): mmgt_relpos_attention against an fp64 restatement, the model against
the reference's goldens (tests/golden/wavlm*.npz) in both storage modes, batch == alone, and audio2vid --wavlm."""
import json
import math
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from tests import wavlm_cases as wc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"


def _attn_case(B, H, T, seed=0):
    """q|k|v rows as the q|k|v GEMM writes them (B*T, 3*H*64), the LN rows x, grep weights, and a bias table with +-30 planted on the
    bucket boundaries in half of the heads (a wrong offset moves those by far), O(1) in the others (where the gate moves the
    softmax); gate inputs reach both sigmoid ends."""
    from mmgt_amd.wavlm import relative_position_buckets
    g = torch.Generator().manual_seed(seed + 1000 * T + B)
    C = H * 64
    qkv = torch.randn((B * T, 3 * C), generator=g) * 0.6
    x = torch.randn((B * T, C), generator=g)
    gw = torch.randn((8, 64), generator=g) * 0.2
    gb = torch.randn((8,), generator=g)
    ga = 1.0 + torch.rand((H,), generator=g)
    emb = torch.randn((320, H), generator=g) * 2.0
    bk = relative_position_buckets(T, 320, 800)
    edges = torch.nonzero(bk[1:] != bk[:-1]).flatten()
    planted = 30.0 * torch.sign(torch.randn((edges.numel(), H // 2), generator=g))
    emb[bk[edges], :H // 2] = planted                                       # heads 0 .. H/2-1: +-30 on the bucket boundaries
    tab = emb[bk].t().contiguous()
    return qkv, x, gw, gb, ga, tab


def _attn_ref64(qkv, x, gw, gb, ga, tab, B, H, T, no_gate=False, shift=0):
    C = H * 64
    d = lambda t: t.double()
    q, k, v = (d(qkv[:, i * C:(i + 1) * C]).view(B, T, H, 64).transpose(1, 2) for i in range(3))
    xl = d(x).view(B, T, H, 64).transpose(1, 2)
    s8 = xl @ d(gw).t() + d(gb)
    a, c = torch.sigmoid(s8.view(B, H, T, 2, 4).sum(-1)).unbind(-1)
    gate = a * (c * d(ga).view(1, H, 1) - 1.0) + 2.0
    if no_gate:
        gate = torch.ones_like(gate)
    idx = (torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1 + shift).clamp(0, 2 * T - 2)
    bias = d(tab)[:, idx]                                                   # (H, T, T)
    s = q @ k.transpose(-1, -2) / 8.0 + gate[..., None] * bias[None]
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * T, C)


def _run_attn(qkv, x, gw, gb, ga, tab, B, H, T, dtype, out=None):
    from mmgt_amd import hip
    C = H * 64
    qd, xd = qkv.to(DEV, dtype).contiguous(), x.to(DEV, dtype).contiguous()
    if out is None:
        out = torch.full((B * T, C), float("nan"), device=DEV, dtype=dtype)
    st3, st1 = (T * 3 * C, 3 * C), (T * C, C)
    f = lambda t: t.to(DEV, torch.float32).contiguous()
    hip.relpos_attention(qd, qd[:, C:], qd[:, 2 * C:], out, xd, f(gw), f(gb), f(ga), f(tab), batch=B, heads=H, T=T, scale=0.125,
                         q_str=st3, k_str=st3, v_str=st3, o_str=st1, x_str=st1)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T", [1, 17, 64, 159, 1500])
@pytest.mark.parametrize("B", [1, 3])
def test_relpos_attention_matches_fp64(B, T):
    H = 16
    case = _attn_case(B, H, T)
    ref = _attn_ref64(*case, B, H, T)
    o32 = _run_attn(*case, B, H, T, torch.float32).cpu().double()
    torch.testing.assert_close(o32, ref, rtol=1e-5, atol=1e-5 * ref.abs().max().item())
    # bf16 mode: against the fp64 restatement of the bf16-rounded inputs; one bf16 ulp of the output plus the rounding of the probabilities
    # to bf16 for the P.V product (relative 2^-9 each, bounded by max |v|) and the fp32 accumulation
    c16 = [t.to(torch.bfloat16).float() if i < 2 else t for i, t in enumerate(case)]
    ref16 = _attn_ref64(*c16, B, H, T)
    o16 = _run_attn(*case, B, H, T, torch.bfloat16).cpu().double()
    vmax = c16[0][:, 2 * H * 64:].abs().max().item()
    bound = 2.0 ** -8 * ref16.abs() + 2.0 ** -8 * vmax + 1e-6
    assert torch.isfinite(o16).all() and ((o16 - ref16).abs() <= bound).all(), ((o16 - ref16).abs() - bound).max()
    # a missing gate or a shifted offset is far outside that bound
    if T > 1:
        for bad in (_attn_ref64(*case, B, H, T, no_gate=True), _attn_ref64(*case, B, H, T, shift=1)):
            assert (bad - ref).abs().max() > 100 * 1e-5 * ref.abs().max()


def test_relpos_attention_runs_are_bitwise_equal():
    B, H, T = 2, 16, 159
    case = _attn_case(B, H, T, seed=7)
    for dtype in (torch.float32, torch.bfloat16):
        first = _run_attn(*case, B, H, T, dtype).clone()
        assert torch.isfinite(first).all()
        for _ in range(9):
            assert torch.equal(_run_attn(*case, B, H, T, dtype), first)


def test_relpos_attention_refuses_bad_shapes():
    from mmgt_amd import hip
    case = _attn_case(1, 16, 17)
    with pytest.raises(RuntimeError, match="head_dim"):
        qd = case[0].to(DEV).contiguous()
        out = torch.empty((17, 1024), device=DEV)
        f = lambda t: t.to(DEV, torch.float32).contiguous()
        hip.relpos_attention(qd, qd, qd, out, case[1].to(DEV), f(case[2]), f(case[3]), f(case[4]), f(case[5]), batch=1, heads=16, T=17,
                             scale=0.125, q_str=(0, 3072), k_str=(0, 3072), v_str=(0, 3072), o_str=(0, 1024), x_str=(0, 1024), hd=80)
    T = 4097
    with pytest.raises(RuntimeError, match="sequence length"):
        qd = torch.zeros((T, 3 * 1024), device=DEV)
        f = lambda t: t.to(DEV, torch.float32).contiguous()
        hip.relpos_attention(qd, qd, qd, torch.empty((T, 1024), device=DEV), torch.zeros((T, 1024), device=DEV), f(case[2]), f(case[3]),
                             f(case[4]), torch.zeros((16, 2 * T - 1), device=DEV), batch=1, heads=16, T=T, scale=0.125, q_str=(0, 3072),
                             k_str=(0, 3072), v_str=(0, 3072), o_str=(0, 1024), x_str=(0, 1024))


def _model(cfg_dict, dtype):
    from mmgt_amd.wavlm import WavLM, WavLMConfig, wavlm_spec
    cfg = WavLMConfig(cfg_dict)
    m = WavLM(cfg, device=DEV, dtype=dtype)
    m.load_state_dict(wc.wavlm_state_dict(wavlm_spec(cfg)))
    return m


def test_wavlm_tiny_matches_reference_golden():
    gold = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "wavlm_tiny.npz")).items()}
    from tests import wavlm_ref as R
    waves = R.normalize(wc.wavlm_waves(2, wc.TINY_SAMPLES, tag="tiny")).to(DEV)
    m = _model(wc.TINY, torch.float32)
    torch.testing.assert_close(m.conv_features(waves).cpu(), gold["features"], rtol=1e-3, atol=1e-4)
    x, pm = m.extract_features(waves)
    assert pm is None
    torch.testing.assert_close(x.cpu(), gold["x"], rtol=1e-3, atol=2e-4)


def test_wavlm_large_matches_reference_golden_fp32_and_bf16():
    gold = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "wavlm.npz")).items()}
    from tests import wavlm_ref as R
    raw = wc.wavlm_waves(2, wc.SLICE_SAMPLES)
    waves = R.normalize(raw).to(DEV)
    XC, FC = wc.X_COLS, wc.FEAT_COLS
    m = _model(None, torch.float32)
    torch.testing.assert_close(m.conv_features(waves)[..., FC].cpu(), gold["features"], rtol=1e-3, atol=1e-4)
    x, _ = m.extract_features(waves)
    assert x.shape == (2, 159, 1024)
    torch.testing.assert_close(x[..., XC].cpu(), gold["x"], rtol=1e-3, atol=2e-4)
    post = m.slice_features(raw.to(DEV))
    assert post.shape == (2, 80, 1024)
    torch.testing.assert_close(post[..., XC].cpu(), gold["post"], rtol=1e-3, atol=2e-4)
    del m
    m16 = _model(None, torch.bfloat16)
    x16, _ = m16.extract_features(waves)
    p16 = m16.slice_features(raw.to(DEV))
    for out, ref, floor in ((x16, gold["x"], gold["x_bf16_floor"]), (p16, gold["post"], gold["post_bf16_floor"])):
        d = (out[..., XC].cpu() - ref).abs()
        print(f"wavlm bf16: max|d| {d.max().item():.3e} mean {d.mean().item():.3e}; CPU-bf16 floor max {floor[1]:.3e} mean {floor[0]:.3e}")
        assert torch.isfinite(out).all() and d.mean() <= 1.5 * floor[0] and d.max() <= 1.5 * floor[1]


def test_slice_features_batched_equals_alone():
    raw = wc.wavlm_waves(3, wc.SLICE_SAMPLES, tag="batch").to(DEV)
    for dtype in (torch.bfloat16, torch.float32):
        m = _model(None, dtype)
        both = m.slice_features(raw)
        for i in range(3):
            assert torch.equal(m.slice_features(raw[i:i + 1])[0], both[i])
        del m


def test_wavlm_extract_features_refuses_unbuilt_options():
    m = _model(wc.TINY, torch.float32)
    w = torch.zeros((1, wc.TINY_SAMPLES), device=DEV)
    with pytest.raises(NotImplementedError):
        m.extract_features(w, padding_mask=torch.zeros((1, wc.TINY_SAMPLES), dtype=torch.bool, device=DEV))
    with pytest.raises(NotImplementedError):
        m.extract_features(w, output_layer=3)


def _a2v(tmp_path, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "audio2vid.py"), "--synthetic", "-W", "64", "-H", "64", "-L", "80",
                        "--steps", "2", "--out_dir", str(tmp_path), *args], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_audio2vid_with_wavlm_random(tmp_path):
    """--wavlm random on a 10-s wav: 2 slices (the first window skipped), wavlm_s reported, cond columns 0:1024 = slice_features of the
    slices the script ran; without --wavlm the script's output is what it was."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from mmgt_amd.synthetic import synth_state_dict
    from mmgt_amd.wavlm import WavLM, WavLMConfig, audio_slices, wavlm_spec
    t = np.arange(160000) / 16000.0
    pcm = ((0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 3.1 * t) * np.sin(2 * np.pi * 880 * t)) * 32767).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    rec = _a2v(tmp_path, "--audio_path", str(tmp_path / "a.wav"), "--wavlm", "random", "--save_cond", str(tmp_path / "cond.npy"))
    assert rec["slices"] == 1 and rec["wavlm_slices"] == 2 and rec["wavlm"] == "random" and rec["wavlm_s"] > 0 and rec["baseline_feats"] == "hash"
    cond = torch.from_numpy(np.load(tmp_path / "cond.npy"))
    from audio2vid import read_wav_16k
    slices = audio_slices(read_wav_16k(str(tmp_path / "a.wav")))
    assert slices.shape == (2, 51200)
    m = WavLM(WavLMConfig(), device=DEV, dtype=torch.bfloat16)
    m.load_state_dict(synth_state_dict(wavlm_spec(), prefix="wavlm.", device=DEV))
    feats = m.slice_features(slices.to(DEV)).cpu()
    assert torch.isfinite(feats).all() and torch.equal(cond[:, :, :1024], feats[:1])
    del m
    # 160 frames need both slices; the baseline columns from a file
    bf = np.random.default_rng(0).standard_normal((2, 80, 35)).astype(np.float32)
    np.save(tmp_path / "bf.npy", bf)
    rec2 = _a2v(tmp_path, "--audio_path", str(tmp_path / "a.wav"), "--wavlm", "random", "-L", "160", "--baseline_feats", str(tmp_path / "bf.npy"),
                "--save_cond", str(tmp_path / "cond2.npy"))
    assert rec2["slices"] == 2 and rec2["baseline_feats"] == str(tmp_path / "bf.npy")
    cond2 = np.load(tmp_path / "cond2.npy")
    assert np.array_equal(cond2[:, :, 1024:], bf) and np.array_equal(cond2[:1, :, :1024], cond[:, :, :1024].numpy())
    # without --wavlm: today's output, key for key and frame for frame
    off = _a2v(tmp_path, "--audio_path", str(tmp_path / "a.wav"), "--save_cond", str(tmp_path / "cond_off.npy"))
    assert "wavlm_s" not in off and "wavlm" not in off
    from mmgt_amd.synthetic import hash_uniform
    assert np.array_equal(np.load(tmp_path / "cond_off.npy"), hash_uniform("a2v.wavlm+baseline", (1, 80, 1059), 1.0).numpy())
