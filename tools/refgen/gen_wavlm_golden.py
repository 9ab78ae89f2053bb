"""Generate tests/golden/wavlm_keys.json, wavlm.npz and wavlm_tiny.npz by running the REFERENCE's `WavLM` (data/wavlm/WavLM.py +
modules_wavlm.py) on CPU, with the hash-seeded weights and waveforms of tests/wavlm_cases.py.  The reference's extract_wo_init
post-processing (data/audio_extraction/wavlm_features.py:128-145) hard-codes cuda:0, so it is restated here on CPU, line for line.
Only key names / shapes, outputs (column subsets of the Large ones), the CPU-bf16 floor and the bucket tables are stored.

    python tools/refgen/gen_wavlm_golden.py"""
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, "/root/reference/data/wavlm")
sys.dont_write_bytecode = True
from tests import wavlm_cases as wc  # noqa: E402

from WavLM import WavLM, WavLMConfig  # noqa: E402  (the reference's classes)
from modules_wavlm import MultiheadAttention  # noqa: E402

torch.manual_seed(0)
GOLD = os.path.join(ROOT, "tests", "golden")


def extract_wo_init(model, cfg, wav):
    """wavlm_features.py:128-145 for one (samples,) slice, on CPU."""
    wav_input_16khz = wav.unsqueeze(0)
    if cfg.normalize:
        wav_input_16khz = torch.nn.functional.layer_norm(wav_input_16khz, wav_input_16khz.shape)
    wavlm_feats = model.extract_features(wav_input_16khz)[0]
    x = wavlm_feats.detach().float()
    last_feature = wavlm_feats[:, -1, :].unsqueeze(1)
    wavlm_feats = torch.cat((wavlm_feats, last_feature), dim=1)
    wavlm_feats = F.interpolate(wavlm_feats.transpose(1, 2), size=math.ceil(wavlm_feats.shape[1] / 2), align_corners=True,
                                mode='linear').transpose(1, 2).squeeze(0)
    return x[0], wavlm_feats.float()


def run(cfg_dict, waves, bias_scale=4.0, keys_out=None):
    cfg = WavLMConfig(cfg_dict)
    m = WavLM(cfg).eval()
    keys = {k: list(v.shape) for k, v in m.state_dict().items()}
    if keys_out:
        json.dump(keys, open(keys_out, "w"), indent=0)
    sd = wc.wavlm_state_dict(keys, bias_scale=bias_scale)
    m.load_state_dict(sd, strict=True)
    out = {}
    with torch.no_grad():
        for dt in (torch.float32, torch.bfloat16):
            mm = m.to(dt)
            xs, posts, feats = [], [], []
            for w in waves:
                x, post = extract_wo_init(mm, cfg, w.to(dt))
                xs.append(x)
                posts.append(post)
                feats.append(mm.extract_features(torch.nn.functional.layer_norm(w[None].to(dt), (1, w.shape[0])), ret_conv=True)[0][0].float())
            out[dt] = (torch.stack(feats), torch.stack(xs), torch.stack(posts))
            if dt == torch.float32:
                m = m.float()
    return keys, out


# ---- Large, two 3.2-s slices
waves = wc.wavlm_waves(2, wc.SLICE_SAMPLES)
keys, out = run(wc.LARGE, waves, keys_out=os.path.join(GOLD, "wavlm_keys.json"))
feats, x, post = out[torch.float32]
_, x16, post16 = out[torch.bfloat16]
_, off = run(wc.LARGE, waves, bias_scale=0.0)
d_off = (off[torch.float32][1] - x).abs()
print(f"Large: x {tuple(x.shape)} mean|x| {x.abs().mean():.3f}; bias off moves x by max {d_off.max():.3e} mean {d_off.mean():.3e}")
assert d_off.mean() > 1e-2 and d_off.max() > 0.1, "the relative-position bias does not matter enough at these scales"
XC, FC = wc.X_COLS, wc.FEAT_COLS
fx = (x16[..., XC] - x[..., XC]).abs()
fp = (post16[..., XC] - post[..., XC]).abs()
print(f"Large bf16 floor: x max {fx.max():.3e} mean {fx.mean():.3e}; post max {fp.max():.3e} mean {fp.mean():.3e}")
res = {"features": feats[..., FC].numpy(), "x": x[..., XC].numpy(), "post": post[..., XC].numpy(),
       "x_bf16_floor": np.array([fx.mean().item(), fx.max().item()], np.float32),
       "post_bf16_floor": np.array([fp.mean().item(), fp.max().item()], np.float32)}
# bucket tables of the reference's _relative_positions_bucket, by offset j - i = -(T-1) .. T-1
for T, md in wc.BUCKET_POINTS:
    mha = MultiheadAttention(64, 1, self_attention=True, has_relative_attention_bias=True, num_buckets=320, max_distance=md)
    rp = torch.arange(T)[None, :] - torch.arange(T)[:, None]
    full = mha._relative_positions_bucket(rp, bidirectional=True)
    tab = torch.cat([full[T - 1, :], full[0, 1:]])
    idx = rp + T - 1
    assert torch.equal(tab[idx], full)
    res[f"buckets_T{T}_md{md}"] = tab.to(torch.int16).numpy()
path = os.path.join(GOLD, "wavlm.npz")
np.savez_compressed(path, **res)
print("wrote", path, os.path.getsize(path), "B;", len(keys), "keys,", sum(int(np.prod(s)) for s in keys.values()), "parameters")

# ---- tiny: 2 layers, 256 wide, 4 heads, 37 frames
tw = wc.wavlm_waves(2, wc.TINY_SAMPLES, tag="tiny")
tkeys, tout = run(wc.TINY, tw)
tf, tx, tp = tout[torch.float32]
_, tx16, tp16 = tout[torch.bfloat16]
ft = (tx16 - tx).abs()
res = {"features": tf.numpy(), "x": tx.numpy(), "post": tp.numpy(), "x_bf16_floor": np.array([ft.mean().item(), ft.max().item()], np.float32)}
path = os.path.join(GOLD, "wavlm_tiny.npz")
np.savez_compressed(path, **res)
print("wrote", path, os.path.getsize(path), "B;", tuple(tx.shape), f"mean|x| {tx.abs().mean():.3f}")
