"""CPU restatement of the reference's WavLM forward (data/wavlm/WavLM.py, modules_wavlm.py: extract_features in eval mode, layer_norm
extractor, pre-LN encoder, gated relative-position bias) and of its post-processing (data/audio_extraction/wavlm_features.py:128-145),
functional over a state dict.  Pinned against tests/golden/wavlm*.npz, which the reference's own classes produced; the tests then use
it as the fp64 / fp32 yardstick of the HIP model where no golden exists."""
import math

import torch
import torch.nn.functional as F

from mmgt_amd.wavlm import relative_position_buckets


def _ln(x, g, b, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), g.to(x.dtype), b.to(x.dtype), eps)


def conv_features(sd, cfg, source):
    """(B, samples) -> (B, T, 512): the 7 convs, each + LayerNorm(512) over channels + GELU (extractor_mode="layer_norm")."""
    x = source[:, None]
    for i, (dim, k, st) in enumerate(eval(cfg.conv_feature_layers)):
        p = f"feature_extractor.conv_layers.{i}."
        x = F.conv1d(x, sd[p + "0.weight"].to(x.dtype), sd.get(p + "0.bias"), stride=st)
        x = _ln(x.transpose(1, 2), sd[p + "2.1.weight"], sd[p + "2.1.bias"]).transpose(1, 2)
        x = F.gelu(x)
    return x.transpose(1, 2)


def relpos_gate(sd, layer, ln_x, heads):
    """gate (B, H, T, 1) of modules_wavlm.py:517-525 from the layer's LayerNorm output (B, T, C)."""
    p = f"encoder.layers.{layer}.self_attn."
    B, T, C = ln_x.shape
    ql = ln_x.view(B, T, heads, C // heads).permute(0, 2, 1, 3)
    g = F.linear(ql, sd[p + "grep_linear.weight"].to(ln_x.dtype), sd[p + "grep_linear.bias"].to(ln_x.dtype))
    ga, gb = torch.sigmoid(g.view(B, heads, T, 2, 4).sum(-1)).chunk(2, dim=-1)
    return ga * (gb * sd[p + "grep_a"].to(ln_x.dtype) - 1.0) + 2.0


def position_bias(sd, cfg, T, dtype=torch.float32):
    """(H, T, T) raw bias of layer 0 (compute_bias)."""
    off = relative_position_buckets(T, cfg.num_buckets, cfg.max_distance)            # bucket of offset j - i, index j - i + T - 1
    idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + (T - 1)
    return sd["encoder.layers.0.self_attn.relative_attention_bias.weight"].to(dtype)[off[idx]].permute(2, 0, 1)


def attention(q, k, v, gate, bias, heads):
    """softmax(q k^T / sqrt(d) + gate * bias) v over (B, T, C) projections; bias (H, T, T), gate (B, H, T, 1)."""
    B, T, C = q.shape
    hd = C // heads
    sp = lambda t: t.view(B, T, heads, hd).transpose(1, 2)
    s = (sp(q) * hd ** -0.5) @ sp(k).transpose(-1, -2) + gate * bias[None]
    return (torch.softmax(s, dim=-1) @ sp(v)).transpose(1, 2).reshape(B, T, C)


def extract_features(sd, cfg, source, bias_scale=1.0, return_features=False):
    """WavLM.extract_features(source)[0]: (B, T, C).  bias_scale multiplies the relative-position table (0: bias off)."""
    heads, L = cfg.encoder_attention_heads, cfg.encoder_layers
    dt = source.dtype
    feats = _ln(conv_features(sd, cfg, source), sd["layer_norm.weight"], sd["layer_norm.bias"])
    feats = F.linear(feats, sd["post_extract_proj.weight"].to(dt), sd["post_extract_proj.bias"].to(dt))
    pre = "encoder.pos_conv.0."
    g = sd.get(pre + "weight_g", sd.get(pre + "parametrizations.weight.original0"))
    v = sd.get(pre + "weight_v", sd.get(pre + "parametrizations.weight.original1"))
    w = (g * v / v.norm(dim=(0, 1), keepdim=True)).to(dt)
    xc = F.conv1d(feats.transpose(1, 2), w, sd[pre + "bias"].to(dt), padding=cfg.conv_pos // 2, groups=cfg.conv_pos_groups)
    x = feats + F.gelu(xc[:, :, :-1] if cfg.conv_pos % 2 == 0 else xc).transpose(1, 2)
    T = x.shape[1]
    bias = position_bias(sd, cfg, T, dt) * bias_scale
    for i in range(L):
        p = f"encoder.layers.{i}."
        a = p + "self_attn."
        h = _ln(x, sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"])
        q, k, vv = (F.linear(h, sd[a + f"{n}_proj.weight"].to(dt), sd[a + f"{n}_proj.bias"].to(dt)) for n in ("q", "k", "v"))
        o = attention(q, k, vv, relpos_gate(sd, i, h, heads), bias, heads)
        x = x + F.linear(o, sd[a + "out_proj.weight"].to(dt), sd[a + "out_proj.bias"].to(dt))
        h = _ln(x, sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"])
        h = F.gelu(F.linear(h, sd[p + "fc1.weight"].to(dt), sd[p + "fc1.bias"].to(dt)).float()).to(dt)
        x = x + F.linear(h, sd[p + "fc2.weight"].to(dt), sd[p + "fc2.bias"].to(dt))
    x = _ln(x, sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"])
    return (x, feats) if return_features else x


def post_process(x):
    """extract_wo_init's tail (wavlm_features.py:138-145) per slice: append the last row, linear interpolation (align_corners=True) to
    ceil((T + 1) / 2) rows.  (B, T, C) -> (B, ceil((T + 1) / 2), C)."""
    x = torch.cat((x, x[:, -1:]), dim=1)
    return F.interpolate(x.transpose(1, 2), size=math.ceil(x.shape[1] / 2), align_corners=True, mode="linear").transpose(1, 2)


def normalize(waves):
    """cfg.normalize: F.layer_norm over each whole slice (wavlm_features.py:134-135)."""
    return torch.stack([F.layer_norm(w[None], (1, w.shape[0]))[0] for w in waves])
