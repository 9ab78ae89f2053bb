"""Configurations, weights and waveforms of the WavLM parity cases, shared by tools/refgen/gen_wavlm_golden.py (which runs the reference's
WavLM) and tests/test_wavlm*.py: pure functions of names via mmgt_amd/synthetic.py."""

SLICE_SAMPLES = 51200           # one 3.2-s slice at 16 kHz -> 159 frames
TINY_SAMPLES = 400 + 320 * 36   # 11920 samples -> 37 frames (ragged: no multiple of any tile)

# WavLM-Large (the published checkpoint's cfg as far as it is known; see mmgt_amd/wavlm.py)
LARGE = dict(extractor_mode="layer_norm", encoder_layers=24, encoder_embed_dim=1024, encoder_ffn_embed_dim=4096, encoder_attention_heads=16,
             layer_norm_first=True, normalize=True, relative_position_embedding=True, num_buckets=320, max_distance=800, gru_rel_pos=True,
             conv_bias=False)
TINY = dict(LARGE, encoder_layers=2, encoder_embed_dim=256, encoder_ffn_embed_dim=1024, encoder_attention_heads=4)

# the columns of the Large outputs the golden keeps (an fp32 (2, 159, 1024) tensor alone exceeds the size limit of a committed file)
FEAT_COLS = slice(0, 128)
X_COLS = slice(0, 256)

BUCKET_POINTS = ((159, 800), (159, 1280), (1500, 800), (1500, 1280))


def wavlm_state_dict(keys, device="cpu", bias_scale=4.0):
    """Hash-seeded weights for every key of the reference's WavLM.state_dict().  Matrices U(+- 1.5 / sqrt(fan_in)), norm gains
    1 +- 0.1, biases +- 0.05, the positional conv's weight-norm gain 2 +- 0.5, grep_linear U(+- 3 / sqrt(64)) and grep_a 1 +- 0.5 (gates spread over (1, 2.5)), and the relative-position embedding
    U(+- bias_scale): at torch's default init the bias moves WavLM-Large's output less than the bf16 noise, so the golden would not see it."""
    import math
    import torch
    from mmgt_amd.synthetic import hash_uniform
    sd = {}
    for k, shape in keys.items():
        shape = tuple(shape)
        name = "wavlm." + k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        if k.endswith("original0") or k.endswith("weight_g"):
            sd[k] = 2.0 + hash_uniform(name, shape, 0.5, device)
        elif k.endswith("relative_attention_bias.weight"):
            sd[k] = hash_uniform(name, shape, bias_scale, device)
        elif k.endswith("grep_a"):
            sd[k] = 1.0 + hash_uniform(name, shape, 0.5, device)
        elif k == "mask_emb":
            sd[k] = hash_uniform(name, shape, 1.0, device)
        elif len(shape) == 1 and "norm" in k and k.endswith("weight"):
            sd[k] = 1.0 + hash_uniform(name, shape, 0.1, device)
        elif len(shape) == 1:
            sd[k] = hash_uniform(name, shape, 0.05, device)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            gain = 3.0 if "grep_linear" in k else 1.5
            sd[k] = hash_uniform(name, shape, gain / math.sqrt(fan_in), device)
    return {k: v.to(torch.float32) for k, v in sd.items()}


def wavlm_waves(n, samples, tag="wave", device="cpu"):
    """(n, samples) waveforms: a hash-seeded signal with a slow envelope (so layer-norm-normalised slices still differ in level)."""
    import torch
    from mmgt_amd.synthetic import hash_uniform
    w = hash_uniform(f"wavlm.{tag}", (n, samples), 0.5, device)
    t = torch.arange(samples, dtype=torch.float32, device=device) / 16000.0
    env = 0.5 + 0.4 * torch.sin(2 * 3.141592653589793 * 3.0 * t)[None] * torch.arange(1, n + 1, dtype=torch.float32, device=device)[:, None] / n
    return (w * env).contiguous()
