"""WavLM-Large audio features on MI355X: the 1024 WavLM columns of audio2vid's SMGA pose conditioning.

The reference loads `WavLM(WavLMConfig(checkpoint["cfg"]))` from WavLM-Large.pt (its data/audio_extraction/wavlm_features.py:102-116,
`wavlm_init`) and, per 3.2-s slice of the driving audio, runs `extract_wo_init` (:118-147): layer-norm the whole slice, `extract_features`,
append a copy of the last frame, interpolate linearly (align_corners=True) to half as many frames -- (80, 1024) per 51 200-sample slice
(scripts/audio2vid.py:299-315 of the reference).  This module keeps the reference's state-dict key names (either weight-norm spelling of
encoder.pos_conv.0) and runs on the HIP kernels of libmmgt_hip.so:

  conv feature extractor  7 Conv1d layers (no bias) as GEMMs over strided views of the channels-last (T, 512) signal, each followed by
                          LayerNorm(512) over the channels and the exact GELU (extractor_mode="layer_norm")
  feature LayerNorm(512) -> post_extract_proj Linear(512, 1024)
  positional conv         Conv1d(1024, 1024, 128, padding 64, groups 16) + SamePad + GELU + residual: 16 GEMMs over strided views of the
                          group-major padded signal; the weight norm w = g v / |v| is folded once at load time
  24 pre-LN layers        LN -> q|k|v GEMM -> mmgt_relpos_attention (csrc/wavlm.hip: softmax(QK^T scale + gate * bias) V, the gate
                          computed in the kernel from the LN rows) -> out-proj + residual -> LN -> fc1 + GELU -> fc2 + residual
  encoder.layer_norm; the post-processing on mmgt_lerp_rows.

The relative-position buckets are computed on the host with the reference's own integer / float32 torch arithmetic
(`_relative_positions_bucket`, modules_wavlm.py:417-442) and cached per (T, num_buckets, max_distance); the (heads, 2T - 1) bias table
is gathered from layer 0's embedding once per forward and shared by all layers (WavLM.py:596-601).

Slices run through the model one after another, each with exactly the kernels a slice run alone takes (the GEMM's tile choice depends
on the row count), so a batch of slices equals the slices run one at a time bitwise.  Only the layer_norm extractor, pre-LN encoders with
the gated relative bias and bias-free convs are built (WavLM Large); other configurations raise NotImplementedError.
"""
import functools
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from . import hip

DEFAULT_CONV_LAYERS = "[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2"
SAMPLE_RATE = 16000


class WavLMConfig:
    """The reference's WavLMConfig field names (WavLM.py:162-219) with WavLM-Large defaults.  The Large values are the published
    checkpoint's cfg as documented, unverified against the checkpoint itself (the reference's own default max_distance is 1280): a
    checkpoint's cfg overrides every field.  Configurations the HIP path does not build raise NotImplementedError."""

    def __init__(self, cfg_dict=None):
        self.extractor_mode = "layer_norm"
        self.encoder_layers = 24
        self.encoder_embed_dim = 1024
        self.encoder_ffn_embed_dim = 4096
        self.encoder_attention_heads = 16
        self.activation_fn = "gelu"
        self.layer_norm_first = True
        self.conv_feature_layers = DEFAULT_CONV_LAYERS
        self.conv_bias = False
        self.feature_grad_mult = 1.0
        self.normalize = True
        self.dropout = 0.1
        self.attention_dropout = 0.1
        self.activation_dropout = 0.0
        self.encoder_layerdrop = 0.0
        self.dropout_input = 0.0
        self.dropout_features = 0.0
        self.mask_length = 10
        self.mask_prob = 0.65
        self.mask_selection = "static"
        self.mask_other = 0
        self.no_mask_overlap = False
        self.mask_min_space = 1
        self.mask_channel_length = 10
        self.mask_channel_prob = 0.0
        self.mask_channel_selection = "static"
        self.mask_channel_other = 0
        self.no_mask_channel_overlap = False
        self.mask_channel_min_space = 1
        self.conv_pos = 128
        self.conv_pos_groups = 16
        self.relative_position_embedding = True
        self.num_buckets = 320
        self.max_distance = 800
        self.gru_rel_pos = True
        if cfg_dict is not None:
            self.__dict__.update(dict(cfg_dict))
        self._validate()

    def _validate(self):
        def no(msg):
            raise NotImplementedError(f"WavLMConfig: {msg} is not built on the HIP path (WavLM-Large geometry only)")
        if self.extractor_mode != "layer_norm":
            no(f"extractor_mode={self.extractor_mode!r} (only 'layer_norm'; WavLM Base / Base+ use 'default')")
        if not self.layer_norm_first:
            no("a post-LN encoder (layer_norm_first=False)")
        if not self.relative_position_embedding:
            no("an encoder without relative position embedding")
        if not self.gru_rel_pos:
            no("an ungated relative position bias (gru_rel_pos=False)")
        if self.conv_bias:
            no("conv_bias=True")
        if self.activation_fn != "gelu":
            no(f"activation_fn={self.activation_fn!r}")
        if [tuple(c) for c in eval(self.conv_feature_layers)] != [tuple(c) for c in eval(DEFAULT_CONV_LAYERS)]:
            no(f"conv_feature_layers={self.conv_feature_layers!r}")
        C, H = self.encoder_embed_dim, self.encoder_attention_heads
        if H <= 0 or C % H or C // H != 64:
            no(f"head_dim {C / max(H, 1):g} (only 64)")
        if C % (8 * self.conv_pos_groups) or self.conv_pos % 2:
            no(f"the positional conv geometry (embed {C}, groups {self.conv_pos_groups}, kernel {self.conv_pos})")


@functools.lru_cache(maxsize=32)
def _buckets_cached(T, num_buckets, max_distance):
    # the reference's _relative_positions_bucket (modules_wavlm.py:417-442, bidirectional) over the offsets j - i = -(T-1) .. T-1,
    # in its own torch integer / float32 arithmetic (element-wise: the same bits as over the (T, T) matrix of compute_bias)
    relative_positions = torch.arange(-(T - 1), T, dtype=torch.long)
    num_buckets = num_buckets // 2
    relative_buckets = (relative_positions > 0).to(torch.long) * num_buckets
    relative_positions = torch.abs(relative_positions)
    max_exact = num_buckets // 2
    is_small = relative_positions < max_exact
    relative_postion_if_large = max_exact + (
        torch.log(relative_positions.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)
    ).to(torch.long)
    relative_postion_if_large = torch.min(relative_postion_if_large, torch.full_like(relative_postion_if_large, num_buckets - 1))
    relative_buckets += torch.where(is_small, relative_positions, relative_postion_if_large)
    return relative_buckets


def relative_position_buckets(T, num_buckets=320, max_distance=800):
    """(2T - 1,) int64: bucket of the offset j - i at index j - i + T - 1 (host, cached per (T, num_buckets, max_distance))."""
    return _buckets_cached(int(T), int(num_buckets), int(max_distance)).clone()


def wavlm_spec(cfg=None, weight_norm_keys="checkpoint"):
    """{key: shape} of the reference's WavLM(cfg).state_dict(), in its order.  weight_norm_keys: "checkpoint" (weight_g / weight_v of
    nn.utils.weight_norm, what WavLM-Large.pt holds) or "parametrized" (parametrizations.weight.original0/1)."""
    cfg = cfg or WavLMConfig()
    C, F_, H, L = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads, cfg.encoder_layers
    convs = eval(cfg.conv_feature_layers)
    s = OrderedDict()
    s["mask_emb"] = (C,)
    cin = 1
    for i, (dim, k, _st) in enumerate(convs):
        p = f"feature_extractor.conv_layers.{i}."
        s[p + "0.weight"] = (dim, cin, k)
        s[p + "2.1.weight"], s[p + "2.1.bias"] = (dim,), (dim,)
        cin = dim
    embed = convs[-1][0]
    if embed != C:
        s["post_extract_proj.weight"], s["post_extract_proj.bias"] = (C, embed), (C,)
    s["encoder.pos_conv.0.bias"] = (C,)
    g, v = ("weight_g", "weight_v") if weight_norm_keys == "checkpoint" else ("parametrizations.weight.original0", "parametrizations.weight.original1")
    s[f"encoder.pos_conv.0.{g}"] = (1, 1, cfg.conv_pos)
    s[f"encoder.pos_conv.0.{v}"] = (C, C // cfg.conv_pos_groups, cfg.conv_pos)
    for i in range(L):
        p = f"encoder.layers.{i}."
        s[p + "self_attn.grep_a"] = (1, H, 1, 1)
        if i == 0:
            s[p + "self_attn.relative_attention_bias.weight"] = (cfg.num_buckets, H)
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            s[p + f"self_attn.{n}.weight"], s[p + f"self_attn.{n}.bias"] = (C, C), (C,)
        s[p + "self_attn.grep_linear.weight"], s[p + "self_attn.grep_linear.bias"] = (8, C // H), (8,)
        s[p + "self_attn_layer_norm.weight"], s[p + "self_attn_layer_norm.bias"] = (C,), (C,)
        s[p + "fc1.weight"], s[p + "fc1.bias"] = (F_, C), (F_,)
        s[p + "fc2.weight"], s[p + "fc2.bias"] = (C, F_), (C,)
        s[p + "final_layer_norm.weight"], s[p + "final_layer_norm.bias"] = (C,), (C,)
    s["encoder.layer_norm.weight"], s["encoder.layer_norm.bias"] = (C,), (C,)
    s["layer_norm.weight"], s["layer_norm.bias"] = (embed,), (embed,)
    return s


def audio_slice_starts(n_samples, sr=SAMPLE_RATE):
    """First samples of the reference's slices of a clip (scripts/audio2vid.py:299-309 of the reference), or None for "the whole file".
    Clips longer than 3.3 s go through slice_audio(f, 3.2, 3.2) (data/slice.py:12-29), which -- a quirk kept here -- SKIPS the first
    window (start_idx == 0 only advances) and keeps only full 3.2-s windows; shorter clips are one slice."""
    if n_samples / sr <= 3.3:
        return None
    window = stride = int(3.2 * sr)
    starts, start = [], 0
    while start <= n_samples - window:
        if start != 0:
            starts.append(start)
        start += stride
    return starts


def audio_slices(wave_16k):
    """(n_slices, samples) of a 1-D 16-kHz waveform, as the reference slices the driving audio."""
    wave = torch.as_tensor(wave_16k)
    if wave.dim() != 1:
        raise ValueError("audio_slices: expects a 1-D mono waveform")
    starts = audio_slice_starts(wave.shape[0])
    if starts is None:
        return wave[None].clone()
    window = int(3.2 * SAMPLE_RATE)
    if not starts:
        return wave.new_zeros((0, window))
    return torch.stack([wave[s:s + window] for s in starts])


class WavLM:
    def __init__(self, cfg=None, device="cuda", dtype=torch.bfloat16):
        self.cfg = cfg if isinstance(cfg, WavLMConfig) else WavLMConfig(cfg)
        self._device, self._dtype = torch.device(device), dtype
        hip.dtype_code(dtype)
        c = self.cfg
        self.C, self.H, self.L, self.cd = c.encoder_embed_dim, c.encoder_attention_heads, c.encoder_layers, eval(c.conv_feature_layers)[-1][0]
        self.convs = [tuple(x) for x in eval(c.conv_feature_layers)]
        self.w = {}
        self._tabs = {}
        self._loaded = False

    dtype = property(lambda self: self._dtype)
    device = property(lambda self: self._device)

    def eval(self):
        return self

    def _t(self, x):
        return x.to(device=self._device, dtype=self._dtype).contiguous()

    def _f(self, x):
        return x.to(device=self._device, dtype=torch.float32).contiguous()

    @classmethod
    def from_checkpoint(cls, path, device="cuda", dtype=torch.bfloat16):
        """A WavLM-Large.pt-style file {"cfg": {...}, "model": state_dict} (wavlm_features.py:102-116): every field from its cfg."""
        from .inputs import load_checkpoint
        ck = load_checkpoint(path)
        if not isinstance(ck, dict) or "model" not in ck:
            raise RuntimeError(f"WavLM.from_checkpoint: {path} holds no 'model' state dict")
        m = cls(WavLMConfig(ck.get("cfg")), device=device, dtype=dtype)
        m.load_state_dict(ck["model"])
        return m

    def load_state_dict(self, sd, strict=True):
        pre = "encoder.pos_conv.0."
        style = "checkpoint" if (pre + "weight_g") in sd else "parametrized"
        spec = wavlm_spec(self.cfg, style)
        missing = [k for k in spec if k not in sd and k != "mask_emb"]
        if missing:
            raise RuntimeError(f"WavLM.load_state_dict: missing {len(missing)} keys, e.g. {missing[:3]}")
        for k, shape in spec.items():
            if k in sd and tuple(sd[k].shape) != tuple(shape):
                raise RuntimeError(f"shape mismatch for {k}: {tuple(sd[k].shape)} vs {shape}")
        w, C, H = self.w, self.C, self.H
        for i, (dim, k, _st) in enumerate(self.convs):
            cw = sd[f"feature_extractor.conv_layers.{i}.0.weight"].float()                      # (512, cin, k)
            if i == 0:
                w0 = torch.zeros((dim, 64))                                                     # K = 10 taps, padded to the GEMM's 64
                w0[:, :k] = cw[:, 0]
                w["c0.w"] = self._t(w0)
            else:
                w[f"c{i}.w"] = self._t(cw.permute(0, 2, 1).reshape(dim, -1))                    # [cout][tap][cin]: a patch = k consecutive rows
            w[f"c{i}.g"], w[f"c{i}.b"] = self._f(sd[f"feature_extractor.conv_layers.{i}.2.1.weight"]), self._f(sd[f"feature_extractor.conv_layers.{i}.2.1.bias"])
        w["fln.g"], w["fln.b"] = self._f(sd["layer_norm.weight"]), self._f(sd["layer_norm.bias"])
        w["proj.w"], w["proj.b"] = self._t(sd["post_extract_proj.weight"]), self._f(sd["post_extract_proj.bias"])
        g_key, v_key = (pre + "weight_g", pre + "weight_v") if style == "checkpoint" else (pre + "parametrizations.weight.original0", pre + "parametrizations.weight.original1")
        v = sd[v_key].double()                                                                  # weight_norm(dim=2): norm over (out, in) per tap
        pw = (sd[g_key].double() * v / v.norm(dim=(0, 1), keepdim=True)).float()               # (C, C / groups, kernel)
        G, K = self.cfg.conv_pos_groups, self.cfg.conv_pos
        cg = C // G
        w["pos.w"] = self._t(pw.view(G, cg, cg, K).permute(0, 1, 3, 2).reshape(G, cg, K * cg))    # [g][cout][tap][cin]
        w["pos.b"] = self._f(sd[pre + "bias"])
        w["enc.g"], w["enc.b"] = self._f(sd["encoder.layer_norm.weight"]), self._f(sd["encoder.layer_norm.bias"])
        w["relpos"] = sd["encoder.layers.0.self_attn.relative_attention_bias.weight"].float().to(self._device)    # (num_buckets, H)
        for i in range(self.L):
            p, q = f"encoder.layers.{i}.", f"l{i}."
            a = p + "self_attn."
            w[q + "qkv.w"] = self._t(torch.cat([sd[a + f"{n}_proj.weight"] for n in ("q", "k", "v")], 0))
            w[q + "qkv.b"] = self._f(torch.cat([sd[a + f"{n}_proj.bias"] for n in ("q", "k", "v")], 0))
            w[q + "o.w"], w[q + "o.b"] = self._t(sd[a + "out_proj.weight"]), self._f(sd[a + "out_proj.bias"])
            w[q + "gw"], w[q + "gb"] = self._f(sd[a + "grep_linear.weight"]), self._f(sd[a + "grep_linear.bias"])
            w[q + "ga"] = self._f(sd[a + "grep_a"].reshape(H))
            w[q + "ln1.g"], w[q + "ln1.b"] = self._f(sd[p + "self_attn_layer_norm.weight"]), self._f(sd[p + "self_attn_layer_norm.bias"])
            w[q + "fc1.w"], w[q + "fc1.b"] = self._t(sd[p + "fc1.weight"]), self._f(sd[p + "fc1.bias"])
            w[q + "fc2.w"], w[q + "fc2.b"] = self._t(sd[p + "fc2.weight"]), self._f(sd[p + "fc2.bias"])
            w[q + "ln2.g"], w[q + "ln2.b"] = self._f(sd[p + "final_layer_norm.weight"]), self._f(sd[p + "final_layer_norm.bias"])
        self._tabs = {}
        self._loaded = True
        return [], [k for k in sd if k not in spec]

    # ------------------------------------------------------------------------------------------ pieces
    def _check_input(self, source):
        if not self._loaded:
            raise RuntimeError("WavLM: extract_features before load_state_dict")
        if not torch.is_tensor(source) or not source.is_cuda:
            raise RuntimeError("mmgt_amd.WavLM runs on the GPU only (no CPU path exists)")
        if source.dim() != 2:
            raise RuntimeError("WavLM: source must be (batch, samples)")

    def bias_table(self, T):
        """(H, 2T - 1) fp32: layer 0's relative-position bias by offset j - i (index j - i + T - 1), shared by every layer."""
        tab = self._tabs.get(T)
        if tab is None:
            idx = relative_position_buckets(T, self.cfg.num_buckets, self.cfg.max_distance).to(self._device)
            tab = self._tabs[T] = self.w["relpos"][idx].t().contiguous()
        return tab

    def _conv_features(self, wave):
        """(samples,) fp32 -> (T, 512): the conv stack (conv GEMM -> LayerNorm(512) over channels -> GELU per layer)."""
        w = self.w
        dim, k, st = self.convs[0]
        t = (wave.shape[0] - k) // st + 1
        if t < 1:
            raise RuntimeError(f"WavLM: a source of {wave.shape[0]} samples is shorter than the conv front end's receptive field")
        a = torch.zeros((t, 64), device=self._device, dtype=self._dtype)       # layer 0 patches: 10 samples every 5 (one input channel)
        a[:, :k] = wave.unfold(0, k, st).to(self._dtype)
        h = hip.gemm(a, w["c0.w"])
        h = hip.activation(hip.layernorm(h, w["c0.g"], w["c0.b"], 1e-5), hip.ACT_GELU)
        for i in range(1, len(self.convs)):
            dim, k, st = self.convs[i]
            t = (h.shape[0] - k) // st + 1
            if t < 1:
                raise RuntimeError("WavLM: source too short for the conv front end")
            patches = h.as_strided((t, k * h.shape[1]), (st * h.shape[1], 1))  # row r = rows st r .. st r + k - 1, contiguous
            h = hip.gemm(patches, w[f"c{i}.w"])
            h = hip.activation(hip.layernorm(h, w[f"c{i}.g"], w[f"c{i}.b"], 1e-5), hip.ACT_GELU)
        return h

    def _features(self, wave):
        """(T, C): feature LayerNorm + post_extract_proj of the conv features (the reference's res["features"])."""
        h = self._conv_features(wave)
        return hip.gemm(hip.layernorm(h, self.w["fln.g"], self.w["fln.b"], 1e-5), self.w["proj.w"], self.w["proj.b"])

    def _encode(self, x):
        """(T, C) -> (T, C): positional conv + residual, the pre-LN layers, encoder.layer_norm."""
        w, C, H = self.w, self.C, self.H
        S = x.shape[0]
        G, K = self.cfg.conv_pos_groups, self.cfg.conv_pos
        cg = C // G
        xp = torch.zeros((G, S + K - 1, cg), device=self._device, dtype=self._dtype)    # group-major, zero padded by K / 2 on the left
        xp[:, K // 2: K // 2 + S] = x.view(S, G, cg).permute(1, 0, 2)
        xs = torch.empty((S, C), device=self._device, dtype=self._dtype)               # x + gelu(pos_conv(x)): residual epilogue
        for g in range(G):
            patches = xp[g].as_strided((S, K * cg), (cg, 1))
            sl = slice(g * cg, (g + 1) * cg)
            hip.gemm(patches, w["pos.w"][g], w["pos.b"][sl].contiguous(), act=hip.ACT_GELU, residual=x[:, sl], out=xs[:, sl])
        x = xs
        tab = self.bias_table(S)
        st3, st1 = (S * 3 * C, 3 * C), (S * C, C)
        for i in range(self.L):
            q = f"l{i}."
            h = hip.layernorm(x, w[q + "ln1.g"], w[q + "ln1.b"], 1e-5)
            qkv = hip.gemm(h, w[q + "qkv.w"], w[q + "qkv.b"])
            o = torch.empty((S, C), device=self._device, dtype=self._dtype)
            hip.relpos_attention(qkv, qkv[:, C:], qkv[:, 2 * C:], o, h, w[q + "gw"], w[q + "gb"], w[q + "ga"], tab, batch=1, heads=H, T=S,
                                 scale=(C // H) ** -0.5, q_str=st3, k_str=st3, v_str=st3, o_str=st1, x_str=st1)
            x = hip.gemm(o, w[q + "o.w"], w[q + "o.b"], residual=x)
            h = hip.layernorm(x, w[q + "ln2.g"], w[q + "ln2.b"], 1e-5)
            f1 = hip.gemm(h, w[q + "fc1.w"], w[q + "fc1.b"], act=hip.ACT_GELU)
            x = hip.gemm(f1, w[q + "fc2.w"], w[q + "fc2.b"], residual=x)
        return hip.layernorm(x, w["enc.g"], w["enc.b"], 1e-5)

    def conv_features(self, source):
        """(B, samples) -> (B, T, C) fp32: the reference's res["features"] (extract_features(..., ret_conv=True)[0])."""
        self._check_input(source)
        return torch.stack([self._features(s.float().contiguous()) for s in source]).float()

    def extract_features(self, source, padding_mask=None, output_layer=None):
        """WavLM.extract_features(source) (WavLM.py:315-373): (x (B, T, C) fp32, None).  Padding masks and output_layer are not built."""
        if padding_mask is not None:
            raise NotImplementedError("WavLM.extract_features: padding_mask is not built on the HIP path")
        if output_layer is not None:
            raise NotImplementedError("WavLM.extract_features: output_layer / layer results are not built on the HIP path")
        self._check_input(source)
        return torch.stack([self._encode(self._features(s.float().contiguous())) for s in source]).float(), None

    __call__ = extract_features

    def slice_features(self, waves):
        """extract_wo_init (wavlm_features.py:128-145) for a batch of equal-length slices: F.layer_norm over each whole slice (cfg.normalize,
        no affine, eps 1e-5), extract_features, a copy of the last frame appended, linear interpolation (align_corners=True) to
        ceil((T + 1) / 2) frames.  (B, 51200) -> (B, 80, C) fp32; each slice runs exactly as it would alone."""
        self._check_input(waves)
        out = []
        for s in waves:
            s = s.float().contiguous()
            if self.cfg.normalize:
                s = F.layer_norm(s, s.shape)
            x = self._encode(self._features(s))
            x = torch.cat((x, x[-1:]), 0)
            out.append(hip.lerp_rows(x, math.ceil(x.shape[0] / 2)))
        return torch.stack(out).float()
