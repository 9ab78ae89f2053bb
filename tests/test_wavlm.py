"""WavLM-Large features for audio2vid's pose conditioning (mmgt_amd/wavlm.py), CPU side: the key layout, the host bucket function and the
CPU restatement (tests/wavlm_ref.py) against goldens the REFERENCE's own WavLM produced (tools/refgen/gen_wavlm_golden.py); slicing,
configuration refusals and the script's interface."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import wavlm_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def keys():
    return {k: tuple(v) for k, v in json.load(open(os.path.join(GOLD, "wavlm_keys.json"))).items()}


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "wavlm.npz")).items()}


@pytest.fixture(scope="module")
def tiny():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLD, "wavlm_tiny.npz")).items()}


def test_wavlm_spec_matches_reference_keys(keys):
    from mmgt_amd.wavlm import WavLMConfig, wavlm_spec
    mine = wavlm_spec(WavLMConfig())
    assert len(keys) == 488 and list(mine) == list(keys) and all(tuple(mine[k]) == keys[k] for k in keys)
    assert sum(int(np.prod(s)) for s in mine.values()) == 315_453_120
    par = wavlm_spec(WavLMConfig(), weight_norm_keys="parametrized")
    assert "encoder.pos_conv.0.parametrizations.weight.original0" in par and len(par) == 488


def test_bucket_function_matches_reference_tables(gold):
    from mmgt_amd.wavlm import relative_position_buckets
    for T, md in wc.BUCKET_POINTS:
        mine = relative_position_buckets(T, 320, md)
        assert torch.equal(mine, gold[f"buckets_T{T}_md{md}"].long()), (T, md)
    # the two max_distance values really differ (the table depends on the checkpoint's cfg)
    assert not torch.equal(relative_position_buckets(1500, 320, 800), relative_position_buckets(1500, 320, 1280))


def _cfg(d):
    from mmgt_amd.wavlm import WavLMConfig
    return WavLMConfig(d)


def test_cpu_restatement_matches_reference_tiny(tiny):
    from tests import wavlm_ref as R
    from mmgt_amd.wavlm import wavlm_spec
    cfg = _cfg(wc.TINY)
    sd = wc.wavlm_state_dict(wavlm_spec(cfg))
    waves = wc.wavlm_waves(2, wc.TINY_SAMPLES, tag="tiny")
    with torch.no_grad():
        nw = R.normalize(waves)
        x, feats = R.extract_features(sd, cfg, nw, return_features=True)
        post = R.post_process(x)
        x_off = R.extract_features(sd, cfg, nw, bias_scale=0.0)
    torch.testing.assert_close(feats, tiny["features"], rtol=1e-4, atol=5e-5)
    torch.testing.assert_close(x, tiny["x"], rtol=1e-4, atol=5e-5)
    torch.testing.assert_close(post, tiny["post"], rtol=1e-4, atol=5e-5)
    assert x.shape == (2, 37, 256) and post.shape == (2, 19, 256)
    with pytest.raises(AssertionError):      # the relative bias is visible in the golden
        torch.testing.assert_close(x_off, tiny["x"], rtol=1e-4, atol=5e-5)


def test_cpu_restatement_matches_reference_large(gold):
    from tests import wavlm_ref as R
    from mmgt_amd.wavlm import wavlm_spec
    cfg = _cfg(None)
    sd = wc.wavlm_state_dict(wavlm_spec(cfg))
    waves = wc.wavlm_waves(2, wc.SLICE_SAMPLES)
    with torch.no_grad():
        nw = R.normalize(waves)
        x = R.extract_features(sd, cfg, nw)
        post = R.post_process(x)
        x_off = R.extract_features(sd, cfg, nw, bias_scale=0.0)
    assert x.shape == (2, 159, 1024) and post.shape == (2, 80, 1024)
    torch.testing.assert_close(x[..., wc.X_COLS], gold["x"], rtol=1e-4, atol=5e-5)
    torch.testing.assert_close(post[..., wc.X_COLS], gold["post"], rtol=1e-4, atol=5e-5)
    d = (x_off[..., wc.X_COLS] - gold["x"]).abs()
    assert d.mean() > 1e-2 and d.max() > 0.1, (d.mean(), d.max())


def test_audio_slices_follow_reference_slicing():
    from mmgt_amd.wavlm import audio_slice_starts, audio_slices
    w10 = torch.arange(160000, dtype=torch.float32)
    s = audio_slices(w10)
    assert audio_slice_starts(160000) == [51200, 102400]          # the first window is skipped (slice_audio quirk)
    assert s.shape == (2, 51200) and s[0, 0] == 51200 and s[1, 0] == 102400
    w33 = torch.arange(52800, dtype=torch.float32)                   # 3.3 s: not > 3.3, the whole file
    s = audio_slices(w33)
    assert audio_slice_starts(52800) is None and s.shape == (1, 52800) and torch.equal(s[0], w33)
    s = audio_slices(torch.arange(104000, dtype=torch.float32))      # 6.5 s: one full window after the skipped one
    assert s.shape == (1, 51200) and s[0, 0] == 51200


@pytest.mark.parametrize("field,value", [("extractor_mode", "default"), ("layer_norm_first", False),
                                         ("relative_position_embedding", False), ("conv_bias", True), ("gru_rel_pos", False),
                                         ("encoder_attention_heads", 8)])
def test_config_refuses_unbuilt_fields(field, value):
    from mmgt_amd.wavlm import WavLMConfig
    with pytest.raises(NotImplementedError):
        WavLMConfig({field: value})


def test_config_defaults_and_checkpoint_override():
    from mmgt_amd.wavlm import WavLMConfig
    c = WavLMConfig()
    assert (c.encoder_layers, c.encoder_embed_dim, c.encoder_ffn_embed_dim, c.encoder_attention_heads) == (24, 1024, 4096, 16)
    assert c.extractor_mode == "layer_norm" and c.layer_norm_first and c.normalize and c.gru_rel_pos and c.max_distance == 800
    assert WavLMConfig({"max_distance": 1280, "num_buckets": 320}).max_distance == 1280


def test_wavlm_model_refuses_cpu_tensors():
    from mmgt_amd.wavlm import WavLM
    m = WavLM(dtype=torch.float32, device="cpu")
    with pytest.raises(RuntimeError):
        m.extract_features(torch.zeros(1, 51200))


def test_audio2vid_help_lists_wavlm_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "audio2vid.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--wavlm" in r.stdout and "--baseline_feats" in r.stdout


def test_package_exports_wavlm_lazily():
    r = subprocess.run([sys.executable, "-c", "import sys, mmgt_amd; assert 'mmgt_amd.wavlm' not in sys.modules; "
                        "from mmgt_amd import WavLM, WavLMConfig; import mmgt_amd.wavlm as w; assert WavLM is w.WavLM and WavLMConfig is w.WavLMConfig"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
