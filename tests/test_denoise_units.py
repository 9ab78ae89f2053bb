"""What the sampler loop tells the HIP operator is true of the tensors it hands over (CPU).

`denoise_window` trusts three statements of its caller without checking them: `cfg_rows_share_input` (the second half of the batch is a copy of the
first), `audio_zero_rows` (the audio of the first rows is all zero) and `window_state` (a memo that belongs to exactly these rows, at every step).  A
wrong one gives silently wrong frames.  The double below has a `boc` attribute, so the loop takes it for the HIP operator and hands it the extras; it
records every call, and the tests hold each call's statements against its tensors and its tensors against the direct gather from the full ones.
"""
import pytest
import torch

from mmgt_amd.longclip import check_guidance_interval, get_context_scheduler, step_is_guided
from mmgt_amd.scheduler import DDIMScheduler
from tests.test_longclip import _install

L, CTX, OV, STEPS, HW, POSE_C = 20, 8, 2, 4, 4, 6
EXTRAS = {"cfg_row", "window_state", "audio_zero_rows", "cfg_rows_share_input"}
LONGCLIP = dict(context_schedule="open", context_fuse="pyramid", guidance_interval=(0.3, 0.8))


class _PlainUNet:
    """CPU double of denoise_window with the operator's full signature (the extras arrive in **kw, so an absent one is seen as absent): every row a
    function of its own latents, audio, mask, CFG row and position in the window, channels-last, 4 valid channels, 1e9 in the padding -- the layout of
    tests/test_longclip.py's _RowUNet.  Every call is recorded.  Without `boc` the loop must not take it for the HIP operator."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def denoise_window(self, latent_in, t, encoder_hidden_states, audio_embedding=None, pose_cond_fea=None, full_mask=None, face_mask=None,
                       body_mask=None, motion_scale=None, **kw):
        assert set(kw) <= EXTRAS, kw
        rows, c, f, h, w = latent_in.shape
        cfg_row = kw.get("cfg_row")
        self.calls.append(dict(t=int(t), latents=latent_in.clone(), contiguous=latent_in.is_contiguous(), audio=audio_embedding, pose=pose_cond_fea,
                               full=full_mask, face=face_mask, lips=body_mask, kw=dict(kw), state=kw.get("window_state")))
        e = encoder_hidden_states.float().mean(dim=(1, 2))
        pos = (1 + 0.25 * (torch.arange(f, dtype=torch.float32) - (f - 1) / 2) / f).view(1, f, 1, 1)
        out = torch.full((rows * f, h, w, 64), 1e9)
        for r in range(rows):
            kind = cfg_row if cfg_row is not None else r // (rows // 2)
            a = audio_embedding[r].float().mean(dim=(1, 2)).view(1, f, 1, 1)
            m = full_mask[0][r * f:(r + 1) * f].float().mean(dim=1).view(1, f, 1, 1)
            pred = (latent_in[r] * (0.9 - 1e-4 * float(t)) * pos + 0.1 * a + 0.01 * m + 0.05 * e[kind]).float()
            out[r * f:(r + 1) * f, :, :, :c] = pred.permute(1, 2, 3, 0)
        return out


class _RecordingUNet(_PlainUNet):
    """The same with `boc`: the loop takes it for the HIP operator and hands it the extras."""
    boc = True


def _run(monkeypatch, unet=None, window_state=1, uncond_audio=0.0, **kw):
    """-> (the double, the full tensors, the latents in front of every step) of the L = 20, 8 / 2, 4-step run"""
    from mmgt_amd import pipeline as PL
    _install(monkeypatch, PL.hip)
    monkeypatch.setattr(PL.hip, "tune_get", lambda key: {"zero_audio_skip": 1, "window_state": window_state}[key])
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    unet = unet or _RecordingUNet()
    pipe = PL.Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=unet, pose_guider=None, scheduler=sched)
    g = torch.Generator().manual_seed(13)
    lat = torch.randn(1, 4, L, HW, HW, generator=g)
    audio = torch.randn(2, L, 3, 5, generator=g)
    audio[0] = 0.0                                               # the reference's unconditional audio: zeros_like
    audio[0, L - 1, 2, 4] = uncond_audio
    full, face, lips = ([torch.rand(2 * L, HW * HW, generator=g), torch.rand(2 * L, HW * HW // 4, generator=g)] for _ in range(3))
    pose = torch.randn(1, POSE_C, L, HW, HW, generator=g)
    ehs = torch.cat([torch.zeros(1, 1, 8), torch.randn(1, 1, 8, generator=g)])
    before = [lat.clone()]
    pipe.denoise(lat, sched.timesteps, ehs, pose, audio, full, face, lips, 3.5, None, context_frames=CTX, context_stride=1, context_overlap=OV,
                 num_inference_steps=STEPS, callback=lambda i, t, x: before.append(x.clone()), **kw)
    return unet, dict(audio=audio, full=full, face=face, lips=lips, pose=pose, timesteps=[int(t) for t in sched.timesteps]), before


def _expected_units(kw, split=False):
    """[(step, window numbers, CFG row or None)] in the order the loop must call the operator, and the window list"""
    windows = list(get_context_scheduler(kw.get("context_schedule", "uniform"))(0, STEPS, L, CTX, 1, OV))
    nw, B = len(windows), kw.get("context_batch_size", 1)
    assert nw == (3 if "context_schedule" in kw else 4), "open: 3 windows, a lone last group at B = 2; uniform: 4 (the last wraps), a lone one at B = 3"
    groups = [list(range(g0, min(g0 + B, nw))) for g0 in range(0, nw, B)]
    s = DDIMScheduler()
    s.set_timesteps(STEPS)
    interval = check_guidance_interval(kw.get("guidance_interval"))
    units = []
    for i, t in enumerate(s.timesteps):
        guided = step_is_guided(int(t), interval, s.num_train_timesteps)
        for ws in groups:
            units += [(i, ws, 0), (i, ws, 1)] if split else [(i, ws, None if guided else 1)]
    return units, windows


def _rows(t, windows, ws, cfg_rows):
    """the direct gather from a full (2, L, ...) tensor for the windows `ws`, CFG row major: (rows n, Fw, ...)"""
    return torch.stack([t[r, windows[w]] for r in cfg_rows for w in ws])


def _check_calls(unet, data, before, kw, split=False, window_state=True, audio_zero=True):
    units, windows = _expected_units(kw, split)
    assert len(unet.calls) == len(units)
    memo = {}
    for call, (i, ws, row) in zip(unet.calls, units):
        n, k, where = len(ws), call["kw"], f"step {i} windows {ws} row {row}"
        assert call["t"] == data["timesteps"][i] and call["contiguous"], where
        lat = torch.cat([before[i][:, :, windows[w]] for w in ws])                               # (n, C, Fw, h, w)
        pose = torch.cat([data["pose"][:, :, windows[w]] for w in ws])
        cfg_rows = (0, 1) if row is None else (row,)
        if row is None:
            assert "cfg_row" not in k and k["cfg_rows_share_input"] is True, where
            assert call["latents"].shape[0] == 2 * n and torch.equal(call["latents"][:n], call["latents"][n:]), where
            assert call["pose"].shape[0] == 2 * n and torch.equal(call["pose"][:n], call["pose"][n:]), where
            assert torch.equal(call["latents"][:n], lat) and torch.equal(call["pose"][:n], pose), where
            zero_rows = n
        else:
            assert k["cfg_row"] == row and "cfg_rows_share_input" not in k, where
            assert torch.equal(call["latents"], lat) and torch.equal(call["pose"], pose), where
            zero_rows = n if row == 0 else 0
        if audio_zero:
            assert k["audio_zero_rows"] == zero_rows and not call["audio"][:zero_rows].ne(0).any(), where
        else:
            assert not k.get("audio_zero_rows"), where
        assert torch.equal(call["audio"], _rows(data["audio"], windows, ws, cfg_rows)), where
        for name in ("full", "face", "lips"):
            assert len(call[name]) == len(data[name])
            for got, level in zip(call[name], data[name]):
                assert torch.equal(got, _rows(level.view(2, L, -1), windows, ws, cfg_rows).flatten(0, 1)) and got.is_contiguous(), (where, name)
        if window_state:
            assert type(call["state"]) is dict, where
            assert memo.setdefault((tuple(ws), row), call["state"]) is call["state"], f"{where}: another memo than at the earlier steps"
        else:
            assert "window_state" not in k, where
    if window_state:                                             # the records keep every dict alive, so equal ids would be one object
        assert len({id(d) for d in memo.values()}) == len(memo), "two units share a memo"
    return memo


@pytest.mark.parametrize("options", [{}, LONGCLIP], ids=["defaults", "open-pyramid-interval"])
@pytest.mark.parametrize("batch", [1, 2, 3])
def test_every_statement_to_the_operator_is_true(monkeypatch, batch, options):
    kw = dict(options, context_batch_size=batch)
    unet, data, before = _run(monkeypatch, **kw)
    memo = _check_calls(unet, data, before, kw)
    groups = -(-(3 if options else 4) // batch)
    if options:                                                  # steps 0 and 3 are unguided: every pair and its own row 1 were seen
        assert len(memo) == 2 * groups and all((ws, None) in memo and (ws, 1) in memo for ws, _ in memo)
    else:
        assert len(memo) == groups and all(row is None for _, row in memo)


def test_single_rows_of_a_window_group(monkeypatch, tmp_path):
    """cfg_split over a group of one rank (gloo): both rows of every window run alone, each with its own memo and its own count of zero rows"""
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        unet, data, before = _run(monkeypatch, window_group=True, cfg_split=True)
    finally:
        dist.destroy_process_group()
    memo = _check_calls(unet, data, before, {}, split=True)
    assert sorted(memo) == [((w,), row) for w in range(4) for row in (0, 1)]


def test_no_memo_when_the_tunable_is_off(monkeypatch):
    kw = dict(LONGCLIP, context_batch_size=2)
    unet, data, before = _run(monkeypatch, window_state=0, **kw)
    _check_calls(unet, data, before, kw, window_state=False)


@pytest.mark.parametrize("batch", [1, 2])
def test_nonzero_unconditional_audio_is_never_called_zero(monkeypatch, batch):
    kw = dict(LONGCLIP, context_batch_size=batch)
    unet, data, before = _run(monkeypatch, uncond_audio=1e-30, **kw)
    assert data["audio"][0].ne(0).sum() == 1
    _check_calls(unet, data, before, kw, audio_zero=False)


def test_a_double_without_boc_receives_no_extras(monkeypatch):
    unet, _, _ = _run(monkeypatch, unet=_PlainUNet(), **LONGCLIP)
    assert not hasattr(unet, "boc") and len(unet.calls) == 3 * STEPS
    assert [set(c["kw"]) for c in unet.calls] == [set() if i in (1, 2) else {"cfg_row"} for i in range(STEPS) for _ in range(3)]
