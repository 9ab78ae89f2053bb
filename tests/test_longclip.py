"""The long-clip options of the sampler on the CPU: `context_schedule="open"`, `context_fuse`, `guidance_interval`.  The window lists,
the weights and the guided steps are pure host arithmetic and are held to the values the definition gives; the loop runs over CPU doubles of the
operator and of the elementwise HIP entries (tests/loop_doubles.py)."""
import pytest
import torch

from mmgt_amd.scheduler import DDIMScheduler
from tests import longclip_ref as LR
from tests import loop_doubles

# ---- window lists -------------------------------------------------------------------------------------------------------------------------------------

TABLE = {(14, 8, 2): [(0, 7), (6, 13)],
         (20, 8, 2): [(0, 7), (6, 13), (12, 19)],
         (20, 12, 4): [(0, 11), (8, 19)],
         (24, 12, 4): [(0, 11), (8, 19), (12, 23)],
         (13, 12, 4): [(0, 11), (1, 12)],
         (80, 12, 4): [(s, s + 11) for s in (0, 8, 16, 24, 32, 40, 48, 56, 64, 68)]}


def _open(L, ctx, ov, **kw):
    from mmgt_amd.longclip import get_context_scheduler
    return list(get_context_scheduler("open")(0, 25, L, ctx, context_overlap=ov, **kw))


@pytest.mark.parametrize("case", list(TABLE), ids=str)
def test_open_window_lists(case):
    L, ctx, ov = case
    wins = _open(L, ctx, ov)
    assert [(w[0], w[-1]) for w in wins] == TABLE[case]
    assert wins == LR.open_windows(L, ctx, ov)
    for w in wins:
        assert len(w) == ctx and all(b == a + 1 for a, b in zip(w, w[1:])), "unwrapped, consecutive, of equal length"
    assert set().union(*wins) == set(range(L))


@pytest.mark.parametrize("L", [1, 7, 12])
def test_open_short_clip_is_one_window(L):
    assert _open(L, 12, 4) == [list(range(L))]


def test_open_refusals_name_the_argument():
    with pytest.raises(ValueError, match="context_overlap"):
        _open(20, 8, 8)
    with pytest.raises(ValueError, match="context_overlap"):
        _open(20, 8, 11)
    with pytest.raises(ValueError, match="context_stride"):
        _open(20, 8, 2, context_stride=2)


def test_uniform_is_unchanged_and_wraps():
    from mmgt_amd.context import uniform
    from mmgt_amd.longclip import get_context_scheduler, open_ended
    assert get_context_scheduler("uniform") is uniform and get_context_scheduler("open") is open_ended
    wins = list(uniform(0, 25, 20, 12, 1, 4))
    assert wins == [list(range(0, 12)), list(range(8, 20)), [16, 17, 18, 19, 0, 1, 2, 3, 4, 5, 6, 7]] == LR.uniform_windows(20, 12, 4)
    assert list(uniform(0, 25, 80, 12, 1, 4))[-1] == [72, 73, 74, 75, 76, 77, 78, 79, 0, 1, 2, 3]
    with pytest.raises(ValueError):
        get_context_scheduler("closed")


# ---- weights ------------------------------------------------------------------------------------------------------------------------------------------

def test_fuse_weights():
    from mmgt_amd.longclip import fuse_weights
    assert fuse_weights("pyramid", 8) == [1, 2, 3, 4, 4, 3, 2, 1]
    assert fuse_weights("pyramid", 7) == [1, 2, 3, 4, 3, 2, 1]
    assert fuse_weights("ramp", 12, 4) == pytest.approx([.2, .4, .6, .8, 1, 1, 1, 1, .8, .6, .4, .2], rel=1e-15, abs=0)
    assert fuse_weights("ramp", 9, 0) == [1.0] * 9
    assert fuse_weights("flat", 5) == [1.0] * 5
    for name in ("flat", "pyramid", "ramp"):
        for n in (1, 2, 7, 8, 12, 24):
            for o in (0, 2, 4, 11, 30):
                w = fuse_weights(name, n, o)
                assert len(w) == n and all(v > 0 for v in w) and w == w[::-1]
                assert torch.equal(torch.tensor(w, dtype=torch.float64).to(torch.float32), LR.weights(name, n, o))
    with pytest.raises(ValueError, match="context_fuse"):
        fuse_weights("cosine", 8)


# ---- the interval -------------------------------------------------------------------------------------------------------------------------------------

def _guided(n, interval):
    from mmgt_amd.longclip import check_guidance_interval, step_is_guided
    s = DDIMScheduler()
    s.set_timesteps(n)
    return [i for i, t in enumerate(s.timesteps) if step_is_guided(int(t), check_guidance_interval(interval), s.num_train_timesteps)]


def test_guided_steps():
    s = DDIMScheduler()
    s.set_timesteps(4)
    assert [int(t) for t in s.timesteps] == [999, 749, 499, 249]
    assert _guided(4, (0.3, 0.8)) == [1, 2]
    # 6 trailing steps: u = 1, .833, .667, .5, .333, .167;  25: u = 1 - .04 i, guided iff .3 < u <= .8: i = 5 .. 17
    assert _guided(6, (0.3, 0.8)) == [2, 3, 4]
    assert _guided(25, (0.3, 0.8)) == list(range(5, 18))
    for n in (4, 6, 25):
        assert _guided(n, (0, 1)) == _guided(n, None) == list(range(n))
        assert _guided(n, (0.5, 0.5 + 1e-9)) == []                   # u = .5 exactly (n = 4, 6) is not above lo; n = 25 has no u in the sliver
        s.set_timesteps(n)
        assert _guided(n, (0.3, 0.8)) == [i for i, f in enumerate(LR.guided_flags(s.timesteps, (0.3, 0.8))) if f]


@pytest.mark.parametrize("bad", [(0.5, 0.5), (0.8, 0.3), (-0.1, 0.5), (0.2, 1.5)])
def test_interval_refusals(bad):
    from mmgt_amd.longclip import check_guidance_interval
    with pytest.raises(ValueError, match="guidance_interval"):
        check_guidance_interval(bad)
    with pytest.raises(ValueError, match="guidance_interval"):
        _run(None, guidance_interval=bad)


# ---- the loop over CPU doubles ------------------------------------------------------------------------------------------------------------------------

L, CTX, OV, STEPS, HW = 20, 8, 2, 4, 4


class _RowUNet:
    """CPU double of denoise_window for CFG pairs of one or more windows and, with cfg_row=1, for their conditional rows alone: every row a function of
    its own latents, audio, mask, CFG row and POSITION in the window (so the fuse matters); channels-last, 4 valid channels, 1e9 in the padding."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def denoise_window(self, latent_in, t, encoder_hidden_states, audio_embedding, pose_cond_fea, full_mask, face_mask, body_mask, motion_scale,
                       cfg_row=None):
        rows, c, f, h, w = latent_in.shape
        assert cfg_row in (None, 1) and encoder_hidden_states.shape[0] == 2
        assert audio_embedding.shape[:2] == (rows, f) and full_mask[0].shape[0] == rows * f
        e = encoder_hidden_states.float().mean(dim=(1, 2))
        pos = (1 + 0.25 * (torch.arange(f, dtype=torch.float32) - (f - 1) / 2) / f).view(1, f, 1, 1)
        out = torch.full((rows * f, h, w, 64), 1e9)
        for r in range(rows):
            kind = 1 if cfg_row == 1 else r // (rows // 2)
            a = audio_embedding[r].float().mean(dim=(1, 2)).view(1, f, 1, 1)
            m = full_mask[0][r * f:(r + 1) * f].float().mean(dim=1).view(1, f, 1, 1)
            pred = (latent_in[r] * (0.9 - 1e-4 * float(t)) * pos + 0.1 * a + 0.01 * m + 0.05 * e[kind]).float()
            out[r * f:(r + 1) * f, :, :, :c] = pred.permute(1, 2, 3, 0)
        self.calls.append((int(t), rows, cfg_row))
        return out


_install = loop_doubles.install


def _run(monkeypatch, frames=L, **kw):
    """-> (latents after every step, the double, the call log of the accumulations that were given weights: (form, rows, row0) each)"""
    from mmgt_amd import pipeline as PL
    own = monkeypatch is None
    mp = pytest.MonkeyPatch() if own else monkeypatch
    try:
        log = _install(mp, PL.hip)
        sched = DDIMScheduler()
        sched.set_timesteps(STEPS)
        unet = _RowUNet()
        pipe = PL.Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=unet, pose_guider=None, scheduler=sched)
        g = torch.Generator().manual_seed(11)
        lat = torch.randn(1, 4, frames, HW, HW, generator=g)
        audio = torch.randn(2, frames, 3, 5, generator=g)
        masks = [torch.rand(2 * frames, HW * HW, generator=g)]
        ehs = torch.cat([torch.zeros(1, 1, 8), torch.randn(1, 1, 8, generator=g)])
        traj = []
        pipe.denoise(lat, sched.timesteps, ehs, None, audio, masks, masks, masks, 3.5, None, context_frames=CTX, context_stride=1,
                     context_overlap=OV, num_inference_steps=STEPS, callback=lambda i, t, x: traj.append(x.clone()), **kw)
        return traj, unet, [entry[:3] for entry in log if entry[3]]
    finally:
        if own:
            mp.undo()


@pytest.mark.parametrize("batch", [1, 2])
def test_defaults_never_call_the_weighted_entries(monkeypatch, batch):
    traj, unet, log = _run(monkeypatch, context_batch_size=batch)
    assert log == [] and len(traj) == STEPS
    assert all(cfg_row is None for _, _, cfg_row in unet.calls)
    _, unet_open, log = _run(monkeypatch, context_schedule="open", context_batch_size=batch)          # a window list alone changes no entry
    assert log == [] and len(unet_open.calls) == STEPS * (3 if batch == 1 else 2)


@pytest.mark.parametrize("schedule", ["uniform", "open"])
@pytest.mark.parametrize("batch", [1, 2, 3])
def test_flat_forced_through_the_weighted_entries_is_bitwise_the_default_run(monkeypatch, schedule, batch):
    want, _, _ = _run(monkeypatch, context_schedule=schedule)
    got, unet, log = _run(monkeypatch, context_schedule=schedule, context_batch_size=batch, guidance_interval=(0, 1))
    assert log and all(entry == ("window" if batch == 1 else "windows", 2, 0) for entry in log)
    assert all(cfg_row is None for _, _, cfg_row in unet.calls)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"step {i}: {(a - b).abs().max().item():.3e}"


@pytest.mark.parametrize("fuse", ["pyramid", "ramp"])
def test_a_single_window_is_flat_whatever_the_fuse(monkeypatch, fuse):
    want, _, _ = _run(monkeypatch, frames=CTX)
    got, _, log = _run(monkeypatch, frames=CTX, context_fuse=fuse)
    assert len(log) == STEPS
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("batch", [1, 2])
def test_unguided_steps_run_the_conditional_row_alone(monkeypatch, batch):
    traj, unet, log = _run(monkeypatch, context_schedule="open", context_fuse="pyramid", guidance_interval=(0.3, 0.8), context_batch_size=batch)
    nwin = 3
    groups = [list(range(g0, min(g0 + batch, nwin))) for g0 in range(0, nwin, batch)]
    want_calls, want_log = [], []
    for i, t in enumerate((999, 749, 499, 249)):
        for ws in groups:
            guided = i in (1, 2)
            want_calls.append((t, (2 if guided else 1) * len(ws), None if guided else 1))
            want_log.append(("window" if batch == 1 else "windows",) + ((2, 0) if guided else (1, 1)))
    assert unet.calls == want_calls and log == want_log
    assert all(torch.isfinite(x).all() for x in traj)


def test_unguided_steps_follow_the_fp64_restatement(monkeypatch):
    """the whole loop against tests/longclip_ref.py's arithmetic on the double's own predictions: weights, the conditional row alone at guidance 1,
    batches of two bitwise as one by one"""
    from tests import sampler_ref as R
    kw = dict(context_schedule="open", context_fuse="pyramid", guidance_interval=(0.3, 0.8))
    one, unet, _ = _run(monkeypatch, **kw)
    two, _, _ = _run(monkeypatch, context_batch_size=2, **kw)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    flat, _, _ = _run(monkeypatch, context_schedule="open", guidance_interval=(0.3, 0.8))
    assert (flat[-1] - one[-1]).abs().max() > 1e-3, "the double's prediction depends on the position: the fuse must matter"
    # restate step 0 (unguided) from the initial latents
    g = torch.Generator().manual_seed(11)
    lat = torch.randn(1, 4, L, HW, HW, generator=g)
    audio = torch.randn(2, L, 3, 5, generator=g)
    masks = [torch.rand(2 * L, HW * HW, generator=g)]
    ehs = torch.cat([torch.zeros(1, 1, 8), torch.randn(1, 1, 8, generator=g)])
    wins, w32 = LR.open_windows(L, CTX, OV), LR.weights("pyramid", CTX, OV)
    twin = _RowUNet()
    preds = []
    for win in wins:
        o = twin.denoise_window(lat[:, :, win], 999, ehs, audio[1:2, win], None, [masks[0].view(2, L, -1)[1, win]], None, None, None, cfg_row=1)
        preds.append(o[..., :4].reshape(1, CTX, HW, HW, 4).permute(0, 4, 1, 2, 3))
    ref, B = LR.step_from_predictions(None, preds, wins, w32, lat, 3.5, LR.ddim_scalars(R.alphas_cumprod(), 999, STEPS))
    # the CPU double of the accumulation rounds every product w p before the add: u |w p| per term, at most the chain's own m u sum |w p| that B
    # carries already, so one more B on top of the gate's two
    assert ((one[0].double() - ref).abs() <= 3 * B).all()


@pytest.mark.parametrize("fuse", ["pyramid", "cosine"])
def test_refusals_name_both_parties(monkeypatch, fuse):
    from mmgt_amd import pipeline as PL
    pipe = PL.Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=_RowUNet(), pose_guider=None,
                                 scheduler=DDIMScheduler())
    if fuse == "cosine":
        with pytest.raises(ValueError, match="context_fuse"):
            _run(monkeypatch, context_fuse=fuse)
        with pytest.raises(ValueError, match="context_fuse"):
            pipe(None, None, None, [], [], [], 32, 32, L, STEPS, 3.5, context_fuse=fuse)
        return
    # window_group is refused before any collective is touched (no process group exists here)
    with pytest.raises(ValueError, match="guidance_interval.*window_group"):
        _run(monkeypatch, guidance_interval=(0.3, 0.8), window_group=True)
    with pytest.raises(ValueError, match="context_fuse.*window_group"):
        _run(monkeypatch, context_fuse=fuse, window_group=True)
    with pytest.raises(ValueError, match="guidance_interval"):
        pipe(None, None, None, [], [], [], 32, 32, L, STEPS, 3.5, guidance_interval=(0.9, 0.1))


def test_call_takes_the_two_options_as_named_parameters():
    import inspect
    from mmgt_amd.pipeline import Pose2VideoPipeline
    for fn in (Pose2VideoPipeline.__call__, Pose2VideoPipeline.denoise):
        p = inspect.signature(fn).parameters
        assert p["context_fuse"].default == "flat" and p["guidance_interval"].default is None


def test_script_arguments():
    import argparse
    from mmgt_amd.longclip import add_longclip_arguments, longclip_kwargs
    p = argparse.ArgumentParser()
    add_longclip_arguments(p)
    assert longclip_kwargs(p.parse_args([])) == {}
    a = p.parse_args("--context_schedule open --context_fuse ramp --guidance_interval 0.25 0.75".split())
    assert longclip_kwargs(a) == dict(context_schedule="open", context_fuse="ramp", guidance_interval=(0.25, 0.75))
    with pytest.raises(SystemExit):
        p.parse_args(["--context_fuse", "cosine"])
