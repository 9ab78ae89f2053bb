"""Sampler logic of `context_batch_size = B` (several context windows per forward) over a CPU double of the operator.

The definition ("Several windows per forward"): the scheduler's window list is taken in its order in groups of B, the last group
may be smaller; one group is ONE call of the operator with the rows in CFG row major order [uncond w0 .. uncond w(B-1), cond w0 ..
cond w(B-1)]; the predictions enter pred_sum / counter window by window in list order.  The double below computes every batch row from
that row's inputs alone, so nothing but the order of the fp32 adds could differ from B = 1 -- and the definition fixes that order: the
latents after every step must be BITWISE those of B = 1.
"""
import os

import numpy as np
import pytest
import torch

from mmgt_amd.context import get_context_scheduler
from mmgt_amd.scheduler import DDIMScheduler
from tests import loop_doubles

L, CTX, OV, STEPS, HW = 40, 12, 4, 4, 4


class _GroupUNet:
    """CPU double of denoise_window that accepts 2 B rows: a deterministic function of each row's own latents, audio, mask and CFG row
    (row r of 2 B is CFG row r // B), in the operator's layout -- channels-last ((2 B Fw), h, w, 64), 4 valid channels, garbage in the
    padding.  Every call's row order is recorded as the list of (CFG row, first latent value of the row)."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def denoise_window(self, latent_in, t, encoder_hidden_states, audio_embedding, pose_cond_fea, full_mask, face_mask, body_mask,
                       motion_scale, cfg_row=None):
        rows, c, f, h, w = latent_in.shape
        assert cfg_row is None and rows % 2 == 0 and encoder_hidden_states.shape[0] == 2
        assert audio_embedding.shape[:2] == (rows, f) and full_mask[0].shape[0] == rows * f
        e = encoder_hidden_states.float().mean(dim=(1, 2))
        out = torch.full((rows * f, h, w, 64), 1e9)
        for r in range(rows):                                     # row by row: a row's output cannot depend on its neighbours
            a = audio_embedding[r].float().mean(dim=(1, 2)).view(1, f, 1, 1)
            m = full_mask[0][r * f:(r + 1) * f].float().mean(dim=1).view(1, f, 1, 1)
            pred = (latent_in[r] * (0.9 - 1e-4 * float(t)) + 0.1 * a + 0.01 * m + 0.05 * e[r // (rows // 2)]).float()    # (C, Fw, h, w)
            out[r * f:(r + 1) * f, :, :, :c] = pred.permute(1, 2, 3, 0)
        self.calls.append((float(t), [(r // (rows // 2), latent_in[r, 0, :, 0, 0].clone()) for r in range(rows)]))
        return out


def _run(monkeypatch, batch, window_group=None):
    """(latents after every step, the double) of the L = 40, 12 / 4, 4-step run at context_batch_size = batch."""
    from mmgt_amd import pipeline as PL
    loop_doubles.install(monkeypatch, PL.hip)
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    unet = _GroupUNet()
    pipe = PL.Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=unet, pose_guider=None, scheduler=sched)
    g = torch.Generator().manual_seed(7)
    lat = torch.randn(1, 4, L, HW, HW, generator=g)
    audio = torch.randn(2, L, 3, 5, generator=g)
    masks = [torch.rand(2 * L, HW * HW, generator=g)]
    ehs = torch.cat([torch.zeros(1, 1, 8), torch.randn(1, 1, 8, generator=g)])
    traj = []
    kw = {} if batch is None else dict(context_batch_size=batch)
    pipe.denoise(lat, sched.timesteps, ehs, None, audio, masks, masks, masks, 3.5, None, context_frames=CTX, context_stride=1,
                 context_overlap=OV, num_inference_steps=STEPS, callback=lambda i, t, x: traj.append(x.clone()), window_group=window_group, **kw)
    return traj, unet, lat


def _windows():
    return list(get_context_scheduler("uniform")(0, STEPS, L, CTX, 1, OV))


def test_the_case_has_several_overlapping_windows():
    wins = _windows()
    assert len(wins) == 5 and all(len(w) == CTX for w in wins)
    assert any(set(a) & set(b) for a, b in zip(wins, wins[1:])), "neighbouring windows must share frames"


@pytest.mark.parametrize("batch", [2, 3, "all", "more"])
def test_batched_windows_are_bitwise_the_b1_sampler(monkeypatch, batch):
    nw = len(_windows())
    B = {"all": nw, "more": nw + 3}.get(batch, batch)
    want, one, _ = _run(monkeypatch, None)
    got, unet, _ = _run(monkeypatch, B)
    assert len(want) == len(got) == STEPS
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"step {i}: context_batch_size={B} differs from 1 by {(a - b).abs().max().item():.3e}"
    # one forward per group and step
    assert len(unet.calls) == STEPS * -(-nw // B) and len(one.calls) == STEPS * nw


@pytest.mark.parametrize("batch", [2, 3, 5, 8])
def test_row_order_is_cfg_row_major_in_window_order(monkeypatch, batch):
    """[uncond w0 .. uncond w(B-1), cond w0 .. cond w(B-1)] with the windows in the scheduler's order, the trailing short group included:
    read back from what the double received at the first step (the latents are still the initial noise there)."""
    wins = _windows()
    _, unet, lat = _run(monkeypatch, batch)
    groups = [list(range(g0, min(g0 + batch, len(wins)))) for g0 in range(0, len(wins), batch)]
    first_step = unet.calls[:len(groups)]
    assert len({t for t, _ in first_step}) == 1
    for ws, (_, rows) in zip(groups, first_step):
        assert len(rows) == 2 * len(ws)
        assert [r for r, _ in rows] == [0] * len(ws) + [1] * len(ws)
        for k, w in enumerate(ws):
            for half in (0, 1):
                assert torch.equal(rows[half * len(ws) + k][1], lat[0, 0, wins[w], 0, 0]), (ws, k, half)
    assert len(groups[-1]) == (len(wins) % batch or batch)


@pytest.mark.parametrize("bad", [0, -2])
def test_batch_below_one_is_a_value_error(monkeypatch, bad):
    with pytest.raises(ValueError, match="context_batch_size"):
        _run(monkeypatch, bad)
    from mmgt_amd import pipeline as PL
    pipe = PL.Pose2VideoPipeline(vae=None, image_encoder=None, reference_unet=None, denoising_unet=_GroupUNet(), pose_guider=None,
                                 scheduler=DDIMScheduler())
    with pytest.raises(ValueError, match="context_batch_size"):
        pipe(None, None, None, [], [], [], 32, 32, L, STEPS, 3.5, context_batch_size=bad)


def _wg_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mp_ = pytest.MonkeyPatch()
    try:
        try:
            _run(mp_, 2, window_group=True)
            q.put((rank, "ran"))
        except ValueError as e:
            q.put((rank, str(e)))
    finally:
        mp_.undo()
        dist.destroy_process_group()


def test_window_group_with_batched_windows_raises_the_documented_error():
    """Window-parallel sampling deals single windows or CFG rows to the ranks; the combination with context_batch_size > 1 is refused with
    a ValueError on every rank (gloo, world 2) instead of running a path nobody tested."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33100 + os.getpid() % 2000
    procs = [ctx.Process(target=_wg_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in range(2):
        assert "context_batch_size > 1 is not combined with window_group" in res[r], res[r]


def test_accumulate_windows_restatement_equals_sequential_windows(monkeypatch):
    """The CPU restatement used above against B sequential accumulate_window calls on overlapping, wrapping lists: bitwise."""
    from mmgt_amd import pipeline as PL
    loop_doubles.install(monkeypatch, PL.hip)
    g = torch.Generator().manual_seed(3)
    F, fw, C = 20, 6, 4
    idx = torch.tensor([[0, 1, 2, 3, 4, 5], [3, 4, 5, 6, 7, 8], [17, 18, 19, 0, 1, 2]], dtype=torch.int32)
    pred = torch.randn(2 * 3 * fw, HW, HW, 64, generator=g)
    ps0 = torch.randn(2, C, F, HW, HW, generator=g)
    a, ca = ps0.clone(), torch.zeros(F)
    PL.hip.accumulate_windows(pred, a, ca, idx, C)
    b, cb = ps0.clone(), torch.zeros(F)
    p = pred.view(2, 3, fw, HW, HW, 64)
    for k in range(3):
        PL.hip.accumulate_window(p[:, k].reshape(2 * fw, HW, HW, 64), b, cb, idx[k], C)
    assert torch.equal(a, b) and torch.equal(ca, cb) and ca.max() == 2 and np.isclose(float(ca.sum()), 18)


def test_group_operand_guard_arithmetic():
    """unet3d.check_group_operands: a multi-window forward whose widest level-0 operand would pass the 2 GiB the kernels address is refused;
    bf16 at 64 x 64 latents: 1024 columns x 2 bytes x 4096 tokens = 8 MiB per image, so 256 images (2 GiB) raise and 240 (the 10 windows of
    an 80-frame clip at 12 / 4) do not.  A lone window -- b = 2, or one row with cfg_row -- is never refused, whatever its size."""
    from mmgt_amd.unet3d import check_group_operands
    bf16, f32 = torch.bfloat16, torch.float32
    check_group_operands(20, 12, 64, 64, 320, bf16)                  # 240 images
    check_group_operands(10, 24, 64, 64, 320, bf16)
    with pytest.raises(RuntimeError, match="2 GiB"):
        check_group_operands(16, 16, 64, 64, 320, bf16)              # 256 images
    with pytest.raises(RuntimeError, match="2 GiB"):
        check_group_operands(22, 12, 64, 64, 320, bf16)
    check_group_operands(4, 24, 64, 64, 320, f32)                    # 96 images x 20 MiB (4 C fp32 columns)
    with pytest.raises(RuntimeError, match="2 GiB"):
        check_group_operands(6, 24, 64, 64, 320, f32)
    with pytest.raises(RuntimeError, match="2 GiB"):
        check_group_operands(9, 32, 64, 64, 320, bf16, cfg_row=1)    # 288 images of one CFG row
    for dtype in (bf16, f32):
        check_group_operands(2, 32, 256, 256, 320, dtype)            # a lone CFG pair, far past 2 GiB: worked in runs of rows, as before
        check_group_operands(1, 32, 256, 256, 320, dtype, cfg_row=0)
