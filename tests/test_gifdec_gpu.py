"""GIF decode on the device (csrc/gifdec.hip through the C ABI, mmgt_amd.video_in) against PIL's ImageSequence.Iterator(Image.open(f)) +
convert("RGB") on every byte: the case sets of tests/test_gifdec.py, the un-LZW launch alone against the yardstick decoder, the way back in of the
project's own .gif output, chunked composition, the device input helpers, and the refusals.  Every comparison is bitwise."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from tests import gifdec_cases as C
from tests import gifdec_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRIES = ("mmgt_gif_unlzw", "mmgt_gif_compose")


def decode(data, **kw):
    from mmgt_amd import video_in
    out = video_in.decode_gif_frames(data, DEV, **kw)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    return out


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- every byte against PIL -------------------------------------------------------------------------------------------------------------------------------
def test_device_equals_pil_on_random_files():
    for k, g in enumerate(C.random_gifs()):
        got = decode(g).cpu().numpy()
        want = C.pil_frames(g)
        assert got.shape == want.shape and np.array_equal(got, want), f"random file {k}"


@pytest.mark.parametrize("name", sorted(C.pil_written()))
def test_device_equals_pil_on_pil_written_files(name):
    g = C.pil_written()[name]
    assert np.array_equal(decode(g).cpu().numpy(), C.pil_frames(g))


@pytest.mark.parametrize("name", sorted(C.stream_cases()))
def test_device_reads_the_unusual_streams(name):
    g = C.stream_cases()[name]
    assert np.array_equal(decode(g).cpu().numpy(), C.pil_frames(g))


@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_at_every_size_interlaced_and_not(size):
    W, H = size
    rng = np.random.default_rng(W * 1000 + H)
    table = C.random_table(rng, 256)
    frames = [dict(idx=rng.integers(0, 256, (H, W)), interlace=bool(k & 1), disposal=k % 4, transparent=int(rng.integers(0, 256))) for k in range(4)]
    g = C.make_gif(W, H, frames, table)
    assert np.array_equal(decode(g).cpu().numpy(), C.pil_frames(g))


def test_unlzw_alone_gives_the_yardsticks_indices_and_touches_nothing_else():
    from mmgt_amd import hip, video_in
    files = [C.stream_cases()[k] for k in ("deferred_clear", "constant_kwkwk", "mcs2", "clear_every_7", "surplus_pixels")] + [C.pil_written()["masks"]]
    for g in files:
        h = video_in.parse_gif(g)
        tab, palette, data, chunks = video_in.gif_operands(h)
        n, idx_bytes, G = len(tab), chunks[0][2], 64
        buf = torch.full((idx_bytes + G,), 0xA5, dtype=torch.uint8, device=DEV)
        st = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        idx, status = hip.gif_unlzw(up(data.copy()), up(tab), idx_bytes, out=(buf[:idx_bytes], st[:n]))
        assert not bool(status.any()) and bool((buf[idx_bytes:] == 0xA5).all()) and bool((st[n:] == 0x5A5A5A5A).all())
        got = idx.cpu().numpy()
        for f, t in zip(h.frames, tab):
            want = R.lzw_decode(f.lzw, f.min_code_size, f.width * f.height)
            assert got[t[4]:t[4] + f.width * f.height].tolist() == want


def test_second_run_into_a_prefilled_buffer():
    g = C.pil_written()["dispose_mixed"]
    a = decode(g)
    buf = torch.full(tuple(a.shape), 0xA5, dtype=torch.uint8, device=DEV)
    b = decode(g, out=buf)
    assert b.data_ptr() == buf.data_ptr() and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), C.pil_frames(g))
    with pytest.raises(RuntimeError, match="out must be"):
        decode(g, out=buf[:2])


# ---- read_frames_device and the way back in of the project's own .gif ---------------------------------------------------------------------------------------
def test_read_frames_device_takes_a_gif_with_and_without_limit(tmp_path):
    import mmgt_amd
    from mmgt_amd import hip, video_in
    g = C.pil_written()["masks"]
    (tmp_path / "clip.gif").write_bytes(g)
    want = C.pil_frames(g)
    got = mmgt_amd.read_frames_device(tmp_path / "clip.gif", None, DEV)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    before = {k: hip.call_count(k) for k in ENTRIES}
    part = video_in.read_frames_device(tmp_path / "clip.gif", 3, DEV)
    assert tuple(part.shape) == (3,) + want.shape[1:] and np.array_equal(part.cpu().numpy(), want[:3])
    assert all(hip.call_count(k) - before[k] == 1 for k in ENTRIES)
    assert tuple(video_in.read_frames_device(tmp_path / "clip.gif", 99, DEV).shape) == want.shape
    with pytest.raises(RuntimeError, match="no frames"):
        video_in.read_frames_device(tmp_path / "clip.gif", 0, DEV)
    # a limit keeps a corrupt later frame out of the launches
    bad, _, frame = C.corrupt_cases()["truncated"]
    assert np.array_equal(decode(bad, limit=frame).cpu().numpy(), R.decode(bad, limit=frame))
    (tmp_path / "stack.npy").write_bytes(b"x")
    with pytest.raises(RuntimeError, match=r"a \.gif file nor a directory"):
        video_in.read_frames_device(tmp_path / "stack.npy", None, DEV)


def test_the_device_gif_writer_round_trips(tmp_path):
    from mmgt_amd import video_in, video_out
    yy, xx = np.mgrid[0:40, 0:56]
    clip = np.stack([np.stack([(xx * 4 + 9 * k) % 256, (yy * 6 + 5 * k) % 256, (xx + yy + 31 * k) % 256], axis=2) for k in range(5)]).astype(np.uint8)
    path = tmp_path / "clip.gif"
    video_out.save_videos_grid(torch.from_numpy(clip)[None], str(path), n_rows=1, fps=25, gif_encoder="device")
    got = video_in.read_frames_device(path, None, DEV)
    want = C.pil_frames(path.read_bytes())
    assert want.shape == clip.shape and np.array_equal(got.cpu().numpy(), want)
    video_out.save_videos_grid(torch.from_numpy(clip)[None], str(tmp_path / "pil.gif"), n_rows=1, fps=25)         # the reference's own .gif branch
    assert np.array_equal(video_in.read_frames_device(tmp_path / "pil.gif", None, DEV).cpu().numpy(), C.pil_frames((tmp_path / "pil.gif").read_bytes()))


def test_chunks_under_the_scratch_budget_equal_the_unsplit_result(monkeypatch):
    from mmgt_amd import hip, video_in
    for name in ("dispose2", "dispose3", "dispose_mixed", "transparency"):
        g = C.pil_written()[name]
        whole = decode(g)
        before = hip.call_count("mmgt_gif_compose")
        with monkeypatch.context() as m:
            m.setattr(video_in, "GIFDEC_SCRATCH_BYTES", 1)                                   # one frame per set of launches
            split = decode(g)
        assert hip.call_count("mmgt_gif_compose") - before == whole.shape[0] >= 3
        assert torch.equal(whole, split) and np.array_equal(split.cpu().numpy(), C.pil_frames(g)), name
    for k, g in enumerate(C.random_gifs()[:60]):
        with monkeypatch.context() as m:
            m.setattr(video_in, "GIFDEC_SCRATCH_BYTES", 600)
            assert np.array_equal(decode(g).cpu().numpy(), C.pil_frames(g)), f"random file {k}"


def _mask_clip(n, H, W, seed):
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        cx, cy = W * (0.3 + 0.05 * k) + seed, H * 0.5 - seed
        out[k][(xx - cx) ** 2 + (yy - cy) ** 2 < (H / (4 + seed)) ** 2] = 255
    return out


def test_gif_clips_through_the_device_input_helpers(tmp_path):
    """The mask clips carry the 256-step grey table, which PIL opens as mode "L": inputs._mask_stack takes a frame's array as read, so on a mask
    .gif whose first frame opens as "P" (PIL's writer shrinks the table of a small image to the greys in use) the HOST route sees palette indices
    in frame 0 where the device route sees the colours.  That is the host helper's reading, not the decoder's, and is left as it is."""
    from mmgt_amd import inputs, video_in
    n, H, W = 6, 48, 64
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    yy, xx = np.mgrid[0:H, 0:W]
    pose = np.stack([np.stack([(xx * 3 + 7 * k) % 256, (yy * 5 + k) % 256, (xx + 2 * yy + 40 * k) % 256], axis=2) for k in range(n)]).astype(np.uint8)
    frames = [Image.fromarray(f) for f in pose]
    frames[0].save(tmp_path / "pose.gif", save_all=True, append_images=frames[1:])
    for name, seed in (("face", 0), ("lips", 1), ("hands", 2)):
        masks = _mask_clip(n, H, W, seed)
        (tmp_path / f"{name}.gif").write_bytes(C.make_gif(W, H, [dict(idx=m, interlace=bool(k & 1)) for k, m in enumerate(masks)], ramp))
    read = lambda name: video_in.read_frames_device(tmp_path / f"{name}.gif", None, DEV)
    got = inputs.pose_tensor_device(read("pose"), W, H)
    ref = inputs.pose_tensor(inputs.read_frames(tmp_path / "pose.gif"), W, H)
    assert got.is_cuda and tuple(got.shape) == (1, 3, n, H, W) and torch.equal(got.cpu(), ref)
    host = {k: inputs.read_frames(tmp_path / f"{k}.gif") for k in ("face", "lips", "hands")}
    for hands in ("hands", None):
        a = inputs.motion_masks_device(read("face"), read("lips"), read(hands) if hands else None, n, 64)
        b = inputs.motion_masks(host["face"], host["lips"], host[hands] if hands else None, n, torch.device(DEV), 64)
        for la, lb in zip(a, b):
            for x, y in zip(la, lb):
                assert torch.equal(x, y)
    assert a[1][0].std() > 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_out_of_scope_files_raise_before_any_launch(tmp_path):
    from mmgt_amd import hip, video_in
    idx = np.arange(35, dtype=np.uint8).reshape(7, 5) % 4
    table = C.random_table(np.random.default_rng(1), 4)
    good = C.make_gif(5, 7, [dict(idx=idx)], table)
    decode(good)                                                                            # the library is loaded and has run
    before = {k: hip.call_count(k) for k in ENTRIES}
    assert before["mmgt_gif_unlzw"] >= 1
    at = good.index(b"\x2c", 13 + 12)
    cases = ((C.make_gif(5, 7, [dict(idx=idx, mcs=2)]), "neither a local nor a global colour table"),
             (C.make_gif(5, 7, [dict(idx=idx), dict(idx=idx, x=1)], table), "leaves the logical screen"),
             (good[:at + 10] + b"\x09" + good[at + 11:], "minimum code size 9"), (good[:-3], "runs past the end"), (b"GIF88a" + good[6:], "bad signature"))
    for bad, word in cases:
        with pytest.raises(ValueError, match=word):
            decode(bad)
    (tmp_path / "bad.gif").write_bytes(cases[1][0])
    with pytest.raises(ValueError, match="leaves the logical screen"):
        video_in.read_frames_device(tmp_path / "bad.gif", None, DEV)
    assert before == {k: hip.call_count(k) for k in ENTRIES}


@pytest.mark.parametrize("name", sorted(C.corrupt_cases()))
def test_corrupt_streams_raise_naming_the_frame(name):
    from mmgt_amd import video_in
    g, status, frame = C.corrupt_cases()[name]
    with pytest.raises(RuntimeError, match=f"frame {frame}, image data: {video_in.GIF_STATUS_TEXT[status]}"):
        decode(g)


def test_the_c_entries_refuse_out_of_range_arguments():
    from mmgt_amd import hip
    L = hip.lib()
    buf = torch.zeros(8192, dtype=torch.uint8, device=DEV)
    tab = torch.zeros((1, 16), dtype=torch.int64, device=DEV)
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    data, idx, pal, carry, out = buf[:1024], buf[1024:2048], buf[2048:2816], buf[4096:4096 + 96], buf[6144:6144 + 48]
    torch.cuda.synchronize()
    calls = [
        L.mmgt_gif_unlzw(p(data), 1024, p(tab), p(idx), 1024, p(st), 0, s),
        L.mmgt_gif_unlzw(p(data), 1024, p(tab), p(idx), 1024, p(st), 65536, s),
        L.mmgt_gif_unlzw(p(data), 1023, p(tab), p(idx), 1024, p(st), 1, s),
        L.mmgt_gif_unlzw(p(data), 0, p(tab), p(idx), 1024, p(st), 1, s),
        L.mmgt_gif_unlzw(p(data), 1024, p(tab), p(idx), 0, p(st), 1, s),
        L.mmgt_gif_unlzw(None, 1024, p(tab), p(idx), 1024, p(st), 1, s),
        L.mmgt_gif_compose(p(tab), p(idx), 1024, p(pal), p(carry), p(out), 0, 4, 4, s),
        L.mmgt_gif_compose(p(tab), p(idx), 1024, p(pal), p(carry), p(out), 1, 0, 4, s),
        L.mmgt_gif_compose(p(tab), p(idx), 1024, p(pal), p(carry), p(out), 1, 4, 16385, s),
        L.mmgt_gif_compose(p(tab), p(idx), 0, p(pal), p(carry), p(out), 1, 4, 4, s),
        L.mmgt_gif_compose(p(tab), p(idx), 1024, p(pal), None, p(out), 1, 4, 4, s),
    ]
    for k, rc in enumerate(calls):
        assert rc != 0, k
    for fn, args in ((L.mmgt_gif_unlzw, (p(data), 1023, p(tab), p(idx), 1024, p(st), 1, s)),
                     (L.mmgt_gif_compose, (p(tab), p(idx), 1024, p(pal), p(carry), p(out), 1, 4, 16385, s))):
        assert fn(*args) != 0 and "range" in L.mmgt_last_error().decode()
    torch.cuda.synchronize()
    assert not bool(buf.any()) and not bool(st.any())                                       # nothing was launched
    # a row that names bytes outside the buffers: a status, and nothing is touched
    row = torch.tensor([[0, 0, 4, 4, 1020, 0, 16, 8, 0, -1, 0, 0, 1, 0, 0, 0]], dtype=torch.int64, device=DEV)
    assert L.mmgt_gif_unlzw(p(data), 1024, p(row), p(idx), 1024, p(st), 1, s) == 0
    assert L.mmgt_gif_compose(p(row), p(idx), 1024, p(pal), p(carry), p(out), 1, 4, 4, s) == 0
    torch.cuda.synchronize()
    assert int(st[0]) == 4 and not bool(buf.any())
