"""mmgt_gif_dither and mmgt_gif_delta (csrc/gif.hip) on the GPU against the plain loops of tests/gif_dither_ref.py, index for index: the rule is
integer arithmetic in a fixed order, so nothing is tolerated.  Then the layers above: encode_gif_frames across sets of launches, and
save_videos_grid(gif_encoder="device", gif_dither="fs", gif_delta=True) read back by PIL and by the project's device reader."""
import numpy as np
import pytest
import torch
from PIL import Image

from mmgt_amd.video_out import gif_lut, gif_palette
from tests import gif_dither_ref as R
from tests.test_gif_dither import SIZES, _hist_of

pytestmark = pytest.mark.gpu
GUARD = 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sizes():
    from mmgt_amd import hip
    return SIZES + [(hip.gif_dither_band() + 1, 9)]


_cache = {}


def _case(H, W):
    """Three frames of different content in one call, and the reference index maps against a median-cut palette and a two-entry one."""
    if (H, W) not in _cache:
        rng = np.random.default_rng(1000 * H + W)
        frames = np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), R.ramp(H, W),
                           rng.integers(0, 2, (H, W, 3), dtype=np.uint8) * 255])
        cut = gif_palette(_hist_of(frames))
        two = np.zeros((256, 3), np.uint8)
        two[1] = 255
        tables = {}
        for name, palette in (("cut", cut), ("two", two)):
            lut = gif_lut(palette)
            want = R.dither(frames, lut, palette)
            want.setflags(write=False)
            tables[name] = (palette, lut, want)
        _cache[(H, W)] = (frames, tables)
    return _cache[(H, W)]


def test_the_band_is_the_headers():
    from mmgt_amd import hip
    from tests.test_gif_dither import band_rows
    assert hip.gif_dither_band() == band_rows()
    assert hip.gif_dither_scratch_bytes(3, hip.gif_dither_band(), 9) == 0
    assert hip.gif_dither_scratch_bytes(3, hip.gif_dither_band() + 1, 9) == 4 * 3 * 9


@pytest.mark.parametrize("k", range(8))
def test_dither_equals_the_rule(k):
    from mmgt_amd import hip
    H, W = _sizes()[k]
    frames, tables = _case(H, W)
    for name, (palette, lut, want) in tables.items():
        got = hip.gif_dither(_dev(frames), _dev(lut), _dev(palette)).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == want.shape
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{H} x {W}, palette {name}: {len(bad)} indices differ, the first at (frame, y, x) = {bad[0].tolist()}"
    assert len(np.unique(tables["two"][2])) == 2 or H * W < 4                                 # both clamps fired: black and white both came out


@pytest.mark.parametrize("k", [4, 7])
def test_nothing_leaks_between_frames_or_calls(k):
    from mmgt_amd import hip
    H, W = _sizes()[k]
    frames, tables = _case(H, W)
    palette, lut, want = tables["cut"]
    x, lut_d, pal_d = _dev(frames), _dev(lut), _dev(palette)
    n = frames.shape[0]
    runs = []
    for fill in (0x00, 0xFF):
        buf = torch.full((n * H * W + GUARD,), 0xA5 ^ fill, device="cuda", dtype=torch.uint8)
        scratch = torch.full((max(4, hip.gif_dither_scratch_bytes(n, H, W)) + GUARD,), fill, device="cuda", dtype=torch.uint8)
        out = hip.gif_dither(x, lut_d, pal_d, out=buf[:n * H * W].view(n, H, W), scratch=scratch[:scratch.numel() - GUARD])
        assert out.data_ptr() == buf.data_ptr()
        assert (buf[n * H * W:] == (0xA5 ^ fill)).all() and (scratch[scratch.numel() - GUARD:] == fill).all()
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], want)
    # a frame's map does not depend on its neighbours in the call
    alone = hip.gif_dither(x[1:2].clone(), lut_d, pal_d).cpu().numpy()                        # a copy: frames are 4-byte aligned
    assert np.array_equal(alone[0], want[1])


def test_dither_refuses_bad_arguments():
    from mmgt_amd import hip
    L = hip.lib()
    band = hip.gif_dither_band()
    x = torch.zeros((1, band + 1, 8, 3), device="cuda", dtype=torch.uint8)
    lut = torch.zeros(32768, device="cuda", dtype=torch.uint8)
    pal = torch.zeros((256, 3), device="cuda", dtype=torch.uint8)
    idx = torch.full((1, band + 1, 8), 7, device="cuda", dtype=torch.uint8)
    scr = torch.zeros(64, device="cuda", dtype=torch.uint8)
    p = lambda t: t.data_ptr()
    assert L.mmgt_gif_dither(p(x), p(lut), p(pal), p(idx), p(scr), 31, 1, band + 1, 8, None) != 0 and b"scratch" in L.mmgt_last_error()
    assert L.mmgt_gif_dither(p(x), p(lut), p(pal), p(idx), None, 0, 1, band + 1, 8, None) != 0
    assert L.mmgt_gif_dither(p(x), p(lut), None, p(idx), p(scr), 64, 1, band + 1, 8, None) != 0
    assert L.mmgt_gif_dither(p(x), p(lut), p(pal), p(idx), p(scr), 64, 1, 70000, 8, None) != 0 and b"range" in L.mmgt_last_error()
    assert L.mmgt_gif_dither(p(x) + 1, p(lut), p(pal), p(idx), p(scr), 64, 1, band + 1, 8, None) != 0 and b"aligned" in L.mmgt_last_error()
    assert L.mmgt_gif_delta(p(idx), None, p(idx), 1, band + 1, 8, None) != 0
    torch.cuda.synchronize()
    assert (idx == 7).all()


# ---- frame differencing --------------------------------------------------------------------------------------------------------------------------
def _moving_clip(n=5, H=23, W=31):
    rng = np.random.default_rng(77)
    idx = np.repeat(rng.integers(0, 255, (1, H, W), dtype=np.uint8), n, axis=0)
    for f in range(n):
        idx[f, 2 + 3 * f:8 + 3 * f, 1 + 4 * f:9 + 4 * f] = 200 + f
    return idx


def test_delta_equals_the_rule():
    from mmgt_amd import hip
    same = np.repeat(np.random.default_rng(2).integers(0, 255, (1, 9, 13), dtype=np.uint8), 3, axis=0)
    got = hip.gif_delta(_dev(same)).cpu().numpy()
    assert np.array_equal(got[0], same[0]) and (got[1:] == 255).all()                         # frame 0 untouched, identical frames all transparent
    one = same.copy()
    one[2, 4, 5] ^= 1
    got = hip.gif_delta(_dev(one)).cpu().numpy()
    assert np.array_equal(got, R.delta(one)) and (got[2] != 255).sum() == 1 and got[2, 4, 5] == one[2, 4, 5]
    for clip in (_moving_clip(), _moving_clip(4, 16, 32), np.random.default_rng(3).integers(0, 3, (6, 7, 5), dtype=np.uint8)):
        assert np.array_equal(hip.gif_delta(_dev(clip)).cpu().numpy(), R.delta(clip))
    # with the frame before: what a clip cut into parts needs
    clip = _moving_clip()
    d = _dev(clip)
    parts = torch.cat([hip.gif_delta(d[:2].clone()), hip.gif_delta(d[2:].clone(), prev=d[1])])            # copies: idx is 4-byte aligned
    assert np.array_equal(parts.cpu().numpy(), R.delta(clip))


def _static_clip():
    """4 frames of 64 x 48: a static noise background and a moving 8 x 8 square."""
    rng = np.random.default_rng(31)
    frames = np.repeat(rng.integers(0, 256, (1, 48, 64, 3), dtype=np.uint8), 4, axis=0)
    for f in range(4):
        frames[f, 6 + 7 * f:14 + 7 * f, 5 + 12 * f:13 + 12 * f] = (240, 40, 10 + 60 * f)
    return frames


def _decode_blobs(palette, blobs, H, W):
    from tests.test_gif import lzw_decode, unblock
    return np.stack([lzw_decode(unblock(b), H * W).reshape(H, W) for b in blobs])


def test_delta_runs_across_the_sets_of_launches(monkeypatch):
    from mmgt_amd import video_out
    frames = _static_clip()
    for dither in (None, "fs"):
        palette, blobs = video_out.encode_gif_frames(frames, dither=dither, delta=True)
        assert not palette[255].any()
        lut = gif_lut(palette, colors=255)
        idx = R.dither(frames, lut, palette) if dither else R.undithered(frames, lut)
        assert np.array_equal(_decode_blobs(palette, blobs, 48, 64), R.delta(idx))
        with monkeypatch.context() as m:
            m.setattr(video_out, "GIF_SCRATCH_BYTES", 1)                                      # one frame per set of launches
            pal1, blobs1 = video_out.encode_gif_frames(frames, dither=dither, delta=True)
        assert np.array_equal(pal1, palette) and blobs1 == blobs


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
def _pil_frames(path):
    img = Image.open(path)
    out = []
    for k in range(img.n_frames):
        img.seek(k)
        out.append(np.asarray(img.convert("RGB")).copy())
    return np.stack(out)


def test_save_videos_grid_dithered_and_differenced(tmp_path):
    from mmgt_amd import video_in, video_out
    frames = _static_clip()
    clip = torch.from_numpy(frames)[None]                                                     # (b, t, h, w, 3) uint8
    assert np.array_equal(video_out.frames_uint8(clip, 1), frames)
    path = tmp_path / "fd.gif"
    video_out.save_videos_grid(clip, str(path), n_rows=1, fps=25, gif_encoder="device", gif_dither="fs", gif_delta=True)
    palette = gif_palette(_hist_of(frames), colors=255)
    idx = R.dither(frames, gif_lut(palette, colors=255), palette)
    assert int(idx.max()) <= 254
    want = palette[idx]
    assert np.array_equal(R.compose(R.delta(idx), palette), want)
    assert np.array_equal(_pil_frames(path), want)
    assert np.array_equal(video_in.read_frames_device(str(path)).cpu().numpy(), want)
    # differencing alone: static noise costs a code per pixel when it is coded, and is one run when it is transparent
    sizes = {}
    for delta in (False, True):
        p = tmp_path / f"d{int(delta)}.gif"
        video_out.save_videos_grid(clip, str(p), n_rows=1, fps=25, gif_encoder="device", gif_delta=delta)
        sizes[delta] = p.stat().st_size
        pal = gif_palette(_hist_of(frames), colors=255 if delta else 256)
        assert np.array_equal(_pil_frames(p), pal[R.undithered(frames, gif_lut(pal, colors=255 if delta else 256))])
    print(f"file bytes: {sizes[False]} coded in full, {sizes[True]} differenced")
    assert sizes[True] < sizes[False]


def test_pose2vid_synthetic_takes_the_options(tmp_path):
    import json
    import os
    import subprocess
    import sys
    from tests.host_check import ROOT
    from tests.test_gif import _walk
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pose2vid.py"), "--synthetic", "-W", "64", "-H", "64", "-L", "8", "--steps", "2",
                        "--format", "gif", "--gif_encoder", "device", "--gif_dither", "fs", "--gif_delta", "--out_dir", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    _, table, items = _walk(open(rec["gif"], "rb").read())
    gces = [v for k, v in items if k == "gce"]
    assert len(gces) == 8 and gces[0] == (0x04, 4, 0) and all(g == (0x05, 4, 255) for g in gces[1:])
    assert table[765:768] == b"\0\0\0"                                                        # 255 colours: entry 255 is not a colour
    frames = _pil_frames(rec["gif"])
    assert frames.shape == (8, 64, 64, 3) and frames[7].std() > 0


def test_defaults_write_what_they_wrote(tmp_path):
    from mmgt_amd import video_out
    frames = _static_clip()
    clip = torch.from_numpy(frames)[None]                                                     # (b, t, h, w, 3) uint8
    a, b, c = tmp_path / "a.gif", tmp_path / "b.gif", tmp_path / "c.gif"
    video_out.save_videos_grid(clip, str(a), n_rows=1, fps=25, gif_encoder="device")
    palette, blobs = video_out.encode_gif_frames(frames)
    video_out.write_gif(str(b), palette, blobs, 64, 48, 25)
    video_out.save_videos_grid(clip, str(c), n_rows=1, fps=25, gif_encoder="device", gif_dither=None, gif_delta=False)
    assert a.read_bytes() == b.read_bytes() == c.read_bytes()
    assert np.array_equal(palette, gif_palette(_hist_of(frames)))
    assert np.array_equal(_pil_frames(a), palette[R.undithered(frames, gif_lut(palette))])
