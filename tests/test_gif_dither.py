"""Dithering and frame differencing of the device GIF writer without a GPU: what the rule of tests/gif_dither_ref.py does to a ramp,
a flat grey and pure colours; gif_palette / gif_lut with colors=255; write_gif(..., transparent=255) block by block and through PIL; the argument
checks; and tools/gif_dither_host_check.cpp, which proves the kernel's lane / step schedule equal to the serial rule under ASan and UBSan."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

from mmgt_amd import video_out
from mmgt_amd.video_out import gif_lut, gif_palette, write_gif
from tests import gif_dither_ref as R
from tests.host_check import ROOT
from tests.test_gif import _walk, lzw_decode, lzw_encode, sub_blocks

SIZES = [(1, 1), (1, 7), (7, 1), (2, 3), (35, 67), (96, 128), (600, 5)]                      # and (rows of one band + 1, 9)


def _hist_of(frames):
    f = frames.reshape(-1, 3).astype(np.int64)
    return np.bincount((f[:, 0] >> 3) << 10 | (f[:, 1] >> 3) << 5 | (f[:, 2] >> 3), minlength=32768)


def _block_error(idx, palette, source):
    """Mean absolute error of the 8 x 8 block means of palette[idx] against the source's."""
    H, W, _ = source.shape
    blocks = lambda a: a.astype(np.float64).reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3))
    return float(np.abs(blocks(palette[idx]) - blocks(source)).mean())


# ---- the rule --------------------------------------------------------------------------------------------------------------------------------------
def test_dithering_brings_the_block_means_of_a_ramp_closer():
    src = R.ramp()
    palette = gif_palette(_hist_of(src))
    lut = gif_lut(palette)
    plain = _block_error(R.undithered(src[None], lut)[0], palette, src)
    fs = _block_error(R.dither_frame(src, lut, palette), palette, src)
    print(f"block-mean error: undithered {plain:.3f}, dithered {fs:.3f}, ratio {fs / plain:.3f}")
    assert fs <= 0.6 * plain                                                                  # the rule gives 0.524 against 1.192


def test_flat_grey_becomes_the_right_share_of_white():
    palette = np.zeros((256, 3), np.uint8)
    palette[1] = 255
    idx = R.dither_frame(np.full((32, 48, 3), 64, np.uint8), gif_lut(palette), palette)
    assert set(np.unique(idx)) <= {0, 1}
    share = float((idx == 1).mean())
    print(f"share of white: {share:.4f} (64 / 255 = {64 / 255:.4f})")
    assert abs(share - 64 / 255) <= 0.01                                                      # the rule gives 0.2487


def test_colours_that_are_palette_entries_are_not_dithered():
    colours = np.array([[4, 4, 4], [252, 4, 4], [4, 252, 4], [4, 4, 252]], np.uint8)          # centres of their bins: entries of case (1)
    src = np.repeat(colours[None, :, :], 12, axis=1).repeat(10, axis=0)                       # four bars
    palette = gif_palette(_hist_of(src))
    assert all(tuple(c) in {tuple(p) for p in palette[:4]} for c in colours)
    lut = gif_lut(palette)
    assert np.array_equal(R.dither_frame(src, lut, palette), R.undithered(src[None], lut)[0])


# ---- 255 colours -----------------------------------------------------------------------------------------------------------------------------------
def _hist_with_bins(nbins, seed):
    rng = np.random.default_rng(seed)
    h = np.zeros(32768, np.int64)
    h[rng.choice(32768, nbins, replace=False)] = rng.integers(1, 1000, nbins)
    return h


@pytest.mark.parametrize("nbins", [255, 256, 300])
def test_255_colours_leave_entry_255_zero_and_unused(nbins):
    h = _hist_with_bins(nbins, nbins)
    palette = gif_palette(h, colors=255)
    assert palette.shape == (256, 3) and palette.dtype == np.uint8 and not palette[255].any()
    lut = gif_lut(palette, colors=255)
    assert lut.shape == (32768,) and lut.dtype == np.uint8 and int(lut.max()) <= 254
    if nbins == 255:                                                                          # rule (1): every occupied bin has its own entry
        occ = np.flatnonzero(h)
        assert np.array_equal(palette[:255], np.stack([8 * (occ >> 10) + 4, 8 * ((occ >> 5) & 31) + 4, 8 * (occ & 31) + 4], axis=1))
        assert np.array_equal(lut[occ], np.arange(255))
    else:                                                                                     # the split stopped at 255 boxes
        assert len({tuple(c) for c in palette[:255]}) == 255
    centre = 8 * np.arange(32) + 4                                                            # the arg-min over entries 0 .. 254, lowest index on a tie
    for b in np.random.default_rng(1).choice(32768, 200, replace=False):
        c = np.array([centre[b >> 10], centre[(b >> 5) & 31], centre[b & 31]])
        assert lut[b] == int(np.argmin(((palette[:255].astype(np.int64) - c) ** 2).sum(1)))


@pytest.mark.parametrize("nbins", [3, 256, 300])
def test_256_colours_are_the_default(nbins):
    h = _hist_with_bins(nbins, 7 + nbins)
    palette = gif_palette(h)
    assert np.array_equal(gif_palette(h, colors=256), palette) and np.array_equal(gif_palette(h, 256), palette)
    assert np.array_equal(gif_lut(palette, colors=256), gif_lut(palette))
    from tests.test_gif import palette_by_the_rule
    assert np.array_equal(palette, palette_by_the_rule(h))                                    # and the default is what it was


def test_colors_other_than_255_and_256_raise():
    h = _hist_with_bins(10, 3)
    for bad in (0, 128, 257, None):
        with pytest.raises(ValueError, match="colors"):
            gif_palette(h, colors=bad)
        with pytest.raises(ValueError, match="colors"):
            gif_lut(np.zeros((256, 3), np.uint8), colors=bad)


# ---- the container ---------------------------------------------------------------------------------------------------------------------------------
def _delta_clip():
    rng = np.random.default_rng(12)
    idx = np.repeat(rng.integers(0, 255, (1, 24, 40), dtype=np.uint8), 4, axis=0)             # a still background of indices 0 .. 254
    for f in range(4):
        idx[f, 4 + 3 * f:10 + 3 * f, 5 + 6 * f:13 + 6 * f] = 17 + f                           # a square that moves
    palette = np.stack([np.random.default_rng(3).permutation(256), np.arange(256)[::-1], np.arange(256)], axis=1).astype(np.uint8)
    palette[255] = 0
    return idx, palette


def test_write_gif_transparent_blocks_and_what_pil_composes(tmp_path):
    idx, palette = _delta_clip()
    coded = R.delta(idx)
    assert (coded[0] == idx[0]).all() and (coded[1:] == 255).mean() > 0.8
    blobs = [sub_blocks(lzw_encode(f)[0]) for f in coded]
    path = tmp_path / "d.gif"
    assert write_gif(str(path), palette, blobs, 40, 24, 25, transparent=255) == path.stat().st_size
    _, table, items = _walk(path.read_bytes())
    assert table == palette.tobytes() and [k for k, _ in items] == ["app"] + ["gce", "image"] * 4
    assert items[1][1] == (0x04, 4, 0)                                                        # frame 0: leave in place, nothing transparent
    for k in range(1, 4):
        assert items[1 + 2 * k][1] == (0x05, 4, 255)                                          # later frames: leave in place, index 255 transparent
        assert np.array_equal(lzw_decode(items[2 + 2 * k][1][2], 24 * 40).reshape(24, 40), coded[k])
    want = R.compose(coded, palette)
    assert np.array_equal(want, palette[idx])                                                 # differencing loses nothing
    img = Image.open(path)
    assert img.n_frames == 4
    for k in range(4):
        img.seek(k)
        assert np.array_equal(np.asarray(img.convert("RGB")), want[k]), k


def test_write_gif_without_transparent_writes_the_bytes_it_wrote(tmp_path):
    idx, palette = _delta_clip()
    blobs = [sub_blocks(lzw_encode(f)[0]) for f in idx]
    want = (b"GIF89a" + struct.pack("<HHBBB", 40, 24, 0xF7, 0, 0) + palette.tobytes() + b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"
            + b"".join(b"\x21\xf9\x04\x00" + struct.pack("<H", 4) + b"\x00\x00" + b"\x2c" + struct.pack("<HHHHB", 0, 0, 40, 24, 0) + b"\x08" + b
                       for b in blobs) + b"\x3b")
    for kw in ({}, {"transparent": None}):
        path = tmp_path / "p.gif"
        write_gif(str(path), palette, blobs, 40, 24, 25, **kw)
        assert path.read_bytes() == want
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="transparent"):
            write_gif(str(tmp_path / "q.gif"), palette, blobs, 40, 24, 25, transparent=bad)


# ---- argument checks (refused before anything touches a GPU) ---------------------------------------------------------------------------------------
def test_bad_options_raise(tmp_path):
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="dither"):
        video_out.encode_gif_frames(frames, dither="bayer")
    with pytest.raises(ValueError, match="dither"):
        video_out.encode_gif_frames(frames, dither=True)
    palette = np.full((256, 3), 9, np.uint8)
    with pytest.raises(ValueError, match="row 255"):
        video_out.encode_gif_frames(frames, palette=palette, delta=True)
    clip = np.zeros((1, 3, 2, 8, 8), np.float32)
    with pytest.raises(ValueError, match="gif_encoder='device'"):
        video_out.save_videos_grid(clip, str(tmp_path / "a.gif"), gif_dither="fs")
    with pytest.raises(ValueError, match="gif_encoder='device'"):
        video_out.save_videos_grid(clip, str(tmp_path / "a.gif"), gif_encoder="pil", gif_delta=True)
    with pytest.raises(ValueError, match="gif_dither"):
        video_out.save_videos_grid(clip, str(tmp_path / "a.gif"), gif_encoder="device", gif_dither="ordered")
    assert not (tmp_path / "a.gif").exists()


# ---- the host program ------------------------------------------------------------------------------------------------------------------------------
def band_rows():
    """GDI_BAND of csrc/gif_dither_core.h: the rows of one band of the kernel."""
    text = open(os.path.join(ROOT, "mmgt_amd", "csrc", "gif_dither_core.h")).read()
    return int(re.search(r"GDI_BAND\s*=\s*(\d+)", text).group(1))


def test_host_program_proves_the_schedule_equal_to_the_rule(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/gif_dither_host_check.cpp with"
    exe = tmp_path / "gif_dither_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "gif_dither_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    sizes = SIZES + [(band_rows() + 1, 9)]
    r = subprocess.run([str(exe)] + [str(v) for hw in sizes for v in hw], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("schedule == rule") == len(sizes)
