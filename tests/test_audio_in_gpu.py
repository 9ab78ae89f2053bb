"""Audio input on the device (csrc/audio.hip): decode + down-mix bit for bit against tests/audio_ref.py, the polyphase resampler
against the fp64 evaluation of its defining sum within a derived bound, the 16-kHz bypass, a file end to end, and scripts/audio2vid.py with
--audio_decoder device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmgt_amd import audio_in as A
from tests import audio_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _noise(seed, *shape):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape)


def _guarded(n):
    """(n + 2 GUARD,) floats of NaN on the device and the view of the middle n a kernel is to fill."""
    full = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    return full, full[GUARD:GUARD + n]


def _guards_intact(full, n):
    return bool(torch.isnan(full[:GUARD]).all() and torch.isnan(full[GUARD + n:]).all())


# --------------------------------------------------------------------------------------------------------------- decode

@pytest.mark.parametrize("fmt", R.FORMATS)
def test_decode_mono_is_bitwise_the_reference_and_stays_in_bounds(fmt):
    """Every format x {1, 2, 3, 6} channels x {1, 255, 4097} frames (a lone frame, a partial workgroup, a partial last one of several; frames of
    3, 9 and 18 bytes among them), the bytes starting at every residue of the address mod 4."""
    from mmgt_amd import hip
    for channels in (1, 2, 3, 6):
        for n in (1, 255, 4097):
            x = _noise(100 * fmt + 10 * channels + n % 7, n, channels)
            x[0] = -1.0
            x[-1] = 1.0                                                     # the rails: the upper one clips in the integer formats
            raw = R.encode_frames(x, fmt)
            skew = (channels + n) % 4
            buf = torch.frombuffer(bytearray(b"\xa5" * skew + raw), dtype=torch.uint8).cuda()
            full, out = _guarded(n)
            hip.audio_decode_mono(buf[skew:], n, channels, fmt, out=out)
            torch.cuda.synchronize()
            want = R.decode_mono(raw, fmt, channels)
            assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), (R.NAMES[fmt], channels, n)
            assert _guards_intact(full, n), (R.NAMES[fmt], channels, n)


# ------------------------------------------------------------------------------------------------------------- resample

@pytest.mark.parametrize("rate", R.RATES)
def test_resample_against_the_fp64_sum_within_the_derived_bound(rate):
    """Lengths: 1, 7, one shorter than a single tap span, 4 099, and 70 001 (several workgroups, both edges).  Two runs into NaN-filled
    outputs are bitwise equal, the guard floats stay NaN, and n_out = ceil(n_in up / down)."""
    from mmgt_amd import hip
    up, down, half, h = A.resample_plan(rate)
    table = torch.from_numpy(A.phase_major(h, up, half).astype(np.float32)).cuda()
    for n in (1, 7, -(-half // up) - 1, 4099, 70001):
        x = _noise(rate + n, n).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        n_out = -(-n * up // down)
        runs = []
        for _ in range(2):
            full, out = _guarded(n_out)
            got = hip.audio_resample(xd, table, up, down, half, out=out)
            torch.cuda.synchronize()
            assert got.shape == (n_out,) and _guards_intact(full, n_out), (rate, n)
            runs.append(out.cpu().numpy())
        assert np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32)), (rate, n)
        want, _ = R.resample_direct(x, h, up, down, half)
        err, bound = np.abs(runs[0] - want), R.resample_bound(x, h, up, down, half)
        print(f"resample {rate} Hz, n_in {n}: max |err| {err.max():.3e}, max err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert np.isfinite(runs[0]).all() and (err <= bound).all(), (rate, n, float((err / np.maximum(bound, 1e-300)).max()))
    assert hip.audio_resample(xd, table, up, down, half).shape == (n_out,)              # and it allocates its own output


def test_resample_device_builds_one_table_per_pair_of_rates():
    x = torch.from_numpy(_noise(5, 1000).astype(np.float32)).cuda()
    y = A.resample_device(x, 48000)
    assert y.shape == (334,) and y.dtype == torch.float32
    table = A.plan_cache()[(48000, 16000, "cuda:0")][3]
    A.resample_device(x, 48000)
    assert A.plan_cache()[(48000, 16000, "cuda:0")][3] is table and table.dtype == torch.float32 and table.shape == (2 * 203 + 1,)


# --------------------------------------------------------------------------------------------------------------- bypass

@pytest.mark.parametrize("channels", [1, 2])
def test_16k_s16_file_is_todays_reader_bit_for_bit_and_builds_no_table(tmp_path, channels):
    from mmgt_amd import hip
    raw = R.encode_frames(_noise(channels, 4097, channels) * 0.9, R.S16)
    path = tmp_path / "a.wav"
    path.write_bytes(R.wav_bytes(raw, R.S16, channels, 16000))
    plans, launches = dict(A.plan_cache()), hip.call_count("mmgt_audio_resample")
    got = A.read_audio_device(str(path))
    pcm = np.frombuffer(raw, dtype="<i2").reshape(-1, channels)
    want = pcm.astype(np.float32).mean(1) / 32768.0                          # scripts/audio2vid.py: read_wav_16k
    assert got.device.type == "cuda" and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    assert A.plan_cache() == plans and not [k for k in A.plan_cache() if k[0] == 16000]
    assert hip.call_count("mmgt_audio_resample") == launches


# ----------------------------------------------------------------------------------------------------------- end to end

def test_read_audio_device_44k1_stereo_24_bit_against_the_composed_reference(tmp_path):
    n = 22050                                                               # 0.5 s
    raw = R.encode_frames(_noise(7, n, 2) * 0.7, R.S24)
    path = tmp_path / "s24.wav"
    path.write_bytes(R.wav_bytes(raw, R.S24, 2, 44100, extensible=True, before=[(b"LIST", b"INFOxyz")]))
    got = A.read_audio_device(str(path)).cpu().numpy()
    up, down, half, h = A.resample_plan(44100)
    mono = R.decode_mono(raw, R.S24, 2)
    want, _ = R.resample_direct(mono, h, up, down, half)
    assert got.shape == want.shape == (8000,)
    assert (np.abs(got - want) <= R.resample_bound(mono, h, up, down, half)).all()
    short = A.read_audio_device(str(path), max_seconds=0.1).cpu().numpy()    # 4 410 frames of the start
    assert short.shape == (1600,) and np.array_equal(short[:1000], got[:1000])          # beyond the filter's reach of the cut: the same sums


# --------------------------------------------------------------------------------------------------------------- script

def _run(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "audio2vid.py"), *args], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_audio2vid_takes_a_44k1_file_with_the_device_decoder(tmp_path):
    t = np.arange(44100) / 44100.0
    raw = R.encode_frames((0.4 * np.sin(2 * np.pi * 220 * t))[:, None], R.S16)
    (tmp_path / "b.wav").write_bytes(R.wav_bytes(raw, R.S16, 1, 44100))
    rec = _run("--synthetic", "--audio_path", str(tmp_path / "b.wav"), "--audio_decoder", "device", "-W", "64", "-H", "64", "-L", "8", "--steps", "1",
               "--out_dir", str(tmp_path))
    assert rec["video"] == [1, 8, 64, 64, 3] and rec["keypoints_finite"]
    assert rec["audio"] == {"rate": 44100, "channels": 1, "fmt": "S16", "samples_16k": 16000}


def test_audio2vid_avi_sound_track_from_a_24_bit_stereo_file(tmp_path):
    """The .avi's 01wb chunks hold 16-bit PCM at the file's own rate and channel count: the 24-bit samples / 2^8 rounded to nearest (ties to
    even), the first L / fps seconds."""
    from mmgt_amd.inputs import _riff_chunks
    n = 22050
    x = _noise(11, n, 2) * 0.8
    x[:3] = [[-1.0, 1.0], [1.0, -1.0], [0.0, 0.0]]                          # the rails: +1 clips at 2^23 - 1, which rounds up to 32768 and clips again
    raw = R.encode_frames(x, R.S24)
    (tmp_path / "c.wav").write_bytes(R.wav_bytes(raw, R.S24, 2, 44100))
    rec = _run("--synthetic", "--audio_path", str(tmp_path / "c.wav"), "--audio_decoder", "device", "--format", "avi", "-W", "64", "-H", "64", "-L", "8",
               "--steps", "1", "--out_dir", str(tmp_path))
    assert rec["audio"]["fmt"] == "S24" and rec["audio"]["channels"] == 2 and rec["audio"]["samples_16k"] == 8000
    buf = open(rec["saved"], "rb").read()
    pcm = b""
    for cc, off, size in _riff_chunks(buf, 12, len(buf)):
        if cc == b"LIST" and buf[off:off + 4] == b"movi":
            pcm = b"".join(buf[o:o + s] for c, o, s in _riff_chunks(buf, off + 4, off + size) if c == b"01wb")
    got = np.frombuffer(pcm, dtype="<i2").reshape(-1, 2)
    v24 = np.clip(np.rint(x * 8388608), -8388608, 8388607)
    keep = int(round(8 / 25 * 44100))
    want = np.clip(np.rint(v24 / 256.0), -32768, 32767).astype(np.int16)[:keep]
    assert got.shape == (keep, 2) and np.array_equal(got, want)
