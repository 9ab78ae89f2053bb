"""Audio input on the host: the WAV container walk, the resampling filter's design, the fp64 direct evaluation against scipy, the
filter's measured response, and csrc/audio_core.h -- the arithmetic csrc/audio.hip runs on the device -- run by tools/audio_host_check.cpp under
ASan + UBSan.  No GPU."""
import math
import os
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from mmgt_amd import audio_in as A
from tests import audio_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _noise(seed, *shape):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape)


# ------------------------------------------------------------------------------------------------------------ parse_wav

@pytest.mark.parametrize("extensible", [False, True])
@pytest.mark.parametrize("channels", [1, 2, 6])
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_parse_wav_reads_every_format_and_layout(fmt, channels, extensible):
    frames = R.encode_frames(_noise(fmt, 5, channels), fmt)
    info = A.parse_wav(R.wav_bytes(frames, fmt, channels, 44100, extensible=extensible))
    ba = channels * R.SAMPLE_BYTES[fmt]
    assert info == A.WavInfo(fmt, 8 * R.SAMPLE_BYTES[fmt], channels, 44100, 12 + 8 + (40 if extensible else 16) + 8, 5 * ba, ba)
    assert A.FORMAT_NAMES[info.fmt] == R.NAMES[fmt]


def test_parse_wav_skips_chunks_before_data_and_honours_the_pad_byte(tmp_path):
    frames = R.encode_frames(_noise(1, 9, 2), R.S16)
    before = [(b"LIST", b"INFOISFT\x05\x00\x00\x00abcde\x00"), (b"fact", struct.pack("<I", 9)), (b"bext", b"x" * 7)]      # bext: odd size + pad
    wav = R.wav_bytes(frames, R.S16, 2, 48000, before=before)
    info = A.parse_wav(wav)
    assert wav[info.data_offset - 8:info.data_offset - 4] == b"data" and wav[info.data_offset:info.data_offset + info.data_bytes] == frames
    assert info.data_offset == 12 + 24 + (8 + 18) + (8 + 4) + (8 + 7 + 1) + 8
    p = tmp_path / "a.wav"
    p.write_bytes(wav)
    assert A.parse_wav(str(p)) == info and A.parse_wav(p) == info            # a path reads the same as the bytes


@pytest.mark.parametrize("size", [0, 0xFFFFFFFF])
def test_parse_wav_streaming_data_size_means_to_the_end_of_the_file(size):
    frames = R.encode_frames(_noise(2, 11, 3), R.S24)                        # 99 bytes: odd, the writer's pad byte follows
    info = A.parse_wav(R.wav_bytes(frames, R.S24, 3, 22050, data_size=size))
    assert info.data_bytes == 99 and info.block_align == 9


def test_parse_wav_truncated_file_is_used_up_to_the_last_whole_frame():
    frames = R.encode_frames(_noise(3, 10, 2), R.F32)                        # 80 bytes in frames of 8
    info = A.parse_wav(R.wav_bytes(frames, R.F32, 2, 16000, cut=5))
    assert info.data_bytes == 72


@pytest.mark.parametrize("kwargs, match", [
    (dict(tag=2), "ADPCM"), (dict(tag=0x11), "IMA ADPCM"), (dict(tag=6), "A-law"), (dict(tag=7), "µ-law"), (dict(tag=0x55), "MPEG"),
    (dict(tag=0x50), "MPEG"), (dict(tag=0x1234), "0x1234"), (dict(tag=7, extensible=True), "µ-law"),
    (dict(bits=12, block_align=2), "12-bit PCM"), (dict(tag=3, bits=16), "16-bit IEEE float"), (dict(channels=0), "0 channels"),
    (dict(channels=17), "17 channels"), (dict(rate=0), "0 Hz"), (dict(block_align=3), "block_align 3"), (dict(riff=b"RF64"), "RF64"),
])
def test_parse_wav_refusals_name_what_they_found(kwargs, match):
    kw = dict(fmt=R.S16, channels=1, rate=16000)
    kw.update(kwargs)
    fmt, channels, rate = kw.pop("fmt"), kw.pop("channels"), kw.pop("rate")
    with pytest.raises(ValueError, match=match):
        A.parse_wav(R.wav_bytes(b"\0" * 64, fmt, channels, rate, **kw))


def test_parse_wav_refuses_a_missing_fmt_or_data_chunk():
    body = b"WAVE" + R.chunk(b"data", b"\0" * 8)
    with pytest.raises(ValueError, match="no `fmt ` chunk"):
        A.parse_wav(b"RIFF" + struct.pack("<I", len(body)) + body)
    body = b"WAVE" + R.fmt_chunk(R.S16, 1, 16000) + R.chunk(b"LIST", b"INFO")
    with pytest.raises(ValueError, match="no `data` chunk"):
        A.parse_wav(b"RIFF" + struct.pack("<I", len(body)) + body)
    with pytest.raises(ValueError, match="not a RIFF/WAVE"):
        A.parse_wav(b"OggS" + b"\0" * 40)


def test_public_names_are_exported():
    import mmgt_amd
    for name in ("parse_wav", "WavInfo", "resample_plan", "resample_device", "read_audio_device"):
        assert getattr(mmgt_amd, name) is getattr(A, name)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_pcm16_host_converts_every_format_for_a_sound_track(fmt):
    """The 16-bit track of --format avi: the file's own rate and channels, full scale 2^15, round to nearest, clip, U8 re-centred."""
    x = _noise(20 + fmt, 300, 2)
    x[:2] = [[-1.0, 1.0], [0.0, 2.0 ** -18]]
    raw = R.encode_frames(x, fmt)
    got, rate = A.pcm16_host(R.wav_bytes(raw, fmt, 2, 22050), seconds=0.01)
    stored = R.raw_values(raw, fmt, 2).astype(np.float64) if fmt not in (R.S32, R.F64) else \
        np.frombuffer(raw, dtype="<i4" if fmt == R.S32 else "<f8").astype(np.float64).reshape(-1, 2)
    full_scale = {R.U8: 2.0 ** 7, R.S16: 2.0 ** 15, R.S24: 2.0 ** 23, R.S32: 2.0 ** 31}.get(fmt, 1.0)
    want = np.clip(np.rint(stored / full_scale * 32768.0), -32768, 32767).astype(np.int16)[:220]
    assert rate == 22050 and got.dtype == np.int16 and got.shape == (220, 2) and np.array_equal(got, want)


# -------------------------------------------------------------------------------------------------------- resample_plan

def _kaiser_at(k, M, beta):
    return float(np.i0(beta * math.sqrt(max(0.0, 1.0 - (2.0 * k / (M - 1) - 1.0) ** 2))) / np.i0(beta))


@pytest.mark.parametrize("rate", R.RATES)
def test_resample_plan_ratio_length_and_tap_formula(rate):
    up, down, half, h = A.resample_plan(rate)
    fr = Fraction(16000, rate)
    assert (up, down) == (fr.numerator, fr.denominator)
    m = max(up, down)
    assert half == math.ceil(64 * m / 0.9475937167399596) and h.shape == (2 * half + 1,) and h.dtype == np.float64
    fc = 0.9475937167399596 / m
    for n in (-half, -half + 1, -m - 1, -1, 0, 1, 3, m, 2 * m + 1, half // 2, half):
        z = math.pi * fc * n
        want = up * fc * (math.sin(z) / z if n else 1.0) * _kaiser_at(n + half, 2 * half + 1, 14.769656459379492)
        assert abs(h[n + half] - want) <= 1e-12 * up * fc, (n, h[n + half], want)
    assert np.array_equal(h, h[::-1])                                        # symmetric: linear phase, no delay on the output grid
    dc = np.array([h[p::up].sum() for p in range(up)])
    assert np.abs(dc - 1.0).max() < 1e-3, np.abs(dc - 1.0).max()            # every phase passes DC with gain 1


def test_resample_plan_worked_cases_and_refusals():
    assert A.resample_plan(44100)[:2] == (160, 441) and A.resample_plan(11025)[0] == 640
    with pytest.raises(ValueError, match=r"15999 Hz -> 16000 Hz.*taps"):
        A.resample_plan(15999, 16000)
    with pytest.raises(ValueError, match=r"500 Hz -> 16000 Hz.*ratio"):
        A.resample_plan(500)
    with pytest.raises(ValueError, match=r"384000 Hz -> 16000 Hz.*ratio"):
        A.resample_plan(384000)
    A.resample_plan(256000), A.resample_plan(1000)                           # 1/16 and 16 themselves are inside


def test_phase_major_table_holds_every_tap_once():
    up, down, half, h = A.resample_plan(11025)
    q = 2 * half // up + 1
    t = A.phase_major(h, up, half).reshape(up, q)
    for p in (0, 1, 334, up - 1):
        row = h[p::up]
        assert np.array_equal(t[p, :row.shape[0]], row) and not t[p, row.shape[0]:].any()
    assert t.sum() == pytest.approx(h.sum(), rel=1e-12)


# ------------------------------------------------------------------------------------------- direct evaluation vs scipy

@pytest.mark.parametrize("rate", R.RATES)
def test_direct_evaluation_equals_scipy_resample_poly(rate):
    """scipy multiplies an explicit window by `up` itself, hence h / up; its output length is ceil(n up / down) as well."""
    from scipy.signal import resample_poly
    up, down, half, h = A.resample_plan(rate)
    for n in (1, 7, 3000):
        x = _noise(rate + n, n)
        y, _ = R.resample_direct(x, h, up, down, half)
        want = resample_poly(x, up, down, window=h / up)
        assert y.shape == want.shape == (-(-n * up // down),)
        assert np.abs(y - want).max() <= 1e-12, (rate, n, np.abs(y - want).max())


def test_filter_record_tone_gain_and_alias_leakage(capsys):
    """What the stated filter does to tones, from the fp64 evaluation (DESIGN 4r quotes these lines): the error of a 1-kHz and a 6-kHz tone
    against the same tone sampled at 16 kHz, and what is left of a 9-kHz tone (above the new Nyquist rate), away from the clip's two ends."""
    lines = []
    for rate in (44100, 48000):
        up, down, half, h = A.resample_plan(rate)
        n = rate // 4
        t_in = np.arange(n) / rate
        reach = -(-half // down) + 1                                         # outputs whose taps leave the clip
        rec = {}
        for f in (1000, 6000, 9000):
            y, _ = R.resample_direct(np.sin(2 * np.pi * f * t_in), h, up, down, half)
            inner = slice(reach, y.shape[0] - reach)
            ideal = np.sin(2 * np.pi * f * np.arange(y.shape[0]) / 16000.0) if f < 8000 else 0.0
            rec[f] = float(np.abs(y - ideal)[inner].max())
        lines.append(f"audio filter {rate} Hz -> 16 kHz: 1 kHz error {rec[1000]:.2e}, 6 kHz error {rec[6000]:.2e}, 9 kHz leakage {rec[9000]:.2e}")
        assert rec[9000] < 1e-6 and rec[1000] < 1e-6, lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ------------------------------------------------------------------------ csrc/audio_core.h on the host, ASan + UBSan

_built = []


@pytest.fixture(scope="module")
def audio_host_check(tmp_path_factory):
    """tools/audio_host_check.cpp built once under ASan + UBSan: a stand-alone program, nothing of it is loaded into Python."""
    if _built:
        return _built[0]
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler (g++ / clang++) to build tools/audio_host_check.cpp with"
    exe = tmp_path_factory.mktemp("audio_host") / "audio_host_check"
    cmd = [cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "mmgt_amd", "csrc"),
           os.path.join(ROOT, "tools", "audio_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    _built.append(str(exe))
    return _built[0]


def _host(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_host_decode_is_bitwise_the_reference_at_odd_offsets(audio_host_check, tmp_path, fmt):
    for channels, offset in ((1, 1), (2, 3), (3, 1), (6, 7), (16, 5)):
        x = _noise(10 * fmt + channels, 255, channels)
        x[:4] = [[-1.0] * channels, [1.0] * channels, [0.0] * channels, [-2.0 ** -20] * channels]          # both rails (the upper one clips), zero
        raw = R.encode_frames(x, fmt)
        (tmp_path / "in").write_bytes(struct.pack("<4q", fmt, channels, 255, offset) + raw)
        _host(audio_host_check, "decode", tmp_path / "in", tmp_path / "out")
        got = np.fromfile(tmp_path / "out", dtype=np.float32)
        want = R.decode_mono(raw, fmt, channels)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (R.NAMES[fmt], channels)
        if fmt in (R.F32, R.F64) and channels == 1:
            assert np.array_equal(got, x[:, 0].astype(np.float32))


def test_s16_mono_and_stereo_decode_is_todays_numpy_formula():
    for channels in (1, 2):
        raw = R.encode_frames(_noise(channels, 4097, channels), R.S16)
        pcm = np.frombuffer(raw, dtype="<i2").reshape(-1, channels)
        assert np.array_equal(R.decode_mono(raw, R.S16, channels), pcm.astype(np.float32).mean(1) / 32768.0)


@pytest.mark.parametrize("rate", R.RATES)
def test_host_resample_in_the_kernels_order_within_the_derived_bound(audio_host_check, tmp_path, rate):
    up, down, half, h = A.resample_plan(rate)
    table = A.phase_major(h, up, half).astype(np.float32)
    for n in (1, 7, -(-half // up) - 1, 4099):
        x = _noise(rate + n, n).astype(np.float32)
        (tmp_path / "in").write_bytes(struct.pack("<4q", up, down, half, n) + x.tobytes() + table.tobytes())
        _host(audio_host_check, "resample", tmp_path / "in", tmp_path / "out")
        got = np.fromfile(tmp_path / "out", dtype=np.float32)
        want, _ = R.resample_direct(x, h, up, down, half)
        assert got.shape == want.shape == (-(-n * up // down),)
        err, bound = np.abs(got - want), R.resample_bound(x, h, up, down, half)
        assert (err <= bound).all(), (rate, n, float((err / np.maximum(bound, 1e-300)).max()))


def test_host_index_arithmetic_is_64_bit(audio_host_check):
    """j * down passes 2^31 and 2^33: i_lo, i_hi and both end taps against Python's integers (no arrays: one hour and more of audio)."""
    for rate in (44100, 96000, 11025):
        up, down, half, _ = A.resample_plan(rate)
        js = [0, 1, half // down, half // down + 1]
        for big in (2 ** 31, 2 ** 33):
            js += [big // down - 1, big // down, big // down + 1, big // down + 257]
        n_in = (2 ** 33 // down + 300) * down // up + 1
        js += [-(-n_in * up // down) - 1]                                    # the last output
        out = _host(audio_host_check, "index", up, down, half, n_in, *js)
        rows = [tuple(map(int, line.split())) for line in out.strip().splitlines()]
        assert len(rows) == len(js)
        for j, row in zip(js, rows):
            c = j * down
            i_lo, i_hi = max(0, -((half - c) // up)), min(n_in - 1, (c + half) // up)
            assert row == (j, i_lo, i_hi, c - i_hi * up + half, c - i_lo * up + half), (rate, j)
            assert 0 <= row[3] <= row[4] <= 2 * half
