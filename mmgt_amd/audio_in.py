"""Audio input: any PCM / IEEE-float WAV file as the mono 16-kHz fp32 waveform the wav2vec2 and WavLM extractors take -- the place of
librosa.load(path, sr=16000) in the reference (data/audio_extraction/wavlm_features.py:61,128, src/dataset/audio_processor.py:106,142).

Host glue only: the RIFF walk, the filter design (fp64, once per pair of rates) and the launches' bookkeeping.  The samples are decoded, mixed
down and resampled on the device (csrc/audio.hip through mmgt_amd.hip): one host-to-device copy of the `data` bytes, one decode launch, at most
one resample launch.

The filter is NOT librosa's.  librosa resamples with soxr ("soxr_hq"), whose coefficients are not published in a form anyone can restate, and
neither library is part of this build; the target here is a stated mathematical filter -- the Kaiser-windowed sinc with resampy's published
`kaiser_best` parameters, evaluated exactly as resample_plan's docstring writes it -- and the tests hold the device to THAT filter in fp64, not to
librosa's bits.

Edges: the whole file is resampled (zeros beyond both ends), then cut at 16 kHz by wavlm.audio_slices.  The reference cuts at the file's own rate
and resamples each 3.2-s slice, so the two differ only within the filter's reach (64 zero crossings, 4 ms at 16 kHz) of a slice edge.
"""
import math
from collections import namedtuple

import numpy as np

U8, S16, S24, S32, F32, F64 = range(6)                      # csrc/audio_core.h
FORMAT_NAMES = ("U8", "S16", "S24", "S32", "F32", "F64")
MAX_CHANNELS = 16
_PCM_BITS = {8: U8, 16: S16, 24: S24, 32: S32}
_FLOAT_BITS = {32: F32, 64: F64}
_TAG_NAMES = {0x0002: "Microsoft ADPCM", 0x0006: "A-law", 0x0007: "mu-law (µ-law)", 0x0011: "IMA ADPCM", 0x0050: "MPEG", 0x0055: "MPEG layer 3 (mp3)"}

WavInfo = namedtuple("WavInfo", "fmt bits channels rate data_offset data_bytes block_align")

# resampy's published `kaiser_best` design: zero crossings, Kaiser beta, roll-off (fraction of the Nyquist rate)
KAISER_ZEROS, KAISER_BETA, KAISER_ROLLOFF = 64, 14.769656459379492, 0.9475937167399596
MAX_TAPS = 1 << 21          # 8 MiB of fp32: 44.1 -> 16 kHz has 59 571 taps, 11.025 -> 16 kHz 86 453; 15 999 -> 16 000 Hz would have 2 161 265
MAX_RATIO = 16


def _chunks(buf, start, end):
    """(fourcc, body offset, stated body size) of the RIFF chunks in buf[start:end]; a chunk of odd size is followed by one pad byte."""
    pos = start
    while pos + 8 <= end:
        size = int.from_bytes(buf[pos + 4:pos + 8], "little")
        yield bytes(buf[pos:pos + 4]), pos + 8, size
        pos += 8 + size + (size & 1)


def parse_wav(path_or_bytes):
    """WavInfo of a RIFF/WAVE file (a path, or its bytes): sample format (U8 .. F64), bit depth, channels, rate, and the byte range of the `data`
    chunk cut to whole frames.  Format tags 1 (PCM), 3 (IEEE float) and 0xFFFE (EXTENSIBLE, resolved through its sub-format GUID); chunks before
    `data` are skipped (LIST, fact, bext, ...); a `data` size of 0 or 0xFFFFFFFF (a streaming writer) and a `data` chunk that the file's end cuts
    short both mean "to the end of the file".  Everything else is a ValueError that names what was found."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        buf, what = path_or_bytes, "wav bytes"
    else:
        what = str(path_or_bytes)
        with open(path_or_bytes, "rb") as fh:
            buf = fh.read()
    if buf[:4] == b"RF64" or buf[:4] == b"BW64":
        raise ValueError(f"parse_wav: {what} is an RF64 file (64-bit sizes), which this reader does not take")
    if len(buf) < 12 or buf[:4] != b"RIFF" or buf[8:12] != b"WAVE":
        raise ValueError(f"parse_wav: {what} is not a RIFF/WAVE file (it starts with {bytes(buf[:12])!r})")
    fmt = data = None
    for cc, off, size in _chunks(buf, 12, len(buf)):
        if cc == b"fmt " and fmt is None:
            fmt = (off, min(size, len(buf) - off))
        elif cc == b"data":
            data = (off, size)
            break                                                       # the samples end the walk: a streaming size says nothing about what follows
    if fmt is None:
        raise ValueError(f"parse_wav: {what} has no `fmt ` chunk before its samples")
    if data is None:
        raise ValueError(f"parse_wav: {what} has no `data` chunk")
    off, size = fmt
    if size < 16:
        raise ValueError(f"parse_wav: {what}: the `fmt ` chunk holds {size} bytes, a WAVEFORMAT needs 16")
    tag, channels = int.from_bytes(buf[off:off + 2], "little"), int.from_bytes(buf[off + 2:off + 4], "little")
    rate = int.from_bytes(buf[off + 4:off + 8], "little")
    block_align, bits = int.from_bytes(buf[off + 12:off + 14], "little"), int.from_bytes(buf[off + 14:off + 16], "little")
    if tag == 0xFFFE:
        if size < 40:
            raise ValueError(f"parse_wav: {what}: format tag 0xFFFE (EXTENSIBLE) with a `fmt ` chunk of {size} bytes, it needs 40")
        tag = int.from_bytes(buf[off + 24:off + 26], "little")         # the sub-format GUID starts with the plain format tag
    if tag == 1:
        code = _PCM_BITS.get(bits)
        if code is None:
            raise ValueError(f"parse_wav: {what}: {bits}-bit PCM; 8, 16, 24 and 32 bits are read")
    elif tag == 3:
        code = _FLOAT_BITS.get(bits)
        if code is None:
            raise ValueError(f"parse_wav: {what}: {bits}-bit IEEE float; 32 and 64 bits are read")
    else:
        name = _TAG_NAMES.get(tag)
        raise ValueError(f"parse_wav: {what}: format tag 0x{tag:04X}" + (f" ({name})" if name else "") +
                         "; PCM (1), IEEE float (3) and EXTENSIBLE (0xFFFE) of those two are read, compressed audio is not")
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"parse_wav: {what}: {channels} channels; 1 .. {MAX_CHANNELS} are read")
    if rate == 0:
        raise ValueError(f"parse_wav: {what}: a sample rate of 0 Hz")
    if block_align != channels * bits // 8:
        raise ValueError(f"parse_wav: {what}: block_align {block_align}, but {channels} channels of {bits} bits are {channels * bits // 8} bytes")
    off, size = data
    avail = len(buf) - off
    if size in (0, 0xFFFFFFFF) or size > avail:
        size = avail
    return WavInfo(code, bits, channels, rate, off, size // block_align * block_align, block_align)


def resample_plan(rate_in, rate_out=16000):
    """(up, down, half, taps) of the polyphase resampler rate_in -> rate_out: up / down = rate_out / rate_in in lowest terms, and the
    2 * half + 1 taps (fp64) of a Kaiser-windowed sinc on the up-sampled grid with resampy's published `kaiser_best` parameters (64 zero
    crossings, beta 14.769656459379492, roll-off 0.9475937167399596):

        m = max(up, down), fc = rolloff / m, half = ceil(64 * m / rolloff),
        h[n] = up * fc * sinc(fc * n) * kaiser(2 * half + 1, beta)[n + half]          for n = -half .. half, sinc(x) = sin(pi x) / (pi x)

    so that y[j] = sum_i x[i] * h[j * down - i * up + half] with zeros beyond both ends of x, ceil(n_in * up / down) outputs.  The reference's
    resampler is soxr through librosa, which nobody can restate here: the target is this filter, not librosa's bits.  A ratio outside
    1/16 .. 16 and a table of more than 2^21 taps (rates with a large common denominator: 15 999 -> 16 000 Hz) are refused."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in <= 0 or rate_out <= 0:
        raise ValueError(f"resample_plan: rates {rate_in} Hz -> {rate_out} Hz must be positive")
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    if up > MAX_RATIO * down or down > MAX_RATIO * up:
        raise ValueError(f"resample_plan: {rate_in} Hz -> {rate_out} Hz is a ratio outside 1/{MAX_RATIO} .. {MAX_RATIO}")
    m = max(up, down)
    fc = KAISER_ROLLOFF / m
    half = math.ceil(KAISER_ZEROS * m / KAISER_ROLLOFF)
    if 2 * half + 1 > MAX_TAPS:
        raise ValueError(f"resample_plan: {rate_in} Hz -> {rate_out} Hz reduces to {up} / {down}: a filter of {2 * half + 1} taps, more than "
                         f"{MAX_TAPS}; resample to a rate with a smaller common denominator first")
    n = np.arange(-half, half + 1, dtype=np.float64)
    taps = up * fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, KAISER_BETA)
    return up, down, half, taps


def phase_major(taps, up, half):
    """The 2 * half + 1 taps as the device takes them: up rows of 2 * half // up + 1 values, row p = h[p], h[p + up], ..., zero past the end."""
    q = 2 * half // up + 1
    padded = np.zeros(up * q, dtype=np.float64)
    padded[:2 * half + 1] = taps
    return np.ascontiguousarray(padded.reshape(q, up).T).reshape(-1)


_PLANS = {}     # (rate_in, rate_out, device) -> (up, down, half, fp32 phase-major table on that device)


def plan_cache():
    """The device tables built so far: {(rate_in, rate_out, device string): (up, down, half, table)}."""
    return _PLANS


def _device_plan(rate_in, rate_out, device):
    import torch
    key = (int(rate_in), int(rate_out), str(device))
    if key not in _PLANS:
        up, down, half, taps = resample_plan(rate_in, rate_out)
        _PLANS[key] = (up, down, half, torch.from_numpy(phase_major(taps, up, half).astype(np.float32)).to(device))
    return _PLANS[key]


def resample_device(wave, rate_in, rate_out=16000):
    """A 1-D fp32 waveform on the device at rate_in -> the same at rate_out, (ceil(n * up / down),): one launch of the polyphase FIR of
    resample_plan, its table built once per (rate_in, rate_out, device).  Equal rates: `wave` itself, no launch and no table."""
    from . import hip
    if int(rate_in) == int(rate_out):
        return wave
    if wave.dim() != 1 or wave.numel() == 0:
        raise ValueError(f"resample_device: expects a 1-D waveform with samples, got {tuple(wave.shape)}")
    up, down, half, table = _device_plan(rate_in, rate_out, wave.device)
    return hip.audio_resample(wave.contiguous(), table, up, down, half)


def read_audio_device(path, sr=16000, device="cuda", max_seconds=None):
    """The PCM / float WAV file at `path` (or its bytes) as a mono fp32 waveform at `sr` Hz on `device`: librosa.load(path, sr=sr) for the
    formats parse_wav reads.  One copy of the `data` bytes to the device, one decode launch, one resample launch unless the file is at `sr`
    already.  max_seconds: only that much of the file's start is copied and decoded."""
    import torch
    from . import hip
    if isinstance(path, (bytes, bytearray, memoryview)):
        buf, what = (path if isinstance(path, bytearray) else bytearray(path)), "wav bytes"
    else:
        what = str(path)
        with open(path, "rb") as fh:
            buf = bytearray(fh.read())                                  # writable: torch.frombuffer takes the `data` bytes from it without a copy
    info = parse_wav(buf)
    n = info.data_bytes // info.block_align
    if max_seconds is not None:
        n = min(n, int(round(float(max_seconds) * info.rate)))
    if n < 1:
        raise ValueError(f"read_audio_device: {what} holds no whole frame")
    raw = torch.frombuffer(buf, dtype=torch.uint8, count=n * info.block_align, offset=info.data_offset).to(device)
    return resample_device(hip.audio_decode_mono(raw, n, info.channels, info.fmt), info.rate, sr)


def pcm16_host(path, seconds=None):
    """(int16 samples (n, channels), rate) of a WAV file at its own rate and channel count, for a 16-bit PCM sound track (video_out.write_avi):
    S16 as stored; the other formats converted on the host from the raw bytes -- U8 re-centred (v - 128) * 256, S24 / 2^8 and S32 / 2^16 and
    float * 2^15 rounded to nearest (ties to even) and clipped to -32768 .. 32767.  seconds: only that much of the file's start."""
    if isinstance(path, (bytes, bytearray, memoryview)):
        buf = bytes(path)
    else:
        with open(path, "rb") as fh:
            buf = fh.read()
    info = parse_wav(buf)
    n = info.data_bytes // info.block_align
    if seconds is not None:
        n = min(n, int(round(float(seconds) * info.rate)))
    raw = np.frombuffer(buf, dtype=np.uint8, count=n * info.block_align, offset=info.data_offset)
    if info.fmt == S16:
        return raw.view("<i2").reshape(n, info.channels).astype(np.int16), info.rate
    if info.fmt == U8:
        v = (raw.astype(np.int32) - 128) * 256
    elif info.fmt == S24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = np.rint(((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) - ((b[:, 2] & 0x80) << 17)) / 256.0)
    elif info.fmt == S32:
        v = np.rint(raw.view("<i4").astype(np.float64) / 65536.0)
    else:
        v = np.rint(np.nan_to_num(raw.view("<f4" if info.fmt == F32 else "<f8").astype(np.float64)) * 32768.0)
    return np.clip(v, -32768, 32767).astype(np.int16).reshape(n, info.channels), info.rate
