"""Reference side of the audio input path, numpy only: a WAV writer for every format and layout mmgt_amd.audio_in.parse_wav reads
(headers built by hand: stdlib `wave` writes neither float nor EXTENSIBLE files), the decode + down-mix in the kernel's fp32 order of operations,
and the direct fp64 evaluation of the resampler's defining sum  y[j] = sum_i x[i] h[j down - i up + half]."""
import struct

import numpy as np

U8, S16, S24, S32, F32, F64 = range(6)
FORMATS = (U8, S16, S24, S32, F32, F64)
NAMES = ("U8", "S16", "S24", "S32", "F32", "F64")
SAMPLE_BYTES = (1, 2, 3, 4, 4, 8)
RATES = (8000, 11025, 22050, 44100, 48000, 96000)
_KSDATAFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")        # the 14 bytes that follow the format tag in a sub-format GUID


def encode_frames(x, fmt):
    """x (n, channels) fp64 in [-1, 1) -> the interleaved little-endian bytes of format fmt (integers: scaled and rounded to nearest)."""
    x = np.asarray(x, dtype=np.float64)
    if fmt == U8:
        return np.clip(np.rint(x * 128) + 128, 0, 255).astype(np.uint8).tobytes()
    if fmt == S16:
        return np.clip(np.rint(x * 32768), -32768, 32767).astype("<i2").tobytes()
    if fmt == S24:
        v = np.clip(np.rint(x * 8388608), -8388608, 8388607).astype("<i4")
        return np.ascontiguousarray(v.reshape(-1, 1).view(np.uint8)[:, :3]).tobytes()
    if fmt == S32:
        return np.clip(np.rint(x * 2147483648.0), -2147483648, 2147483647).astype("<i4").tobytes()
    return x.astype("<f4" if fmt == F32 else "<f8").tobytes()


def chunk(fourcc, body):
    """One RIFF chunk; an odd-sized body is followed by its pad byte."""
    return fourcc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt_chunk(fmt, channels, rate, extensible=False, tag=None, bits=None, block_align=None):
    bits = SAMPLE_BYTES[fmt] * 8 if bits is None else bits
    block_align = channels * bits // 8 if block_align is None else block_align
    tag = (3 if fmt in (F32, F64) else 1) if tag is None else tag
    head = lambda t: struct.pack("<HHIIHH", t, channels, rate, rate * block_align, block_align, bits)
    if not extensible:
        return chunk(b"fmt ", head(tag))
    return chunk(b"fmt ", head(0xFFFE) + struct.pack("<HHI", 22, bits, (1 << channels) - 1) + struct.pack("<H", tag) + _KSDATAFORMAT_TAIL)


def wav_bytes(frames, fmt, channels, rate, extensible=False, before=(), data_size=None, cut=0, riff=b"RIFF", **fmt_fields):
    """A WAVE file around the interleaved bytes `frames`: `before` = (fourcc, body) chunks between `fmt ` and `data`; data_size: the size
    written into the `data` header instead of the true one (0 / 0xFFFFFFFF: a streaming writer); cut: bytes dropped from the file's end."""
    body = b"WAVE" + fmt_chunk(fmt, channels, rate, extensible, **fmt_fields) + b"".join(chunk(cc, b) for cc, b in before)
    body += b"data" + struct.pack("<I", len(frames) if data_size is None else data_size) + frames + (b"\0" if len(frames) & 1 else b"")
    out = riff + struct.pack("<I", len(body)) + body
    return out[:len(out) - cut] if cut else out


def raw_values(raw, fmt, channels):
    """(n, channels) fp32 of the stored values as csrc/audio_core.h's audio_raw reads them: the integer itself (U8 re-centred), a float rounded
    once to fp32."""
    b = np.frombuffer(raw, dtype=np.uint8)
    if fmt == U8:
        v = b.astype(np.int32) - 128
    elif fmt == S16:
        v = b.view("<i2")
    elif fmt == S24:
        t = b.reshape(-1, 3).astype(np.int32)
        v = (t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)) - ((t[:, 2] & 0x80) << 17)
    elif fmt == S32:
        v = b.view("<i4")
    else:
        v = b.view("<f4" if fmt == F32 else "<f8")
    return v.astype(np.float32).reshape(-1, channels)


def decode_mono(raw, fmt, channels):
    """(n,) fp32 in the kernel's order: channels summed in fp32 in channel order, one division by the count, the power-of-two scale -- last for
    U8 and S16 (the raw integers are summed), first for the other formats."""
    v = raw_values(raw, fmt, channels)
    scale = np.float32(2.0 ** -{U8: 7, S16: 15, S24: 23, S32: 31}.get(fmt, 0))
    raw_sum = fmt in (U8, S16)
    s = np.zeros(v.shape[0], dtype=np.float32)
    for ch in range(channels):
        s = s + (v[:, ch] if raw_sum else v[:, ch] * scale)
    s = s / np.float32(channels)
    out = s * scale if raw_sum else s
    assert out.dtype == np.float32
    return out


def spans(n_in, n_out, up, down, half):
    """(i_lo, i_hi) int64 arrays over the outputs, in Python's floor-division semantics."""
    c = np.arange(n_out, dtype=np.int64) * down
    return np.maximum(0, -((half - c) // up)), np.minimum(n_in - 1, (c + half) // up)


def resample_direct(x, h, up, down, half, chunk_outputs=1024):
    """The defining sum in fp64, output by output: (y, taps used per output).  h: the 2 half + 1 taps.  Evaluated on |x| and |h| it is the
    sum_i |x[i]| |h[.]| of an error bound."""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    assert h.shape == (2 * half + 1,)
    n_in = x.shape[0]
    n_out = -(-n_in * up // down)
    lo, hi = spans(n_in, n_out, up, down, half)
    y = np.zeros(n_out)
    kmax = int((hi - lo).max()) + 1
    k = np.arange(kmax, dtype=np.int64)
    for a in range(0, n_out, chunk_outputs):
        b = min(n_out, a + chunk_outputs)
        i = lo[a:b, None] + k[None, :]
        ok = i <= hi[a:b, None]
        i = np.where(ok, i, 0)
        t = np.where(ok, np.arange(a, b, dtype=np.int64)[:, None] * down - i * up + half, 0)
        assert t.min() >= 0 and t.max() <= 2 * half
        y[a:b] = (x[i] * h[t] * ok).sum(1)
    return y, (hi - lo + 1).astype(np.int64)


def resample_bound(x, h, up, down, half):
    """Per output, (K + 3) 2^-24 sum_i |x[i]| |h[.]| with K the taps the output uses.  Derivation: the device multiplies fp32 taps
    h32 = h (1 + d), |d| <= 2^-24, into x by K fused multiply-adds into an fp32 zero, each with ONE rounding of the running sum, so term i
    carries at most K + 1 factors (1 + e), |e| <= 2^-24: the error is at most ((1 + 2^-24)^(K + 1) - 1) sum |x| |h|, which is below
    (K + 3) 2^-24 sum |x| |h| while (K + 1)^2 <= 2^25 (K is 135 .. 813 here).  x is the same fp32 data on both sides; the fp64 reference's own
    error is nine orders of magnitude smaller.  Derived, not fitted."""
    s, k = resample_direct(np.abs(x), np.abs(h), up, down, half)
    return (k + 3) * 2.0 ** -24 * s
