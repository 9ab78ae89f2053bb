// Audio input: the arithmetic that csrc/audio.hip and the host program tools/audio_host_check.cpp must agree on -- the decoding of one
// little-endian sample, the down-mix to mono and the index arithmetic and summation order of the polyphase resampler.  Plain C++: no HIP type, no
// global state; every function works through byte or float pointers the caller bounds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AU_FN __host__ __device__ inline
#else
#define AU_FN inline
#endif

// sample formats of a WAV `data` chunk (mmgt_amd/audio_in.py holds the same numbers)
enum { AU_U8 = 0, AU_S16 = 1, AU_S24 = 2, AU_S32 = 3, AU_F32 = 4, AU_F64 = 5, AU_FORMATS = 6 };
constexpr int AU_MAX_CHANNELS = 16;

AU_FN int audio_sample_bytes(int fmt) { return fmt == AU_U8 ? 1 : fmt == AU_S16 ? 2 : fmt == AU_S24 ? 3 : fmt == AU_F64 ? 8 : 4; }

AU_FN float au_bits_f32(uint32_t u) {
  union { uint32_t u; float f; } c;
  c.u = u;
  return c.f;
}
AU_FN double au_bits_f64(uint64_t u) {
  union { uint64_t u; double f; } c;
  c.u = u;
  return c.f;
}
AU_FN uint32_t au_le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// The RAW value of channel `ch` of the frame at `frame` (any byte address: the bytes are read one by one and assembled): the integer itself for
// the PCM formats (U8 re-centred: v - 128), the value rounded once to fp32 for the float formats.  Integers up to 24 bits are exact in fp32; a
// 32-bit one is rounded to nearest even here, once.
AU_FN float audio_raw(const uint8_t* frame, int fmt, int ch) {
  const uint8_t* p = frame + ch * audio_sample_bytes(fmt);
  switch (fmt) {
    case AU_U8: return (float)((int)p[0] - 128);
    case AU_S16: return (float)(int16_t)(uint16_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8));
    case AU_S24: return (float)((int32_t)(((uint32_t)p[0] << 8) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 24)) >> 8);
    case AU_S32: return (float)(int32_t)au_le32(p);
    case AU_F32: return au_bits_f32(au_le32(p));
    default: return (float)au_bits_f64((uint64_t)au_le32(p) | ((uint64_t)au_le32(p + 4) << 32));
  }
}

// 1 / full scale: a power of two, so the product is exact (the float formats: 1)
AU_FN float audio_scale(int fmt) {
  return fmt == AU_U8 ? 0x1p-7f : fmt == AU_S16 ? 0x1p-15f : fmt == AU_S24 ? 0x1p-23f : fmt == AU_S32 ? 0x1p-31f : 1.f;
}

// One decoded sample: U8 (v - 128) / 128, S16 / 2^15, S24 / 2^23, S32 / 2^31, F32 as stored, F64 rounded once to fp32.
AU_FN float audio_sample(const uint8_t* frame, int fmt, int ch) { return audio_raw(frame, fmt, ch) * audio_scale(fmt); }

// Mono value of one frame, ONE order of operations: the channels summed in fp32 in channel order, one division by the channel count, and the
// power-of-two scale.  U8 and S16 sum the raw integers (exact: 16 channels of 16 bits stay below 2^24) and scale last, which for one or two
// channels of S16 is numpy's pcm.astype(float32).mean(1) / 32768.0 bit for bit; S24, S32, F32 and F64 scale each sample first, then sum, then
// divide.
AU_FN float audio_frame_mono(const uint8_t* frame, int fmt, int channels) {
  const bool raw_sum = fmt == AU_U8 || fmt == AU_S16;
  float s = 0.f;
  for (int ch = 0; ch < channels; ++ch) s += raw_sum ? audio_raw(frame, fmt, ch) : audio_sample(frame, fmt, ch);
  s = s / (float)channels;
  return raw_sum ? s * audio_scale(fmt) : s;
}

// ---- polyphase resampler: y[j] = sum_i x[i] h[c - i up + half], c = j down, zeros beyond both ends of x, n_out = ceil(n_in up / down) ----------
// up and down are reduced by their gcd; h has 2 half + 1 taps on the up-sampled grid.  c is 64-bit: one hour of 44.1-kHz audio puts j * 441 past
// 2^31.  The taps travel phase-major: row p (0 .. up - 1) holds h[p], h[p + up], h[p + 2 up], ... in audio_phase_len(up, half) floats, zero where
// p + q up > 2 half, so that the taps one output uses are consecutive floats of one row.
AU_FN int64_t au_floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }   // b > 0 here
AU_FN int64_t au_ceil_div(int64_t a, int64_t b) { return -au_floor_div(-a, b); }

AU_FN int64_t audio_out_len(int64_t n_in, int up, int down) { return au_ceil_div(n_in * up, down); }
AU_FN int64_t audio_phase_len(int up, int half) { return 2 * (int64_t)half / up + 1; }
AU_FN int64_t audio_table_len(int up, int half) { return up * audio_phase_len(up, half); }

struct AudioSpan {
  int64_t i_lo, i_hi;   // the inputs output j reads (empty if i_lo > i_hi)
  int64_t tap_lo;       // the tap index that goes with i_hi, c - i_hi up + half: the lowest one; input i takes tap_lo + (i_hi - i) up
};
AU_FN AudioSpan audio_span(int64_t j, int64_t n_in, int up, int down, int half) {
  const int64_t c = j * (int64_t)down;
  AudioSpan s;
  s.i_lo = au_ceil_div(c - half, up);
  if (s.i_lo < 0) s.i_lo = 0;
  s.i_hi = au_floor_div(c + half, up);
  if (s.i_hi > n_in - 1) s.i_hi = n_in - 1;
  s.tap_lo = c - s.i_hi * up + half;
  return s;
}

// Samples a run of T consecutive outputs can read: ceil(T down / up) + 2 ceil(half / up) + 1 (what a workgroup stages in LDS)
AU_FN int64_t audio_stage_len(int64_t T, int up, int down, int half) { return au_ceil_div(T * down, up) + 2 * au_ceil_div(half, up) + 1; }

// One output in the ONE summation order: ascending tap index (descending input index), fused multiply-adds into an fp32 zero.  `x` points at
// input x_base (the kernel: the first staged sample); `taps` is the phase-major table.  Reads x[i_lo - x_base .. i_hi - x_base] and the
// floats [p Q + q_lo, p Q + q_hi] of the table, nothing else.
AU_FN float audio_resample_one(const float* x, int64_t x_base, const float* taps, int64_t j, int64_t n_in, int up, int down, int half) {
  const AudioSpan s = audio_span(j, n_in, up, down, half);
  if (s.i_lo > s.i_hi) return 0.f;
  const int64_t Q = audio_phase_len(up, half);
  const float* row = taps + (s.tap_lo % up) * Q + s.tap_lo / up;       // tap_lo = p + q_lo up
  const float* xi = x + (s.i_hi - x_base);
  const int64_t n = s.i_hi - s.i_lo + 1;
  float acc = 0.f;
  int64_t k = 0;
  for (; k + 4 <= n; k += 4) {          // four taps and four samples in flight, the chain itself in the one order
    const float t0 = row[k], t1 = row[k + 1], t2 = row[k + 2], t3 = row[k + 3];
    const float a0 = xi[-k], a1 = xi[-k - 1], a2 = xi[-k - 2], a3 = xi[-k - 3];
    acc = __builtin_fmaf(a0, t0, acc);
    acc = __builtin_fmaf(a1, t1, acc);
    acc = __builtin_fmaf(a2, t2, acc);
    acc = __builtin_fmaf(a3, t3, acc);
  }
  for (; k < n; ++k) acc = __builtin_fmaf(xi[-k], row[k], acc);
  return acc;
}
