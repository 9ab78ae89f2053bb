// PIL's ImagingResample for 8-bit images (src/libImaging/Resample.c: ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc), written once
// as plain inline functions: csrc/resize.hip calls them from its kernels and tools/resize_host_check.cpp from a host program, so the
// bytes a kernel produces and every index it forms can be checked without a GPU.  Integer arithmetic only: the host hands in PIL's own
// coefficient tables (mmgt_amd.conditioning.pil_resample_tables), per output sample o of an axis
//     bounds[2 o] = first input tap,  bounds[2 o + 1] = tap count n,  kk[o * ksize + 0 .. n) = weights with RS_PRECISION_BITS fractional bits,
// and a pass is   out = clip8((2^21 + sum_i in[first + i] * kk[i]) >> 22)   per band.  Images are (n, H, W, C) uint8, interleaved, C = 1 or 3.
//
// One ITEM is the unit of work of one thread (or of one turn of the host program's loop):
//   * rs_h_item<C>   one pixel of the horizontal pass: the C bands of output column x of row (f, y)
//   * rs_v_item<V>   V consecutive bytes of one output row of the vertical pass (V = 4: one 32-bit load per tap, where rows and bases are 4-byte
//                    aligned; V = 1 anywhere)
//   * rs_copy_item   one byte of a call that resamples nothing (same size): the epilogue alone
// Every index is a long.  An item reads in[first .. first + n) of its row / column and nothing else, and writes its own output samples.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ inline
#else
#define RS_HD inline
#endif

enum { RS_PRECISION_BITS = 32 - 8 - 2, RS_MAX_SIDE = 16384 };

// Where the LAST pass of a call writes: u8 -> (n, H, W, C) uint8 interleaved; f32 -> (C, n, H, W) float planar, f32 = lut[c * 256 + value]
// (the caller's table: ToTensor's v / 255, the VAE's v / 255 * 2 - 1, CLIP's (v / 255 - mean) / std, as the host computes them).  The first of
// two passes writes u8 into the workspace.
struct RsOut {
  uint8_t* u8;
  float* f32;
  const float* lut;
};

RS_HD uint8_t rs_clip8(int acc) {
  acc >>= RS_PRECISION_BITS;
  return (uint8_t)(acc < 0 ? 0 : acc > 255 ? 255 : acc);
}

RS_HD void rs_put(const RsOut& o, int n, int H, int W, int C, long f, long y, long x, int c, uint8_t v) {
  if (o.f32)
    o.f32[(((long)c * n + f) * H + y) * W + x] = o.lut[c * 256 + v];
  else
    o.u8[((f * H + y) * W + x) * C + c] = v;
}

// items: n * H * Wd, x fastest.  in (n, H, Ws, C) -> (n, H, Wd, C)
template <int C>
RS_HD void rs_h_item(const uint8_t* in, const RsOut& o, int n, int H, int Ws, int Wd, const int* bounds, const int* kk, int ksize, long item) {
  const long x = item % Wd, row = item / Wd;                      // row = f * H + y
  const int first = bounds[2 * x], cnt = bounds[2 * x + 1];
  const int* k = kk + x * ksize;
  const uint8_t* p = in + (row * Ws + first) * C;
  int acc[C];
  for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PRECISION_BITS - 1);
  for (int i = 0; i < cnt; ++i) {
    const int w = k[i];
    for (int c = 0; c < C; ++c) acc[c] += (int)p[(long)i * C + c] * w;
  }
  const long f = row / H, y = row % H;
  for (int c = 0; c < C; ++c) rs_put(o, n, H, Wd, C, f, y, x, c, rs_clip8(acc[c]));
}

// items: n * Hd * (W * C / V), the byte group fastest.  in (n, Hs, W, C) -> (n, Hd, W, C).  V = 4 needs W * C % 4 == 0 and `in` (and o.u8) 4-byte
// aligned.
template <int V>
RS_HD void rs_v_item(const uint8_t* in, const RsOut& o, int n, int Hs, int Hd, int W, int C, const int* bounds, const int* kk, int ksize,
                     long item) {
  const long pitch = (long)W * C, per = pitch / V;
  const long j = (item % per) * V, row = item / per;              // row = f * Hd + y
  const long f = row / Hd, y = row % Hd;
  const int first = bounds[2 * y], cnt = bounds[2 * y + 1];
  const int* k = kk + y * ksize;
  const uint8_t* p = in + (f * Hs + first) * pitch + j;
  int acc[V];
  for (int b = 0; b < V; ++b) acc[b] = 1 << (RS_PRECISION_BITS - 1);
  for (int i = 0; i < cnt; ++i) {
    const int w = k[i];
    if constexpr (V == 4) {
      const uint32_t q = *reinterpret_cast<const uint32_t*>(p + (long)i * pitch);
      for (int b = 0; b < 4; ++b) acc[b] += (int)((q >> (8 * b)) & 255u) * w;
    } else {
      acc[0] += (int)p[(long)i * pitch] * w;
    }
  }
  if constexpr (V == 4) {
    if (!o.f32) {
      uint32_t q = 0;
      for (int b = 0; b < 4; ++b) q |= (uint32_t)rs_clip8(acc[b]) << (8 * b);
      *reinterpret_cast<uint32_t*>(o.u8 + row * pitch + j) = q;
      return;
    }
  }
  for (int b = 0; b < V; ++b) rs_put(o, n, Hd, W, C, f, y, (j + b) / C, (int)((j + b) % C), rs_clip8(acc[b]));
}

// items: n * H * W * C bytes
RS_HD void rs_copy_item(const uint8_t* in, const RsOut& o, int n, int H, int W, int C, long item) {
  const long pix = item / C, row = pix / W;
  rs_put(o, n, H, W, C, row / H, row % H, pix % W, (int)(item % C), in[item]);
}

// bytes of the intermediate (n, Hs, Wd, C) a call needs: only when both passes run
RS_HD long rs_workspace_bytes(int n, int Hs, int Ws, int Hd, int Wd, int C) {
  return (Ws != Wd && Hs != Hd) ? (long)n * Hs * Wd * C : 0;
}

RS_HD bool rs_shape_ok(int n, int Hs, int Ws, int Hd, int Wd, int C) {
  return n >= 1 && (C == 1 || C == 3) && Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1 && Hs <= RS_MAX_SIDE && Ws <= RS_MAX_SIDE &&
         Hd <= RS_MAX_SIDE && Wd <= RS_MAX_SIDE;
}
