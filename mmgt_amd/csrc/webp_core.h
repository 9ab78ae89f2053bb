// WebP lossless (VP8L) output, the per-pixel arithmetic written once: csrc/webp.hip calls these functions from its kernels and
// tools/webp_host_check.cpp from a host program, so the modes, residuals and tokens a kernel produces can be checked without a GPU.  A pixel is an
// ARGB word (a << 24 | r << 16 | g << 8 | b); the frames are RGB, so a is 255 everywhere and every residual's a is 0.  Nothing here reads outside
// the frame or the strip its arguments name.
#pragma once
#include <stdint.h>

#include "strip_coder.h"

#if defined(__HIPCC__)
#define WP_HD __host__ __device__ inline
#else
#define WP_HD inline
#endif

enum {
  WP_PREDICTOR_BITS = 4,       // blocks of 16 x 16 pixels choose a mode
  WP_MODES = 14,
  WP_MAX_LENGTH = 4096,        // the longest match
  WP_GREEN_SYMS = 280,         // 256 literals + 24 length prefixes (no colour cache)
  WP_HIST_WORDS = 280 + 256 + 256 + 1,  // green + length, red, blue, then the number of matches
  WP_LITERAL = SC_LITERAL,     // wp_token_at: pixel p is a literal
  WP_NONE = SC_NONE            // wp_token_at: no token ends at p
};
#define WP_BLACK 0xff000000u

// pixel (y, x) of an RGB frame of width W after the subtract-green transform
WP_HD uint32_t wp_pixel(const unsigned char* frame, long W, long y, long x) {
  const unsigned char* p = frame + 3 * (y * W + x);
  const uint32_t r = p[0], g = p[1], b = p[2];
  return WP_BLACK | ((r - g) & 255u) << 16 | g << 8 | ((b - g) & 255u);
}

// per channel, no carry from one into the next
WP_HD uint32_t wp_avg(uint32_t p, uint32_t q) { return (((p ^ q) & 0xfefefefeu) >> 1) + (p & q); }
WP_HD uint32_t wp_sub(uint32_t p, uint32_t q) {
  const uint32_t ag = 0x00ff00ffu + (p & 0xff00ff00u) - (q & 0xff00ff00u), rb = 0xff00ff00u + (p & 0x00ff00ffu) - (q & 0x00ff00ffu);
  return (ag & 0xff00ff00u) | (rb & 0x00ff00ffu);
}
WP_HD int wp_ch(uint32_t p, int shift) { return (int)(p >> shift & 255u); }
WP_HD int wp_clamp(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
WP_HD int wp_abs(int v) { return v < 0 ? -v : v; }

// The 14 predictors from the left, top, top-left and top-right pixels.
WP_HD uint32_t wp_predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
  switch (mode) {
    case 0: return WP_BLACK;
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return wp_avg(wp_avg(L, TR), T);
    case 6: return wp_avg(L, TL);
    case 7: return wp_avg(L, T);
    case 8: return wp_avg(TL, T);
    case 9: return wp_avg(T, TR);
    case 10: return wp_avg(wp_avg(L, TL), wp_avg(T, TR));
    case 11: {
      int dt = 0, dl = 0;
      for (int s = 0; s < 32; s += 8) {
        dt += wp_abs(wp_ch(T, s) - wp_ch(TL, s));
        dl += wp_abs(wp_ch(L, s) - wp_ch(TL, s));
      }
      return dt < dl ? L : T;
    }
    case 12: {
      uint32_t out = 0;
      for (int s = 0; s < 32; s += 8) out |= (uint32_t)wp_clamp(wp_ch(L, s) + wp_ch(T, s) - wp_ch(TL, s)) << s;
      return out;
    }
    default: {
      const uint32_t a = wp_avg(L, T);
      uint32_t out = 0;
      for (int s = 0; s < 32; s += 8) out |= (uint32_t)wp_clamp(wp_ch(a, s) + (wp_ch(a, s) - wp_ch(TL, s)) / 2) << s;   // C division: toward zero
      return out;
    }
  }
}

// The neighbours of pixel (y, x) as the decoder has them; what lies outside the frame is black and is never used by a prediction that counts.
struct WpNeighbours {
  uint32_t L, T, TL, TR;
};
WP_HD WpNeighbours wp_neighbours(const unsigned char* frame, long W, long y, long x) {
  WpNeighbours n = {WP_BLACK, WP_BLACK, WP_BLACK, WP_BLACK};
  if (x > 0) n.L = wp_pixel(frame, W, y, x - 1);
  if (y > 0) {
    n.T = wp_pixel(frame, W, y - 1, x);
    if (x > 0) n.TL = wp_pixel(frame, W, y - 1, x - 1);
    n.TR = x + 1 < W ? wp_pixel(frame, W, y - 1, x + 1) : wp_pixel(frame, W, y, 0);   // past the row above's end stands this row's first pixel
  }
  return n;
}

// The prediction of pixel (y, x) under `mode`: forced for pixel (0, 0) (black), row 0 (left) and column 0 (top).
WP_HD uint32_t wp_predict_at(int mode, long y, long x, const WpNeighbours& n) {
  if (y == 0) return x == 0 ? WP_BLACK : n.L;
  if (x == 0) return n.T;
  return wp_predict(mode, n.L, n.T, n.TL, n.TR);
}

// what a residual costs: min(v, 256 - v) over r, g, b
WP_HD unsigned wp_cost(uint32_t res) {
  unsigned c = 0;
  for (int s = 0; s < 24; s += 8) {
    const int v = wp_ch(res, s);
    c += (unsigned)(v < 256 - v ? v : 256 - v);
  }
  return c;
}

// The token that ends at position p of a strip of len pixels: WP_NONE, WP_LITERAL (pixel p itself) or the length 3 .. 4096 of a match from the left
// pixel: strip_coder.h's closed form at 4096.  run_start = the last position q <= p that is 0 or whose pixel differs from pixel q - 1.
WP_HD int wp_token_at(const uint32_t* src, int p, int len, int run_start) {
  return sc_token_at<WP_MAX_LENGTH>(ScSameAsBefore<uint32_t>{src}, p, len, run_start);
}

// A length (or distance) value 1 .. 4096 -> its prefix symbol, the number of extra bits and their value.
WP_HD void wp_prefix(int v, int* sym, int* ebits, int* eval) {
  if (v <= 4) {
    *sym = v - 1, *ebits = 0, *eval = 0;
    return;
  }
  const int d = v - 1;
  int hb = 0;
  while ((d >> (hb + 1)) != 0) ++hb;                               // floor(log2 d), d <= 4095
  *sym = 2 * hb + ((d >> (hb - 1)) & 1), *ebits = hb - 1, *eval = d & ((1 << (hb - 1)) - 1);
}
