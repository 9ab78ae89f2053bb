// The integer arithmetic of re-voicing an existing clip, written once: csrc/vid2vid.hip calls these functions from its kernels and
// tools/vid2vid_host_check.cpp from a host program, which pins them byte for byte against tests/vid2vid_ref.py without a GPU.
//
// mask -> cells   A latent cell (cy, cx) covers the 8 x 8 pixels [8 cy, 8 cy + 8) x [8 cx, 8 cx + 8).  It is SET when one of its pixels is >= 128
//                 (v2v_cell_set).  The cell mask is 1 where a set cell lies within Chebyshev distance `grow` (0 .. 8); cells outside the frame do
//                 not exist (v2v_cell_mask).
// cells -> alpha  The cell mask repeated x 8 (a cell counts when its value is >= 0.5), box-averaged over (2 r + 1)^2 pixels with edge replication:
//                 count = sum over dy, dx in [-r, r] of cell[clamp(y + dy) / 8][clamp(x + dx) / 8],  a = (255 count + area / 2) / area,  area =
//                 (2 r + 1)^2, r = 0 .. 32.  The box is separable and constant over a cell, so the sum runs over cells with the number of taps
//                 that land in each (v2v_axis_taps): at most 10 x 10 terms instead of 65 x 65 (v2v_feather_pixel).
// paste back      byte = (g a + o (255 - a) + 127) / 255 (v2v_blend): a = 0 gives o, a = 255 gives g.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define V2V_HD __host__ __device__ __forceinline__
#else
#define V2V_HD inline
#endif

enum { V2V_CELL = 8, V2V_GROW_MAX = 8, V2V_FEATHER_MAX = 32 };

// one of the 64 pixels of cell (cy, cx) of a frame of W bytes per row is >= 128: eight 8-byte rows, top bits
V2V_HD int v2v_cell_set(const uint8_t* frame, int W, int cy, int cx) {
  const uint8_t* p = frame + (long)cy * V2V_CELL * W + (long)cx * V2V_CELL;
  uint64_t any = 0;
  for (int r = 0; r < V2V_CELL; ++r) {
    uint64_t v;
    memcpy(&v, p + (long)r * W, 8);
    any |= v;
  }
  return (any & 0x8080808080808080ull) != 0;
}

// the dilated cell mask at (cy, cx) of an h x w grid of cells (W = 8 w bytes per pixel row)
V2V_HD int v2v_cell_mask(const uint8_t* frame, int h, int w, int cy, int cx, int grow) {
  const int y0 = cy - grow < 0 ? 0 : cy - grow, y1 = cy + grow > h - 1 ? h - 1 : cy + grow;
  const int x0 = cx - grow < 0 ? 0 : cx - grow, x1 = cx + grow > w - 1 ? w - 1 : cx + grow;
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x)
      if (v2v_cell_set(frame, w * V2V_CELL, y, x)) return 1;
  return 0;
}

// how many of the taps t = x - r .. x + r, clamped to [0, 8 n - 1], land in cell c of n
V2V_HD int v2v_axis_taps(int x, int r, int c, int n) {
  const int lo = c == 0 ? x - r : (c * V2V_CELL > x - r ? c * V2V_CELL : x - r);
  const int hi = c == n - 1 ? x + r : (c * V2V_CELL + V2V_CELL - 1 < x + r ? c * V2V_CELL + V2V_CELL - 1 : x + r);
  return hi >= lo ? hi - lo + 1 : 0;
}

V2V_HD int v2v_clamp_cell(int t, int n) { return t < 0 ? 0 : (t > n * V2V_CELL - 1 ? n - 1 : t / V2V_CELL); }

// alpha of pixel (y, x) from one frame's h x w cell mask
V2V_HD uint8_t v2v_feather_pixel(const float* cells, int h, int w, int y, int x, int r) {
  const int cy0 = v2v_clamp_cell(y - r, h), cy1 = v2v_clamp_cell(y + r, h);
  const int cx0 = v2v_clamp_cell(x - r, w), cx1 = v2v_clamp_cell(x + r, w);
  int count = 0;
  for (int cy = cy0; cy <= cy1; ++cy) {
    int row = 0;
    for (int cx = cx0; cx <= cx1; ++cx)
      if (cells[(long)cy * w + cx] >= 0.5f) row += v2v_axis_taps(x, r, cx, w);
    count += row * v2v_axis_taps(y, r, cy, h);
  }
  const int area = (2 * r + 1) * (2 * r + 1);
  return (uint8_t)((255 * count + area / 2) / area);
}

V2V_HD uint32_t v2v_blend(uint32_t g, uint32_t o, uint32_t a) { return (g * a + o * (255u - a) + 127u) / 255u; }
