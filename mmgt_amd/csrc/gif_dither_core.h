// Floyd-Steinberg dithering against the clip palette, written once: csrc/gif.hip calls these functions from gif_dither_kernel and
// tools/gif_dither_host_check.cpp from a host program, which proves the kernel's lane / step schedule equal to the serial rule without a GPU.
//
// The rule, per frame, raster order (y outer, x inner), integers, per channel; d is 0 outside the frame:
//   E(x, y) = 7 d(x-1, y) + 3 d(x+1, y-1) + 5 d(x, y-1) + d(x-1, y-1)
//   v       = clamp(p(x, y) + floor((E + 8) / 16), 0, 255)
//   idx     = lut[(v_r >> 3) << 10 | (v_g >> 3) << 5 | (v_b >> 3)]
//   d(x, y) = v - palette[idx]                      so |d| <= 255 and |E| <= 4080
//
// The schedule.  Row y may take pixel x once row y - 1 has finished pixel x + 1.  A band is GDI_BAND consecutive rows, one lane each; in step t lane r
// stands at x = t - 2 r (gdi_x), so the band takes W + 2 (rows - 1) steps (gdi_band_steps) and what lane r needs of the row above in step t,
// d(x + 1, y - 1), is exactly what lane r - 1 produced in step t - 1: one cross-lane move per step, kept for two more steps as d(x, y - 1) and
// d(x - 1, y - 1).  The band's last row leaves its errors in a carry row of W words, and lane 0 of the next band reads them in place of a lane
// above.  An error triple travels as one word, 10 bits per channel, biased by 256 (gdi_pack): GDI_ZERO is "no error", not 0.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GDI_HD __host__ __device__ __forceinline__
#else
#define GDI_HD inline
#endif

enum {
  GDI_BAND = 64,       // rows per band = lanes of the workgroup: one wave, so that the move from lane r - 1 to lane r needs no barrier
  GDI_GROUP = 4        // steps per group: a lane fetches the 12 bytes of a group's four pixels at once, one group ahead
};

GDI_HD unsigned gdi_pack(int dr, int dg, int db) { return (unsigned)(dr + 256) | (unsigned)(dg + 256) << 10 | (unsigned)(db + 256) << 20; }
#define GDI_ZERO (256u | 256u << 10 | 256u << 20)
GDI_HD int gdi_r(unsigned e) { return (int)(e & 1023u) - 256; }
GDI_HD int gdi_g(unsigned e) { return (int)((e >> 10) & 1023u) - 256; }
GDI_HD int gdi_b(unsigned e) { return (int)((e >> 20) & 1023u) - 256; }

GDI_HD int gdi_x(long t, int lane) { return (int)(t - 2 * lane); }
GDI_HD long gdi_band_steps(int W, int rows) { return (long)W + 2 * (rows - 1); }

GDI_HD int gdi_channel(int p, int left, int up_next, int up, int up_prev) {
  const int E = 7 * left + 3 * up_next + 5 * up + up_prev;
  const int v = p + ((E + 8) >> 4);                                // an arithmetic shift: the floor, also below zero
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

// One pixel of the rule.  left, up_prev, up, up_next: the packed errors d(x-1, y), d(x-1, y-1), d(x, y-1), d(x+1, y-1); lut: 32768 bytes;
// pal: 256 words r | g << 8 | b << 16.  Returns the index, *d = the packed error the pixel leaves.
GDI_HD unsigned gdi_step(unsigned r, unsigned g, unsigned b, unsigned left, unsigned up_prev, unsigned up, unsigned up_next, const unsigned char* lut,
                         const unsigned* pal, unsigned* d) {
  const int vr = gdi_channel((int)r, gdi_r(left), gdi_r(up_next), gdi_r(up), gdi_r(up_prev));
  const int vg = gdi_channel((int)g, gdi_g(left), gdi_g(up_next), gdi_g(up), gdi_g(up_prev));
  const int vb = gdi_channel((int)b, gdi_b(left), gdi_b(up_next), gdi_b(up), gdi_b(up_prev));
  const unsigned idx = lut[(vr >> 3) << 10 | (vg >> 3) << 5 | (vb >> 3)];
  const unsigned c = pal[idx];
  *d = gdi_pack(vr - (int)(c & 255u), vg - (int)((c >> 8) & 255u), vb - (int)((c >> 16) & 255u));
  return idx;
}

// What a lane carries from step to step.  out is what the lane below reads in the next step: the error of the pixel just done, GDI_ZERO from a lane
// that stood outside the frame.
struct GdiLane {
  unsigned left, up_prev, up, out;
};

GDI_HD void gdi_lane_reset(GdiLane* s, unsigned up0) {
  s->left = s->up_prev = s->out = GDI_ZERO;
  s->up = up0;                                                     // d(0, y - 1): lane 0 of a later band takes it from the carry row
}

// One step of one lane.  in = d(x + 1, y - 1).  The window over the row above moves on in every step, also while the lane stands left of the frame:
// that is how d(0, y - 1), which arrives while x = -1, is in place at x = 0.  Returns the index, or -1 if the lane is not active.
GDI_HD int gdi_lane_step(GdiLane* s, unsigned in, bool active, unsigned r, unsigned g, unsigned b, const unsigned char* lut, const unsigned* pal) {
  int idx = -1;
  unsigned d = GDI_ZERO;
  if (active) idx = (int)gdi_step(r, g, b, s->left, s->up_prev, s->up, in, lut, pal, &d);
  s->left = d;
  s->out = d;
  s->up_prev = s->up;
  s->up = in;
  return idx;
}

// The aligned word at byte offset o (a multiple of 4) of a buffer of `total` bytes whose base is 4-byte aligned; bytes outside [0, total) read as 0
// and are never touched.
GDI_HD unsigned gdi_word(const unsigned char* base, long long o, long long total) {
  if (o >= 0 && o + 4 <= total) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const unsigned*>(base + o);
#else
    unsigned v;
    memcpy(&v, base + o, 4);
    return v;
#endif
  }
  unsigned v = 0;
  for (int k = 0; k < 4; ++k)
    if (o + k >= 0 && o + k < total) v |= (unsigned)base[o + k] << (8 * k);
  return v;
}

// The 12 bytes at offset off (any alignment, possibly partly outside the buffer), the four RGB pixels of a group, in two halves so that a kernel can
// issue the loads a group ahead and touch what they return only when the group begins.  gdi_fetch16: the four aligned words that hold the bytes.
// gdi_align12: the bytes as three little-endian words, shift = gdi_shift(off).  A lane's groups are 12 bytes apart, so its shift never changes.
GDI_HD void gdi_fetch16(const unsigned char* base, long long off, long long total, unsigned q[4]) {
  const long long a = off & ~3ll;                                  // rounds down, also below zero
  for (int k = 0; k < 4; ++k) q[k] = gdi_word(base, a + 4 * k, total);
}
GDI_HD int gdi_shift(long long off) { return 8 * (int)(off & 3ll); }
GDI_HD void gdi_align12(const unsigned q[4], int shift, unsigned w[3]) {
  for (int k = 0; k < 3; ++k) w[k] = (unsigned)(((unsigned long long)q[k + 1] << 32 | q[k]) >> shift);
}

// Pixel k (0 .. 3) of a group's words.
GDI_HD void gdi_pixel(const unsigned w[3], int k, unsigned* r, unsigned* g, unsigned* b) {
  const unsigned long long lo = (unsigned long long)w[1] << 32 | w[0];
  const unsigned v = k < 2 ? (unsigned)(lo >> (24 * k)) : k == 2 ? (w[1] >> 16 | w[2] << 16) : w[2] >> 8;
  *r = v & 255u, *g = (v >> 8) & 255u, *b = (v >> 16) & 255u;
}
