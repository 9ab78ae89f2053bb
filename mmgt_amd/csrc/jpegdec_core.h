// Baseline JPEG decode arithmetic (ITU T.81 sequential DCT, 8 bit), written once as plain inline functions: csrc/jpegdec.hip calls them
// from its kernels and tools/jpegdec_host_check.cpp from a host program, so the bytes a kernel produces can be checked without a GPU.  Nothing here
// touches memory outside the ranges its arguments name, whatever the entropy-coded bytes hold: bad data ends in a status, not in a write.
//
//  * jd_decode_segment   one restart segment -> int16 coefficients in natural order (Huffman decode by T.81 F.2.2.3 from MINCODE / MAXCODE /
//                        VALPTR / HUFFVAL, DC prediction, 0xFF 0x00 unstuffing, zero bits past the end)
//  * jd_idct_block       dequantise + the 8 x 8 inverse DCT of libjpeg's jidctint.c (jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2), + 128, clamp
//  * jd_pixel            chroma up-sampling ("fancy" triangle filters of libjpeg's jdsample.c for 4:2:0 / 4:2:2) and the YCbCr -> RGB of jdcolor.c
//
// Per-frame table block (int32 words, JD_TAB_INTS of them): [0..2] quantiser table of component c, [3..5] DC table, [6..8] AC table,
// [16 + 64 t + i] quantiser table t entry i (natural order), then four Huffman tables (DC 0, DC 1, AC 0, AC 1) of JD_HUFF_INTS words each:
// MINCODE[0..16], MAXCODE[0..16] (-1: no code of that length), VALPTR[0..16], HUFFVAL[0..255]; index 0 of the first three is unused.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ inline
#else
#define JD_HD inline
#endif

enum {
  JD_TAB_SEL = 0,
  JD_TAB_Q = 16,
  JD_TAB_HUFF = JD_TAB_Q + 4 * 64,
  JD_HUFF_MIN = 0,
  JD_HUFF_MAX = 17,
  JD_HUFF_PTR = 34,
  JD_HUFF_VAL = 51,
  JD_HUFF_INTS = 51 + 256,
  JD_TAB_INTS = JD_TAB_HUFF + 4 * JD_HUFF_INTS
};

// per-segment status words
enum {
  JD_OK = 0,
  JD_ST_CODE = 1,        // a code longer than 16 bits
  JD_ST_INDEX = 2,       // a coefficient index past 63
  JD_ST_CATEGORY = 3,    // a DC category above 11 or an AC category above 10
  JD_ST_DC_RANGE = 4,    // an accumulated DC outside [-2048, 2047]
  JD_ST_EXHAUSTED = 5,   // data exhausted before the last block
  JD_ST_DESCRIPTOR = 6   // the segment's own descriptor (frame, MCU range, byte range) is out of range: nothing was read
};

// luma sampling hs x vs in {1x1, 2x1, 2x2}, chroma 1x1; one component: hs = vs = 1 (a single-component scan is not interleaved)
struct JdGeom {
  int H, W, ncomp, hs, vs, mcu_rows, mcu_cols;
};

JD_HD bool jd_geom(int H, int W, int ncomp, int hs, int vs, JdGeom* g) {
  const bool sampling = (hs == 1 && vs == 1) || (ncomp == 3 && hs == 2 && (vs == 1 || vs == 2));
  if (!sampling || (ncomp != 1 && ncomp != 3) || H < 1 || W < 1 || H > 65535 || W > 65535) return false;
  g->H = H, g->W = W, g->ncomp = ncomp, g->hs = hs, g->vs = vs;
  g->mcu_rows = (H + 8 * vs - 1) / (8 * vs);
  g->mcu_cols = (W + 8 * hs - 1) / (8 * hs);
  return true;
}
// blocks per row / rows of blocks of component c's plane, and the plane's first block within a frame (planes follow each other)
JD_HD int jd_bw(const JdGeom& g, int c) { return g.mcu_cols * (c == 0 ? g.hs : 1); }
JD_HD int jd_bh(const JdGeom& g, int c) { return g.mcu_rows * (c == 0 ? g.vs : 1); }
JD_HD long long jd_block0(const JdGeom& g, int c) {
  return c == 0 ? 0 : (long long)jd_bw(g, 0) * jd_bh(g, 0) + (long long)(c - 1) * g.mcu_cols * g.mcu_rows;
}
JD_HD long long jd_frame_blocks(const JdGeom& g) { return jd_block0(g, g.ncomp); }

// zigzag position -> natural index (T.81 figure A.6)
JD_HD int jd_natural(int k) {
  constexpr unsigned char z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k & 63];
}

// ---- entropy decode ---------------------------------------------------------------------------------------------------------------------------
// MSB-first reader over data[pos, end): the 0x00 after a 0xFF is dropped; a 0xFF followed by anything else (fill bytes before a marker) ends the
// data; past the end the bits are zeros, counted in `pad` so that the caller can tell whether it consumed any of them.
struct JdBits {
  const unsigned char* data;
  long long pos, end;
  uint64_t acc;
  int cnt, pad;
};
JD_HD void jd_fill(JdBits& b) {
  while (b.cnt <= 56) {
    unsigned v = 0;
    if (b.pos < b.end) {
      v = b.data[b.pos++];
      if (v == 0xFF) {
        if (b.pos < b.end && b.data[b.pos] == 0) {
          ++b.pos;
        } else {
          b.pos = b.end;
          v = 0;
          b.pad += 8;
        }
      }
    } else {
      b.pad += 8;
    }
    b.acc = b.acc << 8 | v;
    b.cnt += 8;
  }
}
JD_HD int jd_receive(JdBits& b, int n) {                           // n <= 16 bits, cnt >= n
  b.cnt -= n;
  return (int)(b.acc >> b.cnt) & ((1 << n) - 1);
}
// T.81 F.2.2.3 DECODE over a 16-bit look: the symbol, or -1 when no code of up to 16 bits matches
JD_HD int jd_huff(JdBits& b, const int32_t* h) {
  const int look = (int)(b.acc >> (b.cnt - 16)) & 0xFFFF;
  for (int l = 1; l <= 16; ++l) {
    const int code = look >> (16 - l);
    if (code <= h[JD_HUFF_MAX + l]) {
      b.cnt -= l;
      return h[JD_HUFF_VAL + ((code - h[JD_HUFF_MIN + l] + h[JD_HUFF_PTR + l]) & 255)] & 255;
    }
  }
  return -1;
}
JD_HD int jd_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }        // T.81 F.2.2.1, s >= 1

// The MCUs [mcu0, mcu1) of one frame from data[beg, end) into coef (the FRAME's coefficient block, zero-filled by the caller): returns a status.
// Only blocks of those MCUs are written.
JD_HD int jd_decode_segment(const unsigned char* data, long long beg, long long end, const int32_t* tab, const JdGeom& g, int mcu0, int mcu1,
                            int16_t* coef) {
  JdBits b = {data, beg, end, 0, 0, 0};
  int pred[3] = {0, 0, 0};
  for (int m = mcu0; m < mcu1; ++m) {
    const int my = m / g.mcu_cols, mx = m - my * g.mcu_cols;
    for (int c = 0; c < g.ncomp; ++c) {
      const int hs = c == 0 ? g.hs : 1, vs = c == 0 ? g.vs : 1;
      const int32_t* dc = tab + JD_TAB_HUFF + (tab[JD_TAB_SEL + 3 + c] & 1) * JD_HUFF_INTS;
      const int32_t* ac = tab + JD_TAB_HUFF + (2 + (tab[JD_TAB_SEL + 6 + c] & 1)) * JD_HUFF_INTS;
      for (int v = 0; v < vs; ++v)
        for (int h = 0; h < hs; ++h) {
          int16_t* blk = coef + (jd_block0(g, c) + (long long)(my * vs + v) * jd_bw(g, c) + (mx * hs + h)) * 64;
          jd_fill(b);
          int s = jd_huff(b, dc);
          if (s < 0) return JD_ST_CODE;
          if (s > 11) return JD_ST_CATEGORY;
          if (s) pred[c] += jd_extend(jd_receive(b, s), s);
          if (pred[c] < -2048 || pred[c] > 2047) return JD_ST_DC_RANGE;
          blk[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            jd_fill(b);
            const int rs = jd_huff(b, ac);
            if (rs < 0) return JD_ST_CODE;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;                                  // EOB
              k += 16;                                             // ZRL
              if (k > 64) return JD_ST_INDEX;
              continue;
            }
            if (s > 10) return JD_ST_CATEGORY;
            k += r;
            if (k > 63) return JD_ST_INDEX;
            blk[jd_natural(k)] = (int16_t)jd_extend(jd_receive(b, s), s);
            ++k;
          }
          if (b.cnt < b.pad) return JD_ST_EXHAUSTED;               // some of the bits this block took were zeros past the end
        }
    }
  }
  return JD_OK;
}

// ---- dequantise + inverse DCT -------------------------------------------------------------------------------------------------------------------
// jpeg_idct_islow in unsigned 32-bit wrap (no signed overflow for any int16 coefficient x quantiser); the descales shift the wrapped value
// arithmetically.  libjpeg's shortcut for a column / row without AC terms gives the same number as the full pass, which is all that runs here.
JD_HD constexpr uint32_t jd_fix(double x) { return (uint32_t)(int32_t)(x * 8192 + 0.5); }
JD_HD int32_t jd_descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }
// one 1-D pass over in[0..7] (already dequantised / workspace values); out[i] = descale(..., shift)
JD_HD void jd_idct_1d(const uint32_t* in, int32_t* out, int shift) {
  const uint32_t F0_298 = jd_fix(0.298631336), F0_390 = jd_fix(0.390180644), F0_541 = jd_fix(0.541196100), F0_765 = jd_fix(0.765366865),
                 F0_899 = jd_fix(0.899976223), F1_175 = jd_fix(1.175875602), F1_501 = jd_fix(1.501321110), F1_847 = jd_fix(1.847759065),
                 F1_961 = jd_fix(1.961570560), F2_053 = jd_fix(2.053119869), F2_562 = jd_fix(2.562915447), F3_072 = jd_fix(3.072711026);
  uint32_t z1, z2, z3, z4, z5, tmp0, tmp1, tmp2, tmp3, tmp10, tmp11, tmp12, tmp13;
  z2 = in[2], z3 = in[6];
  z1 = (z2 + z3) * F0_541;
  tmp2 = z1 - z3 * F1_847;
  tmp3 = z1 + z2 * F0_765;
  z2 = in[0], z3 = in[4];
  tmp0 = (z2 + z3) << 13;
  tmp1 = (z2 - z3) << 13;
  tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
  z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
  z5 = (z3 + z4) * F1_175;
  tmp0 *= F0_298, tmp1 *= F2_053, tmp2 *= F3_072, tmp3 *= F1_501;
  z1 = 0u - z1 * F0_899, z2 = 0u - z2 * F2_562, z3 = 0u - z3 * F1_961, z4 = 0u - z4 * F0_390;
  z3 += z5, z4 += z5;
  tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
  out[0] = jd_descale(tmp10 + tmp3, shift), out[7] = jd_descale(tmp10 - tmp3, shift);
  out[1] = jd_descale(tmp11 + tmp2, shift), out[6] = jd_descale(tmp11 - tmp2, shift);
  out[2] = jd_descale(tmp12 + tmp1, shift), out[5] = jd_descale(tmp12 - tmp1, shift);
  out[3] = jd_descale(tmp13 + tmp0, shift), out[4] = jd_descale(tmp13 - tmp0, shift);
}
// coef[64] natural order, q[64] natural order -> out[y * stride + x], 8 x 8 samples
JD_HD void jd_idct_block(const int16_t* coef, const int32_t* q, unsigned char* out, long long stride) {
  uint32_t ws[64];
  for (int x = 0; x < 8; ++x) {                                    // columns, descaled by CONST_BITS - PASS1_BITS
    uint32_t in[8];
    int32_t o[8];
    for (int y = 0; y < 8; ++y) in[y] = (uint32_t)(int32_t)coef[y * 8 + x] * (uint32_t)q[y * 8 + x];
    jd_idct_1d(in, o, 11);
    for (int y = 0; y < 8; ++y) ws[y * 8 + x] = (uint32_t)o[y];
  }
  for (int y = 0; y < 8; ++y) {                                    // rows, descaled by CONST_BITS + PASS1_BITS + 3
    int32_t o[8];
    jd_idct_1d(ws + y * 8, o, 18);
    for (int x = 0; x < 8; ++x) {
      const int32_t v = o[x] + 128;
      out[y * stride + x] = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
  }
}

// ---- up-sampling + colour ---------------------------------------------------------------------------------------------------------------------
JD_HD int jd_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// one chroma sample of plane p (row stride `stride`) at output pixel (y, x); cw x ch are the plane's REAL size (ceil(W / hs), ceil(H / vs))
JD_HD int jd_chroma(const unsigned char* p, long long stride, const JdGeom& g, int cw, int ch, int y, int x) {
  if (g.hs == 1) return p[y * stride + x];                                             // 4:4:4
  const int c = x >> 1;
  if (cw <= 2) return p[(g.vs == 2 ? y >> 1 : y) * stride + c];                         // libjpeg replicates a plane of 1 or 2 columns
  if (g.vs == 1) {                                                                     // h2v1
    const unsigned char* row = p + y * stride;
    if (x & 1) return c == cw - 1 ? row[c] : (3 * row[c] + row[c + 1] + 2) >> 2;
    return c == 0 ? row[0] : (3 * row[c] + row[c - 1] + 1) >> 2;
  }
  const int r = y >> 1;                                                                 // h2v2
  int nb = (y & 1) ? r + 1 : r - 1;
  nb = nb < 0 ? 0 : nb > ch - 1 ? ch - 1 : nb;
  const unsigned char *r0 = p + r * stride, *r1 = p + nb * stride;
  const int s = 3 * r0[c] + r1[c];
  if (x & 1) return c == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[c + 1] + r1[c + 1] + 7) >> 4;
  return c == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[c - 1] + r1[c - 1] + 8) >> 4;
}
// planes: one frame's component planes (MCU-padded, in component order) -> rgb[3] of pixel (y, x), y < H, x < W
JD_HD void jd_pixel(const unsigned char* planes, const JdGeom& g, int y, int x, unsigned char* rgb) {
  const long long s0 = (long long)jd_bw(g, 0) * 8;
  const int yy = planes[y * s0 + x];
  if (g.ncomp == 1) {
    rgb[0] = rgb[1] = rgb[2] = (unsigned char)yy;
    return;
  }
  const long long sc = (long long)g.mcu_cols * 8;
  const int cw = (g.W + g.hs - 1) / g.hs, ch = (g.H + g.vs - 1) / g.vs;
  const int cb = jd_chroma(planes + jd_block0(g, 1) * 64, sc, g, cw, ch, y, x) - 128;
  const int cr = jd_chroma(planes + jd_block0(g, 2) * 64, sc, g, cw, ch, y, x) - 128;
  rgb[0] = (unsigned char)jd_clamp255(yy + ((91881 * cr + 32768) >> 16));                             // F(1.402)
  rgb[1] = (unsigned char)jd_clamp255(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16));                // F(0.34414), F(0.71414)
  rgb[2] = (unsigned char)jd_clamp255(yy + ((116130 * cb + 32768) >> 16));                            // F(1.772)
}

// ---- the three units of work, as the kernels and the host program index them ---------------------------------------------------------------
// Segment s of a batch of n frames: data[offsets[s], offsets[s + 1]) holds the MCUs [seginfo[3 s + 1], seginfo[3 s + 2]) of frame seginfo[3 s].
// The descriptor is checked against the batch before anything is read or written.  coef: (n, frame blocks, 64), zero-filled.
JD_HD int jd_segment(const unsigned char* data, long long data_bytes, const long long* offsets, const int32_t* seginfo, const int32_t* tables,
                     int16_t* coef, const JdGeom& g, int n, long long s) {
  const int frame = seginfo[3 * s], mcu0 = seginfo[3 * s + 1], mcu1 = seginfo[3 * s + 2];
  const long long beg = offsets[s], end = offsets[s + 1];
  if (frame < 0 || frame >= n || mcu0 < 0 || mcu1 < mcu0 || mcu1 > g.mcu_rows * g.mcu_cols || beg < 0 || end < beg || end > data_bytes)
    return JD_ST_DESCRIPTOR;
  return jd_decode_segment(data, beg, end, tables + (long long)frame * JD_TAB_INTS, g, mcu0, mcu1, coef + (long long)frame * jd_frame_blocks(g) * 64);
}
// Block b of the batch (b < n * frame blocks): coef (n, frame blocks, 64) -> planes (n, frame blocks * 64), component planes one after another
JD_HD void jd_block(const int16_t* coef, const int32_t* tables, unsigned char* planes, const JdGeom& g, long long b) {
  const long long fb = jd_frame_blocks(g);
  const long long frame = b / fb, k = b - frame * fb;
  const int c = (g.ncomp == 1 || k < jd_block0(g, 1)) ? 0 : k < jd_block0(g, 2) ? 1 : 2;
  const long long kc = k - jd_block0(g, c);
  const int bw = jd_bw(g, c);
  const long long by = kc / bw, bx = kc - by * bw;
  const int32_t* tab = tables + frame * JD_TAB_INTS;
  jd_idct_block(coef + b * 64, tab + JD_TAB_Q + 64 * (tab[JD_TAB_SEL + c] & 3), planes + (frame * fb + jd_block0(g, c)) * 64 + (by * 8 * bw + bx) * 8,
                (long long)bw * 8);
}
// Pixel p of the batch (p < n * H * W): planes -> out (n, H, W, 3)
JD_HD void jd_output_pixel(const unsigned char* planes, unsigned char* out, const JdGeom& g, long long p) {
  const long long hw = (long long)g.H * g.W;
  const long long frame = p / hw, r = p - frame * hw;
  const int y = (int)(r / g.W), x = (int)(r - (long long)y * g.W);
  unsigned char rgb[3];
  jd_pixel(planes + frame * jd_frame_blocks(g) * 64, g, y, x, rgb);
  out[p * 3] = rgb[0], out[p * 3 + 1] = rgb[1], out[p * 3 + 2] = rgb[2];
}
