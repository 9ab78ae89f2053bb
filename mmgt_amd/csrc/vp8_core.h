// Lossy WebP output: VP8 key frames, the per-block and per-symbol arithmetic written once.  csrc/vp8.hip calls these functions from its
// kernels and tools/vp8_host_check.cpp from a host program, so a frame can be run through them without a GPU and held to tests/vp8_ref.py.
//
// The stream: key frames; 16 x 16 luma modes DC / V / H / TM (0 .. 3) and the same four for chroma, no 4 x 4 modes, no segments, no filter deltas, no
// probability updates, mb_no_coeff_skip = 1, one quantiser index, 1 / 2 / 4 / 8 token partitions (macroblock row r in partition r mod P).  The format
// fixes the inverse transforms, the dequantisation, the prediction edges, the trees and the tables (RFC 6386); the colour conversion, the forward
// transforms, the quantiser's rounding, the mode choice and the quality map are ours and use integers only.
//
// A macroblock's levels are 25 blocks of 16 int16 in scan (zigzag) order: 0 .. 15 luma in raster order (entry 0 of each is 0, its DC is in the Y2
// block), 16 .. 19 U, 20 .. 23 V, 24 the Y2 block.  Its non-zero mask has bit b set when block b holds a non-zero level.  Nothing here reads or
// writes outside the planes, the macroblock's levels or the coder's slot.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define V8_HD __host__ __device__ inline
#else
#define V8_HD inline
#endif

enum {
  V8_MAX_SIDE = 16383,           // the 14-bit sizes of the frame header
  V8_MAX_LEVEL = 2047,           // a level's magnitude: the largest category codes 67 .. 2114, a clamp at 2047 keeps its 11 extra bits
  V8_MB_LEVELS = 25 * 16,
  V8_HEADER_SYMBOLS = 1100,      // a first partition before its macroblocks: 29 header bits, 1056 update flags, 9 for the skip probability
  V8_MB_MODE_SYMBOLS = 7,        // skip flag, three for the luma mode, three for the chroma mode
  V8_MB_TOKEN_SYMBOLS = 384 * 19,  // 16 * 15 + 8 * 16 + 16 coefficients, each at most 7 tree bits, 11 extra bits and a sign
  V8_FLUSH_BYTES = 4             // the 32 closing symbols shift one bit each at most
};
// A symbol shifts the coder by at most 8 bits (probabilities are 1 .. 255 of 256), so a slot of one byte per symbol plus the flush holds any
// partition.
V8_HD long long v8_first_slot_bytes(long long mbs) { return V8_HEADER_SYMBOLS + V8_MB_MODE_SYMBOLS * mbs + V8_FLUSH_BYTES; }
V8_HD long long v8_token_slot_bytes(long long mbs) { return V8_MB_TOKEN_SYMBOLS * mbs + V8_FLUSH_BYTES; }

// ---- tables of the format ---------------------------------------------------------------------------------------------------------------------------
V8_HD int v8_dc_q(int q) {
  constexpr unsigned char t[128] = {
      4,5,6,7,8,9,10,10,11,12,13,14,15,16,17,17,18,19,20,20,21,21,22,22,23,23,24,25,25,26,27,28,
      29,30,31,32,33,34,35,36,37,37,38,39,40,41,42,43,44,45,46,46,47,48,49,50,51,52,53,54,55,56,57,58,
      59,60,61,62,63,64,65,66,67,68,69,70,71,72,73,74,75,76,76,77,78,79,80,81,82,83,84,85,86,87,88,89,
      91,93,95,96,98,100,101,102,104,106,108,110,112,114,116,118,122,124,126,128,130,132,134,136,138,140,143,145,148,151,154,157};
  return t[q < 0 ? 0 : q > 127 ? 127 : q];
}
V8_HD int v8_ac_q(int q) {
  constexpr unsigned short t[128] = {
      4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,34,35,
      36,37,38,39,40,41,42,43,44,45,46,47,48,49,50,51,52,53,54,55,56,57,58,60,62,64,66,68,70,72,74,76,
      78,80,82,84,86,88,90,92,94,96,98,100,102,104,106,108,110,112,114,116,119,122,125,128,131,134,137,140,143,146,149,152,
      155,158,161,164,167,170,173,177,181,185,189,193,197,201,205,209,213,217,221,225,229,234,239,245,249,254,259,264,269,274,279,284};
  return t[q < 0 ? 0 : q > 127 ? 127 : q];
}
V8_HD int v8_zigzag(int n) {
  constexpr unsigned char t[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
  return t[n & 15];
}
V8_HD int v8_band(int n) {
  constexpr unsigned char t[17] = {0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0};
  return t[n < 0 ? 0 : n > 16 ? 16 : n];
}
// extra-bit probabilities of the categories 3 .. 6, the most significant bit first
V8_HD int v8_cat_prob(int cat, int k) {
  constexpr unsigned char t[4][11] = {{173, 148, 140}, {176, 155, 140, 135}, {180, 157, 141, 134, 130}, {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129}};
  return t[(cat - 3) & 3][k < 0 ? 0 : k > 10 ? 10 : k];
}
// default coefficient probabilities [type 4][band 8][context 3][node 11]; a row below is one [type][band]
V8_HD int v8_coef_prob(int type, int band, int ctx, int node) {
  constexpr unsigned char t[1056] = {
      128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,
      253,136,254,255,228,219,128,128,128,128,128,189,129,242,255,227,213,255,219,128,128,128,106,126,227,252,214,209,255,255,128,128,128,
      1,98,248,255,236,226,255,255,128,128,128,181,133,238,254,221,234,255,154,128,128,128,78,134,202,247,198,180,255,219,128,128,128,
      1,185,249,255,243,255,128,128,128,128,128,184,150,247,255,236,224,128,128,128,128,128,77,110,216,255,236,230,128,128,128,128,128,
      1,101,251,255,241,255,128,128,128,128,128,170,139,241,252,236,209,255,255,128,128,128,37,116,196,243,228,255,255,255,128,128,128,
      1,204,254,255,245,255,128,128,128,128,128,207,160,250,255,238,128,128,128,128,128,128,102,103,231,255,211,171,128,128,128,128,128,
      1,152,252,255,240,255,128,128,128,128,128,177,135,243,255,234,225,128,128,128,128,128,80,129,211,255,194,224,128,128,128,128,128,
      1,1,255,128,128,128,128,128,128,128,128,246,1,255,128,128,128,128,128,128,128,128,255,128,128,128,128,128,128,128,128,128,128,
      198,35,237,223,193,187,162,160,145,155,62,131,45,198,221,172,176,220,157,252,221,1,68,47,146,208,149,167,221,162,255,223,128,
      1,149,241,255,221,224,255,255,128,128,128,184,141,234,253,222,220,255,199,128,128,128,81,99,181,242,176,190,249,202,255,255,128,
      1,129,232,253,214,197,242,196,255,255,128,99,121,210,250,201,198,255,202,128,128,128,23,91,163,242,170,187,247,210,255,255,128,
      1,200,246,255,234,255,128,128,128,128,128,109,178,241,255,231,245,255,255,128,128,128,44,130,201,253,205,192,255,255,128,128,128,
      1,132,239,251,219,209,255,165,128,128,128,94,136,225,251,218,190,255,255,128,128,128,22,100,174,245,186,161,255,199,128,128,128,
      1,182,249,255,232,235,128,128,128,128,128,124,143,241,255,227,234,128,128,128,128,128,35,77,181,251,193,211,255,205,128,128,128,
      1,157,247,255,236,231,255,255,128,128,128,121,141,235,255,225,227,255,255,128,128,128,45,99,188,251,195,217,255,224,128,128,128,
      1,1,251,255,213,255,128,128,128,128,128,203,1,248,255,255,128,128,128,128,128,128,137,1,177,255,224,255,128,128,128,128,128,
      253,9,248,251,207,208,255,192,128,128,128,175,13,224,243,193,185,249,198,255,255,128,73,17,171,221,161,179,236,167,255,234,128,
      1,95,247,253,212,183,255,255,128,128,128,239,90,244,250,211,209,255,255,128,128,128,155,77,195,248,188,195,255,255,128,128,128,
      1,24,239,251,218,219,255,205,128,128,128,201,51,219,255,196,186,128,128,128,128,128,69,46,190,239,201,218,255,228,128,128,128,
      1,191,251,255,255,128,128,128,128,128,128,223,165,249,255,213,255,128,128,128,128,128,141,124,248,255,255,128,128,128,128,128,128,
      1,16,248,255,255,128,128,128,128,128,128,190,36,230,255,236,255,128,128,128,128,128,149,1,255,128,128,128,128,128,128,128,128,
      1,226,255,128,128,128,128,128,128,128,128,247,192,255,128,128,128,128,128,128,128,128,240,128,255,128,128,128,128,128,128,128,128,
      1,134,252,255,255,128,128,128,128,128,128,213,62,250,255,255,128,128,128,128,128,128,55,93,255,128,128,128,128,128,128,128,128,
      128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,128,
      202,24,213,235,186,191,220,160,240,175,255,126,38,182,232,169,184,228,174,255,187,128,61,46,138,219,151,178,240,170,255,216,128,
      1,112,230,250,199,191,247,159,255,255,128,166,109,228,252,211,215,255,174,128,128,128,39,77,162,232,172,180,245,178,255,255,128,
      1,52,220,246,198,199,249,220,255,255,128,124,74,191,243,183,193,250,221,255,255,128,24,71,130,219,154,170,243,182,255,255,128,
      1,182,225,249,219,240,255,224,128,128,128,149,150,226,252,216,205,255,171,128,128,128,28,108,170,242,183,194,254,223,255,255,128,
      1,81,230,252,204,203,255,192,128,128,128,123,102,209,247,188,196,255,233,128,128,128,20,95,153,243,164,173,255,203,128,128,128,
      1,222,248,255,216,213,128,128,128,128,128,168,175,246,252,235,205,255,255,128,128,128,47,116,215,255,211,212,255,255,128,128,128,
      1,121,236,253,212,214,255,255,128,128,128,141,84,213,252,201,202,255,219,128,128,128,42,80,160,240,162,185,255,205,128,128,128,
      1,1,255,128,128,128,128,128,128,128,128,244,1,255,128,128,128,128,128,128,128,128,238,1,255,128,128,128,128,128,128,128,128};
  return t[(((type & 3) * 8 + (band & 7)) * 3 + (ctx < 0 ? 0 : ctx > 2 ? 2 : ctx)) * 11 + (node < 0 ? 0 : node > 10 ? 10 : node)];
}
// the whole table, for a caller that keeps it close (csrc/vp8.hip copies it into LDS): entry ((type * 8 + band) * 3 + ctx) * 11 + node
V8_HD void v8_coef_table(unsigned char* dst, int first, int step) {
  for (int i = first; i < 1056; i += step) dst[i] = (unsigned char)v8_coef_prob(i / 264, i / 33 % 8, i / 11 % 3, i % 11);
}
// the probability of the "no update" flag of coefficient probability i = 0 .. 1055: 255 but for these 158 (index, value) pairs, ascending
V8_HD int v8_update_prob(int i) {
  constexpr unsigned short t[158][2] = {
      {33, 176}, {34, 246}, {44, 223}, {45, 241}, {46, 252}, {55, 249}, {56, 253}, {57, 253}, {67, 244}, {68, 252}, {77, 234}, {78, 254}, {79, 254},
      {88, 253}, {100, 246}, {101, 254}, {110, 239}, {111, 253}, {112, 254}, {121, 254}, {123, 254}, {133, 248}, {134, 254}, {143, 251}, {145, 254},
      {166, 253}, {167, 254}, {176, 251}, {177, 254}, {178, 254}, {187, 254}, {189, 254}, {199, 254}, {200, 253}, {202, 254}, {209, 250}, {211, 254},
      {213, 254}, {220, 254}, {264, 217}, {275, 225}, {276, 252}, {277, 241}, {278, 253}, {281, 254}, {286, 234}, {287, 250}, {288, 241}, {289, 250},
      {290, 253}, {292, 253}, {293, 254}, {298, 254}, {308, 223}, {309, 254}, {310, 254}, {319, 238}, {320, 253}, {321, 254}, {322, 254}, {331, 248},
      {332, 254}, {341, 249}, {342, 254}, {364, 253}, {374, 247}, {375, 254}, {397, 253}, {398, 254}, {407, 252}, {430, 254}, {431, 254}, {440, 253},
      {463, 254}, {464, 253}, {473, 250}, {484, 254}, {528, 186}, {529, 251}, {530, 250}, {539, 234}, {540, 251}, {541, 244}, {542, 254}, {550, 251},
      {551, 251}, {552, 243}, {553, 253}, {554, 254}, {556, 254}, {562, 253}, {563, 254}, {572, 236}, {573, 253}, {574, 254}, {583, 251}, {584, 253},
      {585, 253}, {586, 254}, {587, 254}, {595, 254}, {596, 254}, {605, 254}, {606, 254}, {607, 254}, {628, 254}, {638, 254}, {639, 254}, {649, 254},
      {671, 254}, {792, 248}, {803, 250}, {804, 254}, {805, 252}, {806, 254}, {814, 248}, {815, 254}, {816, 249}, {817, 253}, {826, 253}, {827, 253},
      {836, 246}, {837, 253}, {838, 253}, {847, 252}, {848, 254}, {849, 251}, {850, 254}, {851, 254}, {859, 254}, {860, 252}, {869, 248}, {870, 254},
      {871, 253}, {880, 253}, {882, 254}, {883, 254}, {892, 251}, {893, 254}, {902, 245}, {903, 251}, {904, 254}, {913, 253}, {914, 253}, {915, 254},
      {925, 251}, {926, 253}, {935, 252}, {936, 253}, {937, 254}, {947, 254}, {958, 252}, {968, 249}, {970, 254}, {981, 254}, {992, 253}, {1001, 250},
      {1034, 254}};
  int lo = 0, hi = 157;                                            // eight steps at most
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid][0] < i) lo = mid + 1; else hi = mid;
  }
  return t[lo][0] == i ? t[lo][1] : 255;
}

// ---- ours: quality, quantisers, default filter level ------------------------------------------------------------------------------------------------
V8_HD int v8_quality_to_q(int quality) { return (100 - quality) * 127 / 100; }   // 100 -> 0 (finest), 0 -> 127
V8_HD int v8_default_filter_level(int q) {                         // by q / 8; chosen from profiles/vp8/filter_level.jsonl
  constexpr unsigned char t[16] = {0, 8, 12, 16, 16, 16, 24, 24, 24, 32, 32, 32, 48, 48, 48, 48};
  return t[(q >> 3) & 15];
}
struct V8Quant {
  int ydc, yac, y2dc, y2ac, uvdc, uvac;
};
V8_HD V8Quant v8_quant(int q) {                                    // the format's, all deltas 0
  V8Quant m;
  m.ydc = v8_dc_q(q), m.yac = v8_ac_q(q);
  m.y2dc = v8_dc_q(q) * 2, m.y2ac = v8_ac_q(q) * 101581 >> 16;
  if (m.y2ac < 8) m.y2ac = 8;
  m.uvdc = v8_dc_q(q > 117 ? 117 : q), m.uvac = v8_ac_q(q);
  return m;
}
// level = sign(c) * min(2047, (|c| + (q * bias >> 3)) / q): bias 4 rounds to nearest (DC terms), 3 leaves a small dead zone (AC terms)
V8_HD int v8_quantise(int c, int q, int bias) {
  int a = c < 0 ? -c : c;
  a = (a + (q * bias >> 3)) / q;
  if (a > V8_MAX_LEVEL) a = V8_MAX_LEVEL;
  return c < 0 ? -a : a;
}
V8_HD int v8_clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// ---- ours: RGB -> studio-range YUV 4:2:0 of the frame padded to whole macroblocks by edge replication ----------------------------------------------
V8_HD const unsigned char* v8_rgb_at(const unsigned char* frame, int H, int W, int y, int x) {
  return frame + 3 * ((long)(y < H ? y : H - 1) * W + (x < W ? x : W - 1));
}
V8_HD int v8_luma(const unsigned char* frame, int H, int W, int y, int x) {
  const unsigned char* p = v8_rgb_at(frame, H, W, y, x);
  return v8_clip255((16839 * p[0] + 33059 * p[1] + 6420 * p[2] + (16 << 16) + 32768) >> 16);
}
V8_HD void v8_chroma(const unsigned char* frame, int H, int W, int cy, int cx, int* u, int* v) {   // from the sums over the 2 x 2 cell
  int r = 0, g = 0, b = 0;
  for (int k = 0; k < 4; ++k) {
    const unsigned char* p = v8_rgb_at(frame, H, W, 2 * cy + (k >> 1), 2 * cx + (k & 1));
    r += p[0], g += p[1], b += p[2];
  }
  *u = v8_clip255((-9719 * r - 19081 * g + 28800 * b + (128 << 18) + (1 << 17)) >> 18);
  *v = v8_clip255((28800 * r - 24116 * g - 4684 * b + (128 << 18) + (1 << 17)) >> 18);
}

// ---- transforms: the forward ones are ours, the inverse ones the format's ---------------------------------------------------------------------------
V8_HD void v8_fdct(const int* d, int* out) {                       // 16 differences -> 16 coefficients, both in raster order
  int t[16];
  for (int i = 0; i < 4; ++i) {
    const int a0 = d[4 * i] + d[4 * i + 3], a1 = d[4 * i + 1] + d[4 * i + 2], a2 = d[4 * i + 1] - d[4 * i + 2], a3 = d[4 * i] - d[4 * i + 3];
    t[4 * i] = (a0 + a1) * 8;
    t[4 * i + 1] = (a2 * 2217 + a3 * 5352 + 1812) >> 9;
    t[4 * i + 2] = (a0 - a1) * 8;
    t[4 * i + 3] = (a3 * 2217 - a2 * 5352 + 937) >> 9;
  }
  for (int i = 0; i < 4; ++i) {
    const int a0 = t[i] + t[12 + i], a1 = t[4 + i] + t[8 + i], a2 = t[4 + i] - t[8 + i], a3 = t[i] - t[12 + i];
    out[i] = (a0 + a1 + 7) >> 4;
    out[4 + i] = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0);
    out[8 + i] = (a0 - a1 + 7) >> 4;
    out[12 + i] = (a3 * 2217 - a2 * 5352 + 51000) >> 16;
  }
}
V8_HD void v8_fwht(const int* dc, int* out) {                      // the 16 blocks' DC terms -> 16 coefficients in raster order
  int t[16];
  for (int i = 0; i < 4; ++i) {
    const int a0 = dc[4 * i] + dc[4 * i + 2], a1 = dc[4 * i + 1] + dc[4 * i + 3], a2 = dc[4 * i + 1] - dc[4 * i + 3], a3 = dc[4 * i] - dc[4 * i + 2];
    t[4 * i] = a0 + a1, t[4 * i + 1] = a3 + a2, t[4 * i + 2] = a3 - a2, t[4 * i + 3] = a0 - a1;
  }
  for (int i = 0; i < 4; ++i) {
    const int a0 = t[i] + t[8 + i], a1 = t[4 + i] + t[12 + i], a2 = t[4 + i] - t[12 + i], a3 = t[i] - t[8 + i];
    out[i] = (a0 + a1) >> 1, out[4 + i] = (a3 + a2) >> 1, out[8 + i] = (a3 - a2) >> 1, out[12 + i] = (a0 - a1) >> 1;
  }
}
V8_HD int v8_mul1(int a) { return ((a * 20091) >> 16) + a; }
V8_HD int v8_mul2(int a) { return (a * 35468) >> 16; }
// the format's inverse DCT of 16 raster coefficients, added to pred (4 x 4, its own array) and written to dst (stride pixels a row)
V8_HD void v8_idct_add(const int* c, const int* pred, unsigned char* dst, long stride) {
  int t[16];
  for (int i = 0; i < 4; ++i) {                                    // vertical pass of column i
    const int a = c[i] + c[8 + i], b = c[i] - c[8 + i];
    const int cc = v8_mul2(c[4 + i]) - v8_mul1(c[12 + i]), d = v8_mul1(c[4 + i]) + v8_mul2(c[12 + i]);
    t[4 * i] = a + d, t[4 * i + 1] = b + cc, t[4 * i + 2] = b - cc, t[4 * i + 3] = a - d;
  }
  for (int i = 0; i < 4; ++i) {                                    // horizontal pass of row i
    const int dc = t[i] + 4, a = dc + t[8 + i], b = dc - t[8 + i];
    const int cc = v8_mul2(t[4 + i]) - v8_mul1(t[12 + i]), d = v8_mul1(t[4 + i]) + v8_mul2(t[12 + i]);
    dst[i * stride] = (unsigned char)v8_clip255(pred[4 * i] + ((a + d) >> 3));
    dst[i * stride + 1] = (unsigned char)v8_clip255(pred[4 * i + 1] + ((b + cc) >> 3));
    dst[i * stride + 2] = (unsigned char)v8_clip255(pred[4 * i + 2] + ((b - cc) >> 3));
    dst[i * stride + 3] = (unsigned char)v8_clip255(pred[4 * i + 3] + ((a - d) >> 3));
  }
}
V8_HD void v8_iwht(const int* c, int* dc) {                        // the format's inverse Walsh-Hadamard transform -> the 16 blocks' DC terms
  int t[16];
  for (int i = 0; i < 4; ++i) {
    const int a0 = c[i] + c[12 + i], a1 = c[4 + i] + c[8 + i], a2 = c[4 + i] - c[8 + i], a3 = c[i] - c[12 + i];
    t[i] = a0 + a1, t[8 + i] = a0 - a1, t[4 + i] = a3 + a2, t[12 + i] = a3 - a2;
  }
  for (int i = 0; i < 4; ++i) {
    const int d0 = t[4 * i] + 3, a0 = d0 + t[4 * i + 3], a1 = t[4 * i + 1] + t[4 * i + 2], a2 = t[4 * i + 1] - t[4 * i + 2], a3 = d0 - t[4 * i + 3];
    dc[4 * i] = (a0 + a1) >> 3, dc[4 * i + 1] = (a3 + a2) >> 3, dc[4 * i + 2] = (a0 - a1) >> 3, dc[4 * i + 3] = (a3 - a2) >> 3;
  }
}

// ---- prediction: the format's edges -----------------------------------------------------------------------------------------------------------------
// The row above, the column to the left and the corner of the n x n block of macroblock (mby, mbx) in a reconstructed plane: a missing row reads
// 127, a missing column 129, the corner 127 on the first macroblock row and 129 at mbx = 0 below it; dc = the DC prediction from the sides that exist.
struct V8Edge {
  int top[16], left[16], tl, dc;
};
V8_HD void v8_edges(const unsigned char* rec, long stride, int mby, int mbx, int n, V8Edge* e) {
  const unsigned char* p = rec + (long)mby * n * stride + (long)mbx * n;
  int st = 0, sl = 0;
  for (int i = 0; i < n; ++i) {
    e->top[i] = mby ? p[i - stride] : 127;
    e->left[i] = mbx ? p[i * stride - 1] : 129;
    st += e->top[i], sl += e->left[i];
  }
  e->tl = mby && mbx ? p[-stride - 1] : mby ? 129 : 127;
  const int shift = n == 8 ? 3 : 4;
  e->dc = mby && mbx ? (st + sl + n) >> (shift + 1) : mby ? (2 * st + n) >> (shift + 1) : mbx ? (2 * sl + n) >> (shift + 1) : 128;
}
V8_HD int v8_predict(const V8Edge* e, int mode, int y, int x) {   // modes: 0 DC, 1 V, 2 H, 3 TM
  return mode == 0 ? e->dc : mode == 1 ? e->top[x] : mode == 2 ? e->left[y] : v8_clip255(e->left[y] + e->top[x] - e->tl);
}

// One block: differences against the prediction, forward transform, quantisation (dcq for entry 0, acq for the rest) -> coefficients' levels in raster
// order in lv.
V8_HD void v8_block_levels(const unsigned char* src, long stride, const V8Edge* e, int mode, int y0, int x0, int dcq, int acq, int* coef, int* lv) {
  int d[16];
  for (int k = 0; k < 16; ++k) d[k] = (int)src[(k >> 2) * stride + (k & 3)] - v8_predict(e, mode, y0 + (k >> 2), x0 + (k & 3));
  v8_fdct(d, coef);
  lv[0] = v8_quantise(coef[0], dcq, 4);
  for (int k = 1; k < 16; ++k) lv[k] = v8_quantise(coef[k], acq, 3);
}
V8_HD void v8_block_recon(const V8Edge* e, int mode, int y0, int x0, const int* deq, unsigned char* dst, long stride) {
  int pred[16];
  for (int k = 0; k < 16; ++k) pred[k] = v8_predict(e, mode, y0 + (k >> 2), x0 + (k & 3));
  v8_idct_add(deq, pred, dst, stride);
}

// One macroblock: mode choice (sum of squared error of the prediction against the source, ties to the lower mode), levels, reconstruction.  Its left,
// top and top-left neighbours must be reconstructed already.  Y / ry: source and reconstructed luma of stride ys; U, V / ru, rv: chroma of stride cs.
// levels: this macroblock's V8_MB_LEVELS int16.  modes: its two bytes (luma, chroma).  Returns the non-zero mask.
V8_HD unsigned v8_encode_mb(const unsigned char* Y, const unsigned char* U, const unsigned char* V, unsigned char* ry, unsigned char* ru,
                            unsigned char* rv, long ys, long cs, int mby, int mbx, const V8Quant& m, short* levels, unsigned char* modes) {
  unsigned nz = 0;
  V8Edge e;
  int coef[16], lv[16], deq[16], dc[16];
  // luma
  v8_edges(ry, ys, mby, mbx, 16, &e);
  const unsigned char* sy = Y + (long)mby * 16 * ys + (long)mbx * 16;
  unsigned char* dy = ry + (long)mby * 16 * ys + (long)mbx * 16;
  long long best = -1;
  int ymode = 0;
  for (int mode = 0; mode < 4; ++mode) {
    long long sse = 0;
    for (int k = 0; k < 256; ++k) {
      const int d = (int)sy[(k >> 4) * ys + (k & 15)] - v8_predict(&e, mode, k >> 4, k & 15);
      sse += d * d;
    }
    if (best < 0 || sse < best) best = sse, ymode = mode;
  }
  for (int b = 0; b < 16; ++b) {
    const int y0 = (b >> 2) * 4, x0 = (b & 3) * 4;
    v8_block_levels(sy + y0 * ys + x0, ys, &e, ymode, y0, x0, m.yac, m.yac, coef, lv);
    dc[b] = coef[0];
    levels[16 * b] = 0;
    bool any = false;
    for (int n = 1; n < 16; ++n) {
      const int l = lv[v8_zigzag(n)];
      levels[16 * b + n] = (short)l;
      any |= l != 0;
    }
    if (any) nz |= 1u << b;
  }
  v8_fwht(dc, coef);
  lv[0] = v8_quantise(coef[0], m.y2dc, 4);
  for (int k = 1; k < 16; ++k) lv[k] = v8_quantise(coef[k], m.y2ac, 3);
  bool any = false;
  for (int n = 0; n < 16; ++n) {
    const int l = lv[v8_zigzag(n)];
    levels[16 * 24 + n] = (short)l;
    any |= l != 0;
  }
  if (any) nz |= 1u << 24;
  deq[0] = lv[0] * m.y2dc;
  for (int k = 1; k < 16; ++k) deq[k] = lv[k] * m.y2ac;
  v8_iwht(deq, dc);
  for (int b = 0; b < 16; ++b) {
    const int y0 = (b >> 2) * 4, x0 = (b & 3) * 4;
    deq[0] = dc[b];
    for (int n = 1; n < 16; ++n) deq[v8_zigzag(n)] = levels[16 * b + n] * m.yac;
    v8_block_recon(&e, ymode, y0, x0, deq, dy + y0 * ys + x0, ys);
  }
  // chroma: one mode for U and V
  V8Edge eu, ev;
  v8_edges(ru, cs, mby, mbx, 8, &eu);
  v8_edges(rv, cs, mby, mbx, 8, &ev);
  const long co = (long)mby * 8 * cs + (long)mbx * 8;
  best = -1;
  int uvmode = 0;
  for (int mode = 0; mode < 4; ++mode) {
    long long sse = 0;
    for (int k = 0; k < 64; ++k) {
      const int du = (int)U[co + (k >> 3) * cs + (k & 7)] - v8_predict(&eu, mode, k >> 3, k & 7);
      const int dv = (int)V[co + (k >> 3) * cs + (k & 7)] - v8_predict(&ev, mode, k >> 3, k & 7);
      sse += du * du + dv * dv;
    }
    if (best < 0 || sse < best) best = sse, uvmode = mode;
  }
  for (int b = 0; b < 8; ++b) {
    const V8Edge* ee = b < 4 ? &eu : &ev;
    const int y0 = ((b & 3) >> 1) * 4, x0 = (b & 1) * 4;
    v8_block_levels((b < 4 ? U : V) + co + y0 * cs + x0, cs, ee, uvmode, y0, x0, m.uvdc, m.uvac, coef, lv);
    bool anyc = false;
    for (int n = 0; n < 16; ++n) {
      const int l = lv[v8_zigzag(n)];
      levels[16 * (16 + b) + n] = (short)l;
      anyc |= l != 0;
    }
    if (anyc) nz |= 1u << (16 + b);
    deq[0] = lv[0] * m.uvdc;
    for (int k = 1; k < 16; ++k) deq[k] = lv[k] * m.uvac;
    v8_block_recon(ee, uvmode, y0, x0, deq, (b < 4 ? ru : rv) + co + y0 * cs + x0, cs);
  }
  modes[0] = (unsigned char)ymode, modes[1] = (unsigned char)uvmode;
  return nz;
}

// ---- the boolean coder (RFC 6386 section 7) ---------------------------------------------------------------------------------------------------------
// Writes into buf[0 .. cap): a byte past the end is counted, not stored, and v8_bool_finish then reports the slot as too small.
struct V8Bool {
  unsigned char* buf;
  long long cap, pos;
  uint32_t range, bottom;
  int count;
};
V8_HD void v8_bool_init(V8Bool* e, unsigned char* buf, long long cap) {
  e->buf = buf, e->cap = cap < 0 ? 0 : cap, e->pos = 0, e->range = 255, e->bottom = 0, e->count = 24;
}
V8_HD int v8_put(V8Bool* e, int bit, int prob) {
  const uint32_t split = 1 + (((e->range - 1) * (uint32_t)prob) >> 8);
  if (bit) {
    e->bottom += split;
    e->range -= split;
  } else {
    e->range = split;
  }
  while (e->range < 128) {                                         // seven shifts at most
    e->range <<= 1;
    if (e->bottom & 0x80000000u) {                                 // a carry: back over the bytes already written, at most pos of them
      for (long long k = (e->pos < e->cap ? e->pos : e->cap) - 1; k >= 0; --k) {
        if (e->buf[k] == 255) {
          e->buf[k] = 0;
        } else {
          ++e->buf[k];
          break;
        }
      }
    }
    e->bottom <<= 1;
    if (!--e->count) {
      if (e->pos < e->cap) e->buf[e->pos] = (unsigned char)(e->bottom >> 24);
      ++e->pos;
      e->bottom &= 0xffffffu;
      e->count = 8;
    }
  }
  return bit;
}
V8_HD void v8_put_bits(V8Bool* e, int value, int n) {              // an n-bit literal, the most significant bit first
  for (int k = n - 1; k >= 0; --k) v8_put(e, value >> k & 1, 128);
}
// 32 closing symbols push every pending bit out; returns the bytes written, or -1 when the slot was too small
V8_HD long long v8_bool_finish(V8Bool* e) {
  for (int k = 0; k < 32; ++k) v8_put(e, 0, 128);
  return e->pos <= e->cap ? e->pos : -1;
}

// One block's 16 levels (scan order) from position first on, as tokens of the given type (0 luma after Y2, 1 Y2, 2 chroma) and context.  probs: the
// 1056 entries of v8_coef_table.
V8_HD void v8_put_coeffs(V8Bool* bw, const unsigned char* probs, int type, int ctx, const short* lv, int first) {
  int last = -1;
  for (int n = first; n < 16; ++n)
    if (lv[n]) last = n;
  int n = first, band = v8_band(n), c = ctx;
#define V8_P(node) probs[(((type & 3) * 8 + band) * 3 + c) * 11 + (node)]
  if (!v8_put(bw, last >= 0, V8_P(0))) return;
  while (n < 16) {
    const int l = lv[n++];
    int v = l < 0 ? -l : l;
    if (v > V8_MAX_LEVEL) v = V8_MAX_LEVEL;
    if (!v8_put(bw, v != 0, V8_P(1))) {
      band = v8_band(n), c = 0;
      continue;
    }
    if (!v8_put(bw, v > 1, V8_P(2))) {
      band = v8_band(n), c = 1;
    } else {
      if (!v8_put(bw, v > 4, V8_P(3))) {
        if (v8_put(bw, v != 2, V8_P(4))) v8_put(bw, v == 4, V8_P(5));
      } else if (!v8_put(bw, v > 10, V8_P(6))) {
        if (!v8_put(bw, v > 6, V8_P(7))) {
          v8_put(bw, v == 6, 159);
        } else {
          v8_put(bw, v >= 9, 165);
          v8_put(bw, !(v & 1), 145);
        }
      } else {
        int cat, bits, extra;
        if (v < 19) cat = 3, bits = 3, extra = v - 11;
        else if (v < 35) cat = 4, bits = 4, extra = v - 19;
        else if (v < 67) cat = 5, bits = 5, extra = v - 35;
        else cat = 6, bits = 11, extra = v - 67;
        v8_put(bw, cat >= 5, V8_P(8));
        v8_put(bw, cat & 1 ? 0 : 1, V8_P(cat >= 5 ? 10 : 9));
        for (int k = 0; k < bits; ++k) v8_put(bw, extra >> (bits - 1 - k) & 1, v8_cat_prob(cat, k));
      }
      band = v8_band(n), c = 2;
    }
    v8_put(bw, l < 0, 128);
    if (n == 16 || !v8_put(bw, n <= last, V8_P(0))) return;
  }
#undef V8_P
}

V8_HD int v8_skip_prob(long long mbs, long long skipped) {         // P(not skipped) of 256 from the frame's own count, kept inside 1 .. 255
  const long long p = (mbs - skipped) * 255 / mbs;
  return (int)(p < 1 ? 1 : p > 255 ? 255 : p);
}

// The first partition: the frame header's fields, then every macroblock's skip flag and modes.  nz: mbh * mbw masks, modes: two bytes a macroblock.
V8_HD long long v8_code_first(const unsigned* nz, const unsigned char* modes, int mbh, int mbw, int q, int log2_parts, int filter_level,
                              long long skipped, unsigned char* buf, long long cap) {
  V8Bool bw;
  v8_bool_init(&bw, buf, cap);
  v8_put_bits(&bw, 0, 2);                                          // colour space, clamping type
  v8_put_bits(&bw, 0, 1);                                          // no segments
  v8_put_bits(&bw, 0, 1);                                          // the normal loop filter
  v8_put_bits(&bw, filter_level, 6);
  v8_put_bits(&bw, 0, 3);                                          // sharpness
  v8_put_bits(&bw, 0, 1);                                          // no filter deltas
  v8_put_bits(&bw, log2_parts, 2);
  v8_put_bits(&bw, q, 7);
  v8_put_bits(&bw, 0, 5);                                          // no quantiser deltas
  v8_put_bits(&bw, 0, 1);                                          // refresh_entropy_probs
  for (int i = 0; i < 1056; ++i) v8_put(&bw, 0, v8_update_prob(i));
  const long long mbs = (long long)mbh * mbw;
  const int prob = v8_skip_prob(mbs, skipped);
  v8_put_bits(&bw, 1, 1);                                          // mb_no_coeff_skip
  v8_put_bits(&bw, prob, 8);
  for (long long k = 0; k < mbs; ++k) {
    v8_put(&bw, nz[k] == 0, prob);
    const int ym = modes[2 * k], uvm = modes[2 * k + 1];
    v8_put(&bw, 1, 145);                                           // a 16 x 16 mode
    if (v8_put(&bw, ym >= 2, 156)) v8_put(&bw, ym == 3, 128);
    else v8_put(&bw, ym == 1, 163);
    if (v8_put(&bw, uvm != 0, 142))
      if (v8_put(&bw, uvm != 1, 114)) v8_put(&bw, uvm != 2, 183);
  }
  return v8_bool_finish(&bw);
}

// Token partition `part` of `parts`: macroblock rows part, part + parts, ...  A block's context is the number of its top and left neighbours with a
// non-zero level, read from the masks; a macroblock outside the frame counts as zero.
V8_HD long long v8_code_tokens(const short* levels, const unsigned* nz, const unsigned char* probs, int mbh, int mbw, int part, int parts,
                               unsigned char* buf, long long cap) {
  V8Bool bw;
  v8_bool_init(&bw, buf, cap);
  for (int my = part; my < mbh; my += parts)
    for (int mx = 0; mx < mbw; ++mx) {
      const long long k = (long long)my * mbw + mx;
      const unsigned me = nz[k];
      if (!me) continue;
      const unsigned up = my ? nz[k - mbw] : 0u, lf = mx ? nz[k - 1] : 0u;
      const short* lv = levels + k * V8_MB_LEVELS;
      v8_put_coeffs(&bw, probs, 1, (int)(up >> 24 & 1u) + (int)(lf >> 24 & 1u), lv + 16 * 24, 0);
      for (int b = 0; b < 16; ++b) {
        const unsigned t = b >= 4 ? me >> (b - 4) : up >> (b + 12), l = b & 3 ? me >> (b - 1) : lf >> (b + 3);
        v8_put_coeffs(&bw, probs, 0, (int)(t & 1u) + (int)(l & 1u), lv + 16 * b, 1);
      }
      for (int b = 16; b < 24; ++b) {
        const unsigned t = b & 2 ? me >> (b - 2) : up >> (b + 2), l = b & 1 ? me >> (b - 1) : lf >> (b + 1);
        v8_put_coeffs(&bw, probs, 2, (int)(t & 1u) + (int)(l & 1u), lv + 16 * b, 0);
      }
    }
  return v8_bool_finish(&bw);
}
