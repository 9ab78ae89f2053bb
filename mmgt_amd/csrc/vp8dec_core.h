// Lossy WebP input: VP8 key frames decoded as libwebp decodes them, the per-symbol, per-block and per-edge arithmetic written once.
// csrc/vp8dec.hip calls these functions from its kernels and tools/vp8dec_host_check.cpp from a host program, so a frame can be run through them
// without a GPU.  What csrc/vp8_core.h already holds (inverse transforms, quantiser tables, 16 x 16 and chroma edges, coefficient tables, trees) is
// used from there; this file adds the half of the format our writer never emits: the boolean decoder, segments, quantiser deltas, probability
// updates, the ten 4 x 4 modes with their contexts, token decoding, both loop filters, and libwebp's fancy upsampling and YUV -> RGB conversion.
//
// A frame's scratch (uint32 words at its table row's V8D_SCR, v8d_frame_words(W, H) of them): 64 header words; one V8dMb (32 bytes) per
// macroblock; 384 int16 dequantised coefficients per macroblock in raster order within each block (blocks 0 .. 15 luma, 16 .. 19 U, 20 .. 23 V);
// the Y, U and V planes padded to whole macroblocks.  Nothing here reads outside a frame's payload or writes outside its scratch and ARGB ranges:
// every address comes from the table row's sizes, never from the stream.
#pragma once
#include "vp8_core.h"

enum {
  V8D_OK = 0,
  V8D_ST_DESCRIPTOR = 1,   // the table row names bytes or words outside the buffers, or sizes outside 1 .. 16383: nothing was touched
  V8D_ST_FRAME = 2,        // the 10-byte frame header: not a shown key frame of profile 0 .. 3, a bad start code, or a size other than the row's
  V8D_ST_FIRST_SIZE = 3,   // the first partition's size runs past the payload
  V8D_ST_PARTITIONS = 4,   // the partition-size table runs past the payload, or the last partition is empty
  V8D_ST_FIRST_END = 5,    // the first partition ended inside the header or the macroblock modes
  V8D_ST_TOKEN_END = 6,    // a token partition ended inside its macroblocks
  V8D_ST_UPSTREAM = 7,     // reconstruct / filter / output: the parse left no valid header block
  V8D_ST_LAST = 7
};
enum {
  V8D_TAB = 8,             // long long words per frame row
  V8D_HDR = 64,            // header words at the start of a frame's scratch
  V8D_MAGIC = 0x56384431,
  V8D_MB_BYTES = 32 + 384 * 2 + 384
};
enum { V8D_BEGIN, V8D_END, V8D_SCR, V8D_CAP, V8D_PIX, V8D_W, V8D_H };
// header words
enum { V8D_H_MAGIC, V8D_H_MBW, V8D_H_MBH, V8D_H_FILTER, V8D_H_PARTS, V8D_H_SKIP, V8D_H_SEGMENTS, V8D_H_MAP, V8D_H_QUANT = 8, V8D_H_FS = 32 };
// the format's mode numbers (a 16 x 16 or chroma mode is DC, TM, V or H under the same numbers)
enum { V8D_DC, V8D_TM, V8D_VE, V8D_HE, V8D_RD, V8D_VR, V8D_LD, V8D_VL, V8D_HD, V8D_HU };

struct V8dMb {
  unsigned char imodes[16];                      // the sub-block modes; a 16 x 16 macroblock holds its mode sixteen times (its neighbours' contexts)
  unsigned char uvmode, i4x4, segment, skip;     // skip: the stream's flag (0 without mb_no_coeff_skip)
  uint32_t nzy, nzuv;                            // libwebp's two-bit codes per block
  unsigned char tnz, tdc, inner, pad;            // the non-zero context this macroblock leaves for the one below; inner edges are filtered
};
static_assert(sizeof(V8dMb) == 32, "a macroblock's record is 32 bytes");

V8_HD long long v8d_frame_words(int W, int H) {
  const long long mbs = (long long)((W + 15) >> 4) * ((H + 15) >> 4);
  return V8D_HDR + mbs * V8D_MB_BYTES / 4;
}

struct V8dFrame {
  int W, H, mbw, mbh;
  long long mbs, begin, end, pix;
  uint32_t* hdr;
  V8dMb* mb;
  short* coef;
  unsigned char *Y, *U, *V;
  long ys, cs;
};
// The row checked against the buffers; every later address derives from what is checked here.
V8_HD int v8d_frame(const long long* t, uint32_t* scratch, long long scratch_words, long long data_bytes, long long argb_words, V8dFrame* f) {
  const long long W = t[V8D_W], H = t[V8D_H];
  if (W < 1 || H < 1 || W > V8_MAX_SIDE || H > V8_MAX_SIDE) return V8D_ST_DESCRIPTOR;
  const long long need = v8d_frame_words((int)W, (int)H);
  if (t[V8D_BEGIN] < 0 || t[V8D_END] < t[V8D_BEGIN] || t[V8D_END] > data_bytes) return V8D_ST_DESCRIPTOR;
  if (t[V8D_SCR] < 0 || (t[V8D_SCR] & 3) || t[V8D_CAP] < need || t[V8D_SCR] > scratch_words || t[V8D_CAP] > scratch_words - t[V8D_SCR]) return V8D_ST_DESCRIPTOR;
  if (t[V8D_PIX] < 0 || t[V8D_PIX] > argb_words || W * H > argb_words - t[V8D_PIX]) return V8D_ST_DESCRIPTOR;
  f->W = (int)W, f->H = (int)H, f->mbw = (int)((W + 15) >> 4), f->mbh = (int)((H + 15) >> 4);
  f->mbs = (long long)f->mbw * f->mbh, f->begin = t[V8D_BEGIN], f->end = t[V8D_END], f->pix = t[V8D_PIX];
  f->hdr = scratch + t[V8D_SCR];
  f->mb = reinterpret_cast<V8dMb*>(f->hdr + V8D_HDR);
  f->coef = reinterpret_cast<short*>(f->mb + f->mbs);
  f->Y = reinterpret_cast<unsigned char*>(f->coef + f->mbs * 384);
  f->U = f->Y + f->mbs * 256, f->V = f->U + f->mbs * 64;
  f->ys = 16l * f->mbw, f->cs = 8l * f->mbw;
  return V8D_OK;
}

// ---- the boolean decoder, as libwebp reads: a byte at a time, zeros past the end, and a flag from the first byte that is not there ------------------
struct V8dBool {
  const unsigned char* buf;
  long long pos, end;
  uint32_t value, range;                         // range is kept minus one
  int bits, eof;
};
V8_HD void v8d_load(V8dBool* b) {
  if (b->pos < b->end) {
    b->bits += 8;
    b->value = (uint32_t)b->buf[b->pos++] | (b->value << 8);
  } else if (!b->eof) {
    b->value <<= 8;
    b->bits += 8;
    b->eof = 1;
  } else {
    b->bits = 0;
  }
}
V8_HD void v8d_bool_init(V8dBool* b, const unsigned char* buf, long long begin, long long end) {
  b->buf = buf, b->pos = begin, b->end = end < begin ? begin : end, b->value = 0, b->range = 254, b->bits = -8, b->eof = 0;
  v8d_load(b);
}
V8_HD int v8d_get(V8dBool* b, int prob) {
  uint32_t range = b->range;
  if (b->bits < 0) v8d_load(b);
  const int pos = b->bits;
  const uint32_t split = (range * (uint32_t)prob) >> 8, value = b->value >> pos;
  const int bit = value > split;
  if (bit) {
    range -= split;
    b->value -= (split + 1) << pos;
  } else {
    range = split + 1;
  }
  int shift = 0;                                 // 7 - floor(log2(range)), range 1 .. 255
  while (shift < 7 && (range << shift) < 128u) ++shift;
  range <<= shift;
  b->bits -= shift;
  b->range = range - 1;
  return bit;
}
V8_HD int v8d_value(V8dBool* b, int n) {
  int v = 0;
  while (n-- > 0) v |= v8d_get(b, 128) << n;
  return v;
}
V8_HD int v8d_signed(V8dBool* b, int n) {
  const int v = v8d_value(b, n);
  return v8d_get(b, 128) ? -v : v;
}
V8_HD int v8d_opt_signed(V8dBool* b, int n) { return v8d_get(b, 128) ? v8d_signed(b, n) : 0; }

// ---- tables -----------------------------------------------------------------------------------------------------------------------------------------
// sub-block mode probabilities [top mode 10][left mode 10][node 9]
V8_HD int v8d_bmode_prob(int top, int left, int node) {
  constexpr unsigned char t[900] = {
      231,120,48,89,115,113,120,152,112,152,179,64,126,170,118,46,70,95,175,69,143,80,85,82,72,155,103,56,58,10,171,218,189,17,13,152,114,26,17,163,44,195,21,10,173,
      121,24,80,195,26,62,44,64,85,144,71,10,38,171,213,144,34,26,170,46,55,19,136,160,33,206,71,63,20,8,114,114,208,12,9,226,81,40,11,96,182,84,29,16,36,
      134,183,89,137,98,101,106,165,148,72,187,100,130,157,111,32,75,80,66,102,167,99,74,62,40,234,128,41,53,9,178,241,141,26,8,107,74,43,26,146,73,166,49,23,157,
      65,38,105,160,51,52,31,115,128,104,79,12,27,217,255,87,17,7,87,68,71,44,114,51,15,186,23,47,41,14,110,182,183,21,17,194,66,45,25,102,197,189,23,18,22,
      88,88,147,150,42,46,45,196,205,43,97,183,117,85,38,35,179,61,39,53,200,87,26,21,43,232,171,56,34,51,104,114,102,29,93,77,39,28,85,171,58,165,90,98,64,
      34,22,116,206,23,34,43,166,73,107,54,32,26,51,1,81,43,31,68,25,106,22,64,171,36,225,114,34,19,21,102,132,188,16,76,124,62,18,78,95,85,57,50,48,51,
      193,101,35,159,215,111,89,46,111,60,148,31,172,219,228,21,18,111,112,113,77,85,179,255,38,120,114,40,42,1,196,245,209,10,25,109,88,43,29,140,166,213,37,43,154,
      61,63,30,155,67,45,68,1,209,100,80,8,43,154,1,51,26,71,142,78,78,16,255,128,34,197,171,41,40,5,102,211,183,4,1,221,51,50,17,168,209,192,23,25,82,
      138,31,36,171,27,166,38,44,229,67,87,58,169,82,115,26,59,179,63,59,90,180,59,166,93,73,154,40,40,21,116,143,209,34,39,175,47,15,16,183,34,223,49,45,183,
      46,17,33,183,6,98,15,32,183,57,46,22,24,128,1,54,17,37,65,32,73,115,28,128,23,128,205,40,3,9,115,51,192,18,6,223,87,37,9,115,59,77,64,21,47,
      104,55,44,218,9,54,53,130,226,64,90,70,205,40,41,23,26,57,54,57,112,184,5,41,38,166,213,30,34,26,133,152,116,10,32,134,39,19,53,221,26,114,32,73,255,
      31,9,65,234,2,15,1,118,73,75,32,12,51,192,255,160,43,51,88,31,35,67,102,85,55,186,85,56,21,23,111,59,205,45,37,192,55,38,70,124,73,102,1,34,98,
      125,98,42,88,104,85,117,175,82,95,84,53,89,128,100,113,101,45,75,79,123,47,51,128,81,171,1,57,17,5,71,102,57,53,41,49,38,33,13,121,57,73,26,1,85,
      41,10,67,138,77,110,90,47,114,115,21,2,10,102,255,166,23,6,101,29,16,10,85,128,101,196,26,57,18,10,102,102,213,34,20,43,117,20,15,36,163,128,68,1,26,
      102,61,71,37,34,53,31,243,192,69,60,71,38,73,119,28,222,37,68,45,128,34,1,47,11,245,171,62,17,19,70,146,85,55,62,70,37,43,37,154,100,163,85,160,1,
      63,9,92,136,28,64,32,201,85,75,15,9,9,64,255,184,119,16,86,6,28,5,64,255,25,248,1,56,8,17,132,137,255,55,116,128,58,15,20,82,135,57,26,121,40,
      164,50,31,137,154,133,25,35,218,51,103,44,131,131,123,31,6,158,86,40,64,135,148,224,45,183,128,22,26,17,131,240,154,14,1,209,45,16,21,91,64,222,7,1,197,
      56,21,39,155,60,138,23,102,213,83,12,13,54,192,255,68,47,28,85,26,85,85,128,128,32,146,171,18,11,7,63,144,171,4,4,246,35,27,10,146,174,171,12,26,128,
      190,80,35,99,180,80,126,54,45,85,126,47,87,176,51,41,20,32,101,75,128,139,118,146,116,128,85,56,41,15,176,236,85,37,9,62,71,30,17,119,118,255,17,18,138,
      101,38,60,138,55,70,43,26,142,146,36,19,30,171,255,97,27,20,138,45,61,62,219,1,81,188,64,32,41,20,117,151,142,20,21,163,112,19,12,61,195,128,48,4,24};
  return t[((top < 0 || top > 9 ? 0 : top) * 10 + (left < 0 || left > 9 ? 0 : left)) * 9 + (node < 0 ? 0 : node > 8 ? 8 : node)];
}
V8_HD int v8d_bmode_tree(int i) {
  constexpr signed char t[18] = {-V8D_DC, 1, -V8D_TM, 2, -V8D_VE, 3, 4, 6, -V8D_HE, 5, -V8D_RD, -V8D_VR, -V8D_LD, 7, -V8D_VL, 8, -V8D_HD, -V8D_HU};
  return t[i < 0 ? 0 : i > 17 ? 17 : i];
}

// ---- the first partition's header -------------------------------------------------------------------------------------------------------------------
struct V8dHdr {
  int filter_type, simple, level, sharpness, parts, use_segment, update_map, use_skip, skip_p, updates;
  int seg_prob[3];
  int quant[4][6];                               // per segment: y dc, y ac, y2 dc, y2 ac, uv dc, uv ac
  int fs[4][2][3];                               // per segment and is-4x4: limit (0: no filtering), interior level, hev threshold
};
V8_HD int v8d_clipq(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
// probs: the 1056 coefficient probabilities, holding the defaults on entry.
V8_HD void v8d_parse_header(V8dBool* br, V8dHdr* h, unsigned char* probs) {
  int quantizer[4] = {0, 0, 0, 0}, strength[4] = {0, 0, 0, 0}, absolute = 1;
  v8d_value(br, 2);                              // colour space and clamping type: libwebp reads and ignores both
  h->use_segment = v8d_get(br, 128), h->update_map = 0;
  h->seg_prob[0] = h->seg_prob[1] = h->seg_prob[2] = 255;
  if (h->use_segment) {
    h->update_map = v8d_get(br, 128);
    if (v8d_get(br, 128)) {
      absolute = v8d_get(br, 128);
      for (int s = 0; s < 4; ++s) quantizer[s] = v8d_opt_signed(br, 7);
      for (int s = 0; s < 4; ++s) strength[s] = v8d_opt_signed(br, 6);
    }
    if (h->update_map)
      for (int s = 0; s < 3; ++s) h->seg_prob[s] = v8d_get(br, 128) ? v8d_value(br, 8) : 255;
  }
  h->simple = v8d_get(br, 128), h->level = v8d_value(br, 6), h->sharpness = v8d_value(br, 3);
  int ref0 = 0, mode0 = 0;
  const int use_lf_delta = v8d_get(br, 128);
  if (use_lf_delta && v8d_get(br, 128)) {
    for (int i = 0; i < 4; ++i)
      if (v8d_get(br, 128)) {
        const int v = v8d_signed(br, 6);
        if (i == 0) ref0 = v;
      }
    for (int i = 0; i < 4; ++i)
      if (v8d_get(br, 128)) {
        const int v = v8d_signed(br, 6);
        if (i == 0) mode0 = v;
      }
  }
  h->filter_type = h->level == 0 ? 0 : h->simple ? 1 : 2;
  h->parts = 1 << v8d_value(br, 2);
  const int base = v8d_value(br, 7);
  const int dy1dc = v8d_opt_signed(br, 4), dy2dc = v8d_opt_signed(br, 4), dy2ac = v8d_opt_signed(br, 4), duvdc = v8d_opt_signed(br, 4),
            duvac = v8d_opt_signed(br, 4);
  for (int s = 0; s < 4; ++s) {
    int q = base;
    if (h->use_segment) q = quantizer[s] + (absolute ? 0 : base);
    int* m = h->quant[s];
    m[0] = v8_dc_q(v8d_clipq(q + dy1dc, 127)), m[1] = v8_ac_q(v8d_clipq(q, 127));
    m[2] = v8_dc_q(v8d_clipq(q + dy2dc, 127)) * 2, m[3] = v8_ac_q(v8d_clipq(q + dy2ac, 127)) * 101581 >> 16;
    if (m[3] < 8) m[3] = 8;
    m[4] = v8_dc_q(v8d_clipq(q + duvdc, 117)), m[5] = v8_ac_q(v8d_clipq(q + duvac, 127));
    int lvl0 = h->level;
    if (h->use_segment) lvl0 = strength[s] + (absolute ? 0 : h->level);
    for (int i4 = 0; i4 < 2; ++i4) {
      int level = lvl0;
      if (use_lf_delta) level += ref0 + (i4 ? mode0 : 0);
      level = level < 0 ? 0 : level > 63 ? 63 : level;
      int* fs = h->fs[s][i4];
      fs[0] = fs[1] = fs[2] = 0;
      if (level > 0) {
        int il = level;
        if (h->sharpness > 0) {
          il >>= h->sharpness > 4 ? 2 : 1;
          if (il > 9 - h->sharpness) il = 9 - h->sharpness;
        }
        if (il < 1) il = 1;
        fs[0] = 2 * level + il, fs[1] = il, fs[2] = level >= 40 ? 2 : level >= 15 ? 1 : 0;
      }
    }
  }
  v8d_get(br, 128);                              // refresh_entropy_probs: read and ignored for a key frame
  h->updates = 0;
  for (int i = 0; i < 1056; ++i)
    if (v8d_get(br, v8_update_prob(i))) probs[i] = (unsigned char)v8d_value(br, 8), ++h->updates;
  h->use_skip = v8d_get(br, 128);
  h->skip_p = h->use_skip ? v8d_value(br, 8) : 0;
}

// The 10-byte frame header and the partition ranges of payload data[begin, end): part[0 .. 2 * parts) = begin and end of each token partition, as
// libwebp lays them out (a size past the data is cut to what is left; the last partition takes the rest and must hold a byte).
V8_HD int v8d_frame_tag(const unsigned char* data, long long begin, long long end, int W, int H, long long* first_end) {
  if (end - begin < 10) return V8D_ST_FRAME;
  const unsigned char* p = data + begin;
  const uint32_t tag = p[0] | p[1] << 8 | (uint32_t)p[2] << 16;
  if ((tag & 1) || (tag >> 1 & 7) > 3 || !(tag >> 4 & 1) || p[3] != 0x9d || p[4] != 0x01 || p[5] != 0x2a) return V8D_ST_FRAME;
  if (((p[6] | p[7] << 8) & 0x3fff) != W || ((p[8] | p[9] << 8) & 0x3fff) != H) return V8D_ST_FRAME;
  if ((long long)(tag >> 5) > end - begin - 10) return V8D_ST_FIRST_SIZE;
  *first_end = begin + 10 + (tag >> 5);
  return V8D_OK;
}
V8_HD int v8d_partitions(const unsigned char* data, long long first_end, long long end, int parts, long long* part) {
  const int last = parts - 1;
  if (end - first_end < 3 * last) return V8D_ST_PARTITIONS;
  long long start = first_end + 3 * last, left = end - start;
  for (int p = 0; p < last; ++p) {
    const unsigned char* sz = data + first_end + 3 * p;
    long long size = sz[0] | sz[1] << 8 | (long long)sz[2] << 16;
    if (size > left) size = left;
    part[2 * p] = start, part[2 * p + 1] = start + size;
    start += size, left -= size;
  }
  part[2 * last] = start, part[2 * last + 1] = end;
  return start < end ? V8D_OK : V8D_ST_PARTITIONS;
}

// ---- a macroblock's segment, skip flag and modes (first partition) ----------------------------------------------------------------------------------
V8_HD void v8d_modes_mb(V8dBool* br, const V8dHdr* h, V8dMb* mb, const V8dMb* up, const V8dMb* lf) {
  mb->segment = 0;
  if (h->update_map)
    mb->segment = (unsigned char)(!v8d_get(br, h->seg_prob[0]) ? v8d_get(br, h->seg_prob[1]) : v8d_get(br, h->seg_prob[2]) + 2);
  mb->skip = h->use_skip ? (unsigned char)v8d_get(br, h->skip_p) : 0;
  mb->i4x4 = (unsigned char)!v8d_get(br, 145);
  if (!mb->i4x4) {
    const int m = v8d_get(br, 156) ? (v8d_get(br, 128) ? V8D_TM : V8D_HE) : (v8d_get(br, 163) ? V8D_VE : V8D_DC);
    for (int i = 0; i < 16; ++i) mb->imodes[i] = (unsigned char)m;
  } else {
    for (int y = 0; y < 4; ++y)
      for (int x = 0; x < 4; ++x) {
        const int top = y ? mb->imodes[4 * y - 4 + x] : up ? up->imodes[12 + x] : V8D_DC;
        const int left = x ? mb->imodes[4 * y + x - 1] : lf ? lf->imodes[4 * y + 3] : V8D_DC;
        int i = v8d_bmode_tree(v8d_get(br, v8d_bmode_prob(top, left, 0)));
        for (int k = 0; k < 9 && i > 0; ++k) i = v8d_bmode_tree(2 * i + v8d_get(br, v8d_bmode_prob(top, left, i)));   // the tree is five levels deep
        mb->imodes[4 * y + x] = (unsigned char)(i > 0 ? 0 : -i);
      }
  }
  mb->uvmode = (unsigned char)(!v8d_get(br, 142) ? V8D_DC : !v8d_get(br, 114) ? V8D_VE : v8d_get(br, 183) ? V8D_TM : V8D_HE);
  mb->nzy = mb->nzuv = 0, mb->tnz = mb->tdc = mb->inner = mb->pad = 0;
}

// ---- tokens -----------------------------------------------------------------------------------------------------------------------------------------
V8_HD int v8d_large(V8dBool* br, const unsigned char* p) {
  if (!v8d_get(br, p[3])) return !v8d_get(br, p[4]) ? 2 : 3 + v8d_get(br, p[5]);
  if (!v8d_get(br, p[6])) {
    if (!v8d_get(br, p[7])) return 5 + v8d_get(br, 159);
    const int v = 7 + 2 * v8d_get(br, 165);
    return v + v8d_get(br, 145);
  }
  const int bit1 = v8d_get(br, p[8]), bit0 = v8d_get(br, p[9 + bit1]), cat = 2 * bit1 + bit0, n = cat == 3 ? 11 : 3 + cat;
  int v = 0;
  for (int k = 0; k < n; ++k) v += v + v8d_get(br, v8_cat_prob(3 + cat, k));
  return v + 3 + (8 << cat);
}
// One block from position n on; out: its 16 coefficients in raster order, dequantised and cut to 16 bits as libwebp stores them.  Returns the
// position behind the last coded coefficient.
V8_HD int v8d_get_coeffs(V8dBool* br, const unsigned char* probs, int type, int ctx, int dcq, int acq, int n, short* out) {
  const unsigned char* tp = probs + (type & 3) * 264;
  const unsigned char* p = tp + (v8_band(n) * 3 + ctx) * 11;
  for (; n < 16; ++n) {
    if (!v8d_get(br, p[0])) return n;
    while (!v8d_get(br, p[1])) {
      p = tp + v8_band(++n) * 33;
      if (n == 16) return 16;
    }
    const unsigned char* pc = tp + v8_band(n + 1) * 33;
    int v;
    if (!v8d_get(br, p[2])) v = 1, p = pc + 11;
    else v = v8d_large(br, p), p = pc + 22;
    if (v8d_get(br, 128)) v = -v;
    out[v8_zigzag(n)] = (short)(v * (n > 0 ? acq : dcq));
  }
  return 16;
}
V8_HD uint32_t v8d_nz_code(uint32_t acc, int nz, int dc_nz) { return acc << 2 | (uint32_t)(nz > 3 ? 3 : nz > 1 ? 2 : dc_nz); }

// One macroblock's residuals.  up: the macroblock above (null on the first row); lnz, ldc: the left context, zero at the start of a row.
V8_HD void v8d_tokens_mb(V8dBool* br, const unsigned char* probs, const V8dHdr* h, V8dMb* mb, const V8dMb* up, unsigned* lnz_io, unsigned* ldc_io,
                         short* coef) {
  unsigned top = up ? up->tnz : 0u, tdc = up ? up->tdc : 0u, left = *lnz_io, ldc = *ldc_io;
  int none;
  if (h->use_skip && mb->skip) {
    top = left = 0;
    if (!mb->i4x4) tdc = ldc = 0;
    mb->nzy = mb->nzuv = 0;
    none = 1;
  } else {
    const int* q = h->quant[mb->segment & 3];
    for (int i = 0; i < 384; ++i) coef[i] = 0;
    short* dst = coef;
    int first, type;
    if (!mb->i4x4) {
      short dc[16];
      for (int i = 0; i < 16; ++i) dc[i] = 0;
      const int nz = v8d_get_coeffs(br, probs, 1, (int)(tdc + ldc), q[2], q[3], 0, dc);
      tdc = ldc = nz > 0;
      if (nz > 1) {
        int c[16], o[16];
        for (int i = 0; i < 16; ++i) c[i] = dc[i];
        v8_iwht(c, o);
        for (int i = 0; i < 16; ++i) dst[16 * i] = (short)o[i];
      } else {
        const int dc0 = (dc[0] + 3) >> 3;
        for (int i = 0; i < 16; ++i) dst[16 * i] = (short)dc0;
      }
      first = 1, type = 0;
    } else {
      first = 0, type = 3;
    }
    unsigned tnz = top & 15u, lnz = left & 15u;
    uint32_t nzy = 0, nzuv = 0;
    for (int y = 0; y < 4; ++y) {
      unsigned l = lnz & 1u;
      uint32_t codes = 0;
      for (int x = 0; x < 4; ++x) {
        const int nz = v8d_get_coeffs(br, probs, type, (int)(l + (tnz & 1u)), q[0], q[1], first, dst);
        l = nz > first;
        tnz = tnz >> 1 | l << 7;
        codes = v8d_nz_code(codes, nz, dst[0] != 0);
        dst += 16;
      }
      tnz >>= 4;
      lnz = lnz >> 1 | l << 7;
      nzy = nzy << 8 | codes;
    }
    unsigned out_t = tnz, out_l = lnz >> 4;
    for (int ch = 0; ch < 4; ch += 2) {
      uint32_t codes = 0;
      tnz = top >> (4 + ch), lnz = left >> (4 + ch);
      for (int y = 0; y < 2; ++y) {
        unsigned l = lnz & 1u;
        for (int x = 0; x < 2; ++x) {
          const int nz = v8d_get_coeffs(br, probs, 2, (int)(l + (tnz & 1u)), q[4], q[5], 0, dst);
          l = nz > 0;
          tnz = tnz >> 1 | l << 3;
          codes = v8d_nz_code(codes, nz, dst[0] != 0);
          dst += 16;
        }
        tnz >>= 2;
        lnz = lnz >> 1 | l << 5;
      }
      nzuv |= codes << (4 * ch);
      out_t |= (tnz << 4) << ch;
      out_l |= (lnz & 0xf0u) << ch;
    }
    top = out_t & 255u, left = out_l & 255u;
    mb->nzy = nzy, mb->nzuv = nzuv;
    none = !(nzy | nzuv);                        // the parsed result, not the flag, decides whether the inner edges are filtered
  }
  mb->tnz = (unsigned char)top, mb->tdc = (unsigned char)tdc;
  mb->inner = (unsigned char)(mb->i4x4 | !none);
  *lnz_io = left, *ldc_io = ldc;
}

// ---- reconstruction ---------------------------------------------------------------------------------------------------------------------------------
V8_HD int v8d_avg2(int a, int b) { return (a + b + 1) >> 1; }
V8_HD int v8d_avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
// One sub-block's prediction.  T[0] is the corner, T[1 .. 8] the eight pixels above and above-right, L[0 .. 3] the left column.
V8_HD void v8d_pred4(int mode, const int* T, const int* L, int* pred) {
  const int X = T[0], A = T[1], B = T[2], C = T[3], D = T[4], E = T[5], F = T[6], G = T[7], Hh = T[8], I = L[0], J = L[1], K = L[2], Ll = L[3];
#define V8D_P(x, y) pred[4 * (y) + (x)]
  switch (mode) {
    case V8D_TM:
      for (int y = 0; y < 4; ++y)
        for (int x = 0; x < 4; ++x) V8D_P(x, y) = v8_clip255(L[y] + T[1 + x] - X);
      break;
    case V8D_VE:
      for (int x = 0; x < 4; ++x) {
        const int v = v8d_avg3(T[x], T[x + 1], T[x + 2]);
        for (int y = 0; y < 4; ++y) V8D_P(x, y) = v;
      }
      break;
    case V8D_HE: {
      const int r[4] = {v8d_avg3(X, I, J), v8d_avg3(I, J, K), v8d_avg3(J, K, Ll), v8d_avg3(K, Ll, Ll)};
      for (int y = 0; y < 4; ++y)
        for (int x = 0; x < 4; ++x) V8D_P(x, y) = r[y];
      break;
    }
    case V8D_RD:
      V8D_P(0, 3) = v8d_avg3(J, K, Ll);
      V8D_P(1, 3) = V8D_P(0, 2) = v8d_avg3(I, J, K);
      V8D_P(2, 3) = V8D_P(1, 2) = V8D_P(0, 1) = v8d_avg3(X, I, J);
      V8D_P(3, 3) = V8D_P(2, 2) = V8D_P(1, 1) = V8D_P(0, 0) = v8d_avg3(A, X, I);
      V8D_P(3, 2) = V8D_P(2, 1) = V8D_P(1, 0) = v8d_avg3(B, A, X);
      V8D_P(3, 1) = V8D_P(2, 0) = v8d_avg3(C, B, A);
      V8D_P(3, 0) = v8d_avg3(D, C, B);
      break;
    case V8D_VR:
      V8D_P(0, 0) = V8D_P(1, 2) = v8d_avg2(X, A);
      V8D_P(1, 0) = V8D_P(2, 2) = v8d_avg2(A, B);
      V8D_P(2, 0) = V8D_P(3, 2) = v8d_avg2(B, C);
      V8D_P(3, 0) = v8d_avg2(C, D);
      V8D_P(0, 3) = v8d_avg3(K, J, I);
      V8D_P(0, 2) = v8d_avg3(J, I, X);
      V8D_P(0, 1) = V8D_P(1, 3) = v8d_avg3(I, X, A);
      V8D_P(1, 1) = V8D_P(2, 3) = v8d_avg3(X, A, B);
      V8D_P(2, 1) = V8D_P(3, 3) = v8d_avg3(A, B, C);
      V8D_P(3, 1) = v8d_avg3(B, C, D);
      break;
    case V8D_LD:
      V8D_P(0, 0) = v8d_avg3(A, B, C);
      V8D_P(1, 0) = V8D_P(0, 1) = v8d_avg3(B, C, D);
      V8D_P(2, 0) = V8D_P(1, 1) = V8D_P(0, 2) = v8d_avg3(C, D, E);
      V8D_P(3, 0) = V8D_P(2, 1) = V8D_P(1, 2) = V8D_P(0, 3) = v8d_avg3(D, E, F);
      V8D_P(3, 1) = V8D_P(2, 2) = V8D_P(1, 3) = v8d_avg3(E, F, G);
      V8D_P(3, 2) = V8D_P(2, 3) = v8d_avg3(F, G, Hh);
      V8D_P(3, 3) = v8d_avg3(G, Hh, Hh);
      break;
    case V8D_VL:
      V8D_P(0, 0) = v8d_avg2(A, B);
      V8D_P(1, 0) = V8D_P(0, 2) = v8d_avg2(B, C);
      V8D_P(2, 0) = V8D_P(1, 2) = v8d_avg2(C, D);
      V8D_P(3, 0) = V8D_P(2, 2) = v8d_avg2(D, E);
      V8D_P(0, 1) = v8d_avg3(A, B, C);
      V8D_P(1, 1) = V8D_P(0, 3) = v8d_avg3(B, C, D);
      V8D_P(2, 1) = V8D_P(1, 3) = v8d_avg3(C, D, E);
      V8D_P(3, 1) = V8D_P(2, 3) = v8d_avg3(D, E, F);
      V8D_P(3, 2) = v8d_avg3(E, F, G);
      V8D_P(3, 3) = v8d_avg3(F, G, Hh);
      break;
    case V8D_HD:
      V8D_P(0, 0) = V8D_P(2, 1) = v8d_avg2(I, X);
      V8D_P(0, 1) = V8D_P(2, 2) = v8d_avg2(J, I);
      V8D_P(0, 2) = V8D_P(2, 3) = v8d_avg2(K, J);
      V8D_P(0, 3) = v8d_avg2(Ll, K);
      V8D_P(3, 0) = v8d_avg3(A, B, C);
      V8D_P(2, 0) = v8d_avg3(X, A, B);
      V8D_P(1, 0) = V8D_P(3, 1) = v8d_avg3(I, X, A);
      V8D_P(1, 1) = V8D_P(3, 2) = v8d_avg3(J, I, X);
      V8D_P(1, 2) = V8D_P(3, 3) = v8d_avg3(K, J, I);
      V8D_P(1, 3) = v8d_avg3(Ll, K, J);
      break;
    case V8D_HU:
      V8D_P(0, 0) = v8d_avg2(I, J);
      V8D_P(2, 0) = V8D_P(0, 1) = v8d_avg2(J, K);
      V8D_P(2, 1) = V8D_P(0, 2) = v8d_avg2(K, Ll);
      V8D_P(1, 0) = v8d_avg3(I, J, K);
      V8D_P(3, 0) = V8D_P(1, 1) = v8d_avg3(J, K, Ll);
      V8D_P(3, 1) = V8D_P(1, 2) = v8d_avg3(K, Ll, Ll);
      V8D_P(3, 2) = V8D_P(2, 2) = V8D_P(0, 3) = V8D_P(1, 3) = V8D_P(2, 3) = V8D_P(3, 3) = Ll;
      break;
    default: {                                   // V8D_DC
      const int dc = (4 + A + B + C + D + I + J + K + Ll) >> 3;
      for (int i = 0; i < 16; ++i) pred[i] = dc;
    }
  }
#undef V8D_P
}
// csrc/vp8_core.h's v8_idct_add for ANY 16-bit coefficients: a damaged stream reaches +-32768, where the second pass's products leave 32 bits, so
// they are formed in 64; for the coefficients a writer can produce the result is the same.
V8_HD void v8d_idct_add(const int* c, const int* pred, unsigned char* dst, long stride) {
  long long t[16];
  for (int i = 0; i < 4; ++i) {
    const int a = c[i] + c[8 + i], b = c[i] - c[8 + i];
    const int cc = v8_mul2(c[4 + i]) - v8_mul1(c[12 + i]), d = v8_mul1(c[4 + i]) + v8_mul2(c[12 + i]);
    t[4 * i] = a + d, t[4 * i + 1] = b + cc, t[4 * i + 2] = b - cc, t[4 * i + 3] = a - d;
  }
  for (int i = 0; i < 4; ++i) {
    const long long dc = t[i] + 4, a = dc + t[8 + i], b = dc - t[8 + i];
    const long long cc = ((t[4 + i] * 35468) >> 16) - (((t[12 + i] * 20091) >> 16) + t[12 + i]);
    const long long d = (((t[4 + i] * 20091) >> 16) + t[4 + i]) + ((t[12 + i] * 35468) >> 16);
    const long long r[4] = {(a + d) >> 3, (b + cc) >> 3, (b - cc) >> 3, (a - d) >> 3};
    for (int k = 0; k < 4; ++k) {
      const long long v = pred[4 * i + k] + r[k];
      dst[i * stride + k] = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
  }
}
V8_HD int v8d_mode16(int m) { return m == V8D_TM ? 3 : m == V8D_VE ? 1 : m == V8D_HE ? 2 : 0; }   // -> csrc/vp8_core.h's v8_predict numbering

// One macroblock: prediction from the UNFILTERED pixels around it plus its residual.  The macroblocks to its left, above and above-right are done.
V8_HD void v8d_recon_mb(const V8dFrame* f, int mby, int mbx) {
  const long long k = (long long)mby * f->mbw + mbx;
  const V8dMb* mb = f->mb + k;
  const short* coef = f->coef + k * 384;
  const bool has = !(mb->nzy == 0 && mb->nzuv == 0);   // without codes every coefficient is zero (or was never written: a skipped macroblock)
  int c[16], pred[16];
  for (int i = 0; i < 16; ++i) c[i] = 0;
  unsigned char* const y0 = f->Y + (long)mby * 16 * f->ys + (long)mbx * 16;
  if (mb->i4x4) {
    for (int n = 0; n < 16; ++n) {
      const int by = n >> 2, bx = n & 3;
      const long py = mby * 16l + by * 4, px = mbx * 16l + bx * 4;
      unsigned char* dst = f->Y + py * f->ys + px;
      int T[9], L[4];
      if (py == 0) {
        for (int i = 0; i < 9; ++i) T[i] = 127;
      } else {
        const unsigned char* row = f->Y + (py - 1) * f->ys;
        T[0] = px ? row[px - 1] : 129;
        for (int i = 0; i < 4; ++i) T[1 + i] = row[px + i];
        if (bx < 3) {
          for (int i = 0; i < 4; ++i) T[5 + i] = row[px + 4 + i];
        } else if (mby == 0) {
          for (int i = 0; i < 4; ++i) T[5 + i] = 127;
        } else {                                 // the right-hand column reads the row above the MACROBLOCK, whatever its own row
          const unsigned char* mrow = f->Y + (mby * 16l - 1) * f->ys + mbx * 16l;
          for (int i = 0; i < 4; ++i) T[5 + i] = mbx == f->mbw - 1 ? mrow[15] : mrow[16 + i];
        }
      }
      for (int i = 0; i < 4; ++i) L[i] = px ? dst[i * f->ys - 1] : 129;
      v8d_pred4(mb->imodes[n], T, L, pred);
      if (has)
        for (int i = 0; i < 16; ++i) c[i] = coef[16 * n + i];
      v8d_idct_add(c, pred, dst, f->ys);
    }
  } else {
    V8Edge e;
    v8_edges(f->Y, f->ys, mby, mbx, 16, &e);
    const int m = v8d_mode16(mb->imodes[0]);
    for (int n = 0; n < 16; ++n) {
      const int yy = (n >> 2) * 4, xx = (n & 3) * 4;
      for (int i = 0; i < 16; ++i) pred[i] = v8_predict(&e, m, yy + (i >> 2), xx + (i & 3));
      if (has)
        for (int i = 0; i < 16; ++i) c[i] = coef[16 * n + i];
      v8d_idct_add(c, pred, y0 + yy * f->ys + xx, f->ys);
    }
  }
  const int m = v8d_mode16(mb->uvmode);
  for (int p = 0; p < 2; ++p) {
    unsigned char* plane = p ? f->V : f->U;
    V8Edge e;
    v8_edges(plane, f->cs, mby, mbx, 8, &e);
    for (int n = 0; n < 4; ++n) {
      const int yy = (n >> 1) * 4, xx = (n & 1) * 4;
      for (int i = 0; i < 16; ++i) pred[i] = v8_predict(&e, m, yy + (i >> 2), xx + (i & 3));
      if (has)
        for (int i = 0; i < 16; ++i) c[i] = coef[16 * (16 + 4 * p + n) + i];
      v8d_idct_add(c, pred, plane + (mby * 8l + yy) * f->cs + mbx * 8l + xx, f->cs);
    }
  }
}

// ---- the loop filters -------------------------------------------------------------------------------------------------------------------------------
V8_HD int v8d_abs(int v) { return v < 0 ? -v : v; }
V8_HD int v8d_sclip1(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }
V8_HD int v8d_sclip2(int v) { return v < -16 ? -16 : v > 15 ? 15 : v; }
V8_HD void v8d_filter2(unsigned char* p, long s) {
  const int p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s];
  const int a = 3 * (q0 - p0) + v8d_sclip1(p1 - q1), a1 = v8d_sclip2((a + 4) >> 3), a2 = v8d_sclip2((a + 3) >> 3);
  p[-s] = (unsigned char)v8_clip255(p0 + a2), p[0] = (unsigned char)v8_clip255(q0 - a1);
}
V8_HD void v8d_filter4(unsigned char* p, long s) {
  const int p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s];
  const int a = 3 * (q0 - p0), a1 = v8d_sclip2((a + 4) >> 3), a2 = v8d_sclip2((a + 3) >> 3), a3 = (a1 + 1) >> 1;
  p[-2 * s] = (unsigned char)v8_clip255(p1 + a3), p[-s] = (unsigned char)v8_clip255(p0 + a2);
  p[0] = (unsigned char)v8_clip255(q0 - a1), p[s] = (unsigned char)v8_clip255(q1 - a3);
}
V8_HD void v8d_filter6(unsigned char* p, long s) {
  const int p2 = p[-3 * s], p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s], q2 = p[2 * s];
  const int a = v8d_sclip1(3 * (q0 - p0) + v8d_sclip1(p1 - q1));
  const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
  p[-3 * s] = (unsigned char)v8_clip255(p2 + a3), p[-2 * s] = (unsigned char)v8_clip255(p1 + a2), p[-s] = (unsigned char)v8_clip255(p0 + a1);
  p[0] = (unsigned char)v8_clip255(q0 - a1), p[s] = (unsigned char)v8_clip255(q1 - a2), p[2 * s] = (unsigned char)v8_clip255(q2 - a3);
}
V8_HD bool v8d_hev(const unsigned char* p, long s, int t) { return v8d_abs(p[-2 * s] - p[-s]) > t || v8d_abs(p[s] - p[0]) > t; }
V8_HD bool v8d_needs(const unsigned char* p, long s, int t) { return 4 * v8d_abs(p[-s] - p[0]) + v8d_abs(p[-2 * s] - p[s]) <= t; }
V8_HD bool v8d_needs2(const unsigned char* p, long s, int t, int it) {
  const int p3 = p[-4 * s], p2 = p[-3 * s], p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s], q2 = p[2 * s], q3 = p[3 * s];
  if (4 * v8d_abs(p0 - q0) + v8d_abs(p1 - q1) > t) return false;
  return v8d_abs(p3 - p2) <= it && v8d_abs(p2 - p1) <= it && v8d_abs(p1 - p0) <= it && v8d_abs(q3 - q2) <= it && v8d_abs(q2 - q1) <= it &&
         v8d_abs(q1 - q0) <= it;
}
// `size` positions along an edge: hs steps across it, vs along it.  mb_edge: the six-tap filter of a macroblock edge, else the four-tap one.
// count (may be null): [0] += positions filtered with high edge variance, [1] += without.
V8_HD void v8d_edge(unsigned char* p, long hs, long vs, int size, int thresh, int ithresh, int hevt, bool mb_edge, int* count) {
  const int t2 = 2 * thresh + 1;
  for (int i = 0; i < size; ++i, p += vs)
    if (v8d_needs2(p, hs, t2, ithresh)) {
      const bool hv = v8d_hev(p, hs, hevt);
      if (count) ++count[hv ? 0 : 1];
      if (hv) v8d_filter2(p, hs);
      else if (mb_edge) v8d_filter6(p, hs);
      else v8d_filter4(p, hs);
    }
}
V8_HD void v8d_simple_edge(unsigned char* p, long hs, long vs, int thresh) {
  const int t2 = 2 * thresh + 1;
  for (int i = 0; i < 16; ++i, p += vs)
    if (v8d_needs(p, hs, t2)) v8d_filter2(p, hs);
}
// One macroblock, in place, in libwebp's order: left edge, inner vertical edges, top edge, inner horizontal edges.  Every macroblock before it in
// raster order is filtered, none after it.  fs: the header block's V8D_H_FS words.
V8_HD void v8d_filter_mb(const V8dFrame* f, int filter_type, const uint32_t* fsw, int mby, int mbx, int* count) {
  const V8dMb* mb = f->mb + (long long)mby * f->mbw + mbx;
  const uint32_t* fs = fsw + ((mb->segment & 3) * 2 + (mb->i4x4 & 1)) * 4;
  const int limit = (int)(fs[0] & 255u), il = (int)(fs[1] & 63u), hevt = (int)(fs[2] & 3u);
  if (filter_type <= 0 || limit == 0) return;
  unsigned char* y = f->Y + mby * 16l * f->ys + mbx * 16l;
  const long ys = f->ys, cs = f->cs;
  if (filter_type == 1) {
    if (mbx > 0) v8d_simple_edge(y, 1, ys, limit + 4);
    if (mb->inner)
      for (int k = 1; k < 4; ++k) v8d_simple_edge(y + 4 * k, 1, ys, limit);
    if (mby > 0) v8d_simple_edge(y, ys, 1, limit + 4);
    if (mb->inner)
      for (int k = 1; k < 4; ++k) v8d_simple_edge(y + 4 * k * ys, ys, 1, limit);
    return;
  }
  unsigned char* u = f->U + mby * 8l * cs + mbx * 8l;
  unsigned char* v = f->V + mby * 8l * cs + mbx * 8l;
  if (mbx > 0) {
    v8d_edge(y, 1, ys, 16, limit + 4, il, hevt, true, count);
    v8d_edge(u, 1, cs, 8, limit + 4, il, hevt, true, count);
    v8d_edge(v, 1, cs, 8, limit + 4, il, hevt, true, count);
  }
  if (mb->inner) {
    for (int k = 1; k < 4; ++k) v8d_edge(y + 4 * k, 1, ys, 16, limit, il, hevt, false, count);
    v8d_edge(u + 4, 1, cs, 8, limit, il, hevt, false, count);
    v8d_edge(v + 4, 1, cs, 8, limit, il, hevt, false, count);
  }
  if (mby > 0) {
    v8d_edge(y, ys, 1, 16, limit + 4, il, hevt, true, count);
    v8d_edge(u, cs, 1, 8, limit + 4, il, hevt, true, count);
    v8d_edge(v, cs, 1, 8, limit + 4, il, hevt, true, count);
  }
  if (mb->inner) {
    for (int k = 1; k < 4; ++k) v8d_edge(y + 4 * k * ys, ys, 1, 16, limit, il, hevt, false, count);
    v8d_edge(u + 4 * cs, cs, 1, 8, limit, il, hevt, false, count);
    v8d_edge(v + 4 * cs, cs, 1, 8, limit, il, hevt, false, count);
  }
}

// ---- output: libwebp's fancy upsampling and fixed-point conversion, one pixel -----------------------------------------------------------------------
V8_HD int v8d_up(const unsigned char* c, long cs, int ch, int cw, int y, int x) {
  const int rn = y >> 1, xn = x >> 1;
  int rf = (y & 1) ? rn + 1 : rn - 1, xf = (x & 1) ? xn + 1 : xn - 1;
  rf = rf < 0 ? 0 : rf > ch - 1 ? ch - 1 : rf;
  xf = xf < 0 ? 0 : xf > cw - 1 ? cw - 1 : xf;
  const int nn = c[rn * cs + xn], nf = c[rn * cs + xf], fn = c[rf * cs + xn], ff = c[rf * cs + xf];
  if (xn == xf) return (3 * nn + fn + 2) >> 2;
  return (((nn + 3 * nf + 3 * fn + ff + 8) >> 3) + nn) >> 1;
}
V8_HD int v8d_clip8(int v) { return (v & ~16383) == 0 ? v >> 6 : v < 0 ? 0 : 255; }
V8_HD uint32_t v8d_pixel(const V8dFrame* f, int y, int x) {        // the ARGB word of pixel (y, x), alpha 255
  const int ch = (f->H + 1) >> 1, cw = (f->W + 1) >> 1;
  const int Y = f->Y[y * f->ys + x], u = v8d_up(f->U, f->cs, ch, cw, y, x), v = v8d_up(f->V, f->cs, ch, cw, y, x);
  const int yy = Y * 19077 >> 8;
  const int r = v8d_clip8(yy + (v * 26149 >> 8) - 14234), g = v8d_clip8(yy - (u * 6419 >> 8) - (v * 13320 >> 8) + 8708),
            b = v8d_clip8(yy + (u * 33050 >> 8) - 17685);
  return 0xff000000u | (uint32_t)r << 16 | (uint32_t)g << 8 | (uint32_t)b;
}

// ---- the parse of a frame, in the pieces the kernel's threads run -----------------------------------------------------------------------------------
// The serial part (one thread): frame header, first-partition header, partition ranges, every macroblock's modes; the header block is written
// last.  probs holds the default coefficient probabilities on entry.  part: 16 words.
V8_HD int v8d_parse_first(const V8dFrame* f, const unsigned char* data, V8dHdr* h, unsigned char* probs, long long* part) {
  long long first_end = 0;
  f->hdr[V8D_H_MAGIC] = 0;
  int st = v8d_frame_tag(data, f->begin, f->end, f->W, f->H, &first_end);
  if (st) return st;
  V8dBool br;
  v8d_bool_init(&br, data, f->begin + 10, first_end);
  v8d_parse_header(&br, h, probs);
  if (br.eof) return V8D_ST_FIRST_END;
  st = v8d_partitions(data, first_end, f->end, h->parts, part);
  if (st) return st;
  for (int my = 0; my < f->mbh; ++my)
    for (int mx = 0; mx < f->mbw; ++mx) {
      V8dMb* mb = f->mb + (long long)my * f->mbw + mx;
      v8d_modes_mb(&br, h, mb, my ? mb - f->mbw : nullptr, mx ? mb - 1 : nullptr);
    }
  if (br.eof) return V8D_ST_FIRST_END;
  uint32_t* w = f->hdr;
  w[V8D_H_MBW] = (uint32_t)f->mbw, w[V8D_H_MBH] = (uint32_t)f->mbh, w[V8D_H_FILTER] = (uint32_t)h->filter_type, w[V8D_H_PARTS] = (uint32_t)h->parts;
  w[V8D_H_SKIP] = (uint32_t)h->use_skip, w[V8D_H_SEGMENTS] = (uint32_t)h->use_segment, w[V8D_H_MAP] = (uint32_t)h->update_map;
  for (int s = 0; s < 4; ++s) {
    for (int i = 0; i < 6; ++i) w[V8D_H_QUANT + 6 * s + i] = (uint32_t)h->quant[s][i];
    for (int i4 = 0; i4 < 2; ++i4) {
      for (int i = 0; i < 3; ++i) w[V8D_H_FS + (2 * s + i4) * 4 + i] = (uint32_t)h->fs[s][i4][i];
      w[V8D_H_FS + (2 * s + i4) * 4 + 3] = 0;
    }
  }
  return V8D_OK;
}
// Token partition p's macroblock rows are p, p + parts, ...  Worker p runs step t = round * stride + x + p on macroblock (round * parts + p, x):
// the macroblock above it was step t - 1 of worker p - 1 (or, for p = 0, of worker parts - 1 a round earlier, stride >= parts steps ago), so with a
// barrier between steps every top context is there when it is read.
V8_HD int v8d_token_stride(const V8dFrame* f, int parts) { return f->mbw > parts ? f->mbw : parts; }
V8_HD long long v8d_token_steps(const V8dFrame* f, int parts) { return (long long)((f->mbh + parts - 1) / parts) * v8d_token_stride(f, parts) + parts; }
struct V8dWorker {
  V8dBool br;
  unsigned lnz, ldc;
};
V8_HD void v8d_token_step(const V8dFrame* f, const V8dHdr* h, const unsigned char* probs, V8dWorker* w, int p, long long t) {
  const long long l = t - p;
  if (l < 0) return;
  const int stride = v8d_token_stride(f, h->parts);
  const long long round = l / stride;
  const int mx = (int)(l - round * stride);
  const long long my = round * h->parts + p;
  if (mx >= f->mbw || my >= f->mbh) return;
  if (mx == 0) w->lnz = w->ldc = 0;
  const long long k = my * f->mbw + mx;
  v8d_tokens_mb(&w->br, probs, h, f->mb + k, my ? f->mb + k - f->mbw : nullptr, &w->lnz, &w->ldc, f->coef + k * 384);
}
