// GIF decode (LZW to palette indices, de-interlace, PIL's frame composition), written once: csrc/gifdec.hip calls these functions from its
// two kernels and tools/gifdec_host_check.cpp from a host program, so the bytes a kernel produces can be checked without a GPU.  Nothing here touches
// memory outside the ranges its arguments name, whatever the code stream or the frame table hold: bad data ends in a status, not in a write, and every
// round of the stream loop consumes at least one code or stops.
//
// gd_unlzw_stream is written for ONE WAVE of 64 lanes per frame, in the style of csrc/pngdec_core.h: values every lane computes alike are plain
// variables, work that differs per lane stands in a GD_FOR_LANES(lane) { ... } body, GD_BARRIER() separates a body that writes memory from one that
// reads what another lane wrote.  On the device a body runs once with lane = threadIdx.x; in a host build it is a loop over lanes 0 .. 63.
//
// The table holds no prefix chains.  The string of a new code is "the previous string plus the first byte of the current one", which is exactly the
// len(prev) + 1 bytes of this frame's own output that start where the previous string was emitted; so an entry is (output offset, length), and
// emitting a code is an LZ77-style copy from earlier output (the KwKwK code, code == next, is the overlapping copy of length len(prev) + 1 from where
// prev was emitted).  A round of the loop:
//   A  the width of a code depends only on how many codes came since the last clear, so the bit position of the j-th code after a clear is closed
//      form (gd_bits_before): the 64 lanes extract 64 consecutive codes at once;
//   B  the codes are resolved in order, wave-uniformly, to (source offset or literal, length, output position), the table grows, and the round ends
//      at the first clear (the positions behind it were guessed with the wrong widths), at end-of-information, at a bad code, at the end of the data
//      or when the frame's pixels are complete.  Consecutive codes whose sources all lie before the first of them form a group;
//   C  group by group, with a barrier between groups: strings of up to GD_SHORT bytes are copied one per lane, longer ones by all lanes together.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GD_HD __host__ __device__ inline
#define GD_WAVE __device__ inline
#define GD_FOR_LANES(lane) for (int lane = (int)threadIdx.x, gd_once_ = 1; gd_once_; gd_once_ = 0)
#define GD_BARRIER() __syncthreads()
// a value every lane holds alike, said so to the compiler (it then lives in scalar registers and branches on it are scalar branches)
#define GD_UNIFORM(x) (__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define GD_HD inline
#define GD_WAVE inline
#define GD_FOR_LANES(lane) for (int lane = 0; lane < 64; ++lane)
#define GD_BARRIER() ((void)0)
#define GD_UNIFORM(x) ((int)(x))
#endif

// status words, per frame
enum {
  GD_OK = 0,
  GD_ST_CODE = 1,        // a code above the next free one
  GD_ST_FIRST = 2,       // the first code after a clear (or of the stream) is not a literal
  GD_ST_TRUNCATED = 3,   // the stream ends, or says end-of-information, before the rectangle's indices are complete
  GD_ST_DESCRIPTOR = 4,  // the frame's table row names bytes outside the batch or the index buffer, or a code size outside 2 .. 8: nothing was read
  GD_ST_LAST = 4
};

// one frame's row of the table, long long each
enum {
  GD_X = 0, GD_Y, GD_W, GD_H,  // the rectangle on the canvas
  GD_IDX,                      // first byte of its W * H indices (stream order) in the index buffer
  GD_BEGIN, GD_END,            // its code stream, sub-block framing removed: data[begin, end)
  GD_MCS,                      // LZW minimum code size, 2 .. 8
  GD_LACE,                     // 1: the rows come in the four interlace passes
  GD_TRANS,                    // transparent index, or -1
  GD_MODE,                     // what the frame leaves pending for the next: 0 nothing, 2 GD_COLOUR over its rectangle, 3 the canvas as it was before it drew
  GD_COLOUR,                   // r | g << 8 | b << 16
  GD_FIRST,                    // 1: the file's first frame: the canvas starts as GD_FILL and the rectangle is drawn opaque
  GD_FILL,
  GD_TAB = 16
};

#ifndef GD_SHORT_BYTES
#define GD_SHORT_BYTES 8           // strings up to this long are copied one per lane; -D to measure another split (DESIGN 4i has 0, 8 and 32)
#endif
enum { GD_TABLE = 4096, GD_SHORT = GD_SHORT_BYTES, GD_NONE = 0xFFFF, GD_MAX_SIDE = 16384 };
static_assert(GD_SHORT >= 0 && GD_SHORT <= 4096, "GD_SHORT_BYTES: 0 (every string by all lanes) .. 4096 (every string by one lane)");

struct GdShared {
  int32_t tbl_off[GD_TABLE];   // per code: where its string stands in the frame's output
  uint16_t tbl_len[GD_TABLE];
  int32_t c_src[64], c_dst[64];  // this round's emitting codes: source offset (or -1 - value for a literal), output position
  uint16_t c_len[64];
  uint16_t code[64];
};

// Bits of the codes 0 .. j - 1 after a clear: code 0 and code k >= 1 are min(12, max(mcs + 1, bit length of first + k - 1)) wide, first = 2^mcs + 2,
// so the codes of at most w bits (w < 12) are the first E(w) = 2^w - 2^mcs - 1 and the sum telescopes to 12 j - sum over w of min(j, E(w)).
GD_HD long long gd_bits_before(long long j, int mcs) {
  long long s = 12 * j;
  for (int w = mcs + 1; w < 12; ++w) {
    const long long e = (1ll << w) - (1ll << mcs) - 1;
    s -= j < e ? j : e;
  }
  return s;
}

// One frame: data[begin, end) -> out[0, npix), returns the status.  The caller has checked 2 <= mcs <= 8 and that the ranges lie inside their
// buffers.  *rounds counts rounds of the loop (each consumes at least one code).
GD_WAVE int gd_unlzw_stream(GdShared* sh, const unsigned char* data, long long begin, long long end, int mcs, unsigned char* out, long long npix,
                            long long* rounds) {
  const int clear = 1 << mcs, eoi = clear + 1, first = clear + 2;
  long long clear_bit = 8 * begin, j = 0, outpos = 0, prev_at = 0;
  int next = first, prev_len = 0, status = GD_OK;
  bool done = false;
  *rounds = 0;
  while (!done) {
    ++*rounds;
    // ---- A: 64 codes at once
    GD_BARRIER();
    GD_FOR_LANES(lane) {
      const long long b0 = clear_bit + gd_bits_before(j + lane, mcs), b1 = clear_bit + gd_bits_before(j + lane + 1, mcs);
      unsigned c = GD_NONE;
      if (b1 <= 8 * end) {
        const long long q = b0 >> 3;
        unsigned v = data[q];
        if (q + 1 < end) v |= (unsigned)data[q + 1] << 8;
        if (q + 2 < end) v |= (unsigned)data[q + 2] << 16;
        c = (v >> (int)(b0 & 7)) & ((1u << (int)(b1 - b0)) - 1u);
      }
      sh->code[lane] = (uint16_t)c;
    }
    GD_BARRIER();
    // ---- B: resolve in order, alike on every lane
    int m = 0, used = 0;
    unsigned long long starts = 0ull, longs = 0ull;
    long long group_at = outpos;
    bool cleared = false;
    for (int i = 0; i < 64; ++i) {
      const int c = GD_UNIFORM(sh->code[i]);
      if (c == GD_NONE) {                                          // the data ends here: fine only without pixels owing (a missing end-of-information)
        status = GD_ST_TRUNCATED, done = true;
        break;
      }
      used = i + 1;
      if (c == clear) {
        cleared = true;
        break;
      }
      if (c == eoi) {
        status = GD_ST_TRUNCATED, done = true;
        break;
      }
      long long src;
      int len;
      if (prev_len == 0) {
        if (c > eoi) {
          status = GD_ST_FIRST, done = true;
          break;
        }
        src = -1 - c, len = 1;
      } else {
        if (c < clear) {
          src = -1 - c, len = 1;
        } else if (c < next) {
          src = GD_UNIFORM(sh->tbl_off[c]), len = GD_UNIFORM(sh->tbl_len[c]);
        } else if (c == next) {
          src = prev_at, len = prev_len + 1;
        } else {
          status = GD_ST_CODE, done = true;
          break;
        }
        if (next < GD_TABLE) {                                     // a full table stays as it is until a clear comes (the deferred clear)
          sh->tbl_off[next] = (int32_t)prev_at;
          sh->tbl_len[next] = (uint16_t)(prev_len + 1);
          ++next;
        }
      }
      prev_at = outpos, prev_len = len;
      if (len >= npix - outpos) len = (int)(npix - outpos), done = true;      // complete; what the stream holds beyond is ignored
      if (m == 0 || (src >= 0 && src + len > group_at)) starts |= 1ull << m, group_at = outpos;
      if (len > GD_SHORT) longs |= 1ull << m;
      sh->c_src[m] = (int32_t)src, sh->c_dst[m] = (int32_t)outpos, sh->c_len[m] = (uint16_t)len;
      ++m;
      outpos += len;
      if (done) break;
    }
    j += used;
    if (cleared) clear_bit += gd_bits_before(j, mcs), j = 0, next = first, prev_len = 0;
    // ---- C: copy, group by group; all sources of a group lie before its first byte (the first string of a group may run into itself: k mod distance)
    for (int i0 = 0; i0 < m;) {
      int i1 = i0 + 1;
      while (i1 < m && !((starts >> i1) & 1ull)) ++i1;
      GD_BARRIER();
      GD_FOR_LANES(lane) {
        const int i = i0 + lane;
        if (i < i1) {
          const int len = sh->c_len[i], src = sh->c_src[i], dst = sh->c_dst[i], dist = dst - src;
          if (len <= GD_SHORT)
            for (int k = 0; k < len; ++k) out[dst + k] = src < 0 ? (unsigned char)(-1 - src) : out[src + (k < dist ? k : k % dist)];
        }
      }
      for (int i = i0; i < i1; ++i) {
        if (!((longs >> i) & 1ull)) continue;
        const int len = GD_UNIFORM(sh->c_len[i]), src = GD_UNIFORM(sh->c_src[i]), dst = GD_UNIFORM(sh->c_dst[i]), dist = dst - src;
        GD_FOR_LANES(lane) {
          for (int k = lane; k < len; k += 64) out[dst + k] = src < 0 ? (unsigned char)(-1 - src) : out[src + (k < dist ? k : k % dist)];
        }
      }
      i0 = i1;
    }
  }
  GD_BARRIER();
  if (outpos >= npix) status = GD_OK;                              // complete: a missing end-of-information, or whatever followed, does not matter
  return status;
}

// The table row's ranges against the buffers: what gd_unlzw_stream and gd_compose_pixel may touch.
GD_HD bool gd_row_ok(const long long* t, long long data_bytes, long long idx_bytes, int H, int W) {
  return t[GD_X] >= 0 && t[GD_Y] >= 0 && t[GD_W] >= 1 && t[GD_H] >= 1 && t[GD_W] <= W - t[GD_X] && t[GD_H] <= H - t[GD_Y] && t[GD_IDX] >= 0 &&
         t[GD_IDX] <= idx_bytes && t[GD_W] * t[GD_H] <= idx_bytes - t[GD_IDX] && t[GD_BEGIN] >= 0 && t[GD_BEGIN] <= t[GD_END] &&
         t[GD_END] <= data_bytes && t[GD_MCS] >= 2 && t[GD_MCS] <= 8;
}

// Row r of an h-row rectangle -> its place in stream order: the passes hold rows 0, 8, ..; 4, 12, ..; 2, 6, ..; 1, 3, ..
GD_HD int gd_interlaced_row(int r, int h) {
  if ((r & 7) == 0) return r >> 3;
  const int n0 = (h + 7) >> 3;
  if ((r & 7) == 4) return n0 + (r >> 3);
  const int n1 = (h + 3) >> 3;
  if ((r & 3) == 2) return n0 + n1 + (r >> 2);
  return n0 + n1 + ((h + 1) >> 2) + (r >> 1);
}

GD_HD unsigned gd_rgb(const unsigned char* p) { return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16; }
GD_HD void gd_put(unsigned char* p, unsigned v) { p[0] = (unsigned char)v, p[1] = (unsigned char)(v >> 8), p[2] = (unsigned char)(v >> 16); }

// Canvas pixel p of H * W through the n frames of the table in order: out[k, p, :] for every frame k (PIL's composition).  `canvas` is what
// the frame shows, `pend` what the canvas becomes before the next frame draws; where nothing is pending, pend is the canvas itself.  carry (2, H, W, 3)
// holds both planes: read unless the first row is the file's first frame, written at the end.  A row whose ranges gd_row_ok refuses draws nothing.
GD_HD void gd_compose_pixel(const long long* tab, int n, const unsigned char* idx, long long idx_bytes, const unsigned char* palette,
                            unsigned char* carry, unsigned char* out, int H, int W, long long p) {
  const long long plane = (long long)H * W;
  const int y = (int)(p / W), x = (int)(p - (long long)y * W);
  unsigned canvas = 0u, pend = 0u;
  if (!tab[GD_FIRST]) canvas = gd_rgb(carry + 3 * p), pend = gd_rgb(carry + 3 * (plane + p));
  for (int k = 0; k < n; ++k) {
    const long long* t = tab + (long long)k * GD_TAB;
    unsigned base = pend;
    if (t[GD_FIRST]) base = (unsigned)t[GD_FILL] & 0xFFFFFFu;
    canvas = base;
    pend = 0xFFFFFFFFu;                                            // "the canvas", until the frame says otherwise
    if (gd_row_ok(t, 0x7fffffffffffffffll, idx_bytes, H, W)) {
      const int rx = x - (int)t[GD_X], ry = y - (int)t[GD_Y], w = (int)t[GD_W], h = (int)t[GD_H];
      if (rx >= 0 && ry >= 0 && rx < w && ry < h) {
        const int row = t[GD_LACE] ? gd_interlaced_row(ry, h) : ry;
        const int v = idx[t[GD_IDX] + (long long)row * w + rx];
        if (t[GD_FIRST] || v != t[GD_TRANS]) canvas = gd_rgb(palette + (long long)k * 768 + 3 * v);
        if (t[GD_MODE] == 2) pend = (unsigned)t[GD_COLOUR] & 0xFFFFFFu;
        else if (t[GD_MODE] == 3) pend = base;
      }
    }
    if (pend == 0xFFFFFFFFu) pend = canvas;
    gd_put(out + 3 * ((long long)k * plane + p), canvas);
  }
  gd_put(carry + 3 * p, canvas), gd_put(carry + 3 * (plane + p), pend);
}
