// WebP lossless (VP8L) decode and libwebp's animation composition, written once: csrc/webpdec.hip calls these functions from its three
// kernels and tools/webpdec_host_check.cpp from a host program, so the words a kernel produces can be checked without a GPU.  Nothing here touches
// memory outside the ranges its arguments name, whatever the compressed bytes hold: bad data ends in a status, not in a write, and every loop over
// the stream consumes at least one bit, produces at least one pixel or stops.
//
// The entropy decode and the inverse predictor are written for ONE WAVE of 64 lanes per stream / frame, in csrc/pngdec_core.h's manner.  Values
// that every lane computes alike (bit position, decoded symbol, pixel position) are plain variables, and a store of such a value to shared memory
// outside any lane body is a store by every lane of the same word to the same place; work that differs per lane stands in a WD_FOR_LANES(lane)
// { ... } body, and WD_BARRIER() separates a body that writes memory from one that reads what another lane wrote.  On the device a body runs once
// with lane = threadIdx.x and the barrier is __syncthreads(); in a host build the body is a loop over lanes 0 .. 63 and the barrier is the loop's
// end.  A body therefore never reads what another lane writes in the same body.
//
//  * wd_decode_stream      one VP8L stream -> the frame's scratch words: a header block (the transforms in the order read), every sub-image, the
//                          entropy-coded main image.  Compressed bytes are staged into a ring in shared memory with 16-byte loads; the bit reader is
//                          the bit position alone; code tables are built in shared memory by the lanes together; the colour cache lives in shared
//                          memory.  A backward reference reads the image's own earlier words from global memory, all lanes together.
//  * wd_untransform_frame  the frame's transforms undone in its own order -> ARGB words of its rectangle; the inverse predictor runs rows skewed
//                          across lanes with a lag of two pixels per row.
//  * wd_compose_pixel      one canvas pixel through the frames of a call: dispose, draw, blend (libwebp's WebPAnimDecoder).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define WD_HD __host__ __device__ inline
#define WD_WAVE __device__ inline
#define WD_FOR_LANES(lane) for (int lane = (int)threadIdx.x, wd_once_ = 1; wd_once_; wd_once_ = 0)
#define WD_BARRIER() __syncthreads()
#define WD_LANES 1
#define WD_LI(lane) 0
#define WD_SHUFFLE_UP(dst, src) (dst)[0] = __shfl_up((src)[0], 1, 64)
#define WD_UNIFORM(x) ((unsigned)__builtin_amdgcn_readfirstlane((int)(x)))
#define WD_SHARED_MAX(p, v) atomicMax((p), (v))
#else
#define WD_HD inline
#define WD_WAVE inline
#define WD_FOR_LANES(lane) for (int lane = 0; lane < 64; ++lane)
#define WD_BARRIER() ((void)0)
#define WD_LANES 64
#define WD_LI(lane) (lane)
#define WD_SHUFFLE_UP(dst, src)                                   \
  do {                                                            \
    for (int l_ = 63; l_ > 0; --l_) (dst)[l_] = (src)[l_ - 1];    \
    (dst)[0] = (src)[0];                                          \
  } while (0)
#define WD_UNIFORM(x) ((unsigned)(x))
#define WD_SHARED_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#endif

// status words: per frame, of the decode and of the untransform
enum {
  WD_OK = 0,
  WD_ST_HEADER = 1,       // a signature other than 0x2f or a version other than 0
  WD_ST_SIZE = 2,         // the stream's own size differs from the rectangle of its table row
  WD_ST_TRANSFORM = 3,    // a transform type read twice
  WD_ST_CODE = 4,         // a prefix code that is over-subscribed, incomplete or empty
  WD_ST_SYMBOL = 5,       // a symbol outside its alphabet, or bits that are no code of the table
  WD_ST_REPEAT = 6,       // a code-length repeat past the alphabet, or max_symbol above it
  WD_ST_CACHE = 7,        // colour-cache bits outside 1 .. 11
  WD_ST_DISTANCE = 8,     // a distance beyond the pixels produced
  WD_ST_TOO_LONG = 9,     // a copy that runs past the image
  WD_ST_EXHAUSTED = 10,   // data exhausted before the last pixel
  WD_ST_SCRATCH = 11,     // the sub-images do not fit the frame's scratch words.  Where only the prefix-code groups do not fit, the status is
                          // NEGATIVE instead: minus the scratch words with which the frame decodes, so that the caller can come again
  WD_ST_DESCRIPTOR = 12,  // the table row names bytes or words outside the buffers: nothing was touched
  WD_ST_UPSTREAM = 13,    // untransform: the decode left no valid header block
  WD_ST_LAST = 13
};

enum {
  WD_RING = 3584,         // staged compressed bytes; with it WdShared is 81 744 B, so that two workgroups fit a CU's 160 KB
  WD_MAX_SIDE = 16384,
  WD_TAB = 16,            // long long words per frame row
  WD_HDR = 32,            // header words at the start of a frame's scratch
  WD_MAGIC = 0x57443031,
  WD_SLOTS = 4,           // prefix-code groups resident in shared memory
  WD_GREEN_MAX = 256 + 24 + 2048,
  WD_SYMS = WD_GREEN_MAX + 3 * 256 + 40,
  WD_FAST_G = 10, WD_FAST_C = 10, WD_FAST_D = 6, WD_FAST_CL = 7,
  WD_LUTS = (1 << WD_FAST_G) + 3 * (1 << WD_FAST_C) + (1 << WD_FAST_D),
  WD_NONE = 0x7fffffff
};

// table row (long long words): the frame's rectangle on the canvas, its stream's byte range in data, its scratch words, where its ARGB words go,
// flags, and the rectangle of the frame before it if that one disposes to background
enum { WD_X, WD_Y, WD_W, WD_H, WD_BEGIN, WD_END, WD_SCR, WD_CAP, WD_PIX, WD_FLAGS, WD_PX, WD_PY, WD_PW, WD_PH };
enum { WD_F_BLEND = 1, WD_F_KEY = 2, WD_F_FIRST = 4, WD_F_PREV_DISPOSED = 8 };

// one group's five prefix codes as the symbol path reads them: 16-byte multiples, copied to and from global memory as 16-byte vectors
struct WdGroup {
  unsigned short sym[WD_SYMS];        // symbols sorted by (length, symbol): green, red, blue, alpha, distance
  unsigned short lut[WD_LUTS];        // (symbol << 4 | length), 0: not a code of <= fast bits
  unsigned short cnt[5][16];          // codes per length; [0] is 0
  short one[8];                       // the code's only symbol (it costs no bits), or -1
};
static_assert(sizeof(WdGroup) == 14768 && sizeof(WdGroup) % 16 == 0, "WdGroup is copied in 16-byte vectors; mmgt_amd/hip.py states its size");

struct WdShared {
  alignas(16) WdGroup slot[WD_SLOTS];
  alignas(16) uint32_t ring[WD_RING / 4];
  uint32_t cache[2048];               // the colour cache
  uint32_t owner[2048];               // 1 + the position of the last pixel that went to a cache entry
  int tag[WD_SLOTS];                  // which group a slot holds, -1: none
  unsigned short lut_cl[1 << WD_FAST_CL], sym_cl[20], cnt_cl[16];
  unsigned char lens[WD_GREEN_MAX + 8];
  unsigned char cl_lens[20];
};

WD_HD int wd_sym_off(int k) { return k == 0 ? 0 : k < 4 ? WD_GREEN_MAX + 256 * (k - 1) : WD_GREEN_MAX + 768; }
WD_HD int wd_lut_off(int k) { return k == 0 ? 0 : k < 4 ? (1 << WD_FAST_G) + (k - 1) * (1 << WD_FAST_C) : (1 << WD_FAST_G) + 3 * (1 << WD_FAST_C); }
WD_HD int wd_fast(int k) { return k == 0 ? WD_FAST_G : k < 4 ? WD_FAST_C : WD_FAST_D; }

// ---- canonical prefix codes --------------------------------------------------------------------------------------------------------------------------
// The code whose bits are `bits` (first bit in bit 0), looking at no more than maxbits of them: (symbol << 4 | length), 0 if none.
WD_HD unsigned wd_canon(const unsigned short* cnt, const unsigned short* sym, uint64_t bits, int maxbits) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= maxbits; ++len) {
    code |= (int)(bits & 1u);
    bits >>= 1;
    const int count = cnt[len];
    if (code - count < first) return (unsigned)sym[index + (code - first)] << 4 | (unsigned)len;
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return 0u;
}

// lens[0 .. n) -> cnt, sym, lut, *one.  Lane l (1 .. 15) counts and then places the symbols of length l; all lanes fill the first-level table.  A code
// must be complete, or have exactly one symbol (of any stated length): that one costs no bits.
WD_WAVE int wd_build(const unsigned char* lens, int n, unsigned short* cnt, unsigned short* sym, unsigned short* lut, int fast, int* one) {
  WD_BARRIER();
  WD_FOR_LANES(lane) {
    if (lane < 16) {
      int c = 0;
      for (int s = 0; s < n; ++s) c += lens[s] == lane;
      cnt[lane] = (unsigned short)(lane ? c : 0);
    }
  }
  WD_BARRIER();
  int left = 1, total = 0;
  for (int l = 1; l < 16; ++l) {
    left = (left << 1) - (int)cnt[l];
    total += cnt[l];
    if (left < 0 && total > 1) return WD_ST_CODE;
  }
  total = (int)WD_UNIFORM(total), left = (int)WD_UNIFORM(left);
  if (total == 0 || (total > 1 && left != 0)) return WD_ST_CODE;
  WD_FOR_LANES(lane) {
    if (lane >= 1 && lane < 16) {
      int o = 0;
      for (int l = 1; l < lane; ++l) o += cnt[l];
      for (int s = 0; s < n; ++s)
        if (lens[s] == lane) sym[o++] = (unsigned short)s;
    }
  }
  WD_BARRIER();
  *one = -1;
  if (total == 1) {
    *one = (int)WD_UNIFORM(sym[0]);
    return WD_OK;
  }
  WD_FOR_LANES(lane) {
    for (int i = lane; i < (1 << fast); i += 64) lut[i] = (unsigned short)wd_canon(cnt, sym, (uint64_t)i, fast);
  }
  WD_BARRIER();
  return WD_OK;
}

// ---- bit reader and staging -----------------------------------------------------------------------------------------------------------------------
// Positions are bits / bytes of the whole batch buffer `data` (data_bytes a multiple of 16, the pointer 16-byte aligned).  The ring holds the bytes
// [rbase, rbase + WD_RING), rbase a multiple of 16; bytes at or past the stream's end are zeros.  `over` is set once a bit past the end was taken:
// every loop looks at it once per iteration, and no iteration takes more than 64 bits.
struct WdIn {
  const unsigned char* data;
  long long data_bytes, begin, end, rbase, gbit;
  int over;
};

WD_WAVE void wd_stage(WdShared* sh, WdIn* in) {
  in->rbase = (in->gbit >> 3) & ~15ll;
  WD_BARRIER();
  WD_FOR_LANES(lane) {
    for (int v = lane; v < WD_RING / 16; v += 64) {
      const long long ga = in->rbase + 16ll * v;
      uint32_t q[4] = {0u, 0u, 0u, 0u};
      if (ga >= 0 && ga < in->end && ga + 16 <= in->data_bytes) {
        memcpy(q, __builtin_assume_aligned(in->data + ga, 16), 16);
        if (ga + 16 > in->end) {
          const int keep = (int)(in->end - ga);                    // 1 .. 15 bytes of this vector belong to the stream
          for (int w = 0; w < 4; ++w) {
            const int kb = keep - 4 * w;
            if (kb <= 0) q[w] = 0u;
            else if (kb < 4) q[w] &= (1u << (8 * kb)) - 1u;
          }
        }
      }
      for (int w = 0; w < 4; ++w) sh->ring[4 * v + w] = q[w];
    }
  }
  WD_BARRIER();
}

// 64 bits from in->gbit on (12 bytes of the ring)
WD_WAVE uint64_t wd_peek(WdShared* sh, WdIn* in) {
  const long long byte0 = (in->gbit >> 5) << 2;
  if (byte0 < in->rbase || byte0 + 12 > in->rbase + WD_RING) wd_stage(sh, in);
  const int w = (int)(((in->gbit >> 5) << 2) - in->rbase) >> 2;
  const uint32_t w0 = WD_UNIFORM(sh->ring[w]), w1 = WD_UNIFORM(sh->ring[w + 1]), w2 = WD_UNIFORM(sh->ring[w + 2]);
  const int s = (int)(in->gbit & 31);
  uint64_t v = ((uint64_t)w1 << 32 | w0) >> s;
  if (s) v |= (uint64_t)w2 << (64 - s);
  return v;
}

WD_HD void wd_take(WdIn* in, int n) {
  in->gbit += n;
  if (in->gbit > 8 * in->end) in->over = 1;
}

WD_WAVE unsigned wd_read(WdShared* sh, WdIn* in, int n) {         // n <= 32
  const uint64_t v = wd_peek(sh, in);
  wd_take(in, n);
  return (unsigned)(v & ((1ull << n) - 1ull));
}

// ---- one prefix code ---------------------------------------------------------------------------------------------------------------------------------
WD_WAVE int wd_read_code(WdShared* sh, WdIn* in, WdGroup* G, int k, int alphabet, long long* steps) {
  ++*steps;
  uint64_t v = wd_peek(sh, in);
  WD_BARRIER();
  WD_FOR_LANES(lane) {
    for (int s = lane; s < alphabet; s += 64) sh->lens[s] = 0;
  }
  WD_BARRIER();
  if (v & 1u) {                                                    // a simple code: one or two symbols of length 1
    const int two = (int)((v >> 1) & 1u), wide = (int)((v >> 2) & 1u);
    const int s0 = (int)((v >> 3) & (wide ? 255u : 1u));
    int used = 3 + (wide ? 8 : 1);
    const int s1 = two ? (int)((v >> used) & 255u) : s0;
    used += two ? 8 : 0;
    wd_take(in, used);
    if (in->over) return WD_ST_EXHAUSTED;
    if (s0 >= alphabet || s1 >= alphabet) return WD_ST_SYMBOL;
    sh->lens[s0] = 1;
    sh->lens[s1] = 1;
  } else {
    const int ncl = (int)((v >> 1) & 15u) + 4;
    wd_take(in, 5);
    v = wd_peek(sh, in);                                           // 19 * 3 = 57 bits at most
    WD_FOR_LANES(lane) {
      if (lane < 19) {
        constexpr unsigned char order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
        sh->cl_lens[order[lane]] = (unsigned char)(lane < ncl ? (v >> (3 * lane)) & 7u : 0u);
      }
    }
    wd_take(in, 3 * ncl);
    if (in->over) return WD_ST_EXHAUSTED;
    int one_cl;
    const int st = wd_build(sh->cl_lens, 19, sh->cnt_cl, sh->sym_cl, sh->lut_cl, WD_FAST_CL, &one_cl);
    if (st) return st;
    v = wd_peek(sh, in);
    int tokens = alphabet;
    if (v & 1u) {
      const int nb = 2 + 2 * (int)((v >> 1) & 7u);
      tokens = 2 + (int)((v >> 4) & ((1u << nb) - 1u));
      wd_take(in, 4 + nb);
      if (tokens > alphabet) return WD_ST_REPEAT;
    } else {
      wd_take(in, 1);
    }
    int n = 0, prev = 8;
    while (n < alphabet && tokens-- > 0) {
      ++*steps;
      if (in->over) return WD_ST_EXHAUSTED;
      v = wd_peek(sh, in);
      unsigned e = one_cl >= 0 ? (unsigned)one_cl << 4 : WD_UNIFORM(sh->lut_cl[v & ((1u << WD_FAST_CL) - 1u)]);
      if (one_cl < 0 && !e) return WD_ST_SYMBOL;
      const int s = (int)(e >> 4), l = (int)(e & 15u);
      int used = l, rep = 1, val = s;
      if (s == 16) rep = 3 + (int)((v >> l) & 3u), val = prev, used += 2;
      else if (s == 17) rep = 3 + (int)((v >> l) & 7u), val = 0, used += 3;
      else if (s == 18) rep = 11 + (int)((v >> l) & 127u), val = 0, used += 7;
      else if (s) prev = s;
      if (n + rep > alphabet) return WD_ST_REPEAT;
      if (val) {
        WD_FOR_LANES(lane) {
          for (int i = lane; i < rep; i += 64) sh->lens[n + i] = (unsigned char)val;
        }
      }
      n += rep;
      wd_take(in, used);
    }
    if (in->over) return WD_ST_EXHAUSTED;
  }
  int one;
  const int st = wd_build(sh->lens, alphabet, G->cnt[k], G->sym + wd_sym_off(k), G->lut + wd_lut_off(k), wd_fast(k), &one);
  if (st) return st;
  G->one[k] = (short)one;                                          // every lane stores the same word
  return WD_OK;
}

// (symbol << 4 | length) of code k at the head of `bits`, WD_NONE if the bits are no code
WD_WAVE unsigned wd_symbol(const WdGroup* G, int k, int one, uint64_t bits) {
  if (one >= 0) return (unsigned)one << 4;
  unsigned e = WD_UNIFORM(G->lut[wd_lut_off(k) + (int)(bits & ((1u << wd_fast(k)) - 1u))]);
  if (!e) e = WD_UNIFORM(wd_canon(G->cnt[k], G->sym + wd_sym_off(k), bits, 15));
  return e ? e : (unsigned)WD_NONE;
}

WD_HD int wd_prefix_extra(int p) { return p < 4 ? 0 : (p - 2) >> 1; }
WD_HD int wd_prefix_value(int p, unsigned extra) { return p < 4 ? p + 1 : (int)(((2u + (unsigned)(p & 1)) << ((p - 2) >> 1)) + extra + 1u); }

WD_HD int wd_distance(int v, int w) {
  if (v > 120) return v - 120;
  constexpr signed char dx[120] = {0, 1,  1, -1, 0, 2,  1, -1, 2,  -2, 2, -2, 0, 3, 1,  -1, 3,  -3, 2, -2, 3, -3, 0, 4,  1, -1, 4,  -4, 3, -3,
                                   2, -2, 4, -4, 0, 3,  -3, 4, -4, 5,  1, -1, 5, -5, 2, -2, 5,  -5, 4, -4, 3, -3, 5, -5, 0, 6,  1,  -1, 6, -6,
                                   2, -2, 6, -6, 4, -4, 5,  -5, 3, -3, 6, -6, 0, 7, 1,  -1, 5,  -5, 7, -7, 4, -4, 6, -6, 2, -2, 7,  -7, 3, -3,
                                   7, -7, 5, -5, 6, -6, 8,  4,  -4, 7, -7, 8, 8, 6, -6, 8,  5,  -5, 7, -7, 8, 6,  -6, 7, -7, 8, 7,  -7, 8, 8};
  constexpr signed char dy[120] = {1, 0, 1, 1, 2, 0, 2, 2, 1, 1, 2, 2, 3, 0, 3, 3, 1, 1, 3, 3, 2, 2, 4, 0, 4, 4, 1, 1, 3, 3, 4, 4, 2, 2, 5, 4, 4, 3, 3, 0,
                                   5, 5, 1, 1, 5, 5, 2, 2, 4, 4, 5, 5, 3, 3, 6, 0, 6, 6, 1, 1, 6, 6, 2, 2, 5, 5, 4, 4, 6, 6, 3, 3, 7, 0, 7, 7, 5, 5, 1, 1,
                                   6, 6, 4, 4, 7, 7, 2, 2, 7, 7, 3, 3, 6, 6, 5, 5, 0, 7, 7, 4, 4, 1, 2, 6, 6, 3, 7, 7, 5, 5, 4, 7, 7, 6, 6, 5, 7, 7, 6, 7};
  const int d = dx[v - 1] + dy[v - 1] * w;
  return d < 1 ? 1 : d;
}

WD_HD unsigned wd_cache_key(uint32_t argb, int cache_bits) { return (0x1e35a7bdu * argb) >> (32 - cache_bits); }

// ---- an entropy-coded image --------------------------------------------------------------------------------------------------------------------------
struct WdFrame {
  uint32_t* scr;          // the frame's scratch words, 16-byte aligned
  long long cap, used;    // in words
};

WD_HD long long wd_alloc(WdFrame* f, long long words) {            // -> offset, or -1
  const long long at = (f->used + 3) & ~3ll;
  if (words < 0 || at + words > f->cap) return -1;
  f->used = at + words;
  return at;
}

WD_WAVE void wd_copy_group(WdGroup* dst, const WdGroup* src) {
  WD_BARRIER();
  WD_FOR_LANES(lane) {
    for (int v = lane; v < (int)(sizeof(WdGroup) / 16); v += 64) {
      uint32_t q[4];
      memcpy(q, __builtin_assume_aligned((const unsigned char*)src + 16 * (size_t)v, 16), 16);
      memcpy(__builtin_assume_aligned((unsigned char*)dst + 16 * (size_t)v, 16), q, 16);
    }
  }
  WD_BARRIER();
}

// The codes of `groups` groups and then w * h pixels -> out.  ent (ew wide, blocks of 2^pb pixels) names each pixel's group; null: one group.
WD_WAVE int wd_coded_pixels(WdShared* sh, WdIn* in, WdFrame* fr, uint32_t* out, int w, int h, int cache_bits, const uint32_t* ent, int pb, int ew,
                            int groups, long long* steps) {
  const int green = 280 + (cache_bits ? 1 << cache_bits : 0);
  WdGroup* global_groups = nullptr;
  if (groups > 1) {
    const long long words = (long long)groups * (long long)(sizeof(WdGroup) / 4);
    const long long at = wd_alloc(fr, words);
    if (at < 0) {                                                  // nothing is allocated after the groups: what the frame needs is known here
      const long long need = ((fr->used + 3) & ~3ll) + words;
      return need <= 0x7fffffffll ? -(int)need : WD_ST_SCRATCH;
    }
    global_groups = (WdGroup*)(fr->scr + at);
  }
  for (int g = 0; g < groups; ++g) {
    for (int k = 0; k < 5; ++k) {
      if (in->over) return WD_ST_EXHAUSTED;
      const int st = wd_read_code(sh, in, &sh->slot[0], k, k == 0 ? green : k == 4 ? 40 : 256, steps);
      if (st) return st;
    }
    if (global_groups) wd_copy_group(global_groups + g, &sh->slot[0]);
  }
  for (int s = 0; s < WD_SLOTS; ++s) sh->tag[s] = global_groups ? -1 : 0;
  if (cache_bits) {
    WD_BARRIER();
    WD_FOR_LANES(lane) {
      for (int i = lane; i < (1 << cache_bits); i += 64) sh->cache[i] = 0u, sh->owner[i] = 0u;
    }
  }
  WD_BARRIER();
  const WdGroup* G = &sh->slot[0];
  int one[5];
  for (int k = 0; k < 5; ++k) one[k] = (int)WD_UNIFORM((int)G->one[k]);
  const long long npix = (long long)w * h;
  long long pos = 0;
  int x = 0, y = 0, bx = -1, by = -1;
  bool dirty = false;                                              // words stored since the last barrier
  while (pos < npix) {
    ++*steps;
    if (in->over) return WD_ST_EXHAUSTED;
    if (global_groups && ((x >> pb) != bx || (y >> pb) != by)) {
      bx = x >> pb, by = y >> pb;
      const int g = (int)(WD_UNIFORM(ent[(size_t)by * ew + bx]) >> 8) & 0xffff;      // < groups: groups is the largest of them + 1
      const int s = g % WD_SLOTS;
      if ((int)WD_UNIFORM(sh->tag[s]) != g) {
        wd_copy_group(&sh->slot[s], global_groups + g);
        sh->tag[s] = g;
      }
      G = &sh->slot[s];
      for (int k = 0; k < 5; ++k) one[k] = (int)WD_UNIFORM((int)G->one[k]);
    }
    const uint64_t v = wd_peek(sh, in);
    unsigned e = wd_symbol(G, 0, one[0], v);
    if (e == (unsigned)WD_NONE) return WD_ST_SYMBOL;
    const int s = (int)(e >> 4);
    int used = (int)(e & 15u);
    if (s < 256 || s >= 280) {
      uint32_t argb;
      if (s < 256) {
        const unsigned r = wd_symbol(G, 1, one[1], v >> used);
        if (r == (unsigned)WD_NONE) return WD_ST_SYMBOL;
        used += (int)(r & 15u);
        const unsigned b = wd_symbol(G, 2, one[2], v >> used);
        if (b == (unsigned)WD_NONE) return WD_ST_SYMBOL;
        used += (int)(b & 15u);
        const unsigned a = wd_symbol(G, 3, one[3], v >> used);
        if (a == (unsigned)WD_NONE) return WD_ST_SYMBOL;
        used += (int)(a & 15u);                                    // 60 bits at most
        argb = (uint32_t)(a >> 4) << 24 | (uint32_t)(r >> 4) << 16 | (uint32_t)s << 8 | (uint32_t)(b >> 4);
      } else {
        if (s - 280 >= (cache_bits ? 1 << cache_bits : 0)) return WD_ST_SYMBOL;
        argb = WD_UNIFORM(sh->cache[s - 280]);
      }
      wd_take(in, used);
      if (in->over) return WD_ST_EXHAUSTED;
      WD_FOR_LANES(lane) {
        if (lane == 0) out[pos] = argb;
      }
      dirty = true;
      if (cache_bits) {
        const unsigned key = wd_cache_key(argb, cache_bits);
        sh->cache[key] = argb;                                     // every lane stores the same word, and reads back its own store
        sh->owner[key] = (uint32_t)(pos + 1);
      }
      ++pos;
      if (++x == w) x = 0, ++y;
      continue;
    }
    const int le = wd_prefix_extra(s - 256);
    const int len = wd_prefix_value(s - 256, (unsigned)((v >> used) & ((1u << le) - 1u)));
    used += le;
    const unsigned d = wd_symbol(G, 4, one[4], v >> used);
    if (d == (unsigned)WD_NONE) return WD_ST_SYMBOL;
    used += (int)(d & 15u);
    const int de = wd_prefix_extra((int)(d >> 4));
    const int dist = wd_distance(wd_prefix_value((int)(d >> 4), (unsigned)((v >> used) & ((1u << de) - 1u))), w);
    used += de;                                                    // 15 + 10 + 15 + 18 = 58 bits at most
    wd_take(in, used);
    if (in->over) return WD_ST_EXHAUSTED;
    if (dist > pos) return WD_ST_DISTANCE;
    if (len > npix - pos) return WD_ST_TOO_LONG;
    // word i of the match is word pos - dist + (i mod dist): every read lies before pos, so no round reads what a round of this copy writes
    if (dirty) WD_BARRIER();
    for (int base = 0; base < len; base += 64) {
      WD_FOR_LANES(lane) {
        const int i = base + lane;
        if (i < len) {
          const uint32_t word = out[pos - dist + i % dist];
          out[pos + i] = word;
          if (cache_bits) WD_SHARED_MAX(&sh->owner[wd_cache_key(word, cache_bits)], (uint32_t)(pos + i + 1));
        }
      }
    }
    WD_BARRIER();
    dirty = false;
    if (cache_bits) {                                              // of the pixels that share an entry the last one stays, as when they go in one by one
      for (int base = 0; base < len; base += 64) {
        WD_FOR_LANES(lane) {
          const int i = base + lane;
          if (i < len) {
            const uint32_t word = out[pos + i];
            const unsigned key = wd_cache_key(word, cache_bits);
            if (sh->owner[key] == (uint32_t)(pos + i + 1)) sh->cache[key] = word;
          }
        }
      }
      WD_BARRIER();
    }
    pos += len;
    y = (int)(pos / w), x = (int)(pos - (long long)y * w);
  }
  WD_BARRIER();
  return WD_OK;
}

WD_WAVE int wd_cache_bits(WdShared* sh, WdIn* in, int* cache_bits) {
  *cache_bits = 0;
  if (wd_read(sh, in, 1)) {
    *cache_bits = (int)wd_read(sh, in, 4);
    if (*cache_bits < 1 || *cache_bits > 11) return WD_ST_CACHE;
  }
  return in->over ? WD_ST_EXHAUSTED : WD_OK;
}

// a sub-image: no meta codes
WD_WAVE int wd_sub_image(WdShared* sh, WdIn* in, WdFrame* fr, int w, int h, long long* at, long long* steps) {
  *at = wd_alloc(fr, (long long)w * h);
  if (*at < 0) return WD_ST_SCRATCH;
  int cache_bits;
  const int st = wd_cache_bits(sh, in, &cache_bits);
  if (st) return st;
  return wd_coded_pixels(sh, in, fr, fr->scr + *at, w, h, cache_bits, nullptr, 0, 0, 1, steps);
}

// One stream -> the frame's scratch.  Header block: [0] WD_MAGIC once everything decoded, [1] transforms, [2] main image offset, [3] its width,
// then per transform in the order read: type, bits, offset of its sub-image, the width it was read at, palette entries.
WD_WAVE int wd_decode_body(WdShared* sh, WdIn* in, WdFrame* fr, int W, int H, long long* steps) {
  uint32_t* hdr = fr->scr;
  const uint64_t v = wd_peek(sh, in);
  wd_take(in, 40);
  if (in->over) return WD_ST_EXHAUSTED;
  if ((v & 255u) != 0x2fu || ((v >> 37) & 7u) != 0u) return WD_ST_HEADER;
  if ((int)((v >> 8) & 0x3fffu) + 1 != W || (int)((v >> 22) & 0x3fffu) + 1 != H) return WD_ST_SIZE;
  int xs = W, ntrans = 0, seen = 0;
  while (wd_read(sh, in, 1)) {
    ++*steps;
    if (in->over) return WD_ST_EXHAUSTED;
    const int type = (int)wd_read(sh, in, 2);
    if (seen >> type & 1) return WD_ST_TRANSFORM;
    seen |= 1 << type;
    int bits = 0, n = 0;
    long long at = 0;
    const int w_read = xs;
    if (type == 0 || type == 1) {
      bits = (int)wd_read(sh, in, 3) + 2;
      const int st = wd_sub_image(sh, in, fr, (xs + (1 << bits) - 1) >> bits, (H + (1 << bits) - 1) >> bits, &at, steps);
      if (st) return st;
    } else if (type == 3) {
      n = (int)wd_read(sh, in, 8) + 1;
      bits = n <= 2 ? 3 : n <= 4 ? 2 : n <= 16 ? 1 : 0;
      const int st = wd_sub_image(sh, in, fr, n, 1, &at, steps);
      if (st) return st;
      xs = (xs + (1 << bits) - 1) >> bits;
    }
    WD_FOR_LANES(lane) {
      if (lane == 0) {
        uint32_t* t = hdr + 4 + 5 * ntrans;
        t[0] = (uint32_t)type, t[1] = (uint32_t)bits, t[2] = (uint32_t)at, t[3] = (uint32_t)w_read, t[4] = (uint32_t)n;
      }
    }
    ++ntrans;
  }
  if (in->over) return WD_ST_EXHAUSTED;
  const long long main_at = wd_alloc(fr, (long long)xs * H);
  if (main_at < 0) return WD_ST_SCRATCH;
  int cache_bits;
  int st = wd_cache_bits(sh, in, &cache_bits);
  if (st) return st;
  const uint32_t* ent = nullptr;
  int pb = 0, ew = 0, groups = 1;
  if (wd_read(sh, in, 1)) {
    pb = (int)wd_read(sh, in, 3) + 2;
    ew = (xs + (1 << pb) - 1) >> pb;
    const int eh = (H + (1 << pb) - 1) >> pb;
    long long at;
    st = wd_sub_image(sh, in, fr, ew, eh, &at, steps);
    if (st) return st;
    ent = fr->scr + at;
    int most[WD_LANES];
    WD_FOR_LANES(lane) {
      int m = 0;
      for (long long i = lane; i < (long long)ew * eh; i += 64) {
        const int g = (int)(ent[i] >> 8) & 0xffff;
        m = g > m ? g : m;
      }
      most[WD_LI(lane)] = m;
    }
#if defined(__HIPCC__)
    for (int o = 32; o; o >>= 1) {
      const int other = __shfl_xor(most[0], o, 64);
      most[0] = other > most[0] ? other : most[0];
    }
    groups = (int)WD_UNIFORM(most[0]) + 1;
#else
    for (int l = 0; l < 64; ++l) groups = most[l] + 1 > groups ? most[l] + 1 : groups;
#endif
  }
  if (in->over) return WD_ST_EXHAUSTED;
  st = wd_coded_pixels(sh, in, fr, fr->scr + main_at, xs, H, cache_bits, ent, pb, ew, groups, steps);
  if (st) return st;
  WD_FOR_LANES(lane) {
    if (lane == 0) hdr[1] = (uint32_t)ntrans, hdr[2] = (uint32_t)main_at, hdr[3] = (uint32_t)xs;
  }
  return WD_OK;
}

WD_HD bool wd_row_ok(const long long* t, long long data_bytes, long long scratch_words, long long argb_words) {
  return t[WD_W] >= 1 && t[WD_H] >= 1 && t[WD_W] <= WD_MAX_SIDE && t[WD_H] <= WD_MAX_SIDE && t[WD_X] >= 0 && t[WD_Y] >= 0 &&
         t[WD_X] <= WD_MAX_SIDE && t[WD_Y] <= WD_MAX_SIDE && t[WD_BEGIN] >= 0 && t[WD_END] >= t[WD_BEGIN] && t[WD_END] <= data_bytes &&
         t[WD_SCR] >= 0 && (t[WD_SCR] & 3) == 0 && t[WD_CAP] >= WD_HDR && t[WD_CAP] <= scratch_words && t[WD_SCR] <= scratch_words - t[WD_CAP] &&
         t[WD_PIX] >= 0 && t[WD_PIX] <= argb_words - t[WD_W] * t[WD_H];
}

// Row t of the batch: data[begin, end) -> scratch + t[WD_SCR]; returns the status (negative: see WD_ST_SCRATCH).  *steps counts loop iterations: at most 131 per payload bit (a
// code of 18 bits or more may state up to 2328 lengths without a further bit) plus one per pixel of the main image and of the sub-images plus 16.
WD_WAVE int wd_decode_stream(WdShared* sh, const unsigned char* data, long long data_bytes, const long long* t, uint32_t* scratch,
                             long long scratch_words, long long* steps) {
  *steps = 0;
  if (!wd_row_ok(t, data_bytes, scratch_words, 1ll << 62)) return WD_ST_DESCRIPTOR;
  WdIn in{data, data_bytes, t[WD_BEGIN], t[WD_END], 0, 8 * t[WD_BEGIN], 0};
  WdFrame fr{scratch + t[WD_SCR], t[WD_CAP], WD_HDR};
  WD_FOR_LANES(lane) {
    if (lane == 0) fr.scr[0] = 0u;
  }
  wd_stage(sh, &in);
  const int st = wd_decode_body(sh, &in, &fr, (int)t[WD_W], (int)t[WD_H], steps);
  WD_FOR_LANES(lane) {
    if (lane == 0 && !st) fr.scr[0] = (uint32_t)WD_MAGIC;
  }
  return st;
}

// ---- inverse transforms ------------------------------------------------------------------------------------------------------------------------------
WD_HD uint32_t wd_add(uint32_t a, uint32_t b) {                     // per channel mod 256
  return (((a & 0xff00ff00u) + (b & 0xff00ff00u)) & 0xff00ff00u) | (((a & 0x00ff00ffu) + (b & 0x00ff00ffu)) & 0x00ff00ffu);
}
WD_HD uint32_t wd_avg(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
WD_HD int wd_ch(uint32_t p, int c) { return (int)(p >> (8 * c)) & 255; }
WD_HD int wd_clamp(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

WD_HD uint32_t wd_predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
  switch (mode) {
    case 0: return 0xff000000u;
    case 1: return L;
    case 2: return T;
    case 3: return TR;
    case 4: return TL;
    case 5: return wd_avg(wd_avg(L, TR), T);
    case 6: return wd_avg(L, TL);
    case 7: return wd_avg(L, T);
    case 8: return wd_avg(TL, T);
    case 9: return wd_avg(T, TR);
    case 10: return wd_avg(wd_avg(L, TL), wd_avg(T, TR));
    case 11: {
      int dl = 0, dt = 0;
      for (int c = 0; c < 4; ++c) {
        const int a = wd_ch(T, c) - wd_ch(TL, c), b = wd_ch(L, c) - wd_ch(TL, c);
        dl += a < 0 ? -a : a, dt += b < 0 ? -b : b;
      }
      return dl < dt ? L : T;
    }
    case 12: {
      uint32_t r = 0u;
      for (int c = 0; c < 4; ++c) r |= (uint32_t)wd_clamp(wd_ch(L, c) + wd_ch(T, c) - wd_ch(TL, c)) << (8 * c);
      return r;
    }
    case 13: {
      const uint32_t a = wd_avg(L, T);
      uint32_t r = 0u;
      for (int c = 0; c < 4; ++c) r |= (uint32_t)wd_clamp(wd_ch(a, c) + (wd_ch(a, c) - wd_ch(TL, c)) / 2) << (8 * c);
      return r;
    }
    default: return 0xff000000u;
  }
}

WD_HD int wd_delta(uint32_t t, uint32_t c) { return ((int)(int8_t)(t & 255u) * (int)(int8_t)(c & 255u)) >> 5; }

// px (h rows of w words) in place.  Lane k owns row r0 + k of a band of 64 and is at pixel t - 2k at step t: the pixel above-right is what lane
// k - 1 produced one step ago (a shuffle), the pixels above and above-left are that value one and two steps later.  Lane 0 reads the row above, the
// last of the band before, from memory.
WD_WAVE void wd_unpredict(uint32_t* px, int w, int h, const uint32_t* modes, int bits) {
  const int bw = (w + (1 << bits) - 1) >> bits;
  for (int r0 = 0; r0 < h; r0 += 64) {
    uint32_t cur[WD_LANES], up[WD_LANES], tr[WD_LANES], tv[WD_LANES], tl[WD_LANES], first[WD_LANES];
    WD_BARRIER();
    WD_FOR_LANES(lane) {
      const int k = WD_LI(lane);
      cur[k] = up[k] = tr[k] = tv[k] = tl[k] = first[k] = 0u;
    }
    for (int t = -1; t < w + 126; ++t) {
      WD_SHUFFLE_UP(up, cur);
      WD_FOR_LANES(lane) {
        const int k = WD_LI(lane), row = r0 + lane, x = t - 2 * lane;
        if (row < h && x >= -1 && x < w) {
          uint32_t above_right = 0u;
          if (row > 0 && x + 1 < w) above_right = lane > 0 ? up[k] : px[(size_t)(row - 1) * w + x + 1];
          tl[k] = tv[k], tv[k] = tr[k], tr[k] = above_right;
          if (x >= 0) {
            uint32_t* p = px + (size_t)row * w + x;
            uint32_t pred;
            if (row == 0) pred = x == 0 ? 0xff000000u : cur[k];
            else if (x == 0) pred = tv[k];
            else pred = wd_predict((int)(modes[(size_t)(row >> bits) * bw + (x >> bits)] >> 8) & 15, cur[k], tv[k], tl[k], x + 1 < w ? tr[k] : first[k]);
            const uint32_t val = wd_add(*p, pred);
            *p = val;
            cur[k] = val;
            if (x == 0) first[k] = val;
          }
        }
      }
    }
  }
  WD_BARRIER();
}

// The frame's scratch (as wd_decode_stream left it) -> out: W * H ARGB words; palette: 256 words of shared memory.  Returns WD_OK, or
// WD_ST_UPSTREAM where the decode left no valid header block (nothing is written then).
WD_WAVE int wd_untransform_frame(uint32_t* palette, const long long* t, uint32_t* scratch, long long scratch_words, uint32_t* argb,
                                 long long argb_words) {
  if (!wd_row_ok(t, 1ll << 62, scratch_words, argb_words)) return WD_ST_DESCRIPTOR;
  uint32_t* scr = scratch + t[WD_SCR];
  const long long cap = t[WD_CAP];
  const int W = (int)t[WD_W], H = (int)t[WD_H];
  uint32_t* out = argb + t[WD_PIX];
  WD_BARRIER();
  if (WD_UNIFORM(scr[0]) != (unsigned)WD_MAGIC) return WD_ST_UPSTREAM;
  const int ntrans = (int)WD_UNIFORM(scr[1]), main_w = (int)WD_UNIFORM(scr[3]);
  const long long main_at = (long long)WD_UNIFORM(scr[2]);
  // the header block is the decode's own, but it is held to the frame's ranges all the same
  if (ntrans < 0 || ntrans > 4 || main_w < 1 || main_w > W || main_at < WD_HDR || main_at + (long long)main_w * H > cap) return WD_ST_UPSTREAM;
  uint32_t* cur = scr + main_at;
  int cw = main_w;
  for (int i = ntrans - 1; i >= 0; --i) {
    const uint32_t* e = scr + 4 + 5 * i;
    const int type = (int)WD_UNIFORM(e[0]), bits = (int)WD_UNIFORM(e[1]), w = (int)WD_UNIFORM(e[3]), n = (int)WD_UNIFORM(e[4]);
    const long long at = (long long)WD_UNIFORM(e[2]);
    const long long px = (long long)w * H;
    if (type == 2) {
      if (w != cw) return WD_ST_UPSTREAM;
      WD_FOR_LANES(lane) {
        for (long long p = lane; p < px; p += 64) {
          const uint32_t v = cur[p], g = (v >> 8) & 255u;
          cur[p] = (v & 0xff00ff00u) | (((v & 0x00ff00ffu) + (g << 16 | g)) & 0x00ff00ffu);
        }
      }
    } else if (type == 0 || type == 1) {
      const int bw = (w + (1 << bits) - 1) >> bits, bh = (H + (1 << bits) - 1) >> bits;
      if (w != cw || bits < 2 || bits > 9 || at < WD_HDR || at + (long long)bw * bh > cap) return WD_ST_UPSTREAM;
      const uint32_t* sub = scr + at;
      if (type == 0) {
        wd_unpredict(cur, w, H, sub, bits);
      } else {
        WD_FOR_LANES(lane) {
          for (long long p = lane; p < px; p += 64) {
            const int y = (int)(p / w), x = (int)(p - (long long)y * w);
            const uint32_t m = sub[(size_t)(y >> bits) * bw + (x >> bits)], v = cur[p];
            const uint32_t g = (v >> 8) & 255u;
            const uint32_t r = ((v >> 16) + (uint32_t)wd_delta(m, g)) & 255u;
            const uint32_t b = (v + (uint32_t)wd_delta(m >> 8, g) + (uint32_t)wd_delta(m >> 16, r)) & 255u;
            cur[p] = (v & 0xff00ff00u) | r << 16 | b;
          }
        }
      }
    } else {
      const int pw = (w + (1 << bits) - 1) >> bits;
      if (w != W || pw != cw || cur == out || n < 1 || n > 256 || bits < 0 || bits > 3 || at < WD_HDR || at + n > cap) return WD_ST_UPSTREAM;
      const uint32_t* sub = scr + at;
      WD_BARRIER();
      WD_FOR_LANES(lane) {
        if (lane == 0) {
          uint32_t acc = 0u;
          for (int k = 0; k < 256; ++k) palette[k] = k < n ? (acc = wd_add(acc, sub[k])) : 0u;
        }
      }
      WD_BARRIER();
      const int per = 8 >> bits, mask = (1 << per) - 1;
      WD_FOR_LANES(lane) {
        for (long long p = lane; p < px; p += 64) {
          const int y = (int)(p / w), x = (int)(p - (long long)y * w);
          const uint32_t packed = cur[(size_t)y * pw + (x >> bits)];
          out[p] = palette[((packed >> 8) >> ((x & ((1 << bits) - 1)) * per)) & (uint32_t)mask];
        }
      }
      cur = out, cw = w;
    }
    WD_BARRIER();
  }
  if (cw != W) return WD_ST_UPSTREAM;
  if (cur != out) {
    WD_FOR_LANES(lane) {
      for (long long p = lane; p < (long long)W * H; p += 64) out[p] = cur[p];
    }
  }
  return WD_OK;
}

// ---- composition -------------------------------------------------------------------------------------------------------------------------------------
// Canvas pixel p through the n frames of the call -> out[(f * H * W + p) * 3 ..]; carry (H * W words, R in the low byte, then G, B, A) is read unless
// row 0 is its file's first frame, and written at the end.  A row whose rectangle leaves the canvas or whose words leave argb draws nothing.
WD_HD void wd_compose_pixel(const long long* tab, int n, const uint32_t* argb, long long argb_words, uint32_t* carry, unsigned char* out, int H, int W,
                            long long p) {
  const int y = (int)(p / W), x = (int)(p - (long long)y * W);
  uint32_t c = (tab[WD_FLAGS] & WD_F_FIRST) ? 0u : carry[p];
  for (int f = 0; f < n; ++f) {
    const long long* t = tab + (size_t)f * WD_TAB;
    const int flags = (int)t[WD_FLAGS];
    const bool key = flags & (WD_F_KEY | WD_F_FIRST);
    const bool cleared = (flags & WD_F_PREV_DISPOSED) && x >= t[WD_PX] && x < t[WD_PX] + t[WD_PW] && y >= t[WD_PY] && y < t[WD_PY] + t[WD_PH];
    if (key || cleared) c = 0u;
    if (wd_row_ok(t, 1ll << 62, 1ll << 62, argb_words) && t[WD_X] + t[WD_W] <= W && t[WD_Y] + t[WD_H] <= H && x >= t[WD_X] && x < t[WD_X] + t[WD_W] &&
        y >= t[WD_Y] && y < t[WD_Y] + t[WD_H]) {
      const uint32_t s = argb[t[WD_PIX] + (long long)(y - t[WD_Y]) * t[WD_W] + (x - t[WD_X])];
      const uint32_t sa = s >> 24, sr = (s >> 16) & 255u, sg = (s >> 8) & 255u, sb = s & 255u;
      if ((flags & WD_F_BLEND) && !key && !cleared && sa != 255u) {
        if (sa != 0u) {
          const uint32_t da = c >> 24, fd = (da * (256u - sa)) >> 8, a = sa + fd, scale = (1u << 24) / a;
          const uint32_t r = (uint32_t)(((uint64_t)(sr * sa + (c & 255u) * fd) * scale) >> 24);
          const uint32_t g = (uint32_t)(((uint64_t)(sg * sa + ((c >> 8) & 255u) * fd) * scale) >> 24);
          const uint32_t b = (uint32_t)(((uint64_t)(sb * sa + ((c >> 16) & 255u) * fd) * scale) >> 24);
          c = (r & 255u) | (g & 255u) << 8 | (b & 255u) << 16 | a << 24;
        }
      } else {
        c = sr | sg << 8 | sb << 16 | sa << 24;
      }
    }
    unsigned char* o = out + ((size_t)f * H * W + (size_t)p) * 3;
    o[0] = (unsigned char)c, o[1] = (unsigned char)(c >> 8), o[2] = (unsigned char)(c >> 16);
  }
  carry[p] = c;
}
