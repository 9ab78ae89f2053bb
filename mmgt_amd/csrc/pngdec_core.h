// PNG decode (zlib inflate, scanline reconstruction, sample expansion), written once: csrc/pngdec.hip calls these functions from its three
// kernels and tools/pngdec_host_check.cpp from a host program, so the bytes a kernel produces can be checked without a GPU.  Nothing here touches
// memory outside the ranges its arguments name, whatever the compressed bytes hold: bad data ends in a status, not in a write, and every loop over
// the stream consumes at least one bit per iteration or stops.
//
// The inflate and the unfilter are written for ONE WAVE of 64 lanes per stream / frame.  Values that every lane computes alike (bit position, decoded
// symbol, output position) are plain variables; work that differs per lane stands in a PD_FOR_LANES(lane) { ... } body, and PD_BARRIER() separates a
// body that writes shared memory from one that reads what another lane wrote.  On the device a body runs once with lane = threadIdx.x and the barrier
// is __syncthreads() (a wait, the workgroup being one wave); in a host build the body is a loop over lanes 0 .. 63 and the barrier is the loop's end.
// A body therefore never reads what another lane writes in the same body.  Per-lane variables that live across a barrier are arrays of PD_LANES
// elements indexed by PD_LI(lane).
//
//  * pd_inflate_stream   one zlib-less deflate stream -> at most out_len bytes.  Compressed bytes are staged into a ring in shared memory with
//                        16-byte loads; the bit reader is the bit position alone (three aligned words of the ring give 64 bits); code tables are
//                        built in shared memory by the lanes together (canonical count / sorted-symbol arrays, and a first-level table of 10 / 8 / 7
//                        bits filled from them); the last 32 KB of output live in a shared window that is flushed with 16-byte stores.
//  * pd_unfilter_frame   rows skewed across lanes: lane k owns row r0 + k of a band of 64 and reconstructs pixel t - k at step t; the pixel above
//                        comes from lane k - 1 by a shuffle, the one up-left is last step's pixel above.  Adds up the two Adler-32 sums per row.
//  * pd_expand_pixel     one output pixel: sub-byte unpacking, grey scaling, palette lookup, alpha drop.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PD_HD __host__ __device__ inline
#define PD_WAVE __device__ inline
#define PD_FOR_LANES(lane) for (int lane = (int)threadIdx.x, pd_once_ = 1; pd_once_; pd_once_ = 0)
#define PD_BARRIER() __syncthreads()
#define PD_LANES 1
#define PD_LI(lane) 0
#define PD_SHUFFLE_UP(dst, src) (dst)[0] = __shfl_up((src)[0], 1, 64)
#define PD_ANY(flag) (__ballot((flag)[0] != 0) != 0ull)
// a value every lane holds alike, said so to the compiler (it then lives in scalar registers and branches on it are scalar branches)
#define PD_UNIFORM(x) ((unsigned)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define PD_HD inline
#define PD_WAVE inline
#define PD_FOR_LANES(lane) for (int lane = 0; lane < 64; ++lane)
#define PD_BARRIER() ((void)0)
#define PD_LANES 64
#define PD_LI(lane) (lane)
#define PD_SHUFFLE_UP(dst, src)                                   \
  do {                                                            \
    for (int l_ = 63; l_ > 0; --l_) (dst)[l_] = (src)[l_ - 1];    \
    (dst)[0] = (src)[0];                                          \
  } while (0)
#define PD_ANY(flag) pd_any_host(flag)
#define PD_UNIFORM(x) ((unsigned)(x))
inline bool pd_any_host(const int* flag) {
  for (int l = 0; l < 64; ++l)
    if (flag[l]) return true;
  return false;
}
#endif

// status words: per stream (inflate), per frame (unfilter: PD_ST_FILTER, expand: PD_ST_PALETTE)
enum {
  PD_OK = 0,
  PD_ST_OVERSUBSCRIBED = 1,  // a code with more codes of some length than that length holds
  PD_ST_INCOMPLETE = 2,      // an incomplete code, where zlib refuses it (all but a distance or literal/length code of one length-1 code or none)
  PD_ST_SYMBOL = 3,          // an invalid symbol: literal/length 286 / 287, distance 30 / 31, or bits that are no code of the table
  PD_ST_DISTANCE = 4,        // a distance beyond the bytes produced
  PD_ST_STORED = 5,          // a stored block whose LEN and NLEN do not match
  PD_ST_EXHAUSTED = 6,       // data exhausted before the final block's end
  PD_ST_TOO_LONG = 7,        // more output than the frame holds
  PD_ST_TOO_SHORT = 8,       // the stream ends before the frame is full
  PD_ST_REPEAT = 9,          // a code-length repeat without a previous length, or running past the lengths the header announced
  PD_ST_COUNTS = 10,         // more than 286 literal/length or 30 distance codes announced
  PD_ST_NO_EOB = 11,         // the literal/length code has no end-of-block symbol
  PD_ST_BLOCK_TYPE = 12,     // block type 3
  PD_ST_DESCRIPTOR = 13,     // the stream's byte range lies outside the batch: nothing was read
  PD_ST_FILTER = 14,         // a scanline's filter type above 4
  PD_ST_PALETTE = 15,        // a palette index beyond the frame's PLTE
  PD_ST_LAST = 15
};

enum {
  PD_WIN = 32768,            // the deflate window; a power of two and a multiple of 16
  PD_RING = 4096,            // staged compressed bytes
  PD_FLUSH = 16384,          // unflushed output at which the window is flushed; PD_FLUSH + 258 + 16 <= PD_WIN
  PD_FAST_LL = 10,
  PD_FAST_D = 8,
  PD_FAST_CL = 7,
  PD_MAX_SIDE = 16384
};

struct PdShared {
  alignas(16) uint32_t window[PD_WIN / 4];
  alignas(16) uint32_t ring[PD_RING / 4];
  unsigned short lut_ll[1 << PD_FAST_LL], lut_d[1 << PD_FAST_D], lut_cl[1 << PD_FAST_CL];       // (symbol << 4 | length), 0: not a code of <= fast bits
  unsigned short sym_ll[288], sym_d[32], sym_cl[20];                                            // symbols sorted by (length, symbol)
  unsigned short cnt_ll[16], cnt_d[16], cnt_cl[16];                                             // codes per length; [0] is 0
  unsigned char lens[288 + 32];                                                                 // literal/length lengths, then the distance lengths
  unsigned char cl_lens[20];
};

// ---- canonical Huffman decode ------------------------------------------------------------------------------------------------------------------
// The code whose bits are `bits` (first bit in bit 0), looking at no more than maxbits of them: (symbol << 4 | length), 0 if none.
PD_HD unsigned pd_canon(const unsigned short* cnt, const unsigned short* sym, uint64_t bits, int maxbits) {
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

enum { PD_KIND_CL = 0, PD_KIND_LL = 1, PD_KIND_D = 2 };

// lens[0 .. n) -> cnt, sym, lut.  Lane l (1 .. 15) counts and then places the symbols of length l; all lanes fill the first-level table.
PD_WAVE int pd_build(const unsigned char* lens, int n, unsigned short* cnt, unsigned short* sym, unsigned short* lut, int fast, int kind) {
  PD_BARRIER();
  PD_FOR_LANES(lane) {
    if (lane < 16) {
      int c = 0;
      for (int s = 0; s < n; ++s) c += lens[s] == lane;
      cnt[lane] = (unsigned short)(lane ? c : 0);
    }
  }
  PD_BARRIER();
  int left = 1, total = 0;
  for (int l = 1; l < 16; ++l) {
    left = (left << 1) - (int)cnt[l];
    if (left < 0) return PD_ST_OVERSUBSCRIBED;
    total += cnt[l];
  }
  if (left > 0) {                                                  // zlib's inflate_table: incomplete only as one length-1 code or none, never CL
    const bool single = total == 0 || (total == 1 && cnt[1] == 1);
    if (kind == PD_KIND_CL || !single) return PD_ST_INCOMPLETE;
  }
  PD_FOR_LANES(lane) {
    if (lane >= 1 && lane < 16) {
      int o = 0;
      for (int l = 1; l < lane; ++l) o += cnt[l];
      for (int s = 0; s < n; ++s)
        if (lens[s] == lane) sym[o++] = (unsigned short)s;
    }
  }
  PD_BARRIER();
  PD_FOR_LANES(lane) {
    for (int i = lane; i < (1 << fast); i += 64) lut[i] = (unsigned short)pd_canon(cnt, sym, (uint64_t)i, fast);
  }
  PD_BARRIER();
  return PD_OK;
}

// ---- bit reader and staging -----------------------------------------------------------------------------------------------------------------------
// Positions are bits / bytes of the whole batch buffer `data` (data_bytes a multiple of 16, the pointer 16-byte aligned).  The ring holds the bytes
// [rbase, rbase + PD_RING), rbase a multiple of 16; bytes at or past the stream's end are zeros.
struct PdIn {
  const unsigned char* data;
  long long data_bytes, begin, end, rbase, gbit;
};

PD_WAVE void pd_stage(PdShared* sh, PdIn* in) {
  in->rbase = (in->gbit >> 3) & ~15ll;
  PD_BARRIER();
  PD_FOR_LANES(lane) {
    for (int v = lane; v < PD_RING / 16; v += 64) {
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
  PD_BARRIER();
}

// 64 bits from in->gbit on (12 bytes of the ring)
PD_WAVE uint64_t pd_peek(PdShared* sh, PdIn* in) {
  const long long byte0 = (in->gbit >> 5) << 2;
  if (byte0 < in->rbase || byte0 + 12 > in->rbase + PD_RING) pd_stage(sh, in);
  const int w = (int)(((in->gbit >> 5) << 2) - in->rbase) >> 2;
  const uint32_t w0 = PD_UNIFORM(sh->ring[w]), w1 = PD_UNIFORM(sh->ring[w + 1]), w2 = PD_UNIFORM(sh->ring[w + 2]);
  const int s = (int)(in->gbit & 31);
  uint64_t v = ((uint64_t)w1 << 32 | w0) >> s;
  if (s) v |= (uint64_t)w2 << (64 - s);
  return v;
}

// ---- output window -----------------------------------------------------------------------------------------------------------------------------------
// Output byte p lives in window slot (p + shift) & (PD_WIN - 1), shift = the low four bits of the frame's byte offset in the output buffer, so that a
// 16-byte store to the (16-byte aligned) buffer reads an aligned 16 bytes of the window.
struct PdOut {
  unsigned char* out;        // the frame's first byte
  int out_len, shift, pos, flushed;
};

PD_HD int pd_slot(const PdOut* o, int p) { return (p + o->shift) & (PD_WIN - 1); }

// bytes [flushed, to) of the window -> out; every byte is stored once over the calls, by exactly one lane
PD_WAVE void pd_flush(PdShared* sh, PdOut* o, int to) {
  const int from = o->flushed;
  if (to <= from) return;
  const unsigned char* win = (const unsigned char*)sh->window;
  int head = from + ((16 - ((from + o->shift) & 15)) & 15);
  if (head > to) head = to;
  const int nv = (to - head) >> 4, tail = head + 16 * nv;
  PD_BARRIER();
  PD_FOR_LANES(lane) {
    if (from + lane < head) o->out[from + lane] = win[pd_slot(o, from + lane)];
    for (int k = lane; k < nv; k += 64) {
      const int p = head + 16 * k;
      uint32_t q[4];
      memcpy(q, __builtin_assume_aligned(win + pd_slot(o, p), 16), 16);
      memcpy(__builtin_assume_aligned(o->out + p, 16), q, 16);
    }
    if (tail + lane < to) o->out[tail + lane] = win[pd_slot(o, tail + lane)];
  }
  PD_BARRIER();
  o->flushed = to;
}

PD_WAVE void pd_flush_if_due(PdShared* sh, PdOut* o) {
  if (o->pos - o->flushed >= PD_FLUSH) pd_flush(sh, o, o->pos - ((o->pos + o->shift) & 15));
}

// RFC 1951 3.2.5
PD_HD void pd_length_code(int sym, int* base, int* extra) {
  const int k = sym - 257;
  if (k < 8) *base = 3 + k, *extra = 0;
  else if (k == 28) *base = 258, *extra = 0;
  else *extra = (k - 4) >> 2, *base = 3 + ((4 + (k & 3)) << *extra);
}
PD_HD void pd_distance_code(int sym, int* base, int* extra) {
  if (sym < 4) *base = 1 + sym, *extra = 0;
  else *extra = (sym >> 1) - 1, *base = 1 + ((2 + (sym & 1)) << *extra);
}

// ---- the blocks ----------------------------------------------------------------------------------------------------------------------------------------
PD_WAVE int pd_stored_block(PdShared* sh, PdIn* in, PdOut* o, long long* steps) {
  in->gbit = (in->gbit + 7) & ~7ll;
  const uint64_t v = pd_peek(sh, in);
  int len = (int)(v & 0xffffu);
  const int nlen = (int)((v >> 16) & 0xffffu);
  in->gbit += 32;
  if (in->gbit > 8 * in->end) return PD_ST_EXHAUSTED;
  if ((len ^ nlen) != 0xffff) return PD_ST_STORED;
  if ((in->gbit >> 3) + len > in->end) return PD_ST_EXHAUSTED;
  if (len > o->out_len - o->pos) return PD_ST_TOO_LONG;
  unsigned char* win = (unsigned char*)sh->window;
  while (len > 0) {
    ++*steps;
    pd_flush_if_due(sh, o);
    const long long at = in->gbit >> 3;
    if (at < in->rbase || at + 12 > in->rbase + PD_RING) pd_stage(sh, in);
    int chunk = (int)(in->rbase + PD_RING - at);                   // >= 12
    if (chunk > len) chunk = len;
    if (chunk > PD_WIN - PD_FLUSH - 32) chunk = PD_WIN - PD_FLUSH - 32;
    const int r0 = (int)(at - in->rbase);
    PD_FOR_LANES(lane) {
      for (int i = lane; i < chunk; i += 64) win[pd_slot(o, o->pos + i)] = (unsigned char)(sh->ring[(r0 + i) >> 2] >> (8 * ((r0 + i) & 3)));
    }
    PD_BARRIER();
    o->pos += chunk;
    in->gbit += 8ll * chunk;
    len -= chunk;
  }
  return PD_OK;
}

PD_WAVE int pd_dynamic_header(PdShared* sh, PdIn* in, int* hlit_out, int* hdist_out, long long* steps) {
  uint64_t v = pd_peek(sh, in);
  const int hlit = (int)(v & 31u) + 257, hdist = (int)((v >> 5) & 31u) + 1, hclen = (int)((v >> 10) & 15u) + 4;
  in->gbit += 14;
  if (hlit > 286 || hdist > 30) return PD_ST_COUNTS;
  v = pd_peek(sh, in);                                             // 19 * 3 = 57 bits at most
  PD_BARRIER();
  PD_FOR_LANES(lane) {
    if (lane < 19) {
      constexpr unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      sh->cl_lens[order[lane]] = (unsigned char)(lane < hclen ? (v >> (3 * lane)) & 7u : 0u);
    }
  }
  in->gbit += 3 * hclen;
  if (in->gbit > 8 * in->end) return PD_ST_EXHAUSTED;
  int st = pd_build(sh->cl_lens, 19, sh->cnt_cl, sh->sym_cl, sh->lut_cl, PD_FAST_CL, PD_KIND_CL);
  if (st) return st;
  const int total = hlit + hdist;
  int n = 0, prev = 0;
  while (n < total) {
    ++*steps;
    v = pd_peek(sh, in);
    const unsigned e = PD_UNIFORM(sh->lut_cl[v & ((1u << PD_FAST_CL) - 1u)]);
    if (!e) return PD_ST_SYMBOL;
    const int s = (int)(e >> 4), l = (int)(e & 15u);
    int used = l, rep = 1, val = s;
    if (s == 16) {
      if (n == 0) return PD_ST_REPEAT;
      rep = 3 + (int)((v >> l) & 3u), val = prev, used += 2;
    } else if (s == 17) {
      rep = 3 + (int)((v >> l) & 7u), val = 0, used += 3;
    } else if (s == 18) {
      rep = 11 + (int)((v >> l) & 127u), val = 0, used += 7;
    }
    if (in->gbit + used > 8 * in->end) return PD_ST_EXHAUSTED;
    if (n + rep > total) return PD_ST_REPEAT;
    PD_FOR_LANES(lane) {
      for (int i = lane; i < rep; i += 64) sh->lens[n + i] = (unsigned char)val;
    }
    n += rep;
    prev = val;
    in->gbit += used;
  }
  PD_BARRIER();
  if (sh->lens[256] == 0) return PD_ST_NO_EOB;
  *hlit_out = hlit, *hdist_out = hdist;
  return PD_OK;
}

PD_WAVE int pd_coded_block(PdShared* sh, PdIn* in, PdOut* o, long long* steps) {
  unsigned char* win = (unsigned char*)sh->window;
  for (;;) {
    ++*steps;
    pd_flush_if_due(sh, o);
    const uint64_t v = pd_peek(sh, in);
    unsigned e;
    {                                                              // up to four literals of the first-level table (40 bits at most) from one peek
      uint64_t w = v;
      unsigned lits = 0u;
      int nlit = 0, bits = 0;
      for (;;) {
        e = PD_UNIFORM(sh->lut_ll[w & ((1u << PD_FAST_LL) - 1u)]);
        if (!e || (e >> 4) >= 256u || nlit == 4) break;
        lits |= (e >> 4) << (8 * nlit);
        ++nlit;
        bits += (int)(e & 15u);
        w >>= (e & 15u);
      }
      if (nlit) {
        if (in->gbit + bits > 8 * in->end) return PD_ST_EXHAUSTED;
        if (nlit > o->out_len - o->pos) return PD_ST_TOO_LONG;
        PD_FOR_LANES(lane) {
          if (lane < nlit) win[pd_slot(o, o->pos + lane)] = (unsigned char)(lits >> (8 * lane));
        }
        o->pos += nlit;
        in->gbit += bits;
        continue;
      }
    }
    if (!e) e = PD_UNIFORM(pd_canon(sh->cnt_ll, sh->sym_ll, v, 15));
    if (!e) return PD_ST_SYMBOL;
    const int sym = (int)(e >> 4);
    int used = (int)(e & 15u);
    if (sym < 256) {
      if (in->gbit + used > 8 * in->end) return PD_ST_EXHAUSTED;
      if (o->pos >= o->out_len) return PD_ST_TOO_LONG;
      PD_FOR_LANES(lane) {
        if (lane == 0) win[pd_slot(o, o->pos)] = (unsigned char)sym;
      }
      o->pos += 1;
      in->gbit += used;
      continue;
    }
    if (sym == 256) {
      if (in->gbit + used > 8 * in->end) return PD_ST_EXHAUSTED;
      in->gbit += used;
      return PD_OK;
    }
    if (sym > 285) return PD_ST_SYMBOL;
    int base, extra;
    pd_length_code(sym, &base, &extra);
    const int len = base + (int)((v >> used) & ((1u << extra) - 1u));
    used += extra;
    unsigned d = PD_UNIFORM(sh->lut_d[(v >> used) & ((1u << PD_FAST_D) - 1u)]);
    if (!d) d = PD_UNIFORM(pd_canon(sh->cnt_d, sh->sym_d, v >> used, 15));
    if (!d) return PD_ST_SYMBOL;
    const int dsym = (int)(d >> 4);
    used += (int)(d & 15u);
    if (dsym > 29) return PD_ST_SYMBOL;
    pd_distance_code(dsym, &base, &extra);
    const int dist = base + (int)((v >> used) & ((1u << extra) - 1u));
    used += extra;                                                 // 15 + 5 + 15 + 13 = 48 bits at most
    if (in->gbit + used > 8 * in->end) return PD_ST_EXHAUSTED;
    if (dist > o->pos) return PD_ST_DISTANCE;
    if (len > o->out_len - o->pos) return PD_ST_TOO_LONG;
    // byte i of the match is output byte pos - dist + (i mod dist): all reads lie before pos, so every lane reads first and writes after
    unsigned char mv[PD_LANES][5];
    PD_BARRIER();
    PD_FOR_LANES(lane) {
#pragma unroll
      for (int r = 0; r < 5; ++r) {                                // 258 bytes at most: five rounds of 64
        const int i = 64 * r + lane;
        if (i < len) mv[PD_LI(lane)][r] = win[pd_slot(o, o->pos - dist + (dist >= len ? i : i % dist))];
      }
    }
    PD_BARRIER();
    PD_FOR_LANES(lane) {
#pragma unroll
      for (int r = 0; r < 5; ++r) {
        const int i = 64 * r + lane;
        if (i < len) win[pd_slot(o, o->pos + i)] = mv[PD_LI(lane)][r];
      }
    }
    o->pos += len;
    in->gbit += used;
  }
}

// Stream s of the batch: data[offsets[s], offsets[s + 1]) -> out[0, out_len); returns the status.  *steps counts loop iterations (at most one per
// consumed bit plus one per 12 stored bytes plus a few per block).
PD_WAVE int pd_inflate_stream(PdShared* sh, const unsigned char* data, long long data_bytes, long long begin, long long end, unsigned char* out,
                              int out_len, int shift, long long* steps) {
  *steps = 0;
  if (begin < 0 || end < begin || end > data_bytes) return PD_ST_DESCRIPTOR;
  PdIn in{data, data_bytes, begin, end, 0, 8 * begin};
  PdOut o{out, out_len, shift & 15, 0, 0};
  pd_stage(sh, &in);
  int st = PD_OK;
  for (;;) {
    ++*steps;
    const uint64_t v = pd_peek(sh, &in);
    const int final = (int)(v & 1u), type = (int)((v >> 1) & 3u);
    in.gbit += 3;
    if (in.gbit > 8 * in.end) {
      st = PD_ST_EXHAUSTED;
      break;
    }
    if (type == 0) {
      st = pd_stored_block(sh, &in, &o, steps);
    } else if (type == 3) {
      st = PD_ST_BLOCK_TYPE;
    } else {
      int hlit = 288, hdist = 32;
      if (type == 1) {
        PD_BARRIER();
        PD_FOR_LANES(lane) {
          for (int s = lane; s < 320; s += 64) sh->lens[s] = (unsigned char)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
        }
      } else {
        st = pd_dynamic_header(sh, &in, &hlit, &hdist, steps);
      }
      if (!st) st = pd_build(sh->lens, hlit, sh->cnt_ll, sh->sym_ll, sh->lut_ll, PD_FAST_LL, PD_KIND_LL);
      if (!st) st = pd_build(sh->lens + hlit, hdist, sh->cnt_d, sh->sym_d, sh->lut_d, PD_FAST_D, PD_KIND_D);
      if (!st) st = pd_coded_block(sh, &in, &o, steps);
    }
    if (st || final) break;
  }
  pd_flush(sh, &o, o.pos);                                         // what was produced is in range whatever the status
  if (!st && o.pos < o.out_len) st = PD_ST_TOO_SHORT;
  return st;
}

// ---- geometry ----------------------------------------------------------------------------------------------------------------------------------------
struct PdGeom {
  int H, W, ct, depth;
  int bits;      // per pixel
  int bpp;       // the filters' pixel in bytes: 1 for sub-byte depths
  int rowbytes;  // without the filter type byte
  int stride;    // with it
};

PD_HD bool pd_geom(int H, int W, int ct, int depth, PdGeom* g) {
  if (H < 1 || W < 1 || H > PD_MAX_SIDE || W > PD_MAX_SIDE) return false;
  const bool sub = depth == 1 || depth == 2 || depth == 4;
  int ch;
  if (ct == 0 || ct == 3) {
    if (!sub && depth != 8) return false;
    ch = 1;
  } else if (ct == 2 || ct == 4 || ct == 6) {
    if (depth != 8) return false;
    ch = ct == 2 ? 3 : ct == 4 ? 2 : 4;
  } else {
    return false;
  }
  g->H = H, g->W = W, g->ct = ct, g->depth = depth;
  g->bits = ch * depth;
  g->bpp = g->bits >= 8 ? g->bits / 8 : 1;
  g->rowbytes = (int)(((long long)W * g->bits + 7) / 8);
  g->stride = 1 + g->rowbytes;
  return true;
}
PD_HD long long pd_frame_bytes(const PdGeom& g) { return (long long)g.H * g.stride; }

// ---- scanline reconstruction --------------------------------------------------------------------------------------------------------------------------
PD_HD int pd_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
PD_HD int pd_predict(int type, int a, int b, int c) {
  return type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : pd_paeth(a, b, c);
}

// One frame's filtered bytes (H, stride), reconstructed in place; sums[2 * row + {0, 1}] = { sum d[i], sum (stride - i) d[i] } over the row's
// FILTERED bytes d[0 .. stride), the type byte included.  Returns 0 or PD_ST_FILTER (a row of a type above 4 is taken as type 0).  A band's last
// row is read back by lane 0 of the next band from where lane 63 stored it.
PD_WAVE int pd_unfilter_frame(unsigned char* fr, long long* sums, const PdGeom& g) {
  const int bpp = g.bpp, npx = g.rowbytes / bpp, L = g.stride;
  int bad[PD_LANES];
  PD_FOR_LANES(lane) { bad[PD_LI(lane)] = 0; }
  for (int r0 = 0; r0 < g.H; r0 += 64) {
    int ft[PD_LANES];
    uint32_t a[PD_LANES], last[PD_LANES], bprev[PD_LANES], up[PD_LANES];
    unsigned long long s1[PD_LANES], s2[PD_LANES];
    PD_BARRIER();
    PD_FOR_LANES(lane) {
      const int k = PD_LI(lane), row = r0 + lane;
      int t = row < g.H ? fr[(size_t)row * L] : 0;
      s1[k] = (unsigned)t, s2[k] = (unsigned long long)L * (unsigned)t;
      if (t > 4) bad[k] = 1, t = 0;
      ft[k] = t, a[k] = 0u, last[k] = 0u, bprev[k] = 0u, up[k] = 0u;
    }
    for (int t = 0; t < npx + 63; ++t) {
      PD_SHUFFLE_UP(up, last);
      PD_FOR_LANES(lane) {
        const int k = PD_LI(lane), row = r0 + lane, x = t - lane;
        if (row < g.H && x >= 0 && x < npx) {
          unsigned char* p = fr + (size_t)row * L + 1 + (size_t)x * bpp;
          uint32_t b = 0u;
          if (row > 0) {
            if (lane > 0) {
              b = up[k];
            } else {
              const unsigned char* q = p - L;
              for (int j = 0; j < bpp; ++j) b |= (uint32_t)q[j] << (8 * j);
            }
          }
          const uint32_t c = x > 0 ? bprev[k] : 0u;
          uint32_t rec = 0u;
          for (int j = 0; j < bpp; ++j) {
            const int d = p[j];
            s1[k] += (unsigned)d;
            s2[k] += (unsigned long long)(L - 1 - x * bpp - j) * (unsigned)d;
            const int v = (d + pd_predict(ft[k], (int)(a[k] >> (8 * j) & 255u), (int)(b >> (8 * j) & 255u), (int)(c >> (8 * j) & 255u))) & 255;
            p[j] = (unsigned char)v;
            rec |= (uint32_t)v << (8 * j);
          }
          a[k] = rec, last[k] = rec, bprev[k] = b;
        }
      }
    }
    PD_FOR_LANES(lane) {
      const int k = PD_LI(lane), row = r0 + lane;
      if (row < g.H) sums[2 * (size_t)row] = (long long)s1[k], sums[2 * (size_t)row + 1] = (long long)s2[k];
    }
  }
  PD_BARRIER();
  return PD_ANY(bad) ? PD_ST_FILTER : PD_OK;
}

// ---- expansion ----------------------------------------------------------------------------------------------------------------------------------------
// Output pixel p of the batch -> out[3 p ..]; PIL's Image.convert("RGB"): grey of 1 / 2 / 4 bits scaled by 255 / 85 / 17, alpha dropped, palette
// entries copied (palette: 768 bytes per frame).  Returns 0, or PD_ST_PALETTE for an index at or past plte_len[frame] (the pixel is then black).
PD_HD int pd_expand_pixel(const unsigned char* filt, const unsigned char* palette, const int* plte_len, unsigned char* out, const PdGeom& g,
                          long long p) {
  const long long per = (long long)g.H * g.W;
  const long long f = p / per, rem = p - f * per;
  const int y = (int)(rem / g.W), x = (int)(rem - (long long)y * g.W);
  const unsigned char* row = filt + (size_t)(f * g.H + y) * g.stride + 1;
  int r, gg, b, st = PD_OK;
  if (g.ct == 2 || g.ct == 6) {
    const unsigned char* q = row + (size_t)x * g.bpp;
    r = q[0], gg = q[1], b = q[2];
  } else {
    int v;
    if (g.ct == 4) {
      v = row[2 * (size_t)x];
    } else if (g.depth == 8) {
      v = row[x];
    } else {
      const int bit = x * g.depth;                                 // < 16384 * 4
      v = (row[bit >> 3] >> (8 - g.depth - (bit & 7))) & ((1 << g.depth) - 1);
    }
    if (g.ct == 3) {
      if (v >= plte_len[f]) {
        r = gg = b = 0, st = PD_ST_PALETTE;
      } else {
        const unsigned char* q = palette + (size_t)f * 768 + 3 * v;
        r = q[0], gg = q[1], b = q[2];
      }
    } else {
      if (g.depth < 8) v *= g.depth == 1 ? 255 : g.depth == 2 ? 85 : 17;
      r = gg = b = v;
    }
  }
  unsigned char* o = out + 3 * (size_t)p;
  o[0] = (unsigned char)r, o[1] = (unsigned char)gg, o[2] = (unsigned char)b;
  return st;
}
