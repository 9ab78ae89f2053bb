// The strip coder that the PNG writer (csrc/png.hip) and the WebP lossless writer (csrc/webp.hip) share.  Both cut a row of
// elements (filtered bytes, residual ARGB words) into strips, turn a strip into literals and matches from the element before, count the tokens'
// symbols (histogram mode), let the host build prefix codes and with them every strip's exact bit count, and then code the strip into a slot of
// exactly that many 32-bit words (emit mode).  What differs between the two is a codec trait; everything else is written here, once.
//
// Tokens.  At position p >= 1 let r = elements from p on that equal element p - 1, at most kMaxLen: r >= 3 is a match of length r, else element p is
// a literal; position 0 is a literal.  That greedy parse has a closed form: in a maximal run of equal elements the first is a literal and the k
// elements after it fall into blocks of kMaxLen (the last one shorter), a block of 3 or more being one match and one of 1 or 2 literals.  A token is
// credited to the position where it ENDS, so that a position needs only the start of its run (a max-scan over the positions before it) and the two
// elements after it: see sc_token_at.
//
// The walker (sc_walk_strip).  One workgroup of 256 threads per strip walks it 256 positions a round.  A round: a max-scan gives every position the
// start of its run (carry_s hands the last position's on to the next round); the codec names the token that ends there; in histogram mode the codec
// counts it into its table and that is all.  In emit mode the codec turns the token into one or two bit fields, an add-scan over their widths gives
// every token its bit position, the fields are ORed (atomicOr) into a window of LDS words whose first word is the partly filled word the round
// before left, the full words of the window are stored to the slot and the partly filled last one is carried on; after the last round thread 0
// stores it.  So every word of a slot is written once, with plain stores, and nothing is written outside the slot: its two offsets are clamped to
// the buffer whatever the caller's table holds, and every store is checked against the slot's size.
//
// Widths.  A field is clamped to 32 bits and a token that would leave the window is not placed, whatever the code table holds; the table comes from
// the caller and only its shape is checked on the way in.  With prefix codes of at most 15 bits a token takes at most Codec::kTokenBits bits (21 for
// PNG, 45 for WebP), a round at most 256 of them behind the 31 carried bits, and the window is sized for exactly that: on tables the host built
// neither check ever triggers and the bytes are those of the unclamped arithmetic.
//
// The host/device part below is plain C++ (tools/webp_host_check.cpp runs it under ASan and UBSan); the device part needs hipcc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SC_HD __host__ __device__ inline
#else
#define SC_HD inline
#endif

enum {
  SC_LITERAL = 0,              // sc_token_at: element p is a literal
  SC_NONE = -1                 // sc_token_at: no token ends at p
};

// The view of a strip that the tokens need: does element q (1 <= q < len) equal the element before it?
template <typename T>
struct ScSameAsBefore {
  const T* src;
  SC_HD bool operator()(int q) const { return src[q] == src[q - 1]; }
};

// The token that ends at position p of a strip of len elements: SC_NONE, SC_LITERAL (element p itself) or the length 3 .. kMaxLen of a match from
// the element before.  run_start = the last position q <= p that is 0 or whose element differs from element q - 1.  With m = (p - run_start - 1) mod
// kMaxLen: m = kMaxLen - 1 ends a match of kMaxLen; a run ending at p ends a match of m + 1 if that is 3 or more, else p is a literal; and m = 0 in
// a run that goes on for one element only is the first of two literals.  `same` is asked about positions p + 1 and p + 2 only, and only inside the
// strip.
template <int kMaxLen, typename Same>
SC_HD int sc_token_at(Same same, int p, int len, int run_start) {
  if (p == run_start) return SC_LITERAL;
  const int m = (p - run_start - 1) % kMaxLen;
  if (m == kMaxLen - 1) return kMaxLen;
  const bool c1 = p + 1 < len && same(p + 1);
  if (!c1) return m >= 2 ? m + 1 : SC_LITERAL;
  const bool c2 = p + 2 < len && same(p + 2);
  return (m == 0 && !c2) ? SC_LITERAL : SC_NONE;
}

// What the strip kernels take: n >= 1 rows of 1 .. max_len elements in strips of at least one, n * strips a grid size.  SC_BAD_STRIPS is the
// message for (the function's name, n, frame_len, strip_len).
inline bool sc_strips_ok(int n, long long frame_len, long long strip_len, long long max_len) {
  if (n < 1 || frame_len < 1 || frame_len > max_len || strip_len < 1) return false;
  const long long strips = (frame_len + strip_len - 1) / strip_len;
  return n * strips <= 0x7fffffffll;
}
#define SC_BAD_STRIPS(elements, unit, max_len)                                                                                        \
  "%s: n = %d rows of %lld " elements " in strips of %lld are outside the range (n >= 1, 1 <= strip_" unit ", 1 <= frame_" unit " <= " \
  max_len ", n * strips < 2^31)"

#if defined(__HIPCC__)
constexpr int kScThreads = 256;

// Inclusive scans over the workgroup's 256 threads (4 waves): within a wave by shuffles, then the totals of the waves before through LDS.  Both end
// with every thread past the barrier that guards part_s, so they can be called back to back.
__device__ __forceinline__ int block_scan_max(int v, int* part_s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v = max(v, o);
  }
  if (lane == 63) part_s[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v = max(v, part_s[w]);
  __syncthreads();
  return v;
}
__device__ __forceinline__ int block_scan_add(int v, int* part_s, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  if (lane == 63) part_s[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += part_s[w];
  *total = part_s[0] + part_s[1] + part_s[2] + part_s[3];
  __syncthreads();
  return v;
}

// ORs the low nb <= 32 bits of v into the window at bit position at.
__device__ __forceinline__ void put_bits(unsigned* w_s, int at, unsigned long long v, int nb) {
  if (nb <= 0) return;
  const unsigned long long sh = v << (at & 31);                    // nb <= 32 and at & 31 <= 31: fits
  atomicOr(&w_s[at >> 5], (unsigned)sh);
  if ((unsigned)(sh >> 32)) atomicOr(&w_s[(at >> 5) + 1], (unsigned)(sh >> 32));
}

// Words [lo, lo + cap) of a buffer of `words` words, from the two offsets a table names: clamped to the buffer whatever the table holds.
struct ScSlot {
  long long lo, cap;
};
__device__ __forceinline__ ScSlot sc_slot(long long lo, long long hi, long long words) {
  long long cap = hi - lo;
  if (lo < 0 || lo > words) lo = words;
  return {lo, max(0ll, min(cap, words - lo))};
}

// A token's bits, LSB-first: v0's low n0, then v1's low n1.
struct ScFields {
  unsigned long long v0 = 0, v1 = 0;
  int n0 = 0, n1 = 0;
};

// Walks one strip: the workgroup's strip is src[0 .. len), tab_s the codec's table in LDS (zeroed for histogram mode, the code table for emit mode;
// the caller fills it and reads the histogram back after the call, which ends behind a barrier).  Emit mode writes the strip's slot, the words
// slot_off[0] .. slot_off[1] of slots: the first front_bits bits of `front` (none if 0), then the tokens' bits; and the bit count to *bits.
//
// A Codec has: Elem, the element type; kTokenBits, the most bits of a token with codes of up to 15 bits; kTail, 1 if a token stands at position len
// behind the strip (an end symbol), else 0; token(src, p, len, run_start) for 0 <= p < len + kTail, negative if no token ends at p;
// count(tab_s, tok, src, p), which adds a token to the histogram with atomicAdd; fields(tab_s, tok, src, p), a token's ScFields under the table.
template <bool kEmit, typename Codec>
__device__ __forceinline__ void sc_walk_strip(const typename Codec::Elem* __restrict__ src, int len, unsigned* tab_s, const unsigned* __restrict__ front,
                                              int front_bits, unsigned* __restrict__ slots, const long long* __restrict__ slot_off, long long slots_words,
                                              long long* __restrict__ bits) {
  constexpr int kChunkWords = (kScThreads * Codec::kTokenBits + 31) / 32 + 2;   // the carried partial word in front, one word for a token straddling the end
  __shared__ unsigned w_s[kChunkWords];
  __shared__ int part_s[4];
  __shared__ int carry_s;
  const int t = threadIdx.x;
  const ScSameAsBefore<typename Codec::Elem> same = {src};

  ScSlot slot = {0, 0};
  long long bitpos = 0;
  unsigned carry = 0u;                                             // the bits of the word that bitpos lies in
  if (kEmit) {
    slot = sc_slot(slot_off[0], slot_off[1], slots_words);
    for (int i = t; i < front_bits / 32; i += kScThreads)
      if (i < slot.cap) slots[slot.lo + i] = front[i];
    if (front_bits & 31) carry = front[front_bits / 32] & ((1u << (front_bits & 31)) - 1u);
    bitpos = front_bits;
  }
  if (t == 0) carry_s = -1;
  __syncthreads();

  for (int base = 0; base < len + Codec::kTail; base += kScThreads) {
    const int p = base + t;
    const bool valid = p < len + Codec::kTail;
    const bool boundary = p < len && (p == 0 || !same(p));
    if (kEmit) {
      for (int i = t; i < kChunkWords; i += kScThreads) w_s[i] = i == 0 ? carry : 0u;
    }
    const int run_start = max(block_scan_max(boundary ? p : -1, part_s), carry_s);
    const int tok = valid ? Codec::token(src, p, len, run_start) : -1;
    if (!kEmit) {
      if (tok >= 0) Codec::count(tab_s, tok, src, p);
      __syncthreads();                                             // carry_s is read above by every thread before it is rewritten
    } else {
      ScFields f;
      if (tok >= 0) f = Codec::fields(tab_s, tok, src, p);
      const int n0 = min(f.n0, 32), n1 = min(f.n1, 32);            // see "Widths" above
      int total;
      const int end = block_scan_add(n0 + n1, part_s, &total);
      const int off0 = (int)(bitpos & 31);
      const int at = off0 + end - n0 - n1;                         // < 32 + 256 * 64, and < 32 + 256 * kTokenBits with codes of up to 15 bits
      if (((at + n0 + n1 + 31) >> 5) < kChunkWords) {
        put_bits(w_s, at, f.v0 & ((1ull << n0) - 1ull), n0);
        put_bits(w_s, at + n0, f.v1 & ((1ull << n1) - 1ull), n1);
      }
      __syncthreads();
      const int full = min((off0 + total) >> 5, kChunkWords - 1);
      const long long w0 = bitpos >> 5;
      for (int i = t; i < full; i += kScThreads)
        if (w0 + i < slot.cap) slots[slot.lo + w0 + i] = w_s[i];
      carry = w_s[full];
      bitpos += total;
      __syncthreads();                                             // w_s is cleared by the next round
    }
    if (t == kScThreads - 1) carry_s = run_start;
    __syncthreads();
  }

  if (kEmit && t == 0) {
    if ((bitpos & 31) && (bitpos >> 5) < slot.cap) slots[slot.lo + (bitpos >> 5)] = carry;
    *bits = bitpos;
  }
}
#endif  // __HIPCC__
