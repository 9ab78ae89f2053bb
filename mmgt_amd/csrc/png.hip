// PNG image data (zlib / deflate) of device-resident uint8 RGB frames: the encoder behind save_videos_grid(".apng" / ".png") and --format apng / pngs
// (mmgt_amd/video_out.py).  Truecolour, 8 bit, no alpha, no interlace.  The host builds the Huffman codes and the block headers
// (video_out.deflate_code_lengths, deflate_block_header) from histograms made here, so it knows every strip's bit count before the bits are written.
//
//  * mmgt_png_filter     (n, H, W, 3) u8 -> (n, H, 1 + 3 W) u8: per scanline the filter type byte and the filtered row, bpp = 3, the row above row 0
//                        is zeros.  One workgroup per scanline: pass 1 sums min(v, 256 - v) of the filtered bytes for each of the five types, the
//                        smallest sum wins, the lowest type on a tie; pass 2 writes the row and adds up the two sums its Adler-32 is made of,
//                        sums[row] = { sum d[i], sum (L - i) d[i] } over the L = 1 + 3 W bytes, in 64 bits (the host reduces and combines them).
//  * mmgt_png_histogram  any bytes, n rows of frame_bytes cut into strips of strip_bytes (the last may be shorter) -> u32[286] per strip: how often
//  * mmgt_png_deflate    each literal/length symbol occurs in the strip's tokens, and those tokens coded with the strip's own table behind the
//                        strip's header bits.  Tokens: distance-1 matches only, never reaching before the strip's first byte.  At position p >= 1 let
//                        r = bytes from p on that equal byte p - 1, at most 258: r >= 3 is a match of length r, else byte p is a literal; position 0
//                        is a literal; symbol 256 closes the block.  That greedy parse has a closed form: in a maximal run of equal bytes the first is
//                        a literal and the k bytes after it fall into blocks of 258 (the last one shorter), a block of 3 or more being one match and
//                        one of 1 or 2 literals.  A token is credited to the position where it ENDS, so that a position needs only the start of
//                        its run (a max-scan over the positions before it) and the two bytes after it: with j = p - run start - 1 and m = j mod 258,
//                        m = 257 ends a match of 258; a run ending at p ends a match of m + 1 if that is 3 or more, else p is a literal; and m = 0
//                        in a run that goes on for one byte only is the first of two literals.  One workgroup per strip walks it 256 positions at a
//                        time: token bits by table, workgroup prefix sum, atomicOr into LDS words, whole words stored to the strip's slot and the
//                        partly filled last word carried on; so every word of a slot is written once, with plain stores.
//  * mmgt_png_pack       joins a frame's strips at the bit offsets the host worked out and writes the frames' deflate bytes back to back.
#include "common.h"
#include "mmgt_hip.h"

namespace {

constexpr int kSyms = 286;
constexpr int kThreads = 256;
constexpr int kMaxSide = 16384;
constexpr int kHeaderWords = MMGT_PNG_HEADER_BYTES / 4;            // 17 + 19 * 3 + 316 * 14 bits at most = 4498 bits = 141 words
constexpr int kTokenBits = 21;                                     // a length code of 15 bits, 5 extra bits, the distance code's single bit
constexpr int kChunkWords = (kThreads * kTokenBits + 31) / 32 + 2; // the carried partial word in front, one word for a token straddling the end

// ---- filter ------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int filtered(int type, int cur, int a, int b, int c) {
  const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
  return (cur - pred) & 255;
}

__global__ __launch_bounds__(kThreads) void png_filter_kernel(const unsigned char* __restrict__ frames, unsigned char* __restrict__ filt,
                                                              unsigned long long* __restrict__ sums, int H, int W) {
  __shared__ unsigned cost_s[5];
  __shared__ unsigned long long adler_s[2];
  const int t = threadIdx.x;
  const size_t row = blockIdx.x;                                   // frame * H + y
  const int y = (int)(row % (size_t)H);
  const int nb = 3 * W, L = nb + 1;
  const unsigned char* cur = frames + row * (size_t)nb;
  const unsigned char* up = cur - nb;                              // read only if y > 0
  if (t < 5) cost_s[t] = 0u;
  if (t < 2) adler_s[t] = 0ull;
  __syncthreads();
  unsigned cost[5] = {0u, 0u, 0u, 0u, 0u};
  for (int i = t; i < nb; i += kThreads) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y > 0 ? up[i] : 0, c = (y > 0 && i >= 3) ? up[i - 3] : 0;
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const int v = filtered(f, x, a, b, c);
      cost[f] += (unsigned)min(v, 256 - v);
    }
  }
#pragma unroll
  for (int f = 0; f < 5; ++f) atomicAdd(&cost_s[f], cost[f]);      // at most 128 * 49152 in all: no overflow
  __syncthreads();
  int type = 0;
  unsigned best = cost_s[0];
#pragma unroll
  for (int f = 1; f < 5; ++f)
    if (cost_s[f] < best) {                                        // strictly smaller: the lowest type keeps a tie
      best = cost_s[f];
      type = f;
    }
  unsigned char* dst = filt + row * (size_t)L;
  unsigned long long s1 = 0, s2 = 0;
  if (t == 0) {
    dst[0] = (unsigned char)type;
    s1 = (unsigned)type;
    s2 = (unsigned long long)L * (unsigned)type;
  }
  for (int i = t; i < nb; i += kThreads) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = y > 0 ? up[i] : 0, c = (y > 0 && i >= 3) ? up[i - 3] : 0;
    const int v = filtered(type, x, a, b, c);
    dst[1 + i] = (unsigned char)v;
    s1 += (unsigned)v;
    s2 += (unsigned long long)(L - 1 - i) * (unsigned)v;
  }
  atomicAdd(&adler_s[0], s1);
  atomicAdd(&adler_s[1], s2);
  __syncthreads();
  if (t < 2) sums[2 * row + t] = adler_s[t];
}

// ---- tokens ------------------------------------------------------------------------------------------------------------------------------------
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

// length 3 .. 258 -> literal/length symbol, extra bits and their value (RFC 1951 3.2.5)
__device__ __forceinline__ void length_symbol(int len, int* sym, int* ebits, int* eval) {
  const int x = len - 3;
  if (len == 258) {
    *sym = 285, *ebits = 0, *eval = 0;
  } else if (x < 8) {
    *sym = 257 + x, *ebits = 0, *eval = 0;
  } else {
    const int e = 29 - __clz(x);                                   // floor(log2 x) - 2
    *sym = 261 + 4 * e + ((x >> e) - 4), *ebits = e, *eval = x & ((1 << e) - 1);
  }
}

// The token that ends at position p of a strip of len bytes: -1 none, 0 .. 255 the literal, 3 .. 258 | 0x1000 a match.  p == len is the end-of-block
// symbol 256.  run_start = the last position q <= p that is 0 or whose byte differs from byte q - 1.
__device__ __forceinline__ int token_at(const unsigned char* __restrict__ src, int p, int len, int run_start) {
  if (p == len) return 256;
  const int d = src[p];
  if (p == run_start) return d;
  const int m = (p - run_start - 1) % 258;
  if (m == 257) return 258 | 0x1000;
  const bool c1 = p + 1 < len && src[p + 1] == d;
  if (!c1) return m >= 2 ? ((m + 1) | 0x1000) : d;
  const bool c2 = p + 2 < len && src[p + 2] == d;
  return (m == 0 && !c2) ? d : -1;
}

template <bool kEmit>
__global__ __launch_bounds__(kThreads) void png_strip_kernel(const unsigned char* __restrict__ data, long long frame_bytes, long long strip_bytes, int strips,
                                                             unsigned* __restrict__ hist, const unsigned* __restrict__ codes,
                                                             const unsigned* __restrict__ header, const int* __restrict__ header_bits,
                                                             unsigned* __restrict__ slots, const long long* __restrict__ slot_off, long long slots_words,
                                                             long long* __restrict__ bits) {
  __shared__ unsigned tab_s[kSyms];                                // the histogram, or the strip's code table
  __shared__ unsigned w_s[kChunkWords];
  __shared__ int part_s[4];
  __shared__ int carry_s;
  const int t = threadIdx.x;
  const int strip = blockIdx.x % strips;
  const size_t frame = blockIdx.x / strips;
  const long long first = (long long)strip * strip_bytes;
  const int len = (int)min(strip_bytes, frame_bytes - first);      // 1 .. 2^30
  const unsigned char* src = data + frame * (size_t)frame_bytes + (size_t)first;

  // the slot: words [w_lo, w_lo + w_cap) of slots, clamped to the buffer whatever slot_off holds
  long long w_lo = 0, w_cap = 0;
  long long bitpos = 0;
  unsigned carry = 0u;                                             // the bits of the word that bitpos lies in
  if (kEmit) {
    w_lo = slot_off[blockIdx.x];
    w_cap = slot_off[blockIdx.x + 1] - w_lo;
    if (w_lo < 0 || w_lo > slots_words) w_lo = slots_words;
    w_cap = max(0ll, min(w_cap, slots_words - w_lo));
    for (int i = t; i < kSyms; i += kThreads) tab_s[i] = codes[(size_t)blockIdx.x * kSyms + i];
    const int hb = max(0, min(header_bits[blockIdx.x], 32 * kHeaderWords));
    const unsigned* hw = header + (size_t)blockIdx.x * kHeaderWords;
    for (int i = t; i < hb / 32; i += kThreads)
      if (i < w_cap) slots[w_lo + i] = hw[i];
    if (hb & 31) carry = hw[hb / 32] & ((1u << (hb & 31)) - 1u);
    bitpos = hb;
  } else {
    for (int i = t; i < kSyms; i += kThreads) tab_s[i] = 0u;
  }
  if (t == 0) carry_s = -1;
  __syncthreads();

  for (int base = 0; base <= len; base += kThreads) {             // position len is the end-of-block symbol
    const int p = base + t;
    const bool valid = p <= len;
    const bool boundary = p < len && (p == 0 || src[p] != src[p - 1]);
    if (kEmit) {
      for (int i = t; i < kChunkWords; i += kThreads) w_s[i] = i == 0 ? carry : 0u;
    }
    const int run_start = max(block_scan_max(boundary ? p : -1, part_s), carry_s);
    const int tok = valid ? token_at(src, p, len, run_start) : -1;
    int sym = tok, ebits = 0, eval = 0;
    if (tok >= 0x1000) length_symbol(tok & 0xfff, &sym, &ebits, &eval);
    if (!kEmit) {
      if (tok >= 0) atomicAdd(&tab_s[sym], 1u);
      __syncthreads();                                             // carry_s is read above by every thread before it is rewritten
    } else {
      unsigned long long v = 0;
      int nb = 0;
      if (tok >= 0) {
        const unsigned c = tab_s[sym];
        const int cl = (int)(c >> 16);
        v = (unsigned long long)(c & 0xffffu) | (unsigned long long)eval << cl;       // a match: extra bits, then the distance code 0 (one bit)
        nb = cl + ebits + (tok >= 0x1000 ? 1 : 0);
      }
      int total;
      const int end = block_scan_add(nb, part_s, &total);
      const int off0 = (int)(bitpos & 31);
      if (nb > 0) {
        const int at = off0 + end - nb;                            // < 32 + 256 * 21
        const unsigned long long sh = v << (at & 31);              // nb <= 21 and at & 31 <= 31: fits
        atomicOr(&w_s[at >> 5], (unsigned)sh);
        if ((unsigned)(sh >> 32)) atomicOr(&w_s[(at >> 5) + 1], (unsigned)(sh >> 32));
      }
      __syncthreads();
      const int full = (off0 + total) >> 5;
      const long long w0 = bitpos >> 5;
      for (int i = t; i < full; i += kThreads)
        if (w0 + i < w_cap) slots[w_lo + w0 + i] = w_s[i];
      carry = w_s[full];
      bitpos += total;
      __syncthreads();                                             // w_s is cleared by the next round
    }
    if (t == kThreads - 1) carry_s = run_start;
    __syncthreads();
  }

  if (kEmit) {
    if (t == 0) {
      if ((bitpos & 31) && (bitpos >> 5) < w_cap) slots[w_lo + (bitpos >> 5)] = carry;
      bits[blockIdx.x] = bitpos;
    }
  } else {
    for (int i = t; i < kSyms; i += kThreads) hist[(size_t)blockIdx.x * kSyms + i] = tab_s[i];
  }
}

// ---- pack --------------------------------------------------------------------------------------------------------------------------------------
// bit_off (n, strips + 1): where each strip starts in its frame's stream, and where the last one ends.  Byte j of frame f gathers its 8 bits from the
// strip that holds bit 8 j and, where that strip ends inside the byte, from the next ones.  Reads and writes are clamped to the two buffers.
__global__ __launch_bounds__(256) void png_pack_kernel(const unsigned* __restrict__ slots, const long long* __restrict__ slot_off, long long slots_words,
                                                       const long long* __restrict__ bit_off, unsigned char* __restrict__ out,
                                                       const long long* __restrict__ out_off, long long out_bytes, int strips) {
  const int frame = blockIdx.y;
  const long long* pre = bit_off + (size_t)frame * (strips + 1);
  const long long o0 = out_off[frame];
  const long long nbytes = out_off[frame + 1] - o0;
  const unsigned char* sb = reinterpret_cast<const unsigned char*>(slots);
  const long long sbytes = 4 * slots_words;
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nbytes; j += (long long)gridDim.x * 256) {
    const long long b0 = 8 * j;
    int lo = 0, hi = strips - 1;                                   // the last strip s with pre[s] <= b0
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pre[mid] <= b0) lo = mid; else hi = mid - 1;
    }
    unsigned val = 0;
    int got = 0;
    for (int s = lo; s < strips && got < 8; ++s) {
      const long long local = b0 + got - pre[s];
      const long long avail = pre[s + 1] - pre[s] - local;
      if (local < 0 || avail <= 0) continue;
      const int take = (int)(avail < 8 - got ? avail : 8 - got);
      const long long q = 4 * slot_off[(size_t)frame * strips + s] + (local >> 3);
      unsigned two = 0;
      if (q >= 0 && q < sbytes) two = sb[q];
      if (q + 1 >= 0 && q + 1 < sbytes) two |= (unsigned)sb[q + 1] << 8;
      val |= ((two >> (local & 7)) & ((1u << take) - 1)) << got;
      got += take;
    }
    const long long o = o0 + j;
    if (o >= 0 && o < out_bytes) out[o] = (unsigned char)val;
  }
}

const char* kBadStrips = "%s: n = %d rows of %lld bytes in strips of %lld are outside the range (n >= 1, 1 <= strip_bytes, 1 <= frame_bytes <= 2^30, "
                         "n * strips < 2^31)";
bool strips_ok(int n, long long frame_bytes, long long strip_bytes) {
  if (n < 1 || frame_bytes < 1 || frame_bytes > (1ll << 30) || strip_bytes < 1) return false;
  const long long strips = (frame_bytes + strip_bytes - 1) / strip_bytes;
  return n * strips <= 0x7fffffffll;
}

}  // namespace

extern "C" int mmgt_png_filter(const unsigned char* frames, unsigned char* filt, long long* sums, int n, int H, int W, void* stream) {
  MMGT_CHECK(frames && filt && sums, "png_filter: null pointer");
  MMGT_CHECK(n >= 1 && H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide && (long long)n * H <= 0x7fffffffll,
             "png_filter: n = %d frames of %d x %d are outside the range (n, H, W >= 1, H, W <= %d, n * H < 2^31)", n, H, W, kMaxSide);
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)(n * H)), dim3(kThreads), 0, (hipStream_t)stream, frames, filt,
                     reinterpret_cast<unsigned long long*>(sums), H, W);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_png_histogram(const unsigned char* data, unsigned* hist, int n, long long frame_bytes, long long strip_bytes, void* stream) {
  MMGT_CHECK(data && hist, "png_histogram: null pointer");
  MMGT_CHECK(strips_ok(n, frame_bytes, strip_bytes), kBadStrips, "png_histogram", n, frame_bytes, strip_bytes);
  const int strips = (int)((frame_bytes + strip_bytes - 1) / strip_bytes);
  hipLaunchKernelGGL(png_strip_kernel<false>, dim3((unsigned)(n * strips)), dim3(kThreads), 0, (hipStream_t)stream, data, frame_bytes, strip_bytes,
                     strips, hist, nullptr, nullptr, nullptr, nullptr, nullptr, 0ll, nullptr);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_png_deflate(const unsigned char* data, const unsigned* codes, const unsigned* header, const int* header_bits, unsigned* slots,
                                const long long* slot_off, long long slots_words, long long* bits, int n, long long frame_bytes, long long strip_bytes,
                                void* stream) {
  MMGT_CHECK(data && codes && header && header_bits && slots && slot_off && bits, "png_deflate: null pointer");
  MMGT_CHECK(strips_ok(n, frame_bytes, strip_bytes), kBadStrips, "png_deflate", n, frame_bytes, strip_bytes);
  MMGT_CHECK(slots_words >= 1, "png_deflate: slots_words = %lld", slots_words);
  const int strips = (int)((frame_bytes + strip_bytes - 1) / strip_bytes);
  hipLaunchKernelGGL(png_strip_kernel<true>, dim3((unsigned)(n * strips)), dim3(kThreads), 0, (hipStream_t)stream, data, frame_bytes, strip_bytes,
                     strips, nullptr, codes, header, header_bits, slots, slot_off, slots_words, bits);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_png_pack(const unsigned* slots, const long long* slot_off, long long slots_words, const long long* bit_off, unsigned char* out,
                             const long long* out_off, long long out_bytes, int n, int strips, void* stream) {
  MMGT_CHECK(slots && slot_off && bit_off && out && out_off, "png_pack: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && strips >= 1 && slots_words >= 1 && out_bytes >= 1,
             "png_pack: n = %d (at most 65535 per launch), strips = %d, slots_words = %lld, out_bytes = %lld", n, strips, slots_words, out_bytes);
  const long long want = (out_bytes / n + 4 * 256 - 1) / (4 * 256);
  const unsigned gx = (unsigned)(want < 1 ? 1 : want > 256 ? 256 : want);
  hipLaunchKernelGGL(png_pack_kernel, dim3(gx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, slots, slot_off, slots_words, bit_off, out, out_off,
                     out_bytes, strips);
  MMGT_LAUNCH_CHECK();
  return 0;
}
