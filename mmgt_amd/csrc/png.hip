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
//                        strip's header bits.  Tokens: distance-1 matches only, never reaching before the strip's first byte, at most 258 long, by
//                        the closed form of csrc/strip_coder.h; symbol 256 closes the block.  One workgroup per strip; the walk (scans, LDS window,
//                        carried word, every word of a slot written once with plain stores) is strip_coder.h's sc_walk_strip, shared with
//                        csrc/webp.hip.  What is PNG's own is below: the token's symbol and extra bits, the strip's table and its header in front.
//  * mmgt_png_pack       joins a frame's strips at the bit offsets the host worked out and writes the frames' deflate bytes back to back.
#include "common.h"
#include "mmgt_hip.h"
#include "strip_coder.h"

namespace {

constexpr int kSyms = 286;
constexpr int kThreads = kScThreads;
constexpr int kMaxSide = 16384;
constexpr int kHeaderWords = MMGT_PNG_HEADER_BYTES / 4;            // 17 + 19 * 3 + 316 * 14 bits at most = 4498 bits = 141 words

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

// The token that ends at position p of a strip of len bytes: -1 none, 0 .. 255 the literal, 3 .. 258 | 0x1000 a match (strip_coder.h's closed form
// at 258).  p == len is the end-of-block symbol 256.
__device__ __forceinline__ int token_at(const unsigned char* __restrict__ src, int p, int len, int run_start) {
  if (p == len) return 256;
  const int d = src[p];                                            // read before the token is known: one round trip less for a literal
  const int tok = sc_token_at<258>(ScSameAsBefore<unsigned char>{src}, p, len, run_start);
  return tok == SC_NONE ? -1 : tok == SC_LITERAL ? d : tok | 0x1000;
}

// strip_coder.h's codec of deflate: a token is a literal/length symbol of the strip's table; a match adds its extra bits and the distance code 0.
struct PngCodec {
  using Elem = unsigned char;
  static constexpr int kTokenBits = 21;                            // a length code of 15 bits, 5 extra bits, the distance code's single bit
  static constexpr int kTail = 1;                                  // position len is the end-of-block symbol
  static __device__ __forceinline__ int token(const Elem* src, int p, int len, int run_start) { return token_at(src, p, len, run_start); }
  static __device__ __forceinline__ void count(unsigned* tab_s, int tok, const Elem*, int) {
    int sym = tok, ebits = 0, eval = 0;
    if (tok >= 0x1000) length_symbol(tok & 0xfff, &sym, &ebits, &eval);
    atomicAdd(&tab_s[sym], 1u);
  }
  static __device__ __forceinline__ ScFields fields(const unsigned* tab_s, int tok, const Elem*, int) {
    int sym = tok, ebits = 0, eval = 0;
    if (tok >= 0x1000) length_symbol(tok & 0xfff, &sym, &ebits, &eval);
    const unsigned c = tab_s[sym];
    ScFields f;
    f.v0 = (unsigned long long)(c & 0xffffu) | (unsigned long long)eval << (c >> 16);   // a match: extra bits, then the distance code 0 (one bit)
    f.n0 = (int)(c >> 16) + ebits + (tok >= 0x1000 ? 1 : 0);
    return f;
  }
};

template <bool kEmit>
__global__ __launch_bounds__(kThreads) void png_strip_kernel(const unsigned char* __restrict__ data, long long frame_bytes, long long strip_bytes, int strips,
                                                             unsigned* __restrict__ hist, const unsigned* __restrict__ codes,
                                                             const unsigned* __restrict__ header, const int* __restrict__ header_bits,
                                                             unsigned* __restrict__ slots, const long long* __restrict__ slot_off, long long slots_words,
                                                             long long* __restrict__ bits) {
  __shared__ unsigned tab_s[kSyms];                                // the histogram, or the strip's code table
  const int t = threadIdx.x;
  const int strip = blockIdx.x % strips;
  const size_t frame = blockIdx.x / strips;
  const long long first = (long long)strip * strip_bytes;
  const int len = (int)min(strip_bytes, frame_bytes - first);      // 1 .. 2^30
  const unsigned char* src = data + frame * (size_t)frame_bytes + (size_t)first;
  for (int i = t; i < kSyms; i += kThreads) tab_s[i] = kEmit ? codes[(size_t)blockIdx.x * kSyms + i] : 0u;
  if (kEmit) {                                                     // the strip's own table, and its block header in front of the tokens
    const int hb = max(0, min(header_bits[blockIdx.x], 32 * kHeaderWords));
    sc_walk_strip<true, PngCodec>(src, len, tab_s, header + (size_t)blockIdx.x * kHeaderWords, hb, slots, slot_off + blockIdx.x, slots_words,
                                  bits + blockIdx.x);
  } else {
    sc_walk_strip<false, PngCodec>(src, len, tab_s, nullptr, 0, nullptr, nullptr, 0ll, nullptr);
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

const char* kBadStrips = SC_BAD_STRIPS("bytes", "bytes", "2^30");
constexpr long long kMaxFrameBytes = 1ll << 30;

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
  MMGT_CHECK(sc_strips_ok(n, frame_bytes, strip_bytes, kMaxFrameBytes), kBadStrips, "png_histogram", n, frame_bytes, strip_bytes);
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
  MMGT_CHECK(sc_strips_ok(n, frame_bytes, strip_bytes, kMaxFrameBytes), kBadStrips, "png_deflate", n, frame_bytes, strip_bytes);
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
