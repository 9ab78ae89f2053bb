// WebP lossless (VP8L) bitstreams of device-resident uint8 RGB frames: the encoder behind save_videos_grid(".webp") and --format webp (DESIGN 4j,
// mmgt_amd/video_out.py).  Subtract green, the predictor transform with a mode per 16 x 16 block, matches from the left pixel only, one group of five
// prefix codes per frame.  The host builds the codes and the frame's header (video_out.webp_prefix_code, webp_frame_header) from histograms made
// here, so it knows every strip's bit count before the bits are written.  The arithmetic of a pixel is csrc/webp_core.h's.
//
//  * mmgt_webp_predict    (n, H, W, 3) u8 -> modes (n, bh, bw) u8 and residuals (n, H, W) ARGB words.  One workgroup per block, one thread per pixel:
//                         the 14 modes' costs (sum of min(v, 256 - v) over the residuals' r, g, b) are summed over the block, the smallest wins, the
//                         lowest mode on a tie, and every thread writes its pixel's residual under that mode.  Neighbours are read from the input,
//                         never from residuals, so the pixels are independent.
//  * mmgt_webp_histogram  residual words, n rows of frame_px cut into strips of strip_px (the last may be shorter) -> u32[793] per strip: how often
//  * mmgt_webp_code       each green / length, red and blue symbol occurs in the strip's tokens and how many matches there are, and those tokens
//                         coded with the frame's tables.  Tokens: csrc/png.hip's closed form over pixels, with 4096 for 258 and no end symbol (see
//                         wp_token_at).  One workgroup per strip walks it 256 positions at a time: token bits by table, workgroup prefix sum,
//                         atomicOr into LDS words, whole words stored to the strip's slot and the partly filled last word carried on; so every
//                         word of a slot is written once, with plain stores.  A frame's slots are its header's, then its strips'; strip 0's
//                         workgroup also copies the header words the host built into the header's slot.
//  * packing              mmgt_png_pack as it stands joins a frame's slots at the bit offsets the host worked out (hip.webp_pack).
#include "common.h"
#include "mmgt_hip.h"
#include "webp_core.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSide = 16384;
constexpr int kBlock = 1 << WP_PREDICTOR_BITS;
constexpr int kRed = WP_GREEN_SYMS, kBlue = WP_GREEN_SYMS + 256, kMatches = WP_GREEN_SYMS + 512;
constexpr int kCodeWords = WP_GREEN_SYMS + 512;                    // the frame's tables: green + length, red, blue
constexpr int kTokenBits = 45;                                     // a literal: three codes of 15 bits (a match: 15 + 10 extra bits)
constexpr int kChunkWords = (kThreads * kTokenBits + 31) / 32 + 2; // the carried partial word in front, one word for a token straddling the end
static_assert(kBlock * kBlock == kThreads, "one thread per pixel of a block");

// ---- predict -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void webp_predict_kernel(const unsigned char* __restrict__ frames, unsigned char* __restrict__ modes,
                                                                unsigned* __restrict__ res, int H, int W, int bh, int bw) {
  __shared__ unsigned cost_s[WP_MODES];
  const int t = threadIdx.x;
  const long blk = blockIdx.x;                                     // (frame * bh + by) * bw + bx
  const long frame = blk / ((long)bh * bw);
  const long y = (blk / bw % bh) * kBlock + (t >> WP_PREDICTOR_BITS), x = (blk % bw) * kBlock + (t & (kBlock - 1));
  const bool in = y < H && x < W;
  const unsigned char* f = frames + frame * 3 * (long)H * W;
  if (t < WP_MODES) cost_s[t] = 0u;
  __syncthreads();
  uint32_t cur = WP_BLACK;
  WpNeighbours nb = {WP_BLACK, WP_BLACK, WP_BLACK, WP_BLACK};
  if (in) {
    cur = wp_pixel(f, W, y, x);
    nb = wp_neighbours(f, W, y, x);
  }
#pragma unroll
  for (int m = 0; m < WP_MODES; ++m) {
    unsigned c = in ? wp_cost(wp_sub(cur, wp_predict_at(m, y, x, nb))) : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((t & 63) == 0) atomicAdd(&cost_s[m], c);                   // at most 256 * 3 * 128 in all: no overflow
  }
  __syncthreads();
  int mode = 0;
  unsigned best = cost_s[0];
#pragma unroll
  for (int m = 1; m < WP_MODES; ++m)
    if (cost_s[m] < best) {                                        // strictly smaller: the lowest mode keeps a tie
      best = cost_s[m];
      mode = m;
    }
  if (t == 0) modes[blk] = (unsigned char)mode;
  if (in) res[frame * (long)H * W + y * W + x] = wp_sub(cur, wp_predict_at(mode, y, x, nb));
}

// ---- tokens ------------------------------------------------------------------------------------------------------------------------------------
// Inclusive scans over the workgroup's 256 threads (4 waves), as in csrc/png.hip: within a wave by shuffles, then the totals of the waves before
// through LDS.  Both end with every thread past the barrier that guards part_s, so they can be called back to back.
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

template <bool kEmit>
__global__ __launch_bounds__(kThreads) void webp_strip_kernel(const unsigned* __restrict__ data, long long frame_px, long long strip_px, int strips,
                                                              unsigned* __restrict__ hist, const unsigned* __restrict__ codes,
                                                              const unsigned* __restrict__ header, const long long* __restrict__ header_off,
                                                              long long header_words, unsigned* __restrict__ slots,
                                                              const long long* __restrict__ slot_off, long long slots_words,
                                                              long long* __restrict__ bits) {
  __shared__ unsigned tab_s[WP_HIST_WORDS];                        // the histogram, or the frame's code tables
  __shared__ unsigned w_s[kChunkWords];
  __shared__ int part_s[4];
  __shared__ int carry_s;
  const int t = threadIdx.x;
  const int strip = blockIdx.x % strips;
  const long frame = blockIdx.x / strips;
  const long long first = (long long)strip * strip_px;
  const int len = (int)min(strip_px, frame_px - first);            // 1 .. 2^28
  const unsigned* src = data + frame * frame_px + first;

  // the slot: words [w_lo, w_lo + w_cap) of slots, clamped to the buffer whatever slot_off holds
  long long w_lo = 0, w_cap = 0;
  long long bitpos = 0;
  unsigned carry = 0u;                                             // the bits of the word that bitpos lies in
  if (kEmit) {
    const long k = frame * (strips + 1) + 1 + strip;               // slot 0 of a frame is its header's
    w_lo = slot_off[k];
    w_cap = slot_off[k + 1] - w_lo;
    if (w_lo < 0 || w_lo > slots_words) w_lo = slots_words;
    w_cap = max(0ll, min(w_cap, slots_words - w_lo));
    for (int i = t; i < kCodeWords; i += kThreads) tab_s[i] = codes[frame * kCodeWords + i];
    if (strip == 0) {                                              // the header words, both ranges clamped
      long long h_lo = header_off[frame], h_n = header_off[frame + 1] - h_lo;
      if (h_lo < 0 || h_lo > header_words) h_lo = header_words;
      h_n = max(0ll, min(h_n, header_words - h_lo));
      long long s_lo = slot_off[k - 1], s_cap = w_lo - s_lo;
      if (s_lo < 0 || s_lo > slots_words) s_lo = slots_words;
      s_cap = max(0ll, min(s_cap, slots_words - s_lo));
      for (long long i = t; i < min(h_n, s_cap); i += kThreads) slots[s_lo + i] = header[h_lo + i];
    }
  } else {
    for (int i = t; i < WP_HIST_WORDS; i += kThreads) tab_s[i] = 0u;
  }
  if (t == 0) carry_s = -1;
  __syncthreads();

  for (int base = 0; base < len; base += kThreads) {
    const int p = base + t;
    const bool valid = p < len;
    const bool boundary = valid && (p == 0 || src[p] != src[p - 1]);
    if (kEmit) {
      for (int i = t; i < kChunkWords; i += kThreads) w_s[i] = i == 0 ? carry : 0u;
    }
    const int run_start = max(block_scan_max(boundary ? p : -1, part_s), carry_s);
    const int tok = valid ? wp_token_at(src, p, len, run_start) : WP_NONE;
    const unsigned px = tok == WP_LITERAL ? src[p] : 0u;
    const int g = (int)(px >> 8 & 255u), r = kRed + (int)(px >> 16 & 255u), b = kBlue + (int)(px & 255u);
    int sym = 0, ebits = 0, eval = 0;
    if (tok > 0) wp_prefix(tok, &sym, &ebits, &eval);
    sym += 256;
    if (!kEmit) {
      if (tok == WP_LITERAL) {
        atomicAdd(&tab_s[g], 1u);
        atomicAdd(&tab_s[r], 1u);
        atomicAdd(&tab_s[b], 1u);
      } else if (tok > 0) {
        atomicAdd(&tab_s[sym], 1u);
        atomicAdd(&tab_s[kMatches], 1u);
      }
      __syncthreads();                                             // carry_s is read above by every thread before it is rewritten
    } else {
      // a literal: green, then red and blue together (alpha's one-symbol code takes no bits); a match: the length's code and extra bits (the
      // distance's one-symbol code takes no bits).  A code of a one-symbol alphabet has length 0 in the table.
      unsigned long long v0 = 0, v1 = 0;
      int n0 = 0, n1 = 0;
      if (tok == WP_LITERAL) {
        const unsigned cg = tab_s[g], cr = tab_s[r], cb = tab_s[b];
        n0 = (int)(cg >> 16);
        v0 = cg & 0xffffu;
        n1 = (int)(cr >> 16) + (int)(cb >> 16);
        v1 = (unsigned long long)(cr & 0xffffu) | (unsigned long long)(cb & 0xffffu) << (cr >> 16);
      } else if (tok > 0) {
        const unsigned c = tab_s[sym];
        n0 = (int)(c >> 16) + ebits;
        v0 = (unsigned long long)(c & 0xffffu) | (unsigned long long)eval << (c >> 16);
      }
      n0 = min(n0, 32), n1 = min(n1, 32);                          // 25 and 30 at most with codes of up to 15 bits, whatever the table holds
      int total;
      const int end = block_scan_add(n0 + n1, part_s, &total);
      const int off0 = (int)(bitpos & 31);
      const int at = off0 + end - n0 - n1;                         // < 32 + 256 * 64, and < 32 + 256 * 45 with codes of up to 15 bits
      if (((at + n0 + n1 + 31) >> 5) < kChunkWords) {
        put_bits(w_s, at, v0 & ((1ull << n0) - 1ull), n0);
        put_bits(w_s, at + n0, v1 & ((1ull << n1) - 1ull), n1);
      }
      __syncthreads();
      const int full = min((off0 + total) >> 5, kChunkWords - 1);
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
    for (int i = t; i < WP_HIST_WORDS; i += kThreads) hist[(size_t)blockIdx.x * WP_HIST_WORDS + i] = tab_s[i];
  }
}

const char* kBadStrips = "%s: n = %d rows of %lld pixels in strips of %lld are outside the range (n >= 1, 1 <= strip_px, 1 <= frame_px <= 2^28, "
                         "n * strips < 2^31)";
bool strips_ok(int n, long long frame_px, long long strip_px) {
  if (n < 1 || frame_px < 1 || frame_px > (1ll << 28) || strip_px < 1) return false;
  const long long strips = (frame_px + strip_px - 1) / strip_px;
  return n * strips <= 0x7fffffffll;
}

}  // namespace

extern "C" int mmgt_webp_predict(const unsigned char* frames, unsigned char* modes, unsigned* res, int n, int H, int W, void* stream) {
  MMGT_CHECK(frames && modes && res, "webp_predict: null pointer");
  const long long bh = ((long long)H + kBlock - 1) / kBlock, bw = ((long long)W + kBlock - 1) / kBlock;
  MMGT_CHECK(n >= 1 && H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide && n * bh * bw <= 0x7fffffffll,
             "webp_predict: n = %d frames of %d x %d are outside the range (n, H, W >= 1, H, W <= %d, n * blocks < 2^31)", n, H, W, kMaxSide);
  hipLaunchKernelGGL(webp_predict_kernel, dim3((unsigned)(n * bh * bw)), dim3(kThreads), 0, (hipStream_t)stream, frames, modes, res, H, W, (int)bh,
                     (int)bw);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_webp_histogram(const unsigned* res, unsigned* hist, int n, long long frame_px, long long strip_px, void* stream) {
  MMGT_CHECK(res && hist, "webp_histogram: null pointer");
  MMGT_CHECK(strips_ok(n, frame_px, strip_px), kBadStrips, "webp_histogram", n, frame_px, strip_px);
  const int strips = (int)((frame_px + strip_px - 1) / strip_px);
  hipLaunchKernelGGL(webp_strip_kernel<false>, dim3((unsigned)(n * strips)), dim3(kThreads), 0, (hipStream_t)stream, res, frame_px, strip_px, strips,
                     hist, nullptr, nullptr, nullptr, 0ll, nullptr, nullptr, 0ll, nullptr);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_webp_code(const unsigned* res, const unsigned* codes, const unsigned* header, const long long* header_off, long long header_words,
                              unsigned* slots, const long long* slot_off, long long slots_words, long long* bits, int n, long long frame_px,
                              long long strip_px, void* stream) {
  MMGT_CHECK(res && codes && header && header_off && slots && slot_off && bits, "webp_code: null pointer");
  MMGT_CHECK(strips_ok(n, frame_px, strip_px), kBadStrips, "webp_code", n, frame_px, strip_px);
  const long long strips = (frame_px + strip_px - 1) / strip_px;
  MMGT_CHECK(slots_words >= 1 && header_words >= 1 && n * (strips + 1) <= 0x7fffffffll, "webp_code: slots_words = %lld, header_words = %lld",
             slots_words, header_words);
  hipLaunchKernelGGL(webp_strip_kernel<true>, dim3((unsigned)(n * strips)), dim3(kThreads), 0, (hipStream_t)stream, res, frame_px, strip_px,
                     (int)strips, nullptr, codes, header, header_off, header_words, slots, slot_off, slots_words, bits);
  MMGT_LAUNCH_CHECK();
  return 0;
}
