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
//                         coded with the frame's tables.  Tokens: the closed form of csrc/strip_coder.h over pixels, at most 4096 long and with
//                         no end symbol (wp_token_at).  One workgroup per strip; the walk (scans, LDS window, carried word, every word of a slot
//                         written once with plain stores) is strip_coder.h's sc_walk_strip, shared with csrc/png.hip.  A frame's slots are its
//                         header's, then its strips'; strip 0's workgroup also copies the header words the host built into the header's slot.
//  * packing              mmgt_png_pack as it stands joins a frame's slots at the bit offsets the host worked out (hip.webp_pack).
#include "common.h"
#include "mmgt_hip.h"
#include "strip_coder.h"
#include "webp_core.h"

namespace {

constexpr int kThreads = kScThreads;
constexpr int kMaxSide = 16384;
constexpr int kBlock = 1 << WP_PREDICTOR_BITS;
constexpr int kRed = WP_GREEN_SYMS, kBlue = WP_GREEN_SYMS + 256, kMatches = WP_GREEN_SYMS + 512;
constexpr int kCodeWords = WP_GREEN_SYMS + 512;                    // the frame's tables: green + length, red, blue
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
// strip_coder.h's codec of VP8L: a literal is a green, a red and a blue symbol (alpha's one-symbol code takes no bits), a match the length's prefix
// symbol in the green alphabet and its extra bits (the distance's one-symbol code takes no bits).  A code of a one-symbol alphabet has length 0 in
// the table.
struct WebpCodec {
  using Elem = unsigned;
  static constexpr int kTokenBits = 45;                            // a literal: three codes of 15 bits (a match: 15 + 10 extra bits)
  static constexpr int kTail = 0;
  static __device__ __forceinline__ int token(const Elem* src, int p, int len, int run_start) { return wp_token_at(src, p, len, run_start); }
  static __device__ __forceinline__ int length_symbol(int tok, int* ebits, int* eval) {
    int sym;
    wp_prefix(tok, &sym, ebits, eval);
    return 256 + sym;
  }
  static __device__ __forceinline__ void count(unsigned* tab_s, int tok, const Elem* src, int p) {
    if (tok == WP_LITERAL) {
      const unsigned px = src[p];
      atomicAdd(&tab_s[px >> 8 & 255u], 1u);
      atomicAdd(&tab_s[kRed + (px >> 16 & 255u)], 1u);
      atomicAdd(&tab_s[kBlue + (px & 255u)], 1u);
    } else {
      int ebits, eval;
      atomicAdd(&tab_s[length_symbol(tok, &ebits, &eval)], 1u);
      atomicAdd(&tab_s[kMatches], 1u);
    }
  }
  static __device__ __forceinline__ ScFields fields(const unsigned* tab_s, int tok, const Elem* src, int p) {
    ScFields f;
    if (tok == WP_LITERAL) {                                       // green, then red and blue together
      const unsigned px = src[p];
      const unsigned cg = tab_s[px >> 8 & 255u], cr = tab_s[kRed + (px >> 16 & 255u)], cb = tab_s[kBlue + (px & 255u)];
      f.n0 = (int)(cg >> 16);
      f.v0 = cg & 0xffffu;
      f.n1 = (int)(cr >> 16) + (int)(cb >> 16);
      f.v1 = (unsigned long long)(cr & 0xffffu) | (unsigned long long)(cb & 0xffffu) << (cr >> 16);
    } else {
      int ebits, eval;
      const unsigned c = tab_s[length_symbol(tok, &ebits, &eval)];
      f.n0 = (int)(c >> 16) + ebits;
      f.v0 = (unsigned long long)(c & 0xffffu) | (unsigned long long)eval << (c >> 16);
    }
    return f;
  }
};

template <bool kEmit>
__global__ __launch_bounds__(kThreads) void webp_strip_kernel(const unsigned* __restrict__ data, long long frame_px, long long strip_px, int strips,
                                                              unsigned* __restrict__ hist, const unsigned* __restrict__ codes,
                                                              const unsigned* __restrict__ header, const long long* __restrict__ header_off,
                                                              long long header_words, unsigned* __restrict__ slots,
                                                              const long long* __restrict__ slot_off, long long slots_words,
                                                              long long* __restrict__ bits) {
  __shared__ unsigned tab_s[WP_HIST_WORDS];                        // the histogram, or the frame's code tables
  const int t = threadIdx.x;
  const int strip = blockIdx.x % strips;
  const long frame = blockIdx.x / strips;
  const long long first = (long long)strip * strip_px;
  const int len = (int)min(strip_px, frame_px - first);            // 1 .. 2^28
  const unsigned* src = data + frame * frame_px + first;
  if (kEmit) {
    const long k = frame * (strips + 1) + 1 + strip;               // slot 0 of a frame is its header's
    for (int i = t; i < kCodeWords; i += kThreads) tab_s[i] = codes[frame * kCodeWords + i];
    if (strip == 0) {                                              // the header words, both ranges clamped
      const ScSlot h = sc_slot(header_off[frame], header_off[frame + 1], header_words);
      const ScSlot s = sc_slot(slot_off[k - 1], sc_slot(slot_off[k], slot_off[k + 1], slots_words).lo, slots_words);
      for (long long i = t; i < min(h.cap, s.cap); i += kThreads) slots[s.lo + i] = header[h.lo + i];
    }
    sc_walk_strip<true, WebpCodec>(src, len, tab_s, nullptr, 0, slots, slot_off + k, slots_words, bits + blockIdx.x);
  } else {
    for (int i = t; i < WP_HIST_WORDS; i += kThreads) tab_s[i] = 0u;
    sc_walk_strip<false, WebpCodec>(src, len, tab_s, nullptr, 0, nullptr, nullptr, 0ll, nullptr);
    for (int i = t; i < WP_HIST_WORDS; i += kThreads) hist[(size_t)blockIdx.x * WP_HIST_WORDS + i] = tab_s[i];
  }
}

const char* kBadStrips = SC_BAD_STRIPS("pixels", "px", "2^28");
constexpr long long kMaxFramePx = 1ll << 28;

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
  MMGT_CHECK(sc_strips_ok(n, frame_px, strip_px, kMaxFramePx), kBadStrips, "webp_histogram", n, frame_px, strip_px);
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
  MMGT_CHECK(sc_strips_ok(n, frame_px, strip_px, kMaxFramePx), kBadStrips, "webp_code", n, frame_px, strip_px);
  const long long strips = (frame_px + strip_px - 1) / strip_px;
  MMGT_CHECK(slots_words >= 1 && header_words >= 1 && n * (strips + 1) <= 0x7fffffffll, "webp_code: slots_words = %lld, header_words = %lld",
             slots_words, header_words);
  hipLaunchKernelGGL(webp_strip_kernel<true>, dim3((unsigned)(n * strips)), dim3(kThreads), 0, (hipStream_t)stream, res, frame_px, strip_px,
                     (int)strips, nullptr, codes, header, header_off, header_words, slots, slot_off, slots_words, bits);
  MMGT_LAUNCH_CHECK();
  return 0;
}
