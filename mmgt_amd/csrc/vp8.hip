// Lossy WebP output: VP8 key frames of device-resident uint8 RGB frames, the encoder behind save_videos_grid(".webp", webp_quality=Q) and
// --format webp --webp_quality Q (mmgt_amd/video_out.py).  Every frame is coded on its own; all the arithmetic of a block and of a
// symbol is csrc/vp8_core.h's.
//
//  * mmgt_vp8_convert   (n, H, W, 3) u8 RGB -> Y (n, 16 mbh, 16 mbw), U and V (n, 8 mbh, 8 mbw): the frame padded to whole macroblocks by edge
//                       replication.  One thread per chroma sample and its four luma samples.
//  * mmgt_vp8_analyse   predict, transform, quantise, reconstruct.  A macroblock needs its left, top and top-left neighbours' reconstruction, so a
//                       frame is a wavefront over its anti-diagonals.  ONE workgroup per frame walks them, one thread per macroblock of the
//                       diagonal, a __syncthreads() between diagonals: no workgroup ever waits for another.  Frames are independent, so a clip
//                       gives as many workgroups as frames.  Writes levels, modes, non-zero masks, the reconstructed planes and the skip count.
//  * mmgt_vp8_code      one sequential boolean coder per (frame, partition), each in a workgroup of its own (one lane works): the first partition
//                       (header fields, skip flags, modes) and the P token partitions, each into its own worst-case slot, each reporting its bytes.
//                       Contexts come from the stored masks; no coder reads another's state.  Every loop's trip count is known on entry.
//  * mmgt_vp8_pack      frame tag, start code, sizes, first partition, partition sizes, partitions -> the frame's bytes at out_off[f] of one buffer.
#include "common.h"
#include "mmgt_hip.h"
#include "vp8_core.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void vp8_convert_kernel(const unsigned char* __restrict__ frames, unsigned char* __restrict__ Y,
                                                               unsigned char* __restrict__ U, unsigned char* __restrict__ V, int H, int W, int ch,
                                                               int cw, long long total) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;       // (frame, cy, cx)
  if (i >= total) return;
  const int cx = (int)(i % cw), cy = (int)(i / cw % ch);
  const long long f = i / ((long long)cw * ch);
  const unsigned char* frame = frames + f * 3 * (long long)H * W;
  unsigned char* y = Y + f * 4 * (long long)ch * cw;
  for (int k = 0; k < 4; ++k) {
    const int py = 2 * cy + (k >> 1), px = 2 * cx + (k & 1);
    y[(long long)py * 2 * cw + px] = (unsigned char)v8_luma(frame, H, W, py, px);
  }
  int u, v;
  v8_chroma(frame, H, W, cy, cx, &u, &v);
  U[i] = (unsigned char)u;
  V[i] = (unsigned char)v;
}

__global__ __launch_bounds__(kThreads) void vp8_analyse_kernel(const unsigned char* __restrict__ Y, const unsigned char* __restrict__ U,
                                                               const unsigned char* __restrict__ V, unsigned char* ry, unsigned char* ru,
                                                               unsigned char* rv, short* __restrict__ levels, unsigned char* __restrict__ modes,
                                                               unsigned* __restrict__ nz, int* __restrict__ skipped, int mbh, int mbw, int q) {
  __shared__ int skip_s;
  const long long f = blockIdx.x, mbs = (long long)mbh * mbw;
  const long ys = 16l * mbw, cs = 8l * mbw;
  const long long yo = f * 256 * mbs, co = f * 64 * mbs;
  const V8Quant m = v8_quant(q);
  if (threadIdx.x == 0) skip_s = 0;
  int mine = 0;
  for (int d = 0; d < mbh + mbw - 1; ++d) {                        // uniform over the workgroup: every thread reaches every barrier
    const int lo = d >= mbw ? d - mbw + 1 : 0, hi = d < mbh ? d : mbh - 1;
    for (int my = lo + (int)threadIdx.x; my <= hi; my += kThreads) {
      const int mx = d - my;
      const long long k = f * mbs + (long long)my * mbw + mx;
      const unsigned mask = v8_encode_mb(Y + yo, U + co, V + co, ry + yo, ru + co, rv + co, ys, cs, my, mx, m, levels + k * V8_MB_LEVELS, modes + 2 * k);
      nz[k] = mask;
      mine += mask == 0u;
    }
    __syncthreads();                                               // the diagonal's reconstruction is visible to the next one
  }
  atomicAdd(&skip_s, mine);
  __syncthreads();
  if (threadIdx.x == 0) skipped[f] = skip_s;
}

__global__ __launch_bounds__(64) void vp8_code_kernel(const short* __restrict__ levels, const unsigned* __restrict__ nz,
                                                      const unsigned char* __restrict__ modes, const int* __restrict__ skipped,
                                                      unsigned char* __restrict__ slots, long long* __restrict__ counts, int mbh, int mbw, int q,
                                                      int parts, int filter_level, long long first_bytes, long long token_bytes) {
  __shared__ unsigned char probs_s[1056];                          // the token probabilities, read at every symbol
  v8_coef_table(probs_s, (int)threadIdx.x, 64);
  __syncthreads();
  if (threadIdx.x != 0) return;
  const long long f = blockIdx.x / (parts + 1), mbs = (long long)mbh * mbw;
  const int p = (int)(blockIdx.x % (parts + 1));
  unsigned char* slot = slots + f * (first_bytes + parts * token_bytes);
  long long bytes;
  if (p == 0) {
    const int log2_parts = parts == 8 ? 3 : parts == 4 ? 2 : parts == 2 ? 1 : 0;
    bytes = v8_code_first(nz + f * mbs, modes + 2 * f * mbs, mbh, mbw, q, log2_parts, filter_level, skipped[f], slot, first_bytes);
  } else {
    bytes = v8_code_tokens(levels + f * mbs * V8_MB_LEVELS, nz + f * mbs, probs_s, mbh, mbw, p - 1, parts, slot + first_bytes + (p - 1) * token_bytes,
                           token_bytes);
  }
  counts[blockIdx.x] = bytes;
}

__global__ __launch_bounds__(kThreads) void vp8_pack_kernel(const unsigned char* __restrict__ slots, const long long* __restrict__ counts,
                                                            unsigned char* __restrict__ out, const long long* __restrict__ out_off,
                                                            long long out_bytes, int H, int W, int parts, long long first_bytes,
                                                            long long token_bytes) {
  const long long f = blockIdx.x;
  const int t = threadIdx.x;
  long long lo = out_off[f], len = out_off[f + 1] - lo;                      // the frame's bytes: out[lo, lo + len), clamped to the buffer
  if (lo < 0 || lo > out_bytes) lo = out_bytes;
  len = max(0ll, min(len, out_bytes - lo));
  unsigned char* dst = out + lo;
  const unsigned char* slot = slots + f * (first_bytes + parts * token_bytes);
  const long long* cnt = counts + f * (parts + 1);
  const long long first = max(0ll, min(cnt[0], first_bytes));
  if (t < 10 + 3 * (parts - 1)) {
    unsigned b;
    if (t < 3) b = (unsigned)(((unsigned long long)first << 5 | 1u << 4) >> (8 * t));          // a shown key frame of profile 0
    else if (t < 6) b = t == 3 ? 0x9du : t == 4 ? 0x01u : 0x2au;
    else if (t < 8) b = (unsigned)W >> (8 * (t - 6));
    else if (t < 10) b = (unsigned)H >> (8 * (t - 8));
    else b = (unsigned)(max(0ll, min(cnt[1 + (t - 10) / 3], token_bytes)) >> (8 * ((t - 10) % 3)));
    const long long at = t < 10 ? t : 10 + first + (t - 10);
    if (at < len) dst[at] = (unsigned char)b;
  }
  for (long long i = t; i < first; i += kThreads)
    if (10 + i < len) dst[10 + i] = slot[i];
  long long at = 10 + first + 3 * (parts - 1);
  for (int p = 0; p < parts; ++p) {
    const long long c = max(0ll, min(cnt[1 + p], token_bytes));
    const unsigned char* src = slot + first_bytes + p * token_bytes;
    for (long long i = t; i < c; i += kThreads)
      if (at + i < len) dst[at + i] = src[i];
    at += c;
  }
}

struct Geometry {
  int mbh, mbw;
  long long mbs, first_bytes, token_bytes;
};
bool frame_ok(int n, int H, int W) { return n >= 1 && H >= 1 && W >= 1 && H <= V8_MAX_SIDE && W <= V8_MAX_SIDE; }
bool parts_ok(int parts) { return parts == 1 || parts == 2 || parts == 4 || parts == 8; }
Geometry geometry(int H, int W, int parts) {
  Geometry g;
  g.mbh = (H + 15) / 16, g.mbw = (W + 15) / 16;
  g.mbs = (long long)g.mbh * g.mbw;
  g.first_bytes = v8_first_slot_bytes(g.mbs);
  g.token_bytes = v8_token_slot_bytes((long long)((g.mbh + parts - 1) / parts) * g.mbw);
  return g;
}
const char* kBadFrame = "%s: n = %d frames of %d x %d are outside the range (n, H, W >= 1, H, W <= %d, n * macroblocks < 2^31 / %d)";

}  // namespace

extern "C" int mmgt_vp8_quantiser(int quality, int* q, int* filter_level) {
  MMGT_CHECK(q && filter_level, "vp8_quantiser: null pointer");
  MMGT_CHECK(quality >= 0 && quality <= 100, "vp8_quantiser: quality = %d is outside 0 .. 100", quality);
  *q = v8_quality_to_q(quality);
  *filter_level = v8_default_filter_level(*q);
  return 0;
}

extern "C" int mmgt_vp8_slot_bytes(int H, int W, int parts, long long* first_bytes, long long* token_bytes) {
  MMGT_CHECK(first_bytes && token_bytes, "vp8_slot_bytes: null pointer");
  MMGT_CHECK(frame_ok(1, H, W), kBadFrame, "vp8_slot_bytes", 1, H, W, V8_MAX_SIDE, 1);
  MMGT_CHECK(parts_ok(parts), "vp8_slot_bytes: partitions = %d, must be 1, 2, 4 or 8", parts);
  const Geometry g = geometry(H, W, parts);
  *first_bytes = g.first_bytes, *token_bytes = g.token_bytes;
  return 0;
}

extern "C" int mmgt_vp8_convert(const unsigned char* frames, unsigned char* Y, unsigned char* U, unsigned char* V, int n, int H, int W, void* stream) {
  MMGT_CHECK(frames && Y && U && V, "vp8_convert: null pointer");
  const Geometry g = geometry(H > 0 ? H : 1, W > 0 ? W : 1, 1);
  MMGT_CHECK(frame_ok(n, H, W) && n * g.mbs <= 0x7fffffffll / 64, kBadFrame, "vp8_convert", n, H, W, V8_MAX_SIDE, 64);
  const long long total = n * g.mbs * 64;
  hipLaunchKernelGGL(vp8_convert_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, frames, Y, U, V,
                     H, W, 8 * g.mbh, 8 * g.mbw, total);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_vp8_analyse(const unsigned char* Y, const unsigned char* U, const unsigned char* V, unsigned char* ry, unsigned char* ru,
                                unsigned char* rv, short* levels, unsigned char* modes, unsigned int* nz, int* skipped, int n, int H, int W, int q,
                                void* stream) {
  MMGT_CHECK(Y && U && V && ry && ru && rv && levels && modes && nz && skipped, "vp8_analyse: null pointer");
  const Geometry g = geometry(H > 0 ? H : 1, W > 0 ? W : 1, 1);
  MMGT_CHECK(frame_ok(n, H, W) && n * g.mbs <= 0x7fffffffll / 64, kBadFrame, "vp8_analyse", n, H, W, V8_MAX_SIDE, 64);
  MMGT_CHECK(q >= 0 && q <= 127, "vp8_analyse: quantiser index = %d is outside 0 .. 127", q);
  hipLaunchKernelGGL(vp8_analyse_kernel, dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, Y, U, V, ry, ru, rv, levels, modes, nz, skipped,
                     g.mbh, g.mbw, q);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_vp8_code(const short* levels, const unsigned int* nz, const unsigned char* modes, const int* skipped, unsigned char* slots,
                             long long slots_bytes, long long* counts, int n, int H, int W, int q, int parts, int filter_level, void* stream) {
  MMGT_CHECK(levels && nz && modes && skipped && slots && counts, "vp8_code: null pointer");
  MMGT_CHECK(parts_ok(parts), "vp8_code: partitions = %d, must be 1, 2, 4 or 8", parts);
  const Geometry g = geometry(H > 0 ? H : 1, W > 0 ? W : 1, parts);
  MMGT_CHECK(frame_ok(n, H, W) && n * g.mbs <= 0x7fffffffll / 64, kBadFrame, "vp8_code", n, H, W, V8_MAX_SIDE, 64);
  MMGT_CHECK(q >= 0 && q <= 127, "vp8_code: quantiser index = %d is outside 0 .. 127", q);
  MMGT_CHECK(filter_level >= 0 && filter_level <= 63, "vp8_code: filter level = %d is outside 0 .. 63", filter_level);
  MMGT_CHECK(slots_bytes >= n * (g.first_bytes + parts * g.token_bytes), "vp8_code: slots_bytes = %lld, %d frames need %lld each", slots_bytes, n,
             g.first_bytes + parts * g.token_bytes);
  hipLaunchKernelGGL(vp8_code_kernel, dim3((unsigned)(n * (parts + 1))), dim3(64), 0, (hipStream_t)stream, levels, nz, modes, skipped, slots, counts,
                     g.mbh, g.mbw, q, parts, filter_level, g.first_bytes, g.token_bytes);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_vp8_pack(const unsigned char* slots, long long slots_bytes, const long long* counts, unsigned char* out, const long long* out_off,
                             long long out_bytes, int n, int H, int W, int parts, void* stream) {
  MMGT_CHECK(slots && counts && out && out_off, "vp8_pack: null pointer");
  MMGT_CHECK(parts_ok(parts), "vp8_pack: partitions = %d, must be 1, 2, 4 or 8", parts);
  const Geometry g = geometry(H > 0 ? H : 1, W > 0 ? W : 1, parts);
  MMGT_CHECK(frame_ok(n, H, W) && n * g.mbs <= 0x7fffffffll / 64, kBadFrame, "vp8_pack", n, H, W, V8_MAX_SIDE, 64);
  MMGT_CHECK(out_bytes >= 1 && slots_bytes >= n * (g.first_bytes + parts * g.token_bytes), "vp8_pack: out_bytes = %lld, slots_bytes = %lld, %d frames need %lld each",
             out_bytes, slots_bytes, n, g.first_bytes + parts * g.token_bytes);
  hipLaunchKernelGGL(vp8_pack_kernel, dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, slots, counts, out, out_off, out_bytes, H, W, parts,
                     g.first_bytes, g.token_bytes);
  MMGT_LAUNCH_CHECK();
  return 0;
}
