// Lossy WebP decoder for device-resident input (mmgt_amd/video_in.py): VP8 key frames, the way back in of what csrc/vp8.hip writes and of
// any stock writer's lossy .webp.  The arithmetic is csrc/vp8dec_core.h (also compiled into a host program, tools/vp8dec_host_check.cpp); this file
// is the four launches over a set of frames.  The host parses the container and the 10-byte frame header, refuses what is out of scope and hands
// over the `VP8 ` payloads of all frames as ONE buffer, with a table row per frame (vp8dec_core.h: V8D_BEGIN .. V8D_H).
//
//  * mmgt_vp8dec_parse        one workgroup of eight waves per frame.  Lane 0 of wave 0 reads the first partition (header, then every macroblock's
//                             segment, skip flag and modes); then lane 0 of wave p reads token partition p, the waves one macroblock apart with a
//                             barrier per step, so that the non-zero context of the row above is there when it is read.  The coefficient
//                             probabilities (1056 bytes) and the header sit in LDS.  -> header block, modes, dequantised coefficients
//  * mmgt_vp8dec_reconstruct  one workgroup per frame: prediction + residual along the fronts x + 2 y (a 4 x 4-predicted macroblock reads its
//                             above-right neighbour), a barrier between fronts -> the unfiltered planes
//  * mmgt_vp8dec_filter       the loop filter in place along the same fronts: libwebp filters in raster order, and the left edge of macroblock
//                             (x + 1, y - 1) changes pixels that the top edge of (x, y) reads
//  * mmgt_vp8dec_output       one thread per pixel: fancy upsampling, YUV -> RGB -> the ARGB words (alpha 255) that mmgt_webp_compose takes
//
// No workgroup waits on another and no wave spins on memory: barriers only, reached by every thread, with trip counts from the table row's sizes.
// No atomics on any output: every scratch byte, ARGB word and status word has exactly one writer.
#include "common.h"
#include "vp8dec_core.h"
#include "mmgt_hip.h"

namespace {

struct ParseShared {
  unsigned char probs[1056];
  V8dHdr hdr;
  long long part[16];
  int status, eof[8];
};

__global__ __launch_bounds__(512) void vp8dec_parse_kernel(const unsigned char* __restrict__ data, long long data_bytes, const long long* __restrict__ tab,
                                                           uint32_t* scratch, long long scratch_words, int* __restrict__ status) {
  __shared__ ParseShared sh;
  V8dFrame f;
  const int row = v8d_frame(tab + (size_t)blockIdx.x * V8D_TAB, scratch, scratch_words, data_bytes, 1ll << 62, &f);   // the same for every thread
  if (row) {
    if (threadIdx.x == 0) status[blockIdx.x] = row;
    return;
  }
  v8_coef_table(sh.probs, threadIdx.x, 512);
  if (threadIdx.x < 8) sh.eof[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x == 0) sh.status = v8d_parse_first(&f, data, &sh.hdr, sh.probs, sh.part);
  __syncthreads();
  if (sh.status) {                                                  // uniform: read from LDS after the barrier
    if (threadIdx.x == 0) status[blockIdx.x] = sh.status;
    return;
  }
  const int parts = sh.hdr.parts, p = threadIdx.x >> 6;
  const bool worker = (threadIdx.x & 63) == 0 && p < parts;
  V8dWorker w;
  w.lnz = w.ldc = 0;
  v8d_bool_init(&w.br, data, worker ? sh.part[2 * p] : 0, worker ? sh.part[2 * p + 1] : 0);
  const long long steps = v8d_token_steps(&f, parts);               // from the row's sizes and 1 .. 8 partitions
  for (long long s = 0; s < steps; ++s) {
    if (worker) v8d_token_step(&f, &sh.hdr, sh.probs, &w, p, s);
    __syncthreads();
  }
  if (worker) sh.eof[p] = w.br.eof;
  __syncthreads();
  if (threadIdx.x == 0) {
    int bad = 0;
    for (int i = 0; i < parts && i < f.mbh; ++i) bad |= sh.eof[i];      // a partition without a macroblock row is never read
    if (!bad) f.hdr[V8D_H_MAGIC] = V8D_MAGIC;
    status[blockIdx.x] = bad ? V8D_ST_TOKEN_END : V8D_OK;
  }
}

// pass 0: reconstruct, pass 1: loop filter.  One thread per macroblock of a front.
template <int PASS>
__global__ __launch_bounds__(64) void vp8dec_front_kernel(const long long* __restrict__ tab, uint32_t* scratch, long long scratch_words,
                                                          int* __restrict__ status) {
  V8dFrame f;
  const int row = v8d_frame(tab + (size_t)blockIdx.x * V8D_TAB, scratch, scratch_words, 1ll << 62, 1ll << 62, &f);
  const bool ready = row == V8D_OK && f.hdr[V8D_H_MAGIC] == (uint32_t)V8D_MAGIC;   // uniform: nothing in this launch writes the header block
  if (threadIdx.x == 0) status[blockIdx.x] = row ? row : ready ? V8D_OK : V8D_ST_UPSTREAM;
  if (!ready) return;
  const int filter_type = (int)f.hdr[V8D_H_FILTER];
  if (PASS == 1 && filter_type == 0) return;
  const int fronts = f.mbw + 2 * (f.mbh - 1);
  for (int front = 0; front < fronts; ++front) {
    for (int my = threadIdx.x; my < f.mbh; my += 64) {
      const int mx = front - 2 * my;
      if (mx < 0 || mx >= f.mbw) continue;
      if (PASS == 0) v8d_recon_mb(&f, my, mx);
      else v8d_filter_mb(&f, filter_type, f.hdr + V8D_H_FS, my, mx, nullptr);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void vp8dec_output_kernel(const long long* __restrict__ tab, uint32_t* scratch, long long scratch_words,
                                                            uint32_t* argb, long long argb_words, int* __restrict__ status) {
  V8dFrame f;
  const int row = v8d_frame(tab + (size_t)blockIdx.y * V8D_TAB, scratch, scratch_words, 1ll << 62, argb_words, &f);
  const bool ready = row == V8D_OK && f.hdr[V8D_H_MAGIC] == (uint32_t)V8D_MAGIC;
  if (blockIdx.x == 0 && threadIdx.x == 0) status[blockIdx.y] = row ? row : ready ? V8D_OK : V8D_ST_UPSTREAM;
  if (!ready) return;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)f.W * f.H) return;
  const int y = (int)(p / f.W), x = (int)(p - (long long)y * f.W);
  argb[f.pix + p] = v8d_pixel(&f, y, x);
}

}  // namespace

extern "C" int mmgt_vp8dec_parse(const unsigned char* data, long long data_bytes, const long long* tab, unsigned int* scratch, long long scratch_words,
                                 int* status, int n, void* stream) {
  MMGT_CHECK(data && tab && scratch && status, "vp8dec_parse: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && data_bytes >= 16 && data_bytes % 16 == 0 && scratch_words >= V8D_HDR,
             "vp8dec_parse: n = %d frames, %lld input bytes and %lld scratch words are outside the range (1 <= n <= 65535, data_bytes a positive "
             "multiple of 16, scratch_words >= 64)", n, data_bytes, scratch_words);
  MMGT_CHECK(((uintptr_t)scratch & 15) == 0, "vp8dec_parse: scratch is outside the range (16-byte aligned)");
  hipLaunchKernelGGL(vp8dec_parse_kernel, dim3((unsigned)n), dim3(512), 0, (hipStream_t)stream, data, data_bytes, tab, scratch, scratch_words, status);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_vp8dec_reconstruct(const long long* tab, unsigned int* scratch, long long scratch_words, int* status, int n, void* stream) {
  MMGT_CHECK(tab && scratch && status, "vp8dec_reconstruct: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && scratch_words >= V8D_HDR && ((uintptr_t)scratch & 15) == 0,
             "vp8dec_reconstruct: n = %d frames and %lld scratch words are outside the range (1 <= n <= 65535, scratch_words >= 64, scratch 16-byte "
             "aligned)", n, scratch_words);
  hipLaunchKernelGGL(vp8dec_front_kernel<0>, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, tab, scratch, scratch_words, status);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_vp8dec_filter(const long long* tab, unsigned int* scratch, long long scratch_words, int* status, int n, void* stream) {
  MMGT_CHECK(tab && scratch && status, "vp8dec_filter: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && scratch_words >= V8D_HDR && ((uintptr_t)scratch & 15) == 0,
             "vp8dec_filter: n = %d frames and %lld scratch words are outside the range (1 <= n <= 65535, scratch_words >= 64, scratch 16-byte "
             "aligned)", n, scratch_words);
  hipLaunchKernelGGL(vp8dec_front_kernel<1>, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, tab, scratch, scratch_words, status);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_vp8dec_output(const long long* tab, unsigned int* scratch, long long scratch_words, unsigned int* argb, long long argb_words,
                                  int* status, int n, long long max_pixels, void* stream) {
  MMGT_CHECK(tab && scratch && argb && status, "vp8dec_output: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && scratch_words >= V8D_HDR && argb_words >= 1 && max_pixels >= 1 &&
                 max_pixels <= (long long)V8_MAX_SIDE * V8_MAX_SIDE && ((uintptr_t)scratch & 15) == 0,
             "vp8dec_output: n = %d frames, %lld scratch words, %lld ARGB words and %lld pixels in the largest frame are outside the range (1 <= n <= "
             "65535, scratch_words >= 64, argb_words >= 1, 1 <= max_pixels <= 16383 * 16383, scratch 16-byte aligned)", n, scratch_words, argb_words,
             max_pixels);
  hipLaunchKernelGGL(vp8dec_output_kernel, dim3((unsigned)((max_pixels + 255) / 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream, tab, scratch,
                     scratch_words, argb, argb_words, status);
  MMGT_LAUNCH_CHECK();
  return 0;
}
