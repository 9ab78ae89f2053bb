// GIF decoder for device-resident input (mmgt_amd/video_in.py): the way back in of what csrc/gif.hip writes, and of any stock writer's GIF.
// The arithmetic is csrc/gifdec_core.h (also compiled into a host program, tools/gifdec_host_check.cpp); this file is the two launches over a chunk of
// a file's frames.  The host parses the blocks, refuses what is out of scope, removes the sub-block framing and hands over the code streams of all
// frames as ONE buffer, with a table row per frame (gifdec_core.h: GD_X .. GD_FILL).
//
//  * mmgt_gif_unlzw     one wave (a 64-thread workgroup) per frame -> the W * H palette indices of its rectangle in stream order and a status word
//  * mmgt_gif_compose   one thread per canvas pixel, through the chunk's frames in order with the canvas and the pending restore in registers
//                       -> (n, H, W, 3) uint8 RGB, PIL's composition; the two planes are carried to the next chunk in `carry`
//
// No atomics: every index, pixel and carry byte has exactly one writer.
#include "common.h"
#include "gifdec_core.h"
#include "mmgt_hip.h"

namespace {

__global__ __launch_bounds__(64) void gif_unlzw_kernel(const unsigned char* __restrict__ data, long long data_bytes, const long long* __restrict__ tab,
                                                       unsigned char* idx, long long idx_bytes, int* __restrict__ status) {
  __shared__ GdShared sh;
  const long long* t = tab + (size_t)blockIdx.x * GD_TAB;
  int st = GD_ST_DESCRIPTOR;
  long long rounds;
  if (gd_row_ok(t, data_bytes, idx_bytes, GD_MAX_SIDE, GD_MAX_SIDE))
    st = gd_unlzw_stream(&sh, data, t[GD_BEGIN], t[GD_END], (int)t[GD_MCS], idx + t[GD_IDX], t[GD_W] * t[GD_H], &rounds);
  if (threadIdx.x == 0) status[blockIdx.x] = st;
}

__global__ __launch_bounds__(256) void gif_compose_kernel(const long long* __restrict__ tab, int n, const unsigned char* __restrict__ idx,
                                                          long long idx_bytes, const unsigned char* __restrict__ palette, unsigned char* carry,
                                                          unsigned char* __restrict__ out, int H, int W) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < (long long)H * W) gd_compose_pixel(tab, n, idx, idx_bytes, palette, carry, out, H, W, p);
}

}  // namespace

extern "C" int mmgt_gif_unlzw(const unsigned char* data, long long data_bytes, const long long* tab, unsigned char* idx, long long idx_bytes,
                              int* status, int n, void* stream) {
  MMGT_CHECK(data && tab && idx && status, "gif_unlzw: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && data_bytes >= 16 && data_bytes % 16 == 0 && idx_bytes >= 1,
             "gif_unlzw: n = %d frames, %lld input bytes and %lld index bytes are outside the range (1 <= n <= 65535, data_bytes a positive multiple "
             "of 16, idx_bytes >= 1)", n, data_bytes, idx_bytes);
  hipLaunchKernelGGL(gif_unlzw_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, data, data_bytes, tab, idx, idx_bytes, status);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_gif_compose(const long long* tab, const unsigned char* idx, long long idx_bytes, const unsigned char* palette, unsigned char* carry,
                                unsigned char* out, int n, int H, int W, void* stream) {
  MMGT_CHECK(tab && idx && palette && carry && out, "gif_compose: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && H >= 1 && W >= 1 && H <= GD_MAX_SIDE && W <= GD_MAX_SIDE && idx_bytes >= 1,
             "gif_compose: n = %d frames on a %d x %d canvas with %lld index bytes are outside the range (1 <= n <= 65535, sides 1 .. 16384, "
             "idx_bytes >= 1)", n, W, H, idx_bytes);
  const long long pixels = (long long)H * W;
  hipLaunchKernelGGL(gif_compose_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tab, n, idx, idx_bytes, palette,
                     carry, out, H, W);
  MMGT_LAUNCH_CHECK();
  return 0;
}
