// WebP lossless / animated WebP decoder for device-resident input (mmgt_amd/video_in.py): the way back in of what csrc/webp.hip writes,
// and of any stock writer's VP8L.  The arithmetic is csrc/webpdec_core.h (also compiled into a host program, tools/webpdec_host_check.cpp); this
// file is the three launches over a set of frames.  The host parses the container, refuses what is out of scope and hands over the VP8L payloads of
// all frames as ONE buffer, with a table row per frame (webpdec_core.h: WD_X .. WD_PH).
//
//  * mmgt_webp_decode        one wave (a 64-thread workgroup) per stream -> the frame's scratch words (header block, sub-images, main image) and a
//                            status word
//  * mmgt_webp_untransform   one wave per frame: its transforms undone in its own order -> the ARGB words of its rectangle, and a status word
//  * mmgt_webp_compose       one thread per canvas pixel, through the call's frames in order with the RGBA canvas pixel in registers
//                            -> (n, H, W, 3) uint8 RGB, libwebp's composition; the canvas is carried to the next call in `carry`
//
// No atomics on any output: every scratch word, ARGB word, pixel byte and carry word has exactly one writer.
#include "common.h"
#include "webpdec_core.h"
#include "mmgt_hip.h"

namespace {

__global__ __launch_bounds__(64) void webp_decode_kernel(const unsigned char* __restrict__ data, long long data_bytes, const long long* __restrict__ tab,
                                                         uint32_t* scratch, long long scratch_words, int* __restrict__ status) {
  __shared__ WdShared sh;
  long long steps;
  const int st = wd_decode_stream(&sh, data, data_bytes, tab + (size_t)blockIdx.x * WD_TAB, scratch, scratch_words, &steps);
  if (threadIdx.x == 0) status[blockIdx.x] = st;
}

__global__ __launch_bounds__(64) void webp_untransform_kernel(const long long* __restrict__ tab, uint32_t* scratch, long long scratch_words,
                                                              uint32_t* argb, long long argb_words, int* __restrict__ status) {
  __shared__ uint32_t palette[256];
  const int st = wd_untransform_frame(palette, tab + (size_t)blockIdx.x * WD_TAB, scratch, scratch_words, argb, argb_words);
  if (threadIdx.x == 0) status[blockIdx.x] = st;
}

__global__ __launch_bounds__(256) void webp_compose_kernel(const long long* __restrict__ tab, int n, const uint32_t* __restrict__ argb,
                                                           long long argb_words, uint32_t* carry, unsigned char* __restrict__ out, int H, int W) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < (long long)H * W) wd_compose_pixel(tab, n, argb, argb_words, carry, out, H, W, p);
}

}  // namespace

extern "C" int mmgt_webp_decode(const unsigned char* data, long long data_bytes, const long long* tab, unsigned int* scratch, long long scratch_words,
                                int* status, int n, void* stream) {
  MMGT_CHECK(data && tab && scratch && status, "webp_decode: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && data_bytes >= 16 && data_bytes % 16 == 0 && scratch_words >= WD_HDR,
             "webp_decode: n = %d frames, %lld input bytes and %lld scratch words are outside the range (1 <= n <= 65535, data_bytes a positive "
             "multiple of 16, scratch_words >= 32)", n, data_bytes, scratch_words);
  MMGT_CHECK(((uintptr_t)data & 15) == 0 && ((uintptr_t)scratch & 15) == 0, "webp_decode: data or scratch is outside the range (both pointers 16-byte aligned)");
  hipLaunchKernelGGL(webp_decode_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, data, data_bytes, tab, scratch, scratch_words, status);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_webp_untransform(const long long* tab, unsigned int* scratch, long long scratch_words, unsigned int* argb, long long argb_words,
                                     int* status, int n, void* stream) {
  MMGT_CHECK(tab && scratch && argb && status, "webp_untransform: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && scratch_words >= WD_HDR && argb_words >= 1,
             "webp_untransform: n = %d frames, %lld scratch words and %lld ARGB words are outside the range (1 <= n <= 65535, scratch_words >= 32, "
             "argb_words >= 1)", n, scratch_words, argb_words);
  hipLaunchKernelGGL(webp_untransform_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, tab, scratch, scratch_words, argb, argb_words, status);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_webp_compose(const long long* tab, const unsigned int* argb, long long argb_words, unsigned int* carry, unsigned char* out, int n,
                                 int H, int W, void* stream) {
  MMGT_CHECK(tab && argb && carry && out, "webp_compose: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && H >= 1 && W >= 1 && H <= WD_MAX_SIDE && W <= WD_MAX_SIDE && argb_words >= 1,
             "webp_compose: n = %d frames on a %d x %d canvas with %lld ARGB words are outside the range (1 <= n <= 65535, sides 1 .. 16384, "
             "argb_words >= 1)", n, W, H, argb_words);
  const long long pixels = (long long)H * W;
  hipLaunchKernelGGL(webp_compose_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tab, n, argb, argb_words, carry,
                     out, H, W);
  MMGT_LAUNCH_CHECK();
  return 0;
}
