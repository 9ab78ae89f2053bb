// PNG / APNG decoder for device-resident input (mmgt_amd/video_in.py): the way back in of what csrc/png.hip writes, and of any stock
// writer's non-interlaced 8-bit-or-less PNG.  The arithmetic is csrc/pngdec_core.h (also compiled into a host program, tools/pngdec_host_check.cpp);
// this file is the three launches over a batch of frames of one geometry.  The host parses the chunks, refuses what is out of scope, and hands over
// the raw deflate bytes of all frames as ONE buffer with offsets.
//
//  * mmgt_png_inflate    one wave (a 64-thread workgroup) per stream -> the frame's filtered bytes (H, 1 + row bytes) and a status word
//  * mmgt_png_unfilter   one wave per frame: scanlines reconstructed in place, rows skewed across lanes, and the two Adler-32 sums of every row
//  * mmgt_png_expand     one thread per output pixel -> (n, H, W, 3) uint8 RGB, PIL's convert("RGB")
//
// No atomics and no dependence on launch order: every filtered byte, reconstructed byte and pixel has exactly one writer.
#include "common.h"
#include "pngdec_core.h"
#include "mmgt_hip.h"

namespace {

__global__ __launch_bounds__(64) void png_inflate_kernel(const unsigned char* __restrict__ data, long long data_bytes, const long long* __restrict__ offsets,
                                                         unsigned char* __restrict__ filt, int* __restrict__ status, long long frame_bytes) {
  __shared__ PdShared sh;
  const size_t f = blockIdx.x;
  const long long at = (long long)f * frame_bytes;
  long long steps;
  const int st = pd_inflate_stream(&sh, data, data_bytes, offsets[f], offsets[f + 1], filt + at, (int)frame_bytes, (int)(at & 15), &steps);
  if (threadIdx.x == 0) status[f] = st;
}

__global__ __launch_bounds__(64) void png_unfilter_kernel(unsigned char* __restrict__ filt, long long* __restrict__ sums, int* __restrict__ status, PdGeom g) {
  const size_t f = blockIdx.x;
  const int st = pd_unfilter_frame(filt + f * (size_t)pd_frame_bytes(g), sums + f * 2 * (size_t)g.H, g);
  if (threadIdx.x == 0) status[f] = st;
}

__global__ __launch_bounds__(256) void png_expand_kernel(const unsigned char* __restrict__ filt, const unsigned char* __restrict__ palette,
                                                         const int* __restrict__ plte_len, unsigned char* __restrict__ out, int* __restrict__ status,
                                                         PdGeom g, long long pixels) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  if (pd_expand_pixel(filt, palette, plte_len, out, g, p)) status[p / ((long long)g.H * g.W)] = PD_ST_PALETTE;      // every writer stores the same word
}

const char* kBadGeom = "%s: n = %d frames of %d x %d, colour type %d at %d bits are outside the range (n >= 1, sides 1 .. 16384; colour type 0 or 3 at 1, 2, "
                       "4 or 8 bits, 2, 4 or 6 at 8 bits; n * H * W < 2^39)";
bool geom(int n, int H, int W, int ct, int depth, PdGeom& g) {
  return n >= 1 && pd_geom(H, W, ct, depth, &g) && (long long)n * H * W <= 0x7fffffffLL * 256;
}

}  // namespace

extern "C" int mmgt_png_inflate(const unsigned char* data, long long data_bytes, const long long* offsets, unsigned char* filt, int* status, int n,
                                long long frame_bytes, void* stream) {
  MMGT_CHECK(data && offsets && filt && status, "png_inflate: null pointer");
  MMGT_CHECK(n >= 1 && frame_bytes >= 1 && frame_bytes <= (long long)PD_MAX_SIDE * (1 + 4 * PD_MAX_SIDE) && data_bytes >= 16 && data_bytes % 16 == 0,
             "png_inflate: n = %d streams of %lld output bytes from %lld input bytes are outside the range (n >= 1, 1 <= frame_bytes <= 16384 * 65537, "
             "data_bytes a positive multiple of 16)", n, frame_bytes, data_bytes);
  MMGT_CHECK(((uintptr_t)data & 15) == 0 && ((uintptr_t)filt & 15) == 0, "png_inflate: data or filt is outside the range (both pointers 16-byte aligned)");
  hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, data, data_bytes, offsets, filt, status, frame_bytes);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_png_unfilter(unsigned char* filt, long long* sums, int* status, int n, int H, int W, int colour_type, int depth, void* stream) {
  PdGeom g;
  MMGT_CHECK(filt && sums && status, "png_unfilter: null pointer");
  MMGT_CHECK(geom(n, H, W, colour_type, depth, g), kBadGeom, "png_unfilter", n, W, H, colour_type, depth);
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, filt, sums, status, g);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_png_expand(const unsigned char* filt, const unsigned char* palette, const int* plte_len, unsigned char* out, int* status, int n,
                               int H, int W, int colour_type, int depth, void* stream) {
  PdGeom g;
  MMGT_CHECK(filt && out && status, "png_expand: null pointer");
  MMGT_CHECK(geom(n, H, W, colour_type, depth, g), kBadGeom, "png_expand", n, W, H, colour_type, depth);
  MMGT_CHECK(colour_type != 3 || (palette && plte_len), "png_expand: colour type 3 needs a palette block and its lengths (null pointer)");
  const hipError_t e = hipMemsetAsync(status, 0, (size_t)n * sizeof(int), (hipStream_t)stream);
  MMGT_CHECK(e == hipSuccess, "png_expand: zero fill of the status words: %s", hipGetErrorString(e));
  const long long pixels = (long long)n * H * W;
  hipLaunchKernelGGL(png_expand_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, filt, palette, plte_len, out, status,
                     g, pixels);
  MMGT_LAUNCH_CHECK();
  return 0;
}
