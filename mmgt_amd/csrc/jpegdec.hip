// Baseline JPEG decoder for device-resident Motion-JPEG / .jpg input (mmgt_amd/video_in.py): the way back in of what csrc/mjpeg.hip writes.
// The arithmetic is csrc/jpegdec_core.h (also compiled into a host program, tools/jpegdec_host_check.cpp); this file is the three launches over a
// batch of equally sized frames.  The host parses the markers, refuses what is out of scope, and hands over the entropy-coded bytes of all
// restart segments as ONE buffer with offsets, a descriptor per segment and a table block per frame.
//
//  * mmgt_jpegdec_entropy  one LANE per restart segment (segments are independent: byte-aligned, DC predictors reset).  The coefficient buffer is
//                          zero-filled by a memset on the same stream; a lane writes int16 coefficients in natural order into the blocks of its own
//                          MCU range only and leaves a status word; descriptors are checked against the batch before anything is read.
//  * mmgt_jpegdec_idct     one thread per 8 x 8 block: dequantise + jpeg_idct_islow -> one uint8 plane per component at its MCU-padded size
//  * mmgt_jpegdec_color    one thread per output pixel: chroma up-sampling, YCbCr -> RGB, crop -> (n, H, W, 3) uint8
//
// No atomics and no dependence on launch order: every coefficient, sample and pixel has exactly one writer.
#include "common.h"
#include "jpegdec_core.h"
#include "mmgt_hip.h"

namespace {

__global__ __launch_bounds__(64) void jpegdec_entropy_kernel(const unsigned char* __restrict__ data, const long long* __restrict__ offsets,
                                                             const int* __restrict__ seginfo, const int* __restrict__ tables,
                                                             short* __restrict__ coef, int* __restrict__ status, JdGeom g, int n, int nseg,
                                                             long long data_bytes) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= nseg) return;
  status[s] = jd_segment(data, data_bytes, offsets, seginfo, tables, coef, g, n, s);
}

__global__ __launch_bounds__(64) void jpegdec_idct_kernel(const short* __restrict__ coef, const int* __restrict__ tables,
                                                          unsigned char* __restrict__ planes, JdGeom g, long long blocks) {
  const long long b = (long long)blockIdx.x * 64 + threadIdx.x;
  if (b >= blocks) return;
  jd_block(coef, tables, planes, g, b);
}

__global__ __launch_bounds__(256) void jpegdec_color_kernel(const unsigned char* __restrict__ planes, unsigned char* __restrict__ out, JdGeom g,
                                                            long long pixels) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  jd_output_pixel(planes, out, g, p);
}

const char* kBadGeom = "%s: %d frames of %d x %d with %d components, luma sampling %d x %d are not decoded (1 .. 65535 a side; one component, or three "
                       "with luma 1x1, 2x1 or 2x2 and chroma 1x1; the grids hold 2^31 - 1 blocks / pixels)";
bool geom(int n, int H, int W, int ncomp, int hs, int vs, JdGeom& g) {
  if (n < 1 || !jd_geom(H, W, ncomp, hs, vs, &g)) return false;
  return (long long)n * jd_frame_blocks(g) <= 0x7fffffffLL && (long long)n * H * W <= 0x7fffffffLL * 256;
}

}  // namespace

extern "C" int mmgt_jpegdec_sizes(int H, int W, int ncomp, int hs, int vs, long long* frame_blocks, int* table_ints) {
  JdGeom g;
  MMGT_CHECK(frame_blocks && table_ints, "jpegdec_sizes: null output");
  MMGT_CHECK(geom(1, H, W, ncomp, hs, vs, g), kBadGeom, "jpegdec_sizes", 1, W, H, ncomp, hs, vs);
  *frame_blocks = jd_frame_blocks(g);
  *table_ints = JD_TAB_INTS;
  return 0;
}

extern "C" int mmgt_jpegdec_entropy(const unsigned char* data, long long data_bytes, const long long* offsets, const int* seginfo, const int* tables,
                                    short* coef, int* status, int n, int nseg, int H, int W, int ncomp, int hs, int vs, void* stream) {
  JdGeom g;
  MMGT_CHECK(data && offsets && seginfo && tables && coef && status, "jpegdec_entropy: null pointer");
  MMGT_CHECK(geom(n, H, W, ncomp, hs, vs, g), kBadGeom, "jpegdec_entropy", n, W, H, ncomp, hs, vs);
  MMGT_CHECK(nseg >= n && data_bytes >= 0, "jpegdec_entropy: %d segments for %d frames, %lld bytes", nseg, n, data_bytes);
  const hipError_t e = hipMemsetAsync(coef, 0, (size_t)n * jd_frame_blocks(g) * 64 * sizeof(short), (hipStream_t)stream);
  MMGT_CHECK(e == hipSuccess, "jpegdec_entropy: zero fill of the coefficients: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(jpegdec_entropy_kernel, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, (hipStream_t)stream, data, offsets, seginfo, tables,
                     coef, status, g, n, nseg, data_bytes);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_jpegdec_idct(const short* coef, const int* tables, unsigned char* planes, int n, int H, int W, int ncomp, int hs, int vs,
                                 void* stream) {
  JdGeom g;
  MMGT_CHECK(coef && tables && planes, "jpegdec_idct: null pointer");
  MMGT_CHECK(geom(n, H, W, ncomp, hs, vs, g), kBadGeom, "jpegdec_idct", n, W, H, ncomp, hs, vs);
  const long long blocks = (long long)n * jd_frame_blocks(g);
  hipLaunchKernelGGL(jpegdec_idct_kernel, dim3((unsigned)((blocks + 63) / 64)), dim3(64), 0, (hipStream_t)stream, coef, tables, planes, g, blocks);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_jpegdec_color(const unsigned char* planes, unsigned char* out, int n, int H, int W, int ncomp, int hs, int vs, void* stream) {
  JdGeom g;
  MMGT_CHECK(planes && out, "jpegdec_color: null pointer");
  MMGT_CHECK(geom(n, H, W, ncomp, hs, vs, g), kBadGeom, "jpegdec_color", n, W, H, ncomp, hs, vs);
  const long long pixels = (long long)n * H * W;
  hipLaunchKernelGGL(jpegdec_color_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, planes, out, g, pixels);
  MMGT_LAUNCH_CHECK();
  return 0;
}
