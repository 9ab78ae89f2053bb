// Progressive JPEG (SOF2) entropy stage for device-resident .jpg input (mmgt_amd/video_in.py): the second way of filling the
// coefficient buffer that csrc/jpegdec.hip's idct and colour launches consume.  The arithmetic is csrc/jpegprog_core.h (also compiled into a
// host program, tools/jpegprog_host_check.cpp); this file is the launch.  The host parses the markers, refuses what is out of scope, orders the
// scans of the batch into dependency levels and calls the entry once per level, lowest first.
//
//  * mmgt_jpegprog_entropy  one LANE per (scan of this level, restart segment): segments are independent (byte-aligned, DC predictors and EOBRUN
//                           reset).  The first call zero-fills the coefficient buffer by a memset on the same stream; a lane writes -- and in a
//                           refinement scan reads and rewrites -- int16 coefficients of its own blocks and band only and leaves a status word.
//                           Each lane has a wavefront to itself: the lanes are long serial loops over different scans that diverge at every
//                           symbol, and 24 of them in one wavefront ran three times as long as one alone; a typical batch has a few
//                           hundred lanes, far fewer than the device holds wavefronts.
//
// No atomics: the scans of one level touch disjoint (component, coefficient) pairs and the segments of a scan disjoint blocks, so within a launch
// every int16 has one writer; what a refinement reads was left by an earlier launch on the same stream.
#include "common.h"
#include "jpegprog_core.h"
#include "mmgt_hip.h"

namespace {

__global__ __launch_bounds__(64) void jpegprog_entropy_kernel(const unsigned char* __restrict__ data, const long long* __restrict__ offsets,
                                                              const int* __restrict__ seginfo, const int* __restrict__ scaninfo,
                                                              const int* __restrict__ huff, short* coef, int* __restrict__ status, JdGeom g, int n,
                                                              int nseg, int nscan, int nhuff, long long data_bytes) {
  __shared__ __attribute__((aligned(16))) short block_copy[64];           // a refinement lane's copy of the block it is in (pj_fetch_block)
  const int s = blockIdx.x;
  if (s >= nseg || threadIdx.x != 0) return;
  status[s] = pj_segment(data, data_bytes, offsets, seginfo, scaninfo, huff, coef, block_copy, g, n, nscan, nhuff, s);
}

}  // namespace

extern "C" int mmgt_jpegprog_entropy(const unsigned char* data, long long data_bytes, const long long* offsets, const int* seginfo,
                                     const int* scaninfo, const int* huff, short* coef, int* status, int n, int nseg, int nscan, int nhuff, int H,
                                     int W, int ncomp, int hs, int vs, int zero_fill, void* stream) {
  JdGeom g;
  MMGT_CHECK(data && offsets && seginfo && scaninfo && huff && coef && status, "jpegprog_entropy: null pointer");
  MMGT_CHECK(n >= 1 && jd_geom(H, W, ncomp, hs, vs, &g) && (long long)n * jd_frame_blocks(g) <= 0x7fffffffLL,
             "jpegprog_entropy: %d frames of %d x %d with %d components, luma sampling %d x %d are not decoded", n, W, H, ncomp, hs, vs);
  MMGT_CHECK(nseg >= 1 && nscan >= 1 && nhuff >= 1 && data_bytes >= 0, "jpegprog_entropy: %d segments, %d scans, %d tables, %lld bytes", nseg,
             nscan, nhuff, data_bytes);
  if (zero_fill) {
    const hipError_t e = hipMemsetAsync(coef, 0, (size_t)n * jd_frame_blocks(g) * 64 * sizeof(short), (hipStream_t)stream);
    MMGT_CHECK(e == hipSuccess, "jpegprog_entropy: zero fill of the coefficients: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(jpegprog_entropy_kernel, dim3((unsigned)nseg), dim3(64), 0, (hipStream_t)stream, data, offsets, seginfo,
                     scaninfo, huff, coef, status, g, n, nseg, nscan, nhuff, data_bytes);
  MMGT_LAUNCH_CHECK();
  return 0;
}
