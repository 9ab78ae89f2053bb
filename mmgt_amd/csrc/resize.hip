// Device image resize (gfx950): PIL's two-pass 8-bit resampling -- Image.resize with BILINEAR / BICUBIC / LANCZOS, which is what
// transforms.Resize on a PIL image (scripts/pose2vid.py:232, scripts/audio2vid.py:443), the 224 x 224 resize in front of CLIP
// (pipeline_pose2vid_long.py:383) and VaeImageProcessor.preprocess (:427) are -- on (n, H, W, C) uint8 frames that are already on the device.
// The arithmetic and every index live in resample_core.h, which a host program runs too; this file is the launches.
//
//  * mmgt_resize_u8   a horizontal launch if the width changes (into the caller's workspace when a vertical one follows), a vertical launch if
//                     the height changes, each one thread per item over a grid that covers frames x rows x columns; the last launch applies the
//                     epilogue (uint8 interleaved, or fp32 planar through the caller's lookup table).  A call that changes neither size is the
//                     epilogue alone.  The rounding to uint8 between the passes is PIL's and part of the result.
//  * the vertical pass reads and writes 4 bytes per lane wherever pitch and bases allow (taps of one output byte lie a whole row apart, so the
//    bytes next to each other in a row share their weights); the horizontal pass reads bytes: its taps start at any byte of a row.
#include "common.h"
#include "mmgt_hip.h"
#include "resample_core.h"

namespace {

constexpr int RS_BLOCK = 256;

template <int C>
__global__ __launch_bounds__(RS_BLOCK) void resize_h_kernel(const uint8_t* __restrict__ in, RsOut o, int n, int H, int Ws, int Wd,
                                                            const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, long items) {
  for (long i = blockIdx.x * (long)RS_BLOCK + threadIdx.x; i < items; i += (long)gridDim.x * RS_BLOCK)
    rs_h_item<C>(in, o, n, H, Ws, Wd, bounds, kk, ksize, i);
}

template <int V>
__global__ __launch_bounds__(RS_BLOCK) void resize_v_kernel(const uint8_t* __restrict__ in, RsOut o, int n, int Hs, int Hd, int W, int C,
                                                            const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, long items) {
  for (long i = blockIdx.x * (long)RS_BLOCK + threadIdx.x; i < items; i += (long)gridDim.x * RS_BLOCK)
    rs_v_item<V>(in, o, n, Hs, Hd, W, C, bounds, kk, ksize, i);
}

__global__ __launch_bounds__(RS_BLOCK) void resize_copy_kernel(const uint8_t* __restrict__ in, RsOut o, int n, int H, int W, int C, long items) {
  for (long i = blockIdx.x * (long)RS_BLOCK + threadIdx.x; i < items; i += (long)gridDim.x * RS_BLOCK) rs_copy_item(in, o, n, H, W, C, i);
}

// one thread per item up to 2^20 workgroups (a 1080p frame: 8100 of them on 256 CUs); beyond that the threads stride
inline dim3 grid_for(long items) {
  const long g = (items + RS_BLOCK - 1) / RS_BLOCK;
  return dim3((unsigned)(g > (1L << 20) ? (1L << 20) : g));
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" int mmgt_resize_u8_workspace(int n, int Hs, int Ws, int Hd, int Wd, int C, long long* bytes) {
  MMGT_CHECK(bytes, "resize_u8_workspace: bytes is null");
  MMGT_CHECK(rs_shape_ok(n, Hs, Ws, Hd, Wd, C), "resize_u8: n %d, %d x %d -> %d x %d, %d bands: n >= 1, sides 1 .. %d, 1 or 3 bands", n, Ws, Hs,
             Wd, Hd, C, (int)RS_MAX_SIDE);
  *bytes = rs_workspace_bytes(n, Hs, Ws, Hd, Wd, C);
  return 0;
}

extern "C" int mmgt_resize_u8(const unsigned char* in, unsigned char* tmp, unsigned char* out_u8, float* out_f32, const float* lut, int n, int Hs,
                              int Ws, int Hd, int Wd, int C, const int* bounds_x, const int* kk_x, int ksize_x, const int* bounds_y,
                              const int* kk_y, int ksize_y, void* stream) {
  MMGT_CHECK(rs_shape_ok(n, Hs, Ws, Hd, Wd, C), "resize_u8: n %d, %d x %d -> %d x %d, %d bands: n >= 1, sides 1 .. %d, 1 or 3 bands", n, Ws, Hs,
             Wd, Hd, C, (int)RS_MAX_SIDE);
  MMGT_CHECK(in && ((out_u8 != nullptr) != (out_f32 != nullptr)), "resize_u8: needs `in` and exactly one of out_u8 / out_f32");
  MMGT_CHECK(!out_f32 || lut, "resize_u8: out_f32 needs the lookup table (%d x 256 floats)", C);
  const bool horiz = Ws != Wd, vert = Hs != Hd;
  MMGT_CHECK(!horiz || (bounds_x && kk_x && ksize_x >= 1), "resize_u8: the width changes (%d -> %d): bounds_x, kk_x, ksize_x are needed", Ws, Wd);
  MMGT_CHECK(!vert || (bounds_y && kk_y && ksize_y >= 1), "resize_u8: the height changes (%d -> %d): bounds_y, kk_y, ksize_y are needed", Hs, Hd);
  MMGT_CHECK(!(horiz && vert) || tmp, "resize_u8: both sizes change: a workspace of mmgt_resize_u8_workspace bytes is needed");
  MMGT_CHECK(in != out_u8 && (!tmp || (tmp != in && tmp != out_u8)), "resize_u8: in, tmp and out must be different buffers");
  hipStream_t s = (hipStream_t)stream;
  const RsOut last{out_u8, out_f32, lut};
  const unsigned char* src = in;
  if (horiz) {
    const RsOut o = vert ? RsOut{tmp, nullptr, nullptr} : last;
    const long items = (long)n * Hs * Wd;
    if (C == 1)
      hipLaunchKernelGGL(resize_h_kernel<1>, grid_for(items), dim3(RS_BLOCK), 0, s, src, o, n, Hs, Ws, Wd, bounds_x, kk_x, ksize_x, items);
    else
      hipLaunchKernelGGL(resize_h_kernel<3>, grid_for(items), dim3(RS_BLOCK), 0, s, src, o, n, Hs, Ws, Wd, bounds_x, kk_x, ksize_x, items);
    MMGT_LAUNCH_CHECK();
    src = tmp;                                           // read only if a vertical pass follows
  }
  if (vert) {
    const long pitch = (long)Wd * C;
    if (pitch % 4 == 0 && aligned4(src) && (out_f32 || aligned4(out_u8))) {
      const long items = (long)n * Hd * (pitch / 4);
      hipLaunchKernelGGL(resize_v_kernel<4>, grid_for(items), dim3(RS_BLOCK), 0, s, src, last, n, Hs, Hd, Wd, C, bounds_y, kk_y, ksize_y, items);
    } else {
      const long items = (long)n * Hd * pitch;
      hipLaunchKernelGGL(resize_v_kernel<1>, grid_for(items), dim3(RS_BLOCK), 0, s, src, last, n, Hs, Hd, Wd, C, bounds_y, kk_y, ksize_y, items);
    }
    MMGT_LAUNCH_CHECK();
  }
  if (!horiz && !vert) {
    const long items = (long)n * Hs * Ws * C;
    hipLaunchKernelGGL(resize_copy_kernel, grid_for(items), dim3(RS_BLOCK), 0, s, in, last, n, Hs, Ws, C, items);
    MMGT_LAUNCH_CHECK();
  }
  return 0;
}
