// Re-voicing an existing clip (gfx950): the noised known clip and its kept-region blend, the pixel mask's latent cells, the paste-back
// alpha and the paste-back itself.  Four HBM-bound grid-stride kernels; the integer rules live in vid2vid_core.h, shared with
// tools/vid2vid_host_check.cpp.  Plain loads, vector stores, no state between launches, no atomics: equal inputs give equal bits on every launch.
#include "common.h"
#include "mmgt_hip.h"
#include "vid2vid_core.h"

namespace {

inline int grid_for(long n, int block = 256) {
  long g = (n + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 2048 * 4 ? 2048 * 4 : g));
}

// known = sa x0 + sb z as ONE expression, the same in every instantiation: an explicit fma over the rounded product sb z.  A zero scalar drops its
// term altogether (uniform branches), so (1, 0) hands back x0's bits and (0, 1) z's, signed zeros included, whatever the other tensor holds.
__device__ __forceinline__ float known_of(float x0, float z, float sa, float sb) {
  if (sb == 0.f) return sa * x0;
  if (sa == 0.f) return sb * z;
  return fmaf(sa, x0, sb * z);
}

// mask 1 -> x, mask 0 -> known: selections; in between m x + (1 - m) known
__device__ __forceinline__ float blend_of(float known, float x, float m) {
  if (m == 1.f) return x;
  if (m == 0.f) return known;
  return m * x + (1.f - m) * known;
}

// x and out may be the same buffer: every element is read and written by the same thread, the read first.  VEC: n % 4 == 0 and 16-byte pointers.
template <bool MASKED, bool VEC>
__global__ __launch_bounds__(256) void known_latents_kernel(const float* __restrict__ x0, const float* __restrict__ z, const float* x,
                                                            const float* __restrict__ mask, float* out, long n, int F, int hw, float sa, float sb) {
  const long stride = (long)gridDim.x * blockDim.x;
  if constexpr (VEC) {
    const long n4 = n >> 2;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n4; q += stride) {
      const float4 a = reinterpret_cast<const float4*>(x0)[q], b = reinterpret_cast<const float4*>(z)[q];
      float4 o = {known_of(a.x, b.x, sa, sb), known_of(a.y, b.y, sa, sb), known_of(a.z, b.z, sa, sb), known_of(a.w, b.w, sa, sb)};
      if constexpr (MASKED) {
        const float4 xv = reinterpret_cast<const float4*>(x)[q];
        const long i = q << 2;
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
        float os[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long e = i + k;
          os[k] = blend_of(os[k], xs[k], mask[((e / hw) % F) * (long)hw + e % hw]);
        }
        o = {os[0], os[1], os[2], os[3]};
      }
      reinterpret_cast<float4*>(out)[q] = o;
    }
  } else {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
      float o = known_of(x0[i], z[i], sa, sb);
      if constexpr (MASKED) o = blend_of(o, x[i], mask[((i / hw) % F) * (long)hw + i % hw]);
      out[i] = o;
    }
  }
}

// one thread per latent cell
__global__ __launch_bounds__(256) void mask_to_latent_kernel(const uint8_t* __restrict__ px, float* __restrict__ cells, int L, int h, int w, int grow) {
  const long n = (long)L * h * w, frame_px = (long)h * w * V2V_CELL * V2V_CELL;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int cx = (int)(i % w), cy = (int)((i / w) % h);
    const long l = i / ((long)h * w);
    cells[i] = v2v_cell_mask(px + l * frame_px, h, w, cy, cx, grow) ? 1.f : 0.f;
  }
}

// one thread per four pixels of a row (a row is 8 w pixels), one 4-byte store
__global__ __launch_bounds__(256) void feather_alpha_kernel(const float* __restrict__ cells, uint8_t* __restrict__ alpha, int L, int h, int w, int r) {
  const int W4 = w * V2V_CELL / 4, H = h * V2V_CELL;
  const long n = (long)L * H * W4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W4) * 4, y = (int)((i / W4) % H);
    const float* fr = cells + (i / ((long)W4 * H)) * h * w;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) word |= (uint32_t)v2v_feather_pixel(fr, h, w, y, x + k, r) << (8 * k);
    reinterpret_cast<uint32_t*>(alpha)[i] = word;
  }
}

// groups of four pixels (12 bytes of gen / orig / out as three words, one word of alpha) for the first 4 nvec pixels, then pixel by pixel
__global__ __launch_bounds__(256) void composite_u8_kernel(const uint8_t* __restrict__ gen, const uint8_t* __restrict__ orig,
                                                           const uint8_t* __restrict__ alpha, uint8_t* __restrict__ out, long nvec, long npix) {
  const long stride = (long)gridDim.x * blockDim.x, t0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
  for (long q = t0; q < nvec; q += stride) {
    const uint32_t a4 = reinterpret_cast<const uint32_t*>(alpha)[q];
    uint32_t g[3], o[3], w[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g[k] = reinterpret_cast<const uint32_t*>(gen)[3 * q + k];
      o[k] = reinterpret_cast<const uint32_t*>(orig)[3 * q + k];
    }
#pragma unroll
    for (int b = 0; b < 12; ++b) {
      const uint32_t a = (a4 >> (8 * (b / 3))) & 255u;
      w[b / 4] |= v2v_blend((g[b / 4] >> (8 * (b % 4))) & 255u, (o[b / 4] >> (8 * (b % 4))) & 255u, a) << (8 * (b % 4));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) reinterpret_cast<uint32_t*>(out)[3 * q + k] = w[k];
  }
  for (long p = 4 * nvec + t0; p < npix; p += stride) {
    const uint32_t a = alpha[p];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * p + c] = (uint8_t)v2v_blend(gen[3 * p + c], orig[3 * p + c], a);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace

extern "C" int mmgt_known_latents(const float* x0, const float* z, const float* x, const float* mask, float* out, long n, int F, int hw, float sa,
                                  float sb, void* stream) {
  MMGT_CHECK(x0 && z && out && n > 0 && F > 0 && hw > 0, "known_latents: bad arguments");
  MMGT_CHECK((x == nullptr) == (mask == nullptr), "known_latents: x and mask come together");
  MMGT_CHECK(n % ((long)F * hw) == 0, "known_latents: %ld elements are no multiple of F hw = %d x %d", n, F, hw);
  MMGT_CHECK(out != x0 && out != z, "known_latents: out aliases x0 or z");
  const bool vec = n % 4 == 0 && aligned(x0, 16) && aligned(z, 16) && aligned(out, 16) && (!x || aligned(x, 16));
  const dim3 grid(grid_for(vec ? n / 4 : n)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (x && vec) hipLaunchKernelGGL((known_latents_kernel<true, true>), grid, block, 0, s, x0, z, x, mask, out, n, F, hw, sa, sb);
  else if (x) hipLaunchKernelGGL((known_latents_kernel<true, false>), grid, block, 0, s, x0, z, x, mask, out, n, F, hw, sa, sb);
  else if (vec) hipLaunchKernelGGL((known_latents_kernel<false, true>), grid, block, 0, s, x0, z, x, mask, out, n, F, hw, sa, sb);
  else hipLaunchKernelGGL((known_latents_kernel<false, false>), grid, block, 0, s, x0, z, x, mask, out, n, F, hw, sa, sb);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_mask_to_latent(const unsigned char* mask_px, float* cells, int L, int H, int W, int grow, void* stream) {
  MMGT_CHECK(mask_px && cells && L > 0 && H > 0 && W > 0, "mask_to_latent: bad arguments");
  MMGT_CHECK(H % V2V_CELL == 0 && W % V2V_CELL == 0, "mask_to_latent: %d x %d is no multiple of the %d-pixel cell", H, W, V2V_CELL);
  MMGT_CHECK(grow >= 0 && grow <= V2V_GROW_MAX, "mask_to_latent: grow %d outside 0 .. %d", grow, V2V_GROW_MAX);
  const int h = H / V2V_CELL, w = W / V2V_CELL;
  hipLaunchKernelGGL(mask_to_latent_kernel, dim3(grid_for((long)L * h * w)), dim3(256), 0, (hipStream_t)stream, mask_px, cells, L, h, w, grow);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_feather_alpha(const float* cells, unsigned char* alpha, int L, int h, int w, int r, void* stream) {
  MMGT_CHECK(cells && alpha && L > 0 && h > 0 && w > 0, "feather_alpha: bad arguments");
  MMGT_CHECK(r >= 0 && r <= V2V_FEATHER_MAX, "feather_alpha: radius %d outside 0 .. %d", r, V2V_FEATHER_MAX);
  MMGT_CHECK(aligned(alpha, 4), "feather_alpha: alpha must be 4-byte aligned");
  hipLaunchKernelGGL(feather_alpha_kernel, dim3(grid_for((long)L * h * V2V_CELL * w * 2)), dim3(256), 0, (hipStream_t)stream, cells, alpha, L, h, w, r);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_composite_u8(const unsigned char* gen, const unsigned char* orig, const unsigned char* alpha, unsigned char* out, long npix,
                                 void* stream) {
  MMGT_CHECK(gen && orig && alpha && out && npix > 0, "composite_u8: bad arguments");
  const long nvec = aligned(gen, 4) && aligned(orig, 4) && aligned(alpha, 4) && aligned(out, 4) ? npix / 4 : 0;
  hipLaunchKernelGGL(composite_u8_kernel, dim3(grid_for(nvec > 0 ? nvec : npix)), dim3(256), 0, (hipStream_t)stream, gen, orig, alpha, out, nvec, npix);
  MMGT_LAUNCH_CHECK();
  return 0;
}
