// The sampler's general update (gfx950): guidance-rescale moments and one linear step that carries DDIM with eta > 0 and DPM-Solver++ 2M.
// Both kernels form the guided prediction exactly as cfg_ddim_kernel (elementwise.hip) does.  HBM-bound grid-stride kernels, fp32 values;
// the moments are summed in fp64 in a fixed order (no atomics), so every launch and every rank gets the same bits.
#include "common.h"
#include "mmgt_hip.h"

namespace {

inline int grid_for(long n, int block = 256) {
  long g = (n + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 2048 * 4 ? 2048 * 4 : g));
}

// the partial sums' grid: a function of n alone (four elements per thread up to the cap of 512 workgroups, two per CU)
constexpr int kMomentBlocksMax = 512;
inline int moment_blocks(long n) {
  long g = (n + 1023) / 1024;
  return (int)(g < 1 ? 1 : (g > kMomentBlocksMax ? kMomentBlocksMax : g));
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// part[block][4] = this workgroup's (sum v_c, sum v_c^2, sum v_g, sum v_g^2): per thread in element order, then the butterfly of the wave, then
// the four waves in order.
__global__ __launch_bounds__(256) void cfg_moments_partial_kernel(const float* __restrict__ ps, const float* __restrict__ counter,
                                                                  double* __restrict__ part, long n, int F, int hw, float g) {
  __shared__ double red[4][4];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)((i / hw) % F);
    const float cnt = counter[f];
    const float eu = ps[i] / cnt, ec = ps[n + i] / cnt;
    const float v = eu + g * (ec - eu);
    const double dc = (double)ec, dv = (double)v;
    s[0] += dc;
    s[1] += dc * dc;
    s[2] += dv;
    s[3] += dv * dv;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double w = wave_sum_f64(s[q]);
    if (lane == 0) red[wave][q] = w;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int q = threadIdx.x;
    part[(long)blockIdx.x * 4 + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
  }
}

// One workgroup: all threads bring the partials into LDS, then thread q folds those of quantity q in index order.  (Folding straight from global
// memory, one load per add, made the moments 64 us at 1.3 M elements; staged through LDS they are 15 us: profiles/sampler.)
__global__ __launch_bounds__(256) void cfg_moments_fold_kernel(const double* __restrict__ part, double* __restrict__ mom, int blocks) {
  __shared__ double sh[kMomentBlocksMax * 4];
  for (int i = threadIdx.x; i < blocks * 4; i += blockDim.x) sh[i] = part[i];
  __syncthreads();
  const int q = threadIdx.x;
  if (q >= 4) return;
  double s = 0.0;
  for (int b = 0; b < blocks; ++b) s += sh[b * 4 + q];
  mom[q] = s;
}

// v = rho (eu + g (ec - eu));  x0 = sa_t x - sb_t v;  out = k_x x + k_0 x0 + k_1 x0_prev + k_v v + k_z z.  rho = 1 when phi == 0 (mom is not
// read); n Var cancels its n in the ratio.  xp / z / x0o may be null.
__global__ void sampler_step_kernel(const float* __restrict__ ps, const float* __restrict__ counter, const float* __restrict__ x,
                                    const float* __restrict__ xp, const float* __restrict__ z, const double* __restrict__ mom,
                                    float* __restrict__ xo, float* __restrict__ x0o, long n, int F, int hw, float g, float phi, float sa_t,
                                    float sb_t, float k_x, float k_0, float k_1, float k_v, float k_z) {
  float rho = 1.f;
  if (phi != 0.f) {
    const double inv_n = 1.0 / (double)n;
    const double var_c = mom[1] - mom[0] * mom[0] * inv_n, var_g = mom[3] - mom[2] * mom[2] * inv_n;
    rho = (float)((double)phi * sqrt(var_c / var_g) + (1.0 - (double)phi));
  }
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int f = (int)((i / hw) % F);
    const float cnt = counter[f];
    const float eu = ps[i] / cnt, ec = ps[n + i] / cnt;
    const float v = rho * (eu + g * (ec - eu));
    const float xi = x[i];
    const float x0 = sa_t * xi - sb_t * v;
    float o = k_x * xi + k_0 * x0;
    if (xp) o += k_1 * xp[i];
    o += k_v * v;
    if (z) o += k_z * z[i];
    xo[i] = o;
    if (x0o) x0o[i] = x0;
  }
}

}  // namespace

extern "C" int mmgt_cfg_moments(const float* pred_sum, const float* counter, long n, int F, int hw, float guidance, double* partials,
                                int partials_rows, double* moments, void* stream) {
  MMGT_CHECK(pred_sum && counter && partials && moments && n > 0 && F > 0 && hw > 0, "cfg_moments: bad arguments");
  MMGT_CHECK(((uintptr_t)partials % 8) == 0 && ((uintptr_t)moments % 8) == 0, "cfg_moments: misaligned fp64 buffer");
  const int blocks = moment_blocks(n);
  MMGT_CHECK(partials_rows >= blocks, "cfg_moments: %d rows of partial sums, %d needed (at most %d)", partials_rows, blocks, kMomentBlocksMax);
  hipLaunchKernelGGL(cfg_moments_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pred_sum, counter, partials, n, F, hw, guidance);
  hipLaunchKernelGGL(cfg_moments_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials, moments, blocks);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_sampler_step(const float* pred_sum, const float* counter, const float* latents, const float* prev_x0, const float* noise,
                                 const double* moments, float* latents_out, float* x0_out, long n, int F, int hw, float guidance, float rescale,
                                 float sa_t, float sb_t, float k_x, float k_0, float k_1, float k_v, float k_z, void* stream) {
  MMGT_CHECK(pred_sum && counter && latents && latents_out && n > 0 && F > 0 && hw > 0, "sampler_step: bad arguments");
  MMGT_CHECK(rescale >= 0.f && rescale <= 1.f, "sampler_step: rescale %g outside [0, 1]", (double)rescale);
  MMGT_CHECK(rescale == 0.f || (moments && ((uintptr_t)moments % 8) == 0), "sampler_step: rescale > 0 reads the moments of mmgt_cfg_moments");
  MMGT_CHECK(k_1 == 0.f || prev_x0, "sampler_step: k_1 != 0 without the previous step's x0");
  MMGT_CHECK(k_z == 0.f || noise, "sampler_step: k_z != 0 without noise");
  MMGT_CHECK(x0_out == nullptr || (x0_out != prev_x0 && x0_out != latents_out), "sampler_step: x0_out aliases another operand");
  hipLaunchKernelGGL(sampler_step_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, pred_sum, counter, latents, prev_x0, noise, moments,
                     latents_out, x0_out, n, F, hw, guidance, rescale, sa_t, sb_t, k_x, k_0, k_1, k_v, k_z);
  MMGT_LAUNCH_CHECK();
  return 0;
}
