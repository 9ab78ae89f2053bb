// Audio input (gfx950): the `data` chunk of a PCM / float WAV file, already on the device, becomes a mono fp32 waveform at the model's
// rate -- what the reference gets from librosa.load(path, sr=16000).  The container walk is the host's (mmgt_amd/audio_in.py); the arithmetic and
// every index live in audio_core.h, which a host program runs too; this file is the two launches.
//
//  * mmgt_audio_decode_mono   one thread per frame, 256 frames per workgroup.  A frame is 1 .. 128 bytes at any byte address, so a workgroup first
//                             copies its run of bytes into LDS -- aligned 4-byte words where the global address allows, single bytes at the two
//                             ends, never a wider access through an unaligned pointer and never a byte outside the run -- and decodes from there
//                             byte by byte (audio_frame_mono).  Each global byte is read once, in coalesced words.
//  * mmgt_audio_resample      polyphase FIR, one thread per output, 256 consecutive outputs per workgroup, which stages the input span they read
//                             in LDS (audio_stage_len: 1.1 k floats at 44.1 -> 16 kHz, 6.3 k at the largest ratio).  Every output is one fp32
//                             fma chain in ascending tap order over consecutive floats of ITS row of the phase-major table (audio_resample_one):
//                             no atomics, no cross-lane sum, so the result does not depend on the grid.  There is no MFMA here: per output
//                             2 half / up multiply-adds on operands that sit in LDS and in L2 (the table is 0.2 .. 0.4 MB at the common rates).
#include "common.h"
#include "mmgt_hip.h"
#include "audio_core.h"

namespace {

constexpr int AU_BLOCK = 256;      // threads = frames (decode) = outputs (resample) per workgroup

__global__ __launch_bounds__(AU_BLOCK) void audio_decode_kernel(const uint8_t* __restrict__ raw, float* __restrict__ out, long n_frames, int channels,
                                                                int fmt) {
  extern __shared__ __attribute__((aligned(16))) uint8_t au_bytes[];
  const int tid = threadIdx.x;
  const int fb = channels * audio_sample_bytes(fmt);
  const long f0 = blockIdx.x * (long)AU_BLOCK;
  const int nf = (int)(n_frames - f0 < AU_BLOCK ? n_frames - f0 : AU_BLOCK);
  const uint8_t* g = raw + f0 * fb;
  const int nbytes = nf * fb;
  // LDS byte skew + k holds g[k]: an aligned word of global memory lands on an aligned word of LDS
  const int skew = (int)((uintptr_t)g & 3);
  const int head = nbytes < ((4 - skew) & 3) ? nbytes : ((4 - skew) & 3);
  const int words = (nbytes - head) >> 2;
  const int tail0 = head + 4 * words, tail = nbytes - tail0;       // tail 0 .. 3
  const uint32_t* gw = reinterpret_cast<const uint32_t*>(g + head);
  uint32_t* lw = reinterpret_cast<uint32_t*>(au_bytes + skew + head);
  for (int k = tid; k < words; k += AU_BLOCK) lw[k] = gw[k];
  if (tid < head) au_bytes[skew + tid] = g[tid];
  if (tid >= 64 && tid - 64 < tail) au_bytes[skew + tail0 + tid - 64] = g[tail0 + tid - 64];
  __syncthreads();
  if (tid < nf) out[f0 + tid] = audio_frame_mono(au_bytes + skew + tid * fb, fmt, channels);
}

__global__ __launch_bounds__(AU_BLOCK) void audio_resample_kernel(const float* __restrict__ x, long n_in, const float* __restrict__ taps, int up,
                                                                  int down, int half, float* __restrict__ y, long n_out) {
  extern __shared__ __attribute__((aligned(16))) float au_x[];
  const int tid = threadIdx.x;
  const long j0 = blockIdx.x * (long)AU_BLOCK;
  const long j1 = (j0 + AU_BLOCK < n_out ? j0 + AU_BLOCK : n_out) - 1;
  // i_lo and i_hi grow with j: the workgroup's outputs read x[lo .. hi], at most audio_stage_len(AU_BLOCK) samples
  const long lo = audio_span(j0, n_in, up, down, half).i_lo, hi = audio_span(j1, n_in, up, down, half).i_hi;
  for (long k = tid; k <= hi - lo; k += AU_BLOCK) au_x[k] = x[lo + k];
  __syncthreads();
  const long j = j0 + tid;
  if (j <= j1) y[j] = audio_resample_one(au_x, lo, taps, j, n_in, up, down, half);
}

constexpr long AU_MAX_GRID = 0x7fffffffL;
constexpr long AU_MAX_LDS = 64 * 1024;

}  // namespace

extern "C" int mmgt_audio_decode_mono(const unsigned char* raw, float* out, long long n_frames, int channels, int fmt, void* stream) {
  MMGT_CHECK(raw && out, "audio_decode_mono: raw and out are needed");
  MMGT_CHECK(fmt >= 0 && fmt < AU_FORMATS && channels >= 1 && channels <= AU_MAX_CHANNELS,
             "audio_decode_mono: format %d, %d channels: formats 0 .. %d (U8, S16, S24, S32, F32, F64), 1 .. %d channels", fmt, channels,
             AU_FORMATS - 1, AU_MAX_CHANNELS);
  const long blocks = ((long)n_frames + AU_BLOCK - 1) / AU_BLOCK;
  MMGT_CHECK(n_frames >= 1 && blocks <= AU_MAX_GRID, "audio_decode_mono: %lld frames: 1 .. %ld", n_frames, AU_MAX_GRID * AU_BLOCK);
  const size_t lds = (size_t)AU_BLOCK * channels * audio_sample_bytes(fmt) + 4;            // the run of bytes plus the skew, at most 32 KiB + 4
  hipLaunchKernelGGL(audio_decode_kernel, dim3((unsigned)blocks), dim3(AU_BLOCK), lds, (hipStream_t)stream, raw, out, (long)n_frames, channels, fmt);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_audio_resample(const float* x, long long n_in, const float* taps, int up, int down, int half, float* y, long long n_out,
                                   void* stream) {
  MMGT_CHECK(x && taps && y && x != y, "audio_resample: x, taps and y are needed, and x and y differ");
  MMGT_CHECK(up >= 1 && down >= 1 && up != down && half >= 1 && n_in >= 1 && n_in <= AU_MAX_GRID,
             "audio_resample: up %d, down %d, half %d, n_in %lld: up, down, half >= 1, up != down (equal rates need no launch), n_in 1 .. 2^31 - 1",
             up, down, half, n_in);
  MMGT_CHECK(n_out == audio_out_len(n_in, up, down), "audio_resample: n_out %lld, but ceil(%lld * %d / %d) = %lld", n_out, n_in, up, down,
             (long long)audio_out_len(n_in, up, down));
  const long lds = audio_stage_len(AU_BLOCK, up, down, half) * (long)sizeof(float);
  MMGT_CHECK(lds <= AU_MAX_LDS, "audio_resample: up %d, down %d, half %d: a workgroup's input span (%ld bytes) exceeds %ld bytes of LDS", up, down,
             half, lds, AU_MAX_LDS);
  const long blocks = ((long)n_out + AU_BLOCK - 1) / AU_BLOCK;
  hipLaunchKernelGGL(audio_resample_kernel, dim3((unsigned)blocks), dim3(AU_BLOCK), (size_t)lds, (hipStream_t)stream, x, (long)n_in, taps, up, down,
                     half, y, (long)n_out);
  MMGT_LAUNCH_CHECK();
  return 0;
}
