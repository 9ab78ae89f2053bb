// GIF89a image data of device-resident uint8 RGB frames: the encoder behind save_videos_grid(..., gif_encoder="device") (DESIGN 4d,
// mmgt_amd/video_out.py).  One palette serves the whole clip; the host builds it (median cut, video_out.gif_palette) from a histogram made here.
//
//  * mmgt_gif_histogram   (n, H, W, 3) u8 -> u32[32768] counts of the 5-bit-per-channel bins (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3), ADDED to the
//                         caller's zeroed table: every workgroup counts into its own 128 KB LDS table and adds the bins it touched with global
//                         atomics (integer adds: the result does not depend on the order).
//  * mmgt_gif_index       idx = lut[bin(pixel)] with the 32 KB table in LDS; four pixels (three words in, one word out) per thread.  No dithering.
//  * mmgt_gif_dither      the index map under Floyd-Steinberg error diffusion against the palette (csrc/gif_dither_core.h: rule and schedule); one
//                         single-wave workgroup per frame, a lane per row of a band of 64 rows, each row two pixels behind the row above.
//  * mmgt_gif_delta       frame differencing: 255 where a pixel's index equals the frame before's.
//  * mmgt_gif_lzw         GIF's variable-width LZW, minimum code size 8.  One single-wave workgroup per (frame, strip of strip_rows image rows); lane 0
//                         codes (LZW is a serial recurrence over the pixels), the other lanes stage pixels into LDS and clear the dictionary.
//                         The dictionary is an open-addressed hash table of 8192 words in LDS, entry = (prefix << 8 | byte) << 12 | code.
//                         Every strip's dictionary starts empty, so the strips are independent and their bit strings concatenate to ONE valid
//                         stream.  A Clear code must be written at the width the decoder holds when it reads it, and that is the width the PREVIOUS
//                         strip ended at; therefore strip 0 opens with Clear (9 bits) and every strip but the last CLOSES with the Clear that opens
//                         the next one; the last closes with End-of-Information.  When code 4095 has been assigned the strip writes Clear (12 bits) and
//                         starts over at 9 bits.  Bits go LSB-first into the strip's own slot, its length in bits into bits[frame][strip].
//  * mmgt_gif_strip_stride the slot size no input can exceed (derivation at the function).
//  * mmgt_gif_pack        joins a frame's strips at their bit offsets (exclusive prefix sum of bits) and cuts the bytes into data sub-blocks:
//                         a length byte before every 255 bytes, then the 0x00 terminator.  sizes[frame] = bytes written.
#include "common.h"
#include "gif_dither_core.h"
#include "mmgt_hip.h"

namespace {

constexpr int kBins = 32768;
constexpr int kHistThreads = 1024;
constexpr int kHashWords = 8192;                                   // 2 x the 4096 codes: the load factor stays below 0.47
constexpr unsigned kEmpty = 0xffffffffu;                           // no entry looks like this: a key's top bits are a prefix < 4096
constexpr int kStage = 4096;                                       // pixels staged into LDS at a time
constexpr int kFreeCodes = 4096 - 258;                             // codes 258 .. 4095
constexpr int kMaxStrips = 2048;                                   // pack holds a frame's bit offsets in LDS

__device__ __forceinline__ unsigned bin_of(unsigned r, unsigned g, unsigned b) { return (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3); }

// ---- histogram ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHistThreads) void gif_histogram_kernel(const unsigned char* __restrict__ frames, unsigned* __restrict__ hist, size_t npix) {
  extern __shared__ unsigned h_s[];                                // kBins counters
  for (int i = threadIdx.x; i < kBins; i += kHistThreads) h_s[i] = 0u;
  __syncthreads();
  const size_t step = (size_t)gridDim.x * kHistThreads;
  for (size_t p = (size_t)blockIdx.x * kHistThreads + threadIdx.x; p < npix; p += step) {
    const unsigned char* q = frames + 3 * p;
    atomicAdd(&h_s[bin_of(q[0], q[1], q[2])], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kBins; i += kHistThreads) {
    const unsigned v = h_s[i];
    if (v) atomicAdd(&hist[i], v);
  }
}

// ---- index map ---------------------------------------------------------------------------------------------------------------------------------
// Thread g maps pixels 4 g .. 4 g + 3: bytes 12 g .. 12 g + 11 of the frames (three aligned words) -> one word of idx.  The last group of a clip
// whose pixel count is no multiple of 4 goes byte by byte.
__global__ __launch_bounds__(256) void gif_index_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ lut,
                                                        unsigned char* __restrict__ idx, size_t npix) {
  __shared__ __attribute__((aligned(16))) unsigned char lut_s[kBins];
  for (int i = threadIdx.x; i < kBins / 16; i += 256) reinterpret_cast<u32x4*>(lut_s)[i] = reinterpret_cast<const u32x4*>(lut)[i];
  __syncthreads();
  const size_t groups = (npix + 3) / 4;
  const size_t step = (size_t)gridDim.x * 256;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += step) {
    if (4 * g + 4 <= npix) {
      const unsigned* q = reinterpret_cast<const unsigned*>(frames) + 3 * g;
      const unsigned a = q[0], b = q[1], c = q[2];                 // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
      const unsigned i0 = lut_s[bin_of(a & 255, (a >> 8) & 255, (a >> 16) & 255)];
      const unsigned i1 = lut_s[bin_of(a >> 24, b & 255, (b >> 8) & 255)];
      const unsigned i2 = lut_s[bin_of((b >> 16) & 255, b >> 24, c & 255)];
      const unsigned i3 = lut_s[bin_of((c >> 8) & 255, (c >> 16) & 255, c >> 24)];
      reinterpret_cast<unsigned*>(idx)[g] = i0 | i1 << 8 | i2 << 16 | i3 << 24;
    } else {
      for (size_t p = 4 * g; p < npix; ++p) idx[p] = lut_s[bin_of(frames[3 * p], frames[3 * p + 1], frames[3 * p + 2])];
    }
  }
}

// ---- dithered index map ------------------------------------------------------------------------------------------------------------------------
// One single-wave workgroup per frame; csrc/gif_dither_core.h states the rule and the schedule.  Lane r of a band of GDI_BAND rows stands at
// x = t - 2 r in step t.  What it needs of the row above arrives from lane r - 1 by one DPP move per step (every lane executes it: the loop is
// uniform, a lane outside the frame only computes nothing); lane 0 takes it from the carry row that lane 63 of the band before wrote, or zeros in the
// first band.  Pixels and carry words are fetched a group of GDI_GROUP steps ahead, so that no step waits for global memory.
__device__ __forceinline__ unsigned from_lane_above(unsigned v) {
  // v_mov_b32 dpp wave_shr:1: lane l reads lane l - 1; lane 0 has no source and keeps `old`
  return (unsigned)__builtin_amdgcn_update_dpp((int)GDI_ZERO, (int)v, 0x138, 0xf, 0xf, false);
}

__global__ __launch_bounds__(GDI_BAND) void gif_dither_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ lut,
                                                              const unsigned char* __restrict__ palette, unsigned char* __restrict__ idx, unsigned* carry,
                                                              int H, int W, long long total) {
  __shared__ __attribute__((aligned(16))) unsigned char lut_s[kBins];
  __shared__ unsigned pal_s[256];
  const int lane = threadIdx.x;
  const long long frame = blockIdx.x;
  for (int i = lane; i < kBins / 16; i += GDI_BAND) reinterpret_cast<u32x4*>(lut_s)[i] = reinterpret_cast<const u32x4*>(lut)[i];
  for (int i = lane; i < 256; i += GDI_BAND) pal_s[i] = palette[3 * i] | (unsigned)palette[3 * i + 1] << 8 | (unsigned)palette[3 * i + 2] << 16;
  __syncthreads();
  unsigned* cr = carry + frame * W;                                // touched only if the frame has more than one band
  for (int row0 = 0; row0 < H; row0 += GDI_BAND) {
    const int rows = min((int)GDI_BAND, H - row0);
    const bool first = row0 == 0, more = row0 + GDI_BAND < H;
    const bool has_row = lane < rows, reads_carry = lane == 0 && !first;
    const long long rowpix = (frame * H + row0 + lane) * W;        // of a lane without a row: never used
    const long steps = gdi_band_steps(W, rows);
    GdiLane s;
    gdi_lane_reset(&s, reads_carry ? cr[0] : GDI_ZERO);
    unsigned cur[3], raw[4] = {0u, 0u, 0u, 0u};                    // this group's pixels; the words that hold the next group's, in flight
    unsigned ccur[GDI_GROUP], cnxt[GDI_GROUP];
    for (int k = 0; k < GDI_GROUP; ++k) ccur[k] = cnxt[k] = GDI_ZERO;
    const int shift = gdi_shift(3 * (rowpix - 2 * lane));          // group 0 is x = -2 lane .. 3 - 2 lane
    if (has_row && lane < 2) gdi_fetch16(frames, 3 * (rowpix - 2 * lane), total, raw);
    gdi_align12(raw, shift, cur);
    if (reads_carry)
      for (int k = 0; k < GDI_GROUP; ++k)
        if (k + 1 < W) ccur[k] = cr[k + 1];
    // A group's results are stored when the NEXT group begins, ahead of that group's loads: the wait for the loads at a group's end is a wait for
    // everything in flight (the stores stand in branches, so they cannot be counted), and by then these stores are four steps old.
    unsigned done_idx = 0u, done_err[GDI_GROUP];                   // the group's four indices, a byte each, and the errors they left
    for (int k = 0; k < GDI_GROUP; ++k) done_err[k] = GDI_ZERO;
    auto store_group = [&](long t) {                               // t: the group's first step
#pragma unroll
      for (int k = 0; k < GDI_GROUP; ++k) {
        const int x = gdi_x(t + k, lane);
        if (has_row && x >= 0 && x < W) {
          idx[rowpix + x] = (unsigned char)(done_idx >> (8 * k));
          if (more && lane == GDI_BAND - 1) cr[x] = done_err[k];
        }
      }
    };
    for (long t0 = 0; t0 < steps; t0 += GDI_GROUP) {
      if (t0 > 0) store_group(t0 - GDI_GROUP);
      const long x1 = gdi_x(t0 + GDI_GROUP, lane);                 // the next group: x1 .. x1 + 3
      if (has_row && x1 + GDI_GROUP > 0 && x1 < W) gdi_fetch16(frames, 3 * (rowpix + x1), total, raw);
      if (reads_carry)
        for (int k = 0; k < GDI_GROUP; ++k) cnxt[k] = x1 + k + 1 < W ? cr[x1 + k + 1] : GDI_ZERO;
      done_idx = 0u;
#pragma unroll
      for (int k = 0; k < GDI_GROUP; ++k) {
        const int x = gdi_x(t0 + k, lane);
        const bool active = has_row && x >= 0 && x < W;
        const unsigned above = from_lane_above(s.out);
        const unsigned in = lane == 0 ? ccur[k] : above;
        unsigned r, g, b;
        gdi_pixel(cur, k, &r, &g, &b);
        const int i = gdi_lane_step(&s, in, active, r, g, b, lut_s, pal_s);
        done_idx |= (unsigned)(i & 255) << (8 * k);
        done_err[k] = s.out;
      }
      gdi_align12(raw, shift, cur);                                // the first use of what the loads returned
      for (int k = 0; k < GDI_GROUP; ++k) {
        // an empty statement that "changes" the word: without it hipcc copies the registers the carry loads write to right behind the loads,
        // and that copy waits for every load in flight, the pixels' among them
        asm volatile("" : "+v"(cnxt[k]));
        ccur[k] = cnxt[k];
      }
    }
    store_group((steps - 1) / GDI_GROUP * GDI_GROUP);
    __syncthreads();                                             // the carry row lane 63 wrote is read by lane 0 in the next band
  }
}

// ---- frame differencing ------------------------------------------------------------------------------------------------------------------------
// out = 255 where a pixel's index equals the frame before's, else the index.  Pixel q of the clip is compared with pixel q - plane; the first frame
// with `prev` (the last frame of the launch before), or with nothing.  Thread g takes pixels 4 g .. 4 g + 3.
__device__ __forceinline__ unsigned delta_byte(unsigned cur, int before) { return (int)cur == before ? 255u : cur; }

__global__ __launch_bounds__(256) void gif_delta_kernel(const unsigned char* __restrict__ idx, const unsigned char* __restrict__ prev,
                                                        unsigned char* __restrict__ out, size_t npix, size_t plane) {
  const size_t groups = (npix + 3) / 4;
  const size_t step = (size_t)gridDim.x * 256;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += step) {
    const size_t p = 4 * g;
    if (p + 4 <= npix && p >= plane && (plane & 3) == 0) {
      const unsigned a = reinterpret_cast<const unsigned*>(idx)[g], b = *reinterpret_cast<const unsigned*>(idx + p - plane);
      unsigned v = 0;
      for (int k = 0; k < 4; ++k) v |= delta_byte((a >> (8 * k)) & 255u, (int)((b >> (8 * k)) & 255u)) << (8 * k);
      reinterpret_cast<unsigned*>(out)[g] = v;
    } else {
      for (size_t q = p; q < npix && q < p + 4; ++q)
        out[q] = (unsigned char)delta_byte(idx[q], q >= plane ? (int)idx[q - plane] : prev ? (int)prev[q] : -1);
    }
  }
}

// ---- LZW ---------------------------------------------------------------------------------------------------------------------------------------
// LSB-first bit writer of lane 0 into the strip's slot, a word at a time.  A word is stored only if it lies inside the slot; with
// out_stride >= mmgt_gif_strip_stride that is every word (the bound below), so the test never drops one.
struct BitOut {
  unsigned* o;
  long words;                                                      // words of the slot
  long w = 0;
  long long nbits = 0;
  unsigned long long acc = 0;
  int nacc = 0;
  __device__ __forceinline__ void put(unsigned code, int width) {
    acc |= (unsigned long long)code << nacc;
    nacc += width;
    nbits += width;
    if (nacc >= 32) {
      if (w < words) o[w] = (unsigned)acc;
      ++w;
      acc >>= 32;
      nacc -= 32;
    }
  }
  __device__ __forceinline__ void flush() {
    if (nacc > 0 && w < words) o[w] = (unsigned)acc;               // the bits above nacc are zero
  }
};

__global__ __launch_bounds__(64) void gif_lzw_kernel(const unsigned char* __restrict__ idx, unsigned char* __restrict__ out, long long* __restrict__ bits,
                                                     size_t idx_bytes, int H, int W, int strip_rows, int strips, long out_stride) {
  __shared__ __attribute__((aligned(16))) unsigned tab[kHashWords];
  __shared__ unsigned pix_s[kStage / 4 + 2];
  __shared__ int state_s[2];                                       // pixels of the staged run that lane 0 consumed; dictionary to be cleared
  const int t = threadIdx.x;
  const int strip = blockIdx.x % strips, frame = blockIdx.x / strips;
  const int row0 = strip * strip_rows;
  const long npix = (long)min(strip_rows, H - row0) * W;           // >= 1
  const unsigned char* src = idx + ((size_t)frame * H + row0) * W;
  const unsigned char* idx_end = idx + idx_bytes;

  BitOut bo{reinterpret_cast<unsigned*>(out + (size_t)blockIdx.x * out_stride), out_stride / 4};
  int width = 9, next = 258, prefix = -1;
  if (t == 0 && strip == 0) bo.put(256u, 9);
  long pos = 0;
  bool clear = true;
  while (pos < npix) {
    if (clear)
      for (int i = t; i < kHashWords / 4; i += 64) reinterpret_cast<u32x4*>(tab)[i] = (u32x4)(kEmpty);
    // stage the next run of pixels as the aligned words that hold it (idx is 4-byte aligned, so the first word starts inside the buffer)
    const int run = (int)min((long)kStage, npix - pos);
    const unsigned char* p0 = src + pos;
    const int mis = (int)(reinterpret_cast<uintptr_t>(p0) & 3);
    const unsigned char* w0 = p0 - mis;
    for (int j = t; j < (mis + run + 3) / 4; j += 64) {
      const unsigned char* q = w0 + 4 * j;
      unsigned v;
      if (q + 4 <= idx_end) {
        v = *reinterpret_cast<const unsigned*>(q);
      } else {                                                     // the last word of a buffer whose size is no multiple of 4
        v = 0;
        for (int k = 0; k < 4 && q + k < idx_end; ++k) v |= (unsigned)q[k] << (8 * k);
      }
      pix_s[j] = v;
    }
    __syncthreads();
    if (t == 0) {
      const unsigned char* px = reinterpret_cast<const unsigned char*>(pix_s) + mis;
      int i = 0;
      bool full = false;
      if (prefix < 0) prefix = px[i++];
      while (i < run) {
        const unsigned c = px[i++];
        const unsigned key = (unsigned)prefix << 8 | c;            // 20 bits
        unsigned h = (key * 2654435761u) >> 19;                    // 13 bits
        unsigned e = tab[h];
        while (e != kEmpty && (e >> 12) != key) {
          h = (h + 1) & (kHashWords - 1);
          e = tab[h];
        }
        if (e != kEmpty) {
          prefix = (int)(e & 0xfffu);
          continue;
        }
        bo.put((unsigned)prefix, width);
        tab[h] = key << 12 | (unsigned)next;
        if (next == (1 << width) && width < 12) ++width;           // the decoder widens once it has defined code 2^width - 1
        ++next;
        prefix = (int)c;
        if (next == 4096) {                                        // code 4095 assigned: Clear at 12 bits, start over
          bo.put(256u, width);
          width = 9;
          next = 258;
          full = true;
          break;
        }
      }
      state_s[0] = i;
      state_s[1] = full;
    }
    __syncthreads();
    pos += state_s[0];
    clear = state_s[1] != 0;
    __syncthreads();                                               // state_s and pix_s are rewritten by the next round
  }
  if (t == 0) {
    bo.put((unsigned)prefix, width);
    if (next == (1 << width) && width < 12) ++width;
    bo.put(strip == strips - 1 ? 257u : 256u, width);              // End-of-Information, or the Clear that opens the next strip
    bo.flush();
    bits[blockIdx.x] = bo.nbits;
  }
}

// ---- pack --------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gif_pack_kernel(const unsigned char* __restrict__ out, const long long* __restrict__ bits,
                                                       unsigned char* __restrict__ packed, int* __restrict__ sizes, int strips, long out_stride,
                                                       long packed_stride) {
  __shared__ long long pre[kMaxStrips + 1];                        // pre[s] = bits of the strips before s
  const int t = threadIdx.x, frame = blockIdx.y;
  for (int s = t; s < strips; s += 256) {
    const long long b = bits[(size_t)frame * strips + s];
    pre[s + 1] = b < 0 ? 0 : b > 8 * (long long)out_stride ? 8 * (long long)out_stride : b;       // never read outside a slot
  }
  __syncthreads();
  if (t == 0) {
    pre[0] = 0;
    for (int s = 0; s < strips; ++s) pre[s + 1] += pre[s];
  }
  __syncthreads();
  const long long total = pre[strips];
  const long long nbytes = (total + 7) >> 3;
  const long long size = nbytes + (nbytes + 254) / 255 + 1;
  const unsigned char* slots = out + (size_t)frame * strips * out_stride;
  unsigned char* dst = packed + (size_t)frame * packed_stride;
  for (long long j = (long long)blockIdx.x * 256 + t; j < nbytes; j += (long long)gridDim.x * 256) {
    const long long b0 = 8 * j;
    int lo = 0, hi = strips - 1;                                   // the last strip s with pre[s] <= b0
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pre[mid] <= b0) lo = mid; else hi = mid - 1;
    }
    unsigned val = 0;
    int got = 0;
    for (int s = lo; s < strips && got < 8; ++s) {
      const long long local = b0 + got - pre[s];                   // >= 0
      const long long avail = pre[s + 1] - pre[s] - local;
      if (avail <= 0) continue;
      const int take = (int)(avail < 8 - got ? avail : 8 - got);
      const unsigned char* q = slots + (size_t)s * out_stride + (local >> 3);
      unsigned two = q[0];
      if ((local >> 3) + 1 < out_stride) two |= (unsigned)q[1] << 8;
      val |= ((two >> (local & 7)) & ((1u << take) - 1)) << got;
      got += take;
    }
    const long long p = j + j / 255 + 1;
    if (p < packed_stride) dst[p] = (unsigned char)val;
    if (j % 255 == 0 && p - 1 < packed_stride) dst[p - 1] = (unsigned char)(nbytes - j < 255 ? nbytes - j : 255);
  }
  if (blockIdx.x == 0 && t == 0) {
    if (size <= packed_stride) dst[size - 1] = 0;
    sizes[frame] = size <= packed_stride ? (int)size : -1;
  }
}

const char* kBadClip = "%s: n = %d frames of %d x %d are outside the range (n, H, W >= 1, H, W <= 65535, n * H * W < 2^32)";
bool clip_ok(int n, int H, int W) {
  return n >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && (unsigned long long)n * H * W < (1ull << 32);
}
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" int mmgt_gif_histogram(const unsigned char* frames, unsigned* hist, int n, int H, int W, void* stream) {
  MMGT_CHECK(frames && hist, "gif_histogram: null pointer");
  MMGT_CHECK(clip_ok(n, H, W), kBadClip, "gif_histogram", n, H, W);
  const size_t npix = (size_t)n * H * W;
  static bool opted = false;
  if (!opted) {
    MMGT_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gif_histogram_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kBins * (int)sizeof(unsigned)) == hipSuccess,
               "gif_histogram: cannot reserve %d bytes of LDS", kBins * (int)sizeof(unsigned));
    opted = true;
  }
  const size_t want = (npix + 8 * kHistThreads - 1) / (8 * kHistThreads);               // at least 8 pixels per thread before another table is paid for
  const unsigned grid = (unsigned)(want < 1 ? 1 : want > 256 ? 256 : want);
  hipLaunchKernelGGL(gif_histogram_kernel, dim3(grid), dim3(kHistThreads), kBins * sizeof(unsigned), (hipStream_t)stream, frames, hist, npix);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_gif_index(const unsigned char* frames, const unsigned char* lut, unsigned char* idx, int n, int H, int W, void* stream) {
  MMGT_CHECK(frames && lut && idx, "gif_index: null pointer");
  MMGT_CHECK(clip_ok(n, H, W), kBadClip, "gif_index", n, H, W);
  MMGT_CHECK(aligned4(frames) && aligned4(idx) && (reinterpret_cast<uintptr_t>(lut) & 15) == 0,
             "gif_index: frames and idx must be 4-byte aligned, lut 16-byte aligned");
  const size_t npix = (size_t)n * H * W;
  const size_t want = ((npix + 3) / 4 + 4 * 256 - 1) / (4 * 256);
  const unsigned grid = (unsigned)(want < 1 ? 1 : want > 1024 ? 1024 : want);
  hipLaunchKernelGGL(gif_index_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, frames, lut, idx, npix);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_gif_dither_band(void) { return GDI_BAND; }

// The carry row: one word per pixel of a row, per frame; frames of a single band need none.
extern "C" int mmgt_gif_dither_scratch(int n, int H, int W, long long* bytes) {
  MMGT_CHECK(bytes, "gif_dither_scratch: null output");
  MMGT_CHECK(clip_ok(n, H, W), kBadClip, "gif_dither_scratch", n, H, W);
  *bytes = H > GDI_BAND ? 4ll * n * W : 0;
  return 0;
}

extern "C" int mmgt_gif_dither(const unsigned char* frames, const unsigned char* lut, const unsigned char* palette, unsigned char* idx, void* scratch,
                               long long scratch_bytes, int n, int H, int W, void* stream) {
  long long need = 0;
  MMGT_CHECK(frames && lut && palette && idx, "gif_dither: null pointer");
  if (mmgt_gif_dither_scratch(n, H, W, &need)) return 1;
  MMGT_CHECK(need == 0 || (scratch && scratch_bytes >= need && aligned4(scratch)),
             "gif_dither: %d frames of %d rows of %d pixels need %lld bytes of 4-byte aligned scratch for the carry rows, got %lld", n, H, W, need,
             scratch ? scratch_bytes : 0ll);
  MMGT_CHECK(aligned4(frames) && (reinterpret_cast<uintptr_t>(lut) & 15) == 0, "gif_dither: frames must be 4-byte aligned, lut 16-byte aligned");
  hipLaunchKernelGGL(gif_dither_kernel, dim3((unsigned)n), dim3(GDI_BAND), 0, (hipStream_t)stream, frames, lut, palette, idx,
                     static_cast<unsigned*>(scratch), H, W, 3ll * n * H * W);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_gif_delta(const unsigned char* idx, const unsigned char* prev, unsigned char* out, int n, int H, int W, void* stream) {
  MMGT_CHECK(idx && out && idx != out, "gif_delta: null pointer, or out is idx");
  MMGT_CHECK(clip_ok(n, H, W), kBadClip, "gif_delta", n, H, W);
  MMGT_CHECK(aligned4(idx) && aligned4(out), "gif_delta: idx and out must be 4-byte aligned");
  const size_t npix = (size_t)n * H * W;
  const size_t want = ((npix + 3) / 4 + 4 * 256 - 1) / (4 * 256);
  const unsigned grid = (unsigned)(want < 1 ? 1 : want > 1024 ? 1024 : want);
  hipLaunchKernelGGL(gif_delta_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, idx, prev, out, npix, (size_t)H * W);
  MMGT_LAUNCH_CHECK();
  return 0;
}

// The most bits a strip of P = W * strip_rows pixels can take.  The coder writes (a) one code per dictionary miss and one for the string pending at the
// strip's end: at most one per pixel, P in all; (b) a Clear each time code 4095 has been assigned: every assignment follows a miss on a pixel of its own
// and 3838 codes (258 .. 4095) lie between two such Clears, so at most floor(P / 3838); (c) the leading Clear of strip 0 and the closing Clear or
// End-of-Information: 2.  No code is wider than 12 bits.  Hence bits <= 12 (P + floor(P / 3838) + 2) for ANY indices; the stride is that in bytes,
// rounded up to 16 (so the last, partly filled 32-bit word of the writer lies inside the slot too).
extern "C" int mmgt_gif_strip_stride(int W, int strip_rows, long* stride) {
  MMGT_CHECK(stride, "gif_strip_stride: null output");
  MMGT_CHECK(W >= 1 && W <= 65535 && strip_rows >= 1 && strip_rows <= 65535 && (long)W * strip_rows <= (1L << 28),
             "gif_strip_stride: W = %d, strip_rows = %d are outside the range (1 .. 65535 each, W * strip_rows <= 2^28)", W, strip_rows);
  const long P = (long)W * strip_rows;
  const long bits = 12 * (P + P / kFreeCodes + 2);
  *stride = ((bits + 7) / 8 + 15) / 16 * 16;
  return 0;
}

extern "C" int mmgt_gif_lzw(const unsigned char* idx, unsigned char* out, long long* bits, int n, int H, int W, int strip_rows, long out_stride,
                            void* stream) {
  long need = 0;
  MMGT_CHECK(idx && out && bits, "gif_lzw: null pointer");
  MMGT_CHECK(clip_ok(n, H, W), kBadClip, "gif_lzw", n, H, W);
  if (mmgt_gif_strip_stride(W, strip_rows, &need)) return 1;
  MMGT_CHECK(out_stride >= need && out_stride % 4 == 0, "gif_lzw: out_stride %ld must be a multiple of 4 and at least the worst case of a strip, %ld bytes",
             out_stride, need);
  MMGT_CHECK(aligned4(idx) && aligned4(out), "gif_lzw: idx and out must be 4-byte aligned");
  const long strips = (H + strip_rows - 1) / strip_rows;
  MMGT_CHECK(strips <= kMaxStrips && (long long)n * strips <= 0x7fffffffLL, "gif_lzw: %ld strips per frame (at most %d) x %d frames", strips, kMaxStrips, n);
  hipLaunchKernelGGL(gif_lzw_kernel, dim3((unsigned)(n * strips)), dim3(64), 0, (hipStream_t)stream, idx, out, bits, (size_t)n * H * W, H, W, strip_rows,
                     (int)strips, out_stride);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_gif_pack(const unsigned char* out, const long long* bits, unsigned char* packed, int* sizes, int n, int strips, long out_stride,
                             long packed_stride, void* stream) {
  MMGT_CHECK(out && bits && packed && sizes, "gif_pack: null pointer");
  MMGT_CHECK(n >= 1 && n <= 65535 && strips >= 1 && strips <= kMaxStrips && out_stride >= 1, "gif_pack: n = %d, strips = %d (at most %d), out_stride = %ld",
             n, strips, kMaxStrips, out_stride);
  const long long nbytes = (long long)strips * out_stride;         // a frame's data cannot be longer than its slots
  const long long need = nbytes + (nbytes + 254) / 255 + 1;
  MMGT_CHECK(need <= 0x7fffffffLL && packed_stride >= need, "gif_pack: packed_stride %ld is below the worst case of a frame, %lld bytes (< 2^31)",
             packed_stride, need);
  const long long want = (nbytes + 4 * 256 - 1) / (4 * 256);
  const unsigned gx = (unsigned)(want < 1 ? 1 : want > 64 ? 64 : want);
  hipLaunchKernelGGL(gif_pack_kernel, dim3(gx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, out, bits, packed, sizes, strips, out_stride, packed_stride);
  MMGT_LAUNCH_CHECK();
  return 0;
}
