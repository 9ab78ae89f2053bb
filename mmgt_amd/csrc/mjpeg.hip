// Baseline sequential JPEG (ITU T.81, JFIF 1.01) of device-resident uint8 RGB frames: the encoder behind the .avi ("MJPG") output path
// (mmgt_amd/video_out.py).  Every frame of a call goes through one set of launches:
//
//  * mmgt_jpeg_dct_quant   (n, H, W, 3) u8 -> int16 coefficients (n, mcu_rows, mcu_cols, blocks_per_mcu, 64) in zigzag order, MCU-interleaved
//                          exactly as the scan codes them (4:2:0: Y00 Y01 Y10 Y11 Cb Cr; 4:4:4: Y Cb Cr).  JFIF full-range BT.601 in fp32
//                          (no rounding to 8 bits in between), level shift -128, 2x2 box average of Cb / Cr for 4:2:0, the frame extended to
//                          the MCU multiple by edge replication, orthonormal 8x8 DCT-II as two fp32 matrix passes through LDS, and
//                          sign(c) floor(|c| / q + 0.5) with a true division.  DC is clamped to [-1024, 1023] and AC to [-1023, 1023]: the
//                          ranges T.81 F.1.2 gives 8-bit samples and the largest categories (11 / 10) the Annex K tables have codes for.
//  * mmgt_jpeg_entropy     one workgroup per (frame, MCU row).  A restart interval of one MCU row makes every MCU row a byte-aligned segment
//                          with its DC predictors reset, so the rows are independent.  Per chunk of 256 blocks: one thread per block counts
//                          the block's bits, a workgroup prefix sum gives every block its bit offset, the blocks OR their codes into an LDS
//                          bit buffer (atomicOr on 32-bit words: the result does not depend on the order), then the finished bytes go out
//                          with 0xFF -> 0xFF 0x00 stuffing placed by a second prefix sum.  A partial last word is carried into the next chunk;
//                          the last chunk is padded with 1-bits to the byte.
//  * mmgt_jpeg_scan        exclusive prefix sum of (segment bytes + 2) -> int64 offsets[nseg + 1] (one workgroup)
//  * mmgt_jpeg_compact     gathers the segments into one contiguous buffer and writes the 2-byte marker after each: RSTm (m = MCU row & 7)
//                          or, after a frame's last row, EOI.  A frame's entropy-coded data with all its markers is then
//                          out[offsets[f * mcu_rows] : offsets[(f + 1) * mcu_rows]]; the host only prepends the fixed headers.
//  * mmgt_jpeg_qtables     (host) the two quantiser tables of a quality, for the caller's DQT segments: one source for kernel and header.
#include "common.h"
#include "mmgt_hip.h"

namespace {

// ---- tables ------------------------------------------------------------------------------------------------------------------------------
// T.81 Annex K.1 / K.2 (natural order)
constexpr unsigned char kBaseQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// zigzag position -> natural index (T.81 figure A.6)
constexpr unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Annex K.3: BITS and HUFFVAL of the four standard tables
constexpr unsigned char kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr unsigned char kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// code | length << 16 per symbol (T.81 Annex C): [0] luminance, [1] chrominance; the DC symbols are the categories 0 .. 11 in order
struct HuffTabs {
  unsigned dc[2][16];
  unsigned ac[2][256];
};
constexpr HuffTabs make_huff() {
  HuffTabs t{};
  for (int c = 0; c < 2; ++c) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len, code <<= 1)
      for (int i = 0; i < kDcBits[c][len - 1]; ++i) t.dc[c][k++] = code++ | (unsigned)len << 16;
    code = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len, code <<= 1)
      for (int i = 0; i < kAcBits[c][len - 1]; ++i) t.ac[c][kAcVals[c][k++]] = code++ | (unsigned)len << 16;
  }
  return t;
}
__device__ const HuffTabs g_huff = make_huff();

// C[u][x] = c(u) / 2 cos((2 x + 1) u pi / 16), c(0) = 1 / sqrt 2: the orthonormal DCT-II matrix, from 0.5 cos(k pi / 16) rounded from fp64
constexpr float dct_c(int u, int x) {
  constexpr float h[9] = {0.5f, 0.4903926402016152f, 0.46193976625564337f, 0.4157348061512726f, 0.35355339059327373f, 0.2777851165098011f,
                          0.19134171618254492f, 0.09754516100806417f, 0.f};
  if (u == 0) return 0.35355339059327373f;
  int t = ((2 * x + 1) * u) % 32;
  if (t > 16) t = 32 - t;
  return t > 8 ? -h[16 - t] : h[t];
}

// natural index -> zigzag position
struct ZzPos {
  unsigned char p[64];
};
constexpr ZzPos make_zzpos() {
  ZzPos z{};
  for (int i = 0; i < 64; ++i) z.p[kZigzag[i]] = (unsigned char)i;
  return z;
}
__device__ const ZzPos g_zzpos = make_zzpos();

struct BaseQ {
  unsigned char q[128];
};
constexpr BaseQ make_baseq() {
  BaseQ b{};
  for (int i = 0; i < 128; ++i) b.q[i] = kBaseQ[i >> 6][i & 63];
  return b;
}
__device__ const BaseQ g_baseq = make_baseq();

// IJG quality rule: scale = 5000 / Q below 50, 200 - 2 Q from 50; entry = clamp((base * scale + 50) / 100, 1, 255)
__host__ __device__ inline int ijg_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }
__host__ __device__ inline int ijg_entry(int base, int scale) {
  const int v = (base * scale + 50) / 100;
  return v < 1 ? 1 : v > 255 ? 255 : v;
}

// ---- stage 1: colour, sampling, DCT, quantiser ---------------------------------------------------------------------------------------------
// One workgroup = a strip of 64 pixels x one MCU row: SS = 2 (4:2:0): 4 MCUs of 16 x 16, SS = 1 (4:4:4): 8 MCUs of 8 x 8; 24 blocks either way.
// Thread t colours the pixels (2 (t & 31) + {0, 1}, SS (t >> 5) + {0 .. SS - 1}) of the strip; threads 0 .. 191 then own one row (pass 1) and one
// column (pass 2) of one block.  Block rows are padded to 9 floats: the column pass reads stride-9 words, conflict-free.
template <int SS>
__global__ __launch_bounds__(256) void jpeg_dct_quant_kernel(const unsigned char* __restrict__ frames, short* __restrict__ coef, int H, int W,
                                                             int mcu_rows, int mcu_cols, int strips, int qscale) {
  constexpr int BPM = SS == 2 ? 6 : 3;                 // blocks per MCU
  constexpr int MPS = SS == 2 ? 4 : 8;                 // MCUs per strip
  __shared__ float blk[24][8][9];
  __shared__ unsigned short q_s[2][64];
  __shared__ __attribute__((aligned(16))) short out_s[24 * 64];
  const int t = threadIdx.x;
  int wg = blockIdx.x;
  const int strip = wg % strips;
  wg /= strips;
  const int mrow = wg % mcu_rows, frame = wg / mcu_rows;
  if (t < 128) q_s[t >> 6][t & 63] = (unsigned short)ijg_entry(g_baseq.q[t], qscale);

  {
    const int qx = t & 31, qy = t >> 5;
    const unsigned char* f = frames + (size_t)frame * H * W * 3;
    const int x0 = strip * 64, y0 = mrow * 8 * SS;
    float cb = 0.f, cr = 0.f;
#pragma unroll
    for (int dy = 0; dy < SS; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int px = 2 * qx + dx, py = SS * qy + dy;
        const int gx = min(x0 + px, W - 1), gy = min(y0 + py, H - 1);                  // edge replication
        const unsigned char* p = f + ((size_t)gy * W + gx) * 3;
        const float r = p[0], g = p[1], b = p[2];
        const float y = 0.299f * r + 0.587f * g + 0.114f * b - 128.f;
        const float u = -0.168736f * r - 0.331264f * g + 0.5f * b;
        const float v = 0.5f * r - 0.418688f * g - 0.081312f * b;
        if (SS == 2) {
          blk[(px >> 4) * 6 + (py >> 3) * 2 + ((px >> 3) & 1)][py & 7][px & 7] = y;
          cb += u;
          cr += v;
        } else {
          blk[(px >> 3) * 3][py][px & 7] = y;
          blk[(px >> 3) * 3 + 1][py][px & 7] = u;
          blk[(px >> 3) * 3 + 2][py][px & 7] = v;
        }
      }
    if (SS == 2) {
      blk[(qx >> 3) * 6 + 4][qy][qx & 7] = 0.25f * cb;
      blk[(qx >> 3) * 6 + 5][qy][qx & 7] = 0.25f * cr;
    }
  }
  __syncthreads();
  const int b = t >> 3, k = t & 7;
  if (t < 192) {                                                                       // rows: blk[b][k][u] = sum_x C[u][x] s[k][x]
    float s[8], o[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) s[x] = blk[b][k][x];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float a = 0.f;
#pragma unroll
      for (int x = 0; x < 8; ++x) a = fmaf(dct_c(u, x), s[x], a);
      o[u] = a;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) blk[b][k][u] = o[u];
  }
  __syncthreads();
  if (t < 192) {                                                                       // columns: F[v][k] = sum_y C[v][y] blk[b][y][k]
    float s[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) s[y] = blk[b][y][k];
    const int tbl = (b % BPM) >= BPM - 2;                                              // the last two blocks of an MCU are Cb, Cr
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      float a = 0.f;
#pragma unroll
      for (int y = 0; y < 8; ++y) a = fmaf(dct_c(v, y), s[y], a);
      const int nat = v * 8 + k;
      const float m = floorf(fabsf(a) / (float)q_s[tbl][nat] + 0.5f);
      int c = (int)m;
      c = min(c, 1023);
      c = a < 0.f ? -c : c;
      if (nat == 0 && a < 0.f && m >= 1024.f) c = -1024;
      out_s[b * 64 + g_zzpos.p[nat]] = (short)c;
    }
  }
  __syncthreads();
  // the strip's blocks are contiguous in the output: 16-byte stores, bounded by the MCUs that exist
  const int mcu0 = strip * MPS;
  const int nblk = min(MPS, mcu_cols - mcu0) * BPM;
  short* o = coef + (((size_t)frame * mcu_rows + mrow) * mcu_cols + mcu0) * BPM * 64;
  if (t < nblk * 8) reinterpret_cast<u32x4*>(o)[t] = reinterpret_cast<const u32x4*>(out_s)[t];
}

// ---- stage 2: entropy coder ------------------------------------------------------------------------------------------------------------------
// The most bits one block can take: a DC code of 11 bits (chrominance category 11) with 11 value bits, and 63 AC coefficients of a 16-bit code
// with 10 value bits each (no zero run, so neither ZRL nor EOB) = 22 + 63 * 26 = 1660 bits.  Stuffing can at most double the bytes.  Hence a
// segment (one MCU row of nb blocks, padded to the byte) never exceeds 2 * ceil(1660 nb / 8) bytes: mmgt_jpeg_segment_stride, which holds for ANY
// coefficients in the clamped range, so no input can be truncated.
constexpr int kChunk = 256;                                       // blocks per chunk = threads per workgroup
constexpr int kBlockBits = 22 + 63 * 26;
constexpr int kBufWords = kChunk * kBlockBits / 32 + 3;           // carry (< 32 bits) + chunk, rounded up, + the word the zero fill runs to

// exclusive prefix sum over the 256 threads of a workgroup (wave scans by shuffle, the four wave totals through LDS); *total = sum of all
template <typename T>
__device__ __forceinline__ T wg_exscan(T v, T* total, T* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T n = __shfl_up(inc, o);
    if (lane >= o) inc += n;
  }
  __syncthreads();                                                 // wsum may still be read from the previous scan
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const T s = wsum[i];
    if (i < w) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}

struct CountSink {
  int n = 0;
  __device__ __forceinline__ void put(unsigned, int len) { n += len; }
};
// MSB-first bit writer into 32-bit LDS words (bit 31 of word 0 is the first bit of the stream).  Blocks share words at their borders, so whole
// words go out with atomicOr into a zeroed buffer.
struct PackSink {
  unsigned* buf;
  int word, nacc;
  unsigned long long acc = 0;
  __device__ __forceinline__ PackSink(unsigned* b, int bitoff) : buf(b), word(bitoff >> 5), nacc(bitoff & 31) {}
  __device__ __forceinline__ void put(unsigned bits, int len) {    // len <= 27
    acc = acc << len | bits;
    nacc += len;
    if (nacc >= 32) {
      nacc -= 32;
      atomicOr(&buf[word++], (unsigned)(acc >> nacc));
      acc &= (1ull << nacc) - 1;
    }
  }
  __device__ __forceinline__ void flush() {
    if (nacc) atomicOr(&buf[word], (unsigned)(acc << (32 - nacc)));
  }
};

// T.81 F.1.2: DC difference as category + value bits, AC as (run, category) symbols with ZRL and EOB
template <class Sink>
__device__ __forceinline__ void code_block(const short* __restrict__ c, int pred, const unsigned* dc, const unsigned* ac, Sink& s) {
  const s16x8* p = reinterpret_cast<const s16x8*>(c);
  int run = 0;
  auto value = [](int v, int cat) { return (unsigned)(v < 0 ? v + (1 << cat) - 1 : v); };
  for (int i = 0; i < 8; ++i) {
    const s16x8 x = p[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = x[j];
      if (i == 0 && j == 0) {
        const int d = v - pred;
        const int cat = 32 - __clz(abs(d));
        const unsigned h = dc[cat];
        s.put((h & 0xffffu) << cat | value(d, cat), (int)(h >> 16) + cat);
      } else if (v == 0) {
        ++run;
      } else {
        while (run >= 16) {
          const unsigned h = ac[0xf0];
          s.put(h & 0xffffu, (int)(h >> 16));
          run -= 16;
        }
        const int cat = 32 - __clz(abs(v));
        const unsigned h = ac[run << 4 | cat];
        s.put((h & 0xffffu) << cat | value(v, cat), (int)(h >> 16) + cat);
        run = 0;
      }
    }
  }
  if (run) {
    const unsigned h = ac[0];
    s.put(h & 0xffffu, (int)(h >> 16));
  }
}

// nb = blocks of one MCU row (mcu_cols * bpm), bpm = 6 (4:2:0) or 3 (4:4:4)
__global__ __launch_bounds__(kChunk) void jpeg_entropy_kernel(const short* __restrict__ coef, unsigned char* __restrict__ segs, int* __restrict__ sizes,
                                                              int nb, int bpm, long seg_stride) {
  __shared__ unsigned buf[kBufWords];
  __shared__ unsigned dc_s[2][16], ac_s[2][256];
  __shared__ int wsum[4];
  const int t = threadIdx.x;
  const short* row = coef + (size_t)blockIdx.x * nb * 64;
  unsigned char* out = segs + (size_t)blockIdx.x * seg_stride;
  if (t < 32) dc_s[t >> 4][t & 15] = g_huff.dc[t >> 4][t & 15];
  ac_s[0][t] = g_huff.ac[0][t];
  ac_s[1][t] = g_huff.ac[1][t];
  __syncthreads();

  unsigned carry = 0;                                              // the bits of an unfinished word, left-aligned
  int carry_bits = 0;
  long outpos = 0;
  for (int j0 = 0; j0 < nb; j0 += kChunk) {
    const int j = j0 + t;
    const bool valid = j < nb;
    int pred = 0, tbl = 0;
    const short* c = row + (size_t)j * 64;
    if (valid) {                                                   // DC predictor: the previous block of the same component in this MCU row
      const int k = j % bpm, m = j / bpm;
      tbl = k >= bpm - 2;
      const int back = (bpm == 6 && k > 0 && k < 4) ? 1 : (bpm == 6 && k == 0) ? 3 : bpm;
      if (m > 0 || (bpm == 6 && k > 0 && k < 4)) pred = c[-back * 64];
    }
    CountSink cs;
    if (valid) code_block(c, pred, dc_s[tbl], ac_s[tbl], cs);
    int total;
    const int off = wg_exscan(cs.n, &total, wsum);
    const int T = carry_bits + total;                              // bits in the buffer once this chunk is packed
    const bool last = j0 + kChunk >= nb;
    for (int i = t; i <= (T + 31) >> 5; i += kChunk) buf[i] = i == 0 ? carry : 0u;
    __syncthreads();
    if (valid) {
      PackSink ps(buf, carry_bits + off);
      code_block(c, pred, dc_s[tbl], ac_s[tbl], ps);
      ps.flush();
    }
    __syncthreads();
    int nbytes = (T >> 5) * 4;                                     // whole words now, the rest with the next chunk
    if (last) {                                                    // pad the last byte with 1-bits (T.81 F.1.2.3)
      nbytes = (T + 7) >> 3;
      const int pad = nbytes * 8 - T;
      if (t == 0 && pad) buf[T >> 5] |= ((1u << pad) - 1) << (32 - (T & 31) - pad);
      __syncthreads();
    }
    // bytes out, each 0xFF followed by 0x00: 4 bytes (one word) per thread and round, placed by a prefix sum of the 0xFF counts
    for (int w0 = 0; w0 * 4 < nbytes; w0 += kChunk) {
      const int wi = w0 + t;
      const int nh = min(max(nbytes - 4 * wi, 0), 4);
      const unsigned word = nh > 0 ? buf[wi] : 0u;
      int ff = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) ff += (k < nh && ((word >> (24 - 8 * k)) & 0xffu) == 0xffu);
      int nff;
      const int ex = wg_exscan(ff, &nff, wsum);
      long p = outpos + 4 * t + ex;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nh) {
          const unsigned char b = (unsigned char)(word >> (24 - 8 * k));
          if (p < seg_stride) out[p] = b;
          ++p;
          if (b == 0xff) {
            if (p < seg_stride) out[p] = 0;
            ++p;
          }
        }
      outpos += min(nbytes - 4 * w0, 4 * kChunk) + nff;
    }
    carry = buf[T >> 5];                                           // read by every thread before the next chunk's scan barrier lets the fill start
    carry_bits = T & 31;
  }
  if (t == 0) sizes[blockIdx.x] = (int)outpos;
}

// ---- stage 3: offsets and gather -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_scan_kernel(const int* __restrict__ sizes, long long* __restrict__ offsets, int nseg) {
  __shared__ long long wsum[4];
  long long base = 0;
  for (int i0 = 0; i0 < nseg; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    const long long v = i < nseg ? (long long)sizes[i] + 2 : 0;   // + the RSTm / EOI marker
    long long tot;
    const long long ex = wg_exscan(v, &tot, wsum);
    if (i < nseg) offsets[i] = base + ex;
    base += tot;
  }
  if (threadIdx.x == 0) offsets[nseg] = base;
}

__global__ __launch_bounds__(256) void jpeg_compact_kernel(const unsigned char* __restrict__ segs, long seg_stride, const int* __restrict__ sizes,
                                                           const long long* __restrict__ offsets, unsigned char* __restrict__ out, long long out_bytes,
                                                           int mcu_rows) {
  const int seg = blockIdx.x;
  const unsigned char* s = segs + (size_t)seg * seg_stride;
  const long long o = offsets[seg];
  const int n = sizes[seg];
  if (o + n + 2 > out_bytes) return;                               // a caller's buffer smaller than offsets[nseg]: nothing is written past it
  for (int i = threadIdx.x; i < n; i += 256) out[o + i] = s[i];
  if (threadIdx.x == 0) {
    const int r = seg % mcu_rows;
    out[o + n] = 0xff;
    out[o + n + 1] = r == mcu_rows - 1 ? 0xd9 : (unsigned char)(0xd0 + (r & 7));
  }
}

struct Geom {
  int ss, bpm, mcu_rows, mcu_cols;
};
bool geom(int H, int W, int subsampling, Geom& g) {
  if (subsampling != 420 && subsampling != 444) return false;
  g.ss = subsampling == 420 ? 2 : 1;
  g.bpm = subsampling == 420 ? 6 : 3;
  g.mcu_rows = (H + 8 * g.ss - 1) / (8 * g.ss);
  g.mcu_cols = (W + 8 * g.ss - 1) / (8 * g.ss);
  return true;
}
const char* kBadSampling = "%s: subsampling %d is not built (420 and 444 are)";
// frames, coefficient and segment indices are formed in 64 bits; the grids and the per-frame counts are ints
bool fits(int n, int H, int W, const Geom& g) {
  return H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && n >= 1 &&
         (long long)n * g.mcu_rows * g.mcu_cols * 64 * g.ss * g.ss <= 0x7fffffffLL;
}

}  // namespace

extern "C" int mmgt_jpeg_qtables(int quality, unsigned char* zigzag128) {
  MMGT_CHECK(zigzag128, "jpeg_qtables: null output");
  MMGT_CHECK(quality >= 1 && quality <= 100, "jpeg_qtables: quality %d is outside 1 .. 100", quality);
  const int s = ijg_scale(quality);
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 64; ++i) zigzag128[c * 64 + i] = (unsigned char)ijg_entry(kBaseQ[c][kZigzag[i]], s);
  return 0;
}

extern "C" int mmgt_jpeg_segment_stride(int W, int subsampling, long* stride) {
  Geom g;
  MMGT_CHECK(stride, "jpeg_segment_stride: null output");
  MMGT_CHECK(geom(8, W > 0 ? W : 1, subsampling, g), kBadSampling, "jpeg_segment_stride", subsampling);
  MMGT_CHECK(W >= 1 && W <= 65535, "jpeg_segment_stride: width %d is outside 1 .. 65535", W);
  const long nb = (long)g.mcu_cols * g.bpm;
  *stride = (2 * ((kBlockBits * nb + 7) / 8) + 15) / 16 * 16;
  return 0;
}

extern "C" int mmgt_jpeg_dct_quant(const unsigned char* frames, short* coef, int n, int H, int W, int subsampling, int quality, void* stream) {
  Geom g;
  MMGT_CHECK(frames && coef, "jpeg_dct_quant: null pointer");
  MMGT_CHECK(quality >= 1 && quality <= 100, "jpeg_dct_quant: quality %d is outside 1 .. 100", quality);
  MMGT_CHECK(geom(H, W, subsampling, g), kBadSampling, "jpeg_dct_quant", subsampling);
  MMGT_CHECK(fits(n, H, W, g), "jpeg_dct_quant: n = %d frames of %d x %d are outside the index range (H, W <= 65535, n * padded pixels < 2^31)", n, H, W);
  const int strips = (g.mcu_cols * 8 * g.ss + 63) / 64;
  const dim3 grid((unsigned)((long)n * g.mcu_rows * strips));
  if (g.ss == 2)
    hipLaunchKernelGGL(jpeg_dct_quant_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, frames, coef, H, W, g.mcu_rows, g.mcu_cols, strips,
                       ijg_scale(quality));
  else
    hipLaunchKernelGGL(jpeg_dct_quant_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, frames, coef, H, W, g.mcu_rows, g.mcu_cols, strips,
                       ijg_scale(quality));
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_jpeg_entropy(const short* coef, unsigned char* segs, int* sizes, int n, int H, int W, int subsampling, long seg_stride,
                                 void* stream) {
  Geom g;
  long need = 0;
  MMGT_CHECK(coef && segs && sizes, "jpeg_entropy: null pointer");
  MMGT_CHECK(geom(H, W, subsampling, g), kBadSampling, "jpeg_entropy", subsampling);
  MMGT_CHECK(fits(n, H, W, g), "jpeg_entropy: n = %d frames of %d x %d are outside the index range (H, W <= 65535, n * padded pixels < 2^31)", n, H, W);
  if (mmgt_jpeg_segment_stride(W, subsampling, &need)) return 1;
  MMGT_CHECK(seg_stride >= need, "jpeg_entropy: seg_stride %ld is below the worst case of an MCU row, %ld bytes", seg_stride, need);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)(n * g.mcu_rows)), dim3(kChunk), 0, (hipStream_t)stream, coef, segs, sizes,
                     g.mcu_cols * g.bpm, g.bpm, seg_stride);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_jpeg_scan(const int* sizes, long long* offsets, int nseg, void* stream) {
  MMGT_CHECK(sizes && offsets && nseg >= 1, "jpeg_scan: bad arguments");
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sizes, offsets, nseg);
  MMGT_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmgt_jpeg_compact(const unsigned char* segs, long seg_stride, const int* sizes, const long long* offsets, unsigned char* out,
                                 long long out_bytes, int nseg, int mcu_rows, void* stream) {
  MMGT_CHECK(segs && sizes && offsets && out, "jpeg_compact: null pointer");
  MMGT_CHECK(nseg >= 1 && mcu_rows >= 1 && nseg % mcu_rows == 0 && seg_stride > 0 && out_bytes > 0, "jpeg_compact: bad arguments");
  hipLaunchKernelGGL(jpeg_compact_kernel, dim3((unsigned)nseg), dim3(256), 0, (hipStream_t)stream, segs, seg_stride, sizes, offsets, out, out_bytes,
                     mcu_rows);
  MMGT_LAUNCH_CHECK();
  return 0;
}
