// WavLM's self-attention with the gated relative-position bias (gfx950): the one piece of the WavLM-Large encoder (the reference's
// data/wavlm: WavLM.py + modules_wavlm.py, MultiheadAttention's fast path at modules_wavlm.py:504-540) that the other kernels of
// libmmgt_hip.so cannot do.  Everything else of the model runs on mmgt_gemm / mmgt_layernorm / mmgt_activation / mmgt_lerp_rows.
//
//   o[b, i, h, :] = softmax_j( q_i . k_j * scale + gate[b, h, i] * tab[h, j - i + T - 1] ) V
//   gate[b, h, i] = a (c grep_a[h] - 1) + 2,   (a, c) = sigmoid(sum over groups of 4 of grep_w . x[b, i, h*64 : h*64 + 64] + grep_b)
//
// x is the encoder layer's input AFTER self_attn_layer_norm (the reference's `query`, before the q projection); tab is the raw
// relative-position bias of layer 0 (compute_bias: the Embedding(num_buckets, heads) gathered through the host-computed bucket of
// every offset), shared by all layers.
//
// Structure: one wave per 16 queries, NW waves per workgroup, one (batch, head) pair per workgroup.  The score tile is computed
// TRANSPOSED on 16x16 MFMAs, S^T[key][q] = K . Q^T (v_mfma_f32_16x16x32_bf16; the fp32-I/O parity mode runs the same fragments on
// eight v_mfma_f32_16x16x4_f32, a plain fp32 fma chain), so a lane owns one query column: the gate is ONE register per lane (computed in
// the prologue from the lane's LayerNorm row: 512 FMAs, once per kernel instead of a separate (B, H, T) launch and round trip per layer),
// and the bias is one LDS read per score from the head's 2T - 1 fp32 row, staged once per workgroup.  The accumulator registers of a
// lane are directly the B operand of O^T += V^T . P^T once the keys of V^T are stored in the order the accumulator holds them.
// Softmax, gate and bias are fp32; ragged tails (T = 159 is no multiple of any tile) are clamped on load and masked.
#include "common.h"
#include "mmgt_hip.h"

namespace {

constexpr int HD = 64;     // head_dim (WavLM Base / Large)
constexpr int KT = 32;     // keys per tile (two 16-key score sub-tiles)

struct RelposParams {
  const char *q, *k, *v, *x;
  char* o;
  long q_bs, q_ts, k_bs, k_ts, v_bs, v_ts, o_bs, o_ts, x_bs, x_ts;
  const float *gw, *gb, *ga, *tab;
  int heads, T, nqb;
  float scale;
};

// acc(16x16) += A(16x32) B(32x16): lane (r = lane & 15, g = lane >> 4) supplies A[r][8g + j] and B[8g + j][r], j = 0..7; D: lane holds
// column r, rows 4g .. 4g + 3.  fp32: eight K = 4 instructions, instruction j taking k = 8g + j from lane group g.
__device__ __forceinline__ void mma16(f32x4& acc, const Frag<bf16_t>& a, const Frag<bf16_t>& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma16(f32x4& acc, const Frag<float>& a, const Frag<float>& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

// V^T slot of key kk (0..31) of a tile: the P^T fragment of lane group g holds keys 4g + (0..3) of sub-tile 0 and 16 + 4g + (0..3) of
// sub-tile 1 as its elements 0..3 / 4..7, so V^T row d keeps them at slots 8g .. 8g + 7: one 16-byte (bf16) read per fragment.
__device__ __forceinline__ int vslot(int kk) { return kk < 16 ? 8 * (kk >> 2) + (kk & 3) : 8 * ((kk - 16) >> 2) + 4 + (kk & 3); }

template <typename T, int NW>
__global__ __launch_bounds__(NW * 64) void relpos_attn_kernel(RelposParams p) {
  constexpr int ESZ = sizeof(T);
  constexpr int VEC = 16 / ESZ;
  constexpr int NT = NW * 64;
  constexpr int RSV = KT * ESZ + 16;                         // V^T row stride (bytes): an odd multiple of 16
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lV = smem;                                           // V^T tile: HD rows x KT keys (permuted, see vslot)
  float* lB = reinterpret_cast<float*>(smem + HD * RSV);     // the head's bias row, 2T - 1 fp32

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int pair = blockIdx.x / p.nqb, qblk = blockIdx.x - pair * p.nqb;
  const int b = pair / p.heads, h = pair - b * p.heads;
  const int T_ = p.T;
  const int qreal = (qblk * NW + wid) * 16 + lq;
  const int qi = qreal < T_ ? qreal : T_ - 1;                // rows past the end compute on the last row and store nothing

  for (int r = tid; r < 2 * T_ - 1; r += NT) lB[r] = p.tab[(long)h * (2 * T_ - 1) + r];

  // ---- gate of this lane's query (fp32) ----
  float gate;
  {
    const T* xr = reinterpret_cast<const T*>(p.x) + b * p.x_bs + (long)qi * p.x_ts + h * HD;
    float acc[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = 0.f;
    for (int d = 0; d < HD; ++d) {
      const float xv = Elem<T>::ld(xr + d);
#pragma unroll
      for (int o = 0; o < 8; ++o) acc[o] = fmaf(p.gw[o * HD + d], xv, acc[o]);
    }
    float ga = 0.f, gb = 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      ga += acc[o] + p.gb[o];
      gb += acc[4 + o] + p.gb[4 + o];
    }
    const float sa = 1.f / (1.f + expf(-ga)), sb = 1.f / (1.f + expf(-gb));
    gate = sa * (sb * p.ga[h] - 1.f) + 2.f;
  }

  // ---- Q^T fragments (B operand): lane (lq, lg) holds d = 32 ks + 8 lg + j of query qi ----
  const T* qrow = reinterpret_cast<const T*>(p.q) + b * p.q_bs + (long)qi * p.q_ts + h * HD;
  Frag<T> qf[HD / 32];
#pragma unroll
  for (int ks = 0; ks < HD / 32; ++ks) frag_load(qf[ks], qrow + 32 * ks + 8 * lg);

  const T* kb = reinterpret_cast<const T*>(p.k) + b * p.k_bs + h * HD;
  const T* vb = reinterpret_cast<const T*>(p.v) + b * p.v_bs + h * HD;
  constexpr float LOG2E = 1.4426950408889634f;
  f32x4 o[HD / 16];
#pragma unroll
  for (int i = 0; i < HD / 16; ++i) o[i] = (f32x4)(0.f);
  float m_run = -1e30f, l_run = 0.f;
  const float* brow = lB + (T_ - 1 - qi);                    // brow[j] = tab[h, j - qi + T - 1]

  for (int kt = 0; kt < T_; kt += KT) {
    // ---- stage V^T of keys kt .. kt + 31 (zero past the end: their probabilities are 0, and 0 * garbage must not be NaN) ----
    __syncthreads();                                         // every wave is done with the previous tile (and the bias row is in)
    for (int idx = tid; idx < KT * (HD / VEC); idx += NT) {
      const int kk = idx / (HD / VEC), d0 = (idx - kk * (HD / VEC)) * VEC;
      union { u32x4 u; T e[VEC]; } val;
      val.u = (u32x4)(0u);
      if (kt + kk < T_) val.u = *reinterpret_cast<const u32x4*>(vb + (long)(kt + kk) * p.v_ts + d0);
      const int sl = vslot(kk);
#pragma unroll
      for (int e = 0; e < VEC; ++e) reinterpret_cast<T*>(lV + (d0 + e) * RSV)[sl] = val.e[e];
    }
    __syncthreads();

    // ---- S^T = K . Q^T for two 16-key sub-tiles; K fragments straight from global (rows clamped) ----
    f32x4 s[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      int key = kt + sub * 16 + lq;
      key = key < T_ ? key : T_ - 1;
      const T* krow = kb + (long)key * p.k_ts + 8 * lg;
      s[sub] = (f32x4)(0.f);
#pragma unroll
      for (int ks = 0; ks < HD / 32; ++ks) {
        Frag<T> kf;
        frag_load(kf, krow + 32 * ks);
        mma16(s[sub], kf, qf[ks]);
      }
    }
    // ---- scale, gated bias, mask; tile maximum over the 32 keys of the lane's query ----
    float mt = -1e30f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kt + sub * 16 + 4 * lg + r;
        const float v = j < T_ ? fmaf(s[sub][r], p.scale, gate * brow[j < T_ ? j : 0]) : -1e30f;
        s[sub][r] = v;
        mt = fmaxf(mt, v);
      }
    mt = fmaxf(mt, __shfl_xor(mt, 16));
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = fmaxf(m_run, mt);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
    m_run = m_new;
    float ls = 0.f;
    float p8[8];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = __builtin_amdgcn_exp2f((s[sub][r] - m_new) * LOG2E);
        p8[4 * sub + r] = pv;
        ls += pv;
      }
    l_run = l_run * alpha + ls;
    Frag<T> pf;
    frag_set8(pf, p8);

    // ---- O^T += V^T . P^T ----
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) {
      o[dt] *= alpha;
      Frag<T> vf;
      frag_load(vf, reinterpret_cast<const T*>(lV + (dt * 16 + lq) * RSV) + 8 * lg);
      mma16(o[dt], vf, pf);
    }
  }

  // ---- normalise and store: lane (lq, lg) holds d = 16 dt + 4 lg + (0..3) of query qreal ----
  float l_tot = l_run + __shfl_xor(l_run, 16);
  l_tot += __shfl_xor(l_tot, 32);
  const float inv = 1.f / l_tot;
  if (qreal < T_) {
    T* orow = reinterpret_cast<T*>(p.o) + b * p.o_bs + (long)qreal * p.o_ts + h * HD;
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) {
      const int d = dt * 16 + 4 * lg;
      if (ESZ == 2) {
        union { bf16_t e[4]; u32x2 u; } pk;
#pragma unroll
        for (int e = 0; e < 4; ++e) pk.e[e] = f32_to_bf16(o[dt][e] * inv);
        *reinterpret_cast<u32x2*>(orow + d) = pk.u;
      } else {   // two 8-byte stores (a 16-byte store would be scanned by tools/check_mfma_overlap.py for nothing)
        float* of = reinterpret_cast<float*>(orow + d);
        *reinterpret_cast<f32x2*>(of) = (f32x2){o[dt][0] * inv, o[dt][1] * inv};
        *reinterpret_cast<f32x2*>(of + 2) = (f32x2){o[dt][2] * inv, o[dt][3] * inv};
      }
    }
  }
}

template <typename T, int NW>
void launch(const RelposParams& p, int batch, hipStream_t s) {
  RelposParams q = p;
  q.nqb = (p.T + 16 * NW - 1) / (16 * NW);
  const size_t lds = (size_t)HD * (KT * sizeof(T) + 16) + (size_t)(2 * p.T - 1) * 4;
  hipLaunchKernelGGL((relpos_attn_kernel<T, NW>), dim3((unsigned)((long)q.nqb * batch * p.heads)), dim3(NW * 64), lds, s, q);
}

}  // namespace

extern "C" int mmgt_relpos_attention(const void* q, long q_bs, long q_ts, const void* k, long k_bs, long k_ts, const void* v, long v_bs,
                                     long v_ts, void* o, long o_bs, long o_ts, const void* x, long x_bs, long x_ts, const float* grep_w,
                                     const float* grep_b, const float* grep_a, const float* tab, int batch, int heads, int hd, int T,
                                     float scale, int dtype, void* stream) {
  MMGT_CHECK(q && k && v && o && x && grep_w && grep_b && grep_a && tab, "relpos_attention: null pointer");
  MMGT_CHECK(dtype == MMGT_F32 || dtype == MMGT_BF16, "relpos_attention: bad dtype %d", dtype);
  MMGT_CHECK(hd == HD, "relpos_attention: head_dim %d unsupported (only 64)", hd);
  MMGT_CHECK(T >= 1 && T <= 4096, "relpos_attention: sequence length %d outside 1 .. 4096", T);
  MMGT_CHECK(batch >= 1 && heads >= 1 && (long)batch * heads * ((T + 15) / 16) < (1l << 31), "relpos_attention: bad batch %d / heads %d",
             batch, heads);
  const long vec = dtype == MMGT_BF16 ? 8 : 4;
  MMGT_CHECK(q_ts % vec == 0 && k_ts % vec == 0 && v_ts % vec == 0 && o_ts % vec == 0 && q_bs % vec == 0 && k_bs % vec == 0 &&
                 v_bs % vec == 0 && o_bs % vec == 0 && ((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 == 0,
             "relpos_attention: q/k/v/o and their strides must keep 16-byte alignment");
  RelposParams p{};
  p.q = (const char*)q; p.k = (const char*)k; p.v = (const char*)v; p.x = (const char*)x; p.o = (char*)o;
  p.q_bs = q_bs; p.q_ts = q_ts; p.k_bs = k_bs; p.k_ts = k_ts; p.v_bs = v_bs; p.v_ts = v_ts; p.o_bs = o_bs; p.o_ts = o_ts;
  p.x_bs = x_bs; p.x_ts = x_ts;
  p.gw = grep_w; p.gb = grep_b; p.ga = grep_a; p.tab = tab;
  p.heads = heads; p.T = T; p.scale = scale;
  hipStream_t s = (hipStream_t)stream;
  // one wave per workgroup for the short sequences (T = 159: 10 workgroups per head instead of 3), four from 512 rows on
  if (T < 512) {
    if (dtype == MMGT_BF16) launch<bf16_t, 1>(p, batch, s);
    else launch<float, 1>(p, batch, s);
  } else {
    if (dtype == MMGT_BF16) launch<bf16_t, 4>(p, batch, s);
    else launch<float, 4>(p, batch, s);
  }
  MMGT_LAUNCH_CHECK();
  return 0;
}
