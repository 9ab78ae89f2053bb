// How a dense GEMM or an implicit-GEMM conv runs, decided from the shape alone: shape -> plan -> launch.  Plain C++, no HIP and no pointers, so
// that gemm.hip (which only launches what the plan says) and a host program (tools/gemm_plan_host_check.cpp) read the same rules.
#pragma once

namespace mmgt_plan {

// What the dispatcher knows about one launch (filled by gemm.hip's launch()).
struct GemmShape {
  bool bf16;            // bf16 (else fp32)
  int mode;             // 0 dense, 1 conv gather
  int M, N, K, batch;
  int act;              // Epi::act: 0 none, 1 GEGLU, >= 2 an activation of the FULL epilogue
  bool fast;            // Epi::fast: the vectorised epilogue applies
  bool post;            // row scale, alpha != 1 or a post-scale bias
  bool residual;
  bool bias_unaligned;  // (bias | bias2) & 15, and with the post-scale bias: (bias | bias2 | bias_post) & 15   (bias vectors travel by 16-byte DMA)
  bool bias_post_unaligned;
  int up;               // conv: ADesc::up (>= 2: the four-phase upsample conv and the two-source 1 x 1 conv exist in gemm16.hip only)
  int ksplit;           // conv: ADesc::ksplit
  long img;             // conv: OH * OW, the rows of one image (dense: 1)
};

// The A/B switches (mmgt_tune writes the fields).
struct GemmSwitches {
  int gemm_cfg = 0;   // 0 = heuristic; 1, 3, 6, 9, 12, 16, 17, 19, 20 force a tile configuration (mmgt_tune("gemm_cfg", v), benchmarking only)
  int splitk = 1;     // mmgt_tune("splitk", 0 / 1): A/B switch of the split-K path
  int tailsplit = 1;  // mmgt_tune("tailsplit", 0 / 1): A/B switch of the tail split (below)
  int bm192 = 1;      // mmgt_tune("bm192", 0 / 1): A/B switch of the 192-row gemm16 tile
};

// The instantiations of gemm.hip's gemm_kernel.
// Tiles measured and dropped (tools/ab_gemm.py, one process, one device): 128x128 / 128x64 with a 3-deep ring (round 5 again, with 4-deep
// rings too, on the M = 1536 / 3072 shapes of the 8x8 level: profiles/r5/ab_cfg_deep_r5.txt -- 128x64 x 3 gains 10 % at M = 1536 only), 64x64,
// 256x128 with a 2-deep ring, 256x64, 256x256 with a 3- or 4-deep ring of 64-byte rows, 256x320 on 8 waves (accumulators +
// double-buffered fragments spill inside the main loop; with single-buffered W fragments reloaded right after their last
// MFMA it still spills 56-139 VGPRs and runs 1179 us at 8192^3 against 965) and 256x256 / 256x320 on 4 waves (one wave per SIMD, 512
// registers: +4% at 8192^3, -9% on the 16x16 convs, 2-3x slower wherever the spilling epilogue matters).
enum Tile { T128x128, T128x128_POST, T128x128_FULL, T128x64, T256x128, T256x256, T128x320, N_TILES };
struct TileDims { int BM, BN, WM, WN, NSTAGE, EPI; };
constexpr TileDims TILE_DIMS[N_TILES] = {
    {128, 128, 2, 2, 2, 0},   // gemm_cfg 1: 2 workgroups / CU
    {128, 128, 2, 2, 2, 1},   //   ... with row scale / alpha / post-scale bias (dense, no GEGLU)
    {128, 128, 2, 2, 2, 2},   //   ... the FULL epilogue
    {128, 64, 2, 2, 2, 0},    // gemm_cfg 3: 3 workgroups / CU
    {256, 128, 4, 2, 3, 0},   // gemm_cfg 6: 8 waves, 3-deep ring
    {256, 256, 2, 4, 2, 0},   // gemm_cfg 9: 8 waves, 2-deep ring, barrier inside the chunk
    {128, 320, 4, 2, 2, 0},   // gemm_cfg 12: 8 waves, barrier inside the chunk
};

enum PlanKind {
  PLAN_TILE,        // gemm.hip's gemm_kernel: tile
  PLAN_G16_TILE,    // gemm16.hip, one launch: bm x bn
  PLAN_G16_SPLITK,  // gemm16.hip, S slices of the reduction + the fixed-order reduce: bn, S
  PLAN_G16_TAIL,    // gemm16.hip, rows [0, rows_a) as one launch + the rest split-K at S = 2: bn, rows_a
  PLAN_REFUSE,      // up >= 2 without the gemm16 path
};
struct GemmPlan {
  PlanKind kind;
  Tile tile;       // PLAN_TILE
  int bm, bn;      // PLAN_G16_*: rows (256 or 192) and columns (128, 256 or 320) of the tile
  int S;           // PLAN_G16_SPLITK: slices (PLAN_G16_TAIL: 2)
  int rows_a;      // PLAN_G16_TAIL: rows of the first launch
};

// What the tile choice asks for before the epilogue has its say; the values are the gemm_cfg numbers.
enum Want { W128x128 = 1, W128x64 = 3, W256x128 = 6, W256x256 = 9, W128x320 = 12, G16_256 = 16, G16_320 = 17, G16_192x320 = 19, G16_128 = 20 };

inline Want forced_tile(int gemm_cfg) {
  switch (gemm_cfg) {
    case W128x64: case W256x128: case W256x256: case W128x320: case G16_256: case G16_320: case G16_192x320: case G16_128: return (Want)gemm_cfg;
    default: return W128x128;
  }
}

// Split-K (gemm16.hip): a long reduction on a grid of at most half a tile per CU -- the 8x8-level convs (3072 rows x 1280 columns,
// K = 11 520 / 23 040) and ff2 of that level (K = 5120).  S slices with >= 16 chunks of 64 each, S x tiles <= 256.  Returns S, or 0.
inline int splitk_slices(const GemmShape& sh, int bn) {
  const long tiles = (long)((sh.M + 255) / 256) * (sh.N / bn);
  const int nch = sh.K / 64;
  int S = 0;
  // (measured, tools/ab_cfg.py SET=ctx12 / step: at <= 64 tiles slices of >= 16 chunks pay -- 8x8 convs 126 -> 71 us, 248 -> 101 us, ff2
  // 59 -> 47 us at 12 frames --; between 65 and 128 tiles only long slices do: the 16x16 convs of a 12-frame window -5 %, their ff2 +10 %)
  for (int c = 8; c >= 2; --c)
    if (tiles * c <= 256 && nch % c == 0 && nch / c >= (tiles <= 64 ? 16 : 64)) { S = c; break; }
  // (dense shapes between 33 and 64 tiles -- ff2 of the 8x8 level at 24 frames, 3072 x 1280 x 5120 -- run 8 % faster on the 128 x 64 tile
  //  than split four ways: 58.1 against 63.0 us, profiles/r5/ab_cfg_deep_r5.txt; the convs of that level keep the split: 126 -> 71 us)
  return S >= 2 && tiles <= 128 && (sh.mode == 1 || tiles <= 32 || tiles > 64) ? S : 0;
}

// The tile the measurements prefer for a shape.
inline Want heuristic_tile(const GemmShape& sh, const GemmSwitches& sw) {
  const int M = sh.M, N = sh.N, K = sh.K;
  const bool geglu = sh.act == 1, b16 = sh.bf16;
  // Measured on MI355X with tools/ab_gemm.py / tools/bench_kernels.py (one process, one device; re-swept after the
  // LDS-DMA moved to buffer addressing, which made 128x128 the better small tile for every dense shape):
  //   cfg 6  (256x128, 8 waves, 3-deep ring)    long reductions, GEGLU, and the widest L0 projections;
  //   cfg 1  (128x128, 2 workgroups / CU)       every other dense shape, and the conv gather on the small levels;
  //   cfg 12 (128x320, 8 waves, barrier inside the chunk)   conv outputs whose width is a multiple of 320 on the two
  //          large levels: the im2col gather is staged once per 320 columns instead of once per 128 (-5..-20%);
  //   cfg 3  (128x64, 3 workgroups / CU)        conv grids that would not fill the chip (the 8x8 level).
  const long tiles128 = (long)((M + 127) / 128) * ((N + 127) / 128) * sh.batch;
  const long tiles256 = (long)((M + 255) / 256) * ((N + 127) / 128) * sh.batch;
  //   cfg 9  (256x256, 8 waves, 2-deep ring, barrier inside the chunk)   long reductions whose grid still gives ~one tile
  //          per CU: the 16x16-level convs (-6%); dense shapes: below.
  const long tiles256sq = (long)((M + 255) / 256) * ((N + 255) / 256) * sh.batch;
  const bool big_ok = N % 256 == 0 && K >= 2560 && tiles256sq >= 192 && tiles256sq <= 512;
  // dense: the 256x256 tile wherever N fills its columns to within 7% (N = 960, 1280, 1920, 2560, 3840, 5120, 10240) and
  // the grid still covers the chip -- with the slim common epilogue it no longer spills: GEGLU ff1 -11..-13%, q/k/v
  // projections of the motion modules -13%, the N = 1280 family -5..-10%.
  // (and M: the batched W.X^T projections have M = 320 / 640 rows per problem, 62 / 83 % of two / three 256-row tiles: -13..-17 % on the 128x128 tile)
  const bool sq_ok = ((N + 255) / 256) * 256l * 100 <= (long)N * 107 && ((M + 255) / 256) * 256l * 100 <= (long)M * 115 && tiles256sq >= 192;
  // cfg 16 (gemm16.hip: 256x256, 16x16x32 MFMAs, two wave groups in ping-pong; bf16 only) replaces cfg 9 wherever that ran and
  // takes the convs whose width fills 256-column tiles: measured (tools/ab_cfg.py, one process) -17..-19% on the 16x16-level
  // convs and the 16 -> 32 up-conv, -7..-10% on the long-K / wide dense shapes, -7% on the 32 -> 64 up-conv (N = 640: three
  // tiles with 17% padding still beat the 128x320 tile); K = 320 GEGLU too since the two wave groups run their epilogues side by
  // side (-9%); it loses on N = 320 / 640.
  // cfg 17 = the same core with a 256x320 tile (every width of the UNet is a multiple of 320): the L0 / L1 convs and the
  // 32 -> 64 / 16 -> 32 up-convs (-2..-22%), the dense N = 320 / 640 / 960 shapes of the 64x64 level (-6..-27%) and the long-K,
  // residual or N = 1280 shapes of the 32x32 level (-5..-8%).
  if (sh.mode == 1) {
    if (b16 && N % 320 == 0 && (M >= 49152 || (M >= 24576 && N >= 640))) return G16_320;   // (12-frame windows: the 32x32-level convs, -7..-9 % against 128x128)
    if (b16 && N % 256 == 0 && tiles256sq >= 192) return G16_256;
    return (N % 320 == 0 && M >= 49152) ? W128x320 : big_ok ? W256x256 : (tiles128 < 512 || N <= 64) ? W128x64 : W128x128;   // (N <= 64: conv_out's 3 / 4 channels padded
                                                                                                                             //  to 64 -- VAE 8 x 512^2 x 128 -> 64: 651 -> 503 us on the 128x64 tile)
  }
  if (b16 && !geglu && N % 320 == 0 && N <= 960 && M >= 131072) return G16_320;
  if (b16 && !geglu && N % 320 == 0 && N <= 1280 && M >= 49152 && (K >= 1280 || sh.residual || N == 1280)) return G16_320;   // 32x32 level
  if (b16 && !geglu && N == 640 && M >= 24576 && K >= 2560 && sw.bm192) return G16_320;   // (12-frame windows: ff2 of the 32x32 level on the 192-row tile, 90.4 -> 82.3 us)
  if (sq_ok) return b16 ? G16_256 : W256x256;
  if (geglu || K >= 1280) return tiles256 >= 256 ? W256x128 : (!geglu && tiles128 <= 256) ? W128x64 : W128x128;   // (<= one 128x128 tile per CU: 128x64 tiles, -5..-7 % at M = 3072)
  if (M >= 131072 && N >= 640) return W256x128;
  return W128x128;
}

// gemm16.hip runs bf16 with the plain vectorised epilogue only (max_act 1: GEGLU too)
inline bool gemm16_ok(const GemmShape& sh, int max_act) {
  return sh.bf16 && sh.fast && sh.act <= max_act && !sh.bias_post_unaligned && sh.N % 4 == 0;
}

// cfg 19 = gemm16's 192 x 320 tile (round 5): taken where 256-row tiles leave the last round of the persistent grid half empty.  With T
// tiles on 256 CUs a launch runs ceil(T / 256) rounds of one tile time; a 192-row tile takes ~0.88 of a 256-row tile's time (three MFMA row
// tiles per four W fragment reads instead of four).  Measured (tools/ab_cfg.py SET=bm192, profiles/r5/ab_cfg_bm192_r5.txt): 49 152 x 640
// (384 tiles = 2 rounds against 512 = 2 x 0.88): K = 640 + residual 66.1 -> 62.5 us, K = 2560 + residual 184.8 -> 170.6, K = 1280 89.9 ->
// 83.2; conv 32 x 32, 320 -> 640 185 -> 174; 12-frame windows: 98 304 x 320 + residual 50.3 -> 46.2, 24 576 x 640 x 2560 88.4 -> 82.3, convs
// 175 -> 167 and 190 -> 178.  It loses where the round count does not drop (196 608 rows, N = 1280) and against the tail split of the
// long-reduction convs (48 x 32 x 32, 640 -> 640: 305 us against 322), which therefore keeps its shapes.
inline bool rows192_pay(const GemmShape& sh) {
  if (sh.batch != 1 || sh.N % 320 != 0) return false;
  const long tn = sh.N / 320;
  const long r256 = (((long)(sh.M + 255) / 256) * tn + 255) / 256, r192 = (((long)(sh.M + 191) / 192) * tn + 255) / 256;
  return (double)r192 * 0.88 < (double)r256 * 0.97;
}

// Tail split.  A persistent grid of T tiles runs ceil(T / 256) rounds of one tile per CU; with a long reduction and T = 256 q + r,
// r <= 128 (the 32x32 level: 49 152 rows x 640 columns = 384 tiles), the last round keeps half the chip idle for a whole tile.  The
// rows of the r tail tiles run as a second launch with the reduction split in two (2 r <= 256 half-tiles: one round of half the
// length) + the fixed-order reduce.  Convs only (reductions of 2880 .. 17 280: 32x32 convs 640 -> 640 338 -> 310 us, 1280 -> 640
// 631 -> 556, 1920 -> 640 923 -> 791): the fp32 partial slabs and the reduce cost ~25 us, which a dense K = 2560 tile does not repay.
// Returns the rows of the first launch, or 0.
inline int tail_split_rows(const GemmShape& sh, int bn) {
  const long tiles_n = (sh.N + bn - 1) / bn, tiles_m = (sh.M + 255) / 256, ntile = tiles_m * tiles_n;
  const int nch = sh.K / 64;
  if (!(sh.mode == 1 && sh.batch == 1 && !sh.ksplit && sh.act == 0 && !sh.post && sh.N % bn == 0 && sh.N % 8 == 0 && sh.K >= 2560 && nch % 2 == 0 && ntile > 256)) return 0;
  const long rows_a = (256 * (ntile / 256) / tiles_n) * 256;                  // whole row tiles that fill ntile / 256 full rounds
  const long tail = (tiles_m - rows_a / 256) * tiles_n;
  return rows_a > 0 && rows_a < sh.M && tail > 0 && 2 * tail <= 256 && 4 * tail >= 256 && rows_a % sh.img == 0 ? (int)rows_a : 0;
}

inline GemmPlan plan_gemm(const GemmShape& sh, const GemmSwitches& sw) {
  const bool geglu = sh.act == 1, heuristic = sw.gemm_cfg == 0 || sw.gemm_cfg == 18;   // (18: the heuristic, as 0, but without the 192-row rule)
  auto tile = [](Tile t) { return GemmPlan{PLAN_TILE, t, 0, 0, 0, 0}; };
  auto g16 = [](PlanKind k, int bm, int bn, int S, int rows_a) { return GemmPlan{k, T128x128, bm, bn, S, rows_a}; };
  if (heuristic && sw.splitk && sh.bf16 && sh.batch == 1 && sh.act == 0 && sh.fast && !sh.post && sh.N % 8 == 0 && sh.K >= 2560 &&
      (sh.N % 256 == 0 || sh.N % 320 == 0) && !sh.bias_unaligned) {
    const int bn = sh.N % 256 == 0 ? 256 : 320;
    if (const int S = splitk_slices(sh, bn)) return g16(PLAN_G16_SPLITK, 256, bn, S, 0);
  }
  Want w = heuristic ? heuristic_tile(sh, sw) : forced_tile(sw.gemm_cfg);
  if (geglu && (w == W128x64 || w == W128x320)) w = W128x128;   // GEGLU pairs need 64-column wave tiles
  const bool up2 = sh.mode == 1 && sh.up >= 2;
  if (up2 && w != G16_256 && w != G16_320) w = sh.N % 320 == 0 ? G16_320 : G16_256;   // the four-phase upsample conv exists in gemm16.hip only
  if (w == G16_256 || w == G16_320 || w == G16_192x320) {   // gemm16.hip, 256 / 320 columns: bf16, plain vectorised epilogue only (GEGLU: 256); else fall back
    // (row scale / alpha / post-scale bias: without GEGLU only)
    if (gemm16_ok(sh, w == G16_256 && !sh.post ? 1 : 0)) {
      const int bn = w == G16_256 ? 256 : 320;
      if (sw.tailsplit && w != G16_192x320)   // (a forced 192-row tile stays one launch)
        if (const int rows_a = tail_split_rows(sh, bn)) return g16(PLAN_G16_TAIL, 256, bn, 2, rows_a);
      const bool bm192 = w == G16_192x320 || (w == G16_320 && sw.gemm_cfg == 0 && sw.bm192 && rows192_pay(sh));
      return g16(PLAN_G16_TILE, bm192 ? 192 : 256, bn, 0, 0);
    }
    if (up2) return GemmPlan{PLAN_REFUSE, T128x128, 0, 0, 0, 0};
    w = w == G16_256 ? W256x256 : geglu ? W128x128 : W128x320;   // (GEGLU pairs need 64-column wave tiles: not the 320-column tile)
  }
  if (w == G16_128) {   // gemm16.hip's 256 x 128 tile (round 5): the VAE's 128-wide levels
    if (gemm16_ok(sh, 0)) return g16(PLAN_G16_TILE, 256, 128, 0, 0);
    w = W128x128;
  }
  // anything beyond bias / per-batch bias / GEGLU / residual on the vectorised path runs the FULL instantiation (128x128 tile)
  if (!sh.fast || sh.act >= 2) return tile(T128x128_FULL);
  if (sh.post) return tile(sh.mode == 0 && !geglu ? T128x128_POST : T128x128_FULL);
  switch (w) {
    case W128x64: return tile(T128x64);
    case W256x128: return tile(T256x128);
    case W256x256: return tile(T256x256);
    case W128x320: return tile(T128x320);
    default: return tile(T128x128);
  }
}

}  // namespace mmgt_plan
