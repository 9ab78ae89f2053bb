// Host program over mmgt_amd/csrc/gemm_plan.h: the plan gemm.hip's launch() gets for a shape, without a GPU.  Plain C++ (no HIP);
// tests/test_gemm_plan.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it.
//
//   gemm_plan_host_check plan FILE [gemm_cfg splitk tailsplit bm192]
//       FILE holds one shape per line: bf16 mode M N K batch act fast post residual bias_unaligned bias_post_unaligned up ksplit img.
//       Prints one plan per line: kind BM BN WM WN NSTAGE EPI bm bn S rows_a (fields a kind does not have are 0).
//   gemm_plan_host_check contracts [STEP]
//       The contracts gemm.hip and gemm16.hip rely on, over a sweep of shapes x switches (every STEP-th shape of it; default 1: all, minutes).
//       Prints the number of cases and "ok", or the first case that breaks a contract.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm_plan.h"

using namespace mmgt_plan;

namespace {

const char* KIND[] = {"tile", "g16_tile", "g16_splitk", "g16_tail", "refuse"};

void print_shape(FILE* f, const GemmShape& s, const GemmSwitches& w) {
  fprintf(f, "bf16=%d mode=%d M=%d N=%d K=%d batch=%d act=%d fast=%d post=%d residual=%d bias_unaligned=%d bias_post_unaligned=%d up=%d ksplit=%d img=%ld | "
          "gemm_cfg=%d splitk=%d tailsplit=%d bm192=%d", s.bf16, s.mode, s.M, s.N, s.K, s.batch, s.act, s.fast, s.post, s.residual, s.bias_unaligned,
          s.bias_post_unaligned, s.up, s.ksplit, s.img, w.gemm_cfg, w.splitk, w.tailsplit, w.bm192);
}

void print_plan(FILE* f, const GemmPlan& p) {
  const TileDims d = p.kind == PLAN_TILE ? TILE_DIMS[p.tile] : TileDims{0, 0, 0, 0, 0, 0};
  fprintf(f, "%s %d %d %d %d %d %d %d %d %d %d\n", KIND[p.kind], d.BM, d.BN, d.WM, d.WN, d.NSTAGE, d.EPI, p.bm, p.bn, p.S, p.rows_a);
}

// ---- the sweep: M around every threshold the rules name, the widths and reductions of the models, every flag against every switch
std::vector<int> sweep_rows() {
  std::vector<int> m = {2, 64, 300, 320, 640, 1280, 3072, 4096, 6144, 8192, 12288, 32768, 98304, 196608, 524288, 2097152};   // tools/ab_cfg.py's row counts
  for (int t : {1536, 24576, 49152, 131072})
    for (int d = -1; d <= 1; ++d) m.push_back(t + d);
  for (int step : {192, 256})
    for (int t = step; t <= 2048; t += step)
      for (int d = -1; d <= 1; ++d) m.push_back(t + d);
  std::sort(m.begin(), m.end());
  m.erase(std::unique(m.begin(), m.end()), m.end());
  return m;
}
const int SWEEP_N[] = {3, 4, 36, 64, 128, 200, 256, 320, 512, 640, 960, 1280, 1920, 2560, 3840, 5120, 10240};
const int SWEEP_K[] = {64, 320, 640, 1280, 2496, 2560, 2880, 5120, 5760, 11520, 17280, 23040};
const int SWEEP_CFG[] = {0, 1, 3, 6, 9, 12, 16, 17, 18, 19, 20, 7};

// Calls f(shape, switches) on every case with M rows: every `step`-th shape (`seen` counts them across calls) against every switch setting.  Left out, because the entry points of gemm.hip refuse them: GEGLU with N % 64 != 0
// and GEGLU with an unaligned post-scale bias (gemm_entry), GEGLU on a conv (conv3x3: act 0, 2 or 3), up >= 2 in fp32 or with a width that
// is no multiple of 256 or 320, up == 2 with a residual or an activation, up == 3 with an activation or an unaligned bias (the conv entries).
// (An unaligned post-scale bias behind aligned bias vectors implies post: that is what the two facts mean, not a pruning.)
template <class F>
void sweep_rows_of(int M, long step, long& seen, F&& f) {
  GemmShape s{};
  s.M = M;
  for (int N : SWEEP_N) for (int K : SWEEP_K) for (int mode = 0; mode < 2; ++mode) for (int b16 = 0; b16 < 2; ++b16) for (int act = 0; act < 3; ++act) {
    if (act == 1 && (N % 64 != 0 || mode == 1)) continue;
    for (int fast = 0; fast < 2; ++fast) for (int post = 0; post < 2; ++post) for (int res = 0; res < 2; ++res) for (int al = 0; al < 3; ++al) {
      if (al == 1 && (!post || act == 1)) continue;
      for (int up = 0; up < 4; ++up) {
        if (mode == 1 && up >= 2 && (!b16 || (N % 256 != 0 && N % 320 != 0) || act != 0 || (up == 2 && res) || (up == 3 && al == 2))) continue;
        for (int ksplit = 0; ksplit < 2; ++ksplit) for (int batch : {1, 4, 48}) for (long img : {64l, 256l, 1024l, 4096l}) {
          if ((mode == 0 && img != 64) || seen++ % step) continue;
          s.N = N; s.K = K; s.mode = mode; s.bf16 = b16; s.act = act; s.fast = fast; s.post = post; s.residual = res;
          s.bias_unaligned = al == 2; s.bias_post_unaligned = al >= 1; s.up = up; s.ksplit = ksplit; s.batch = batch; s.img = mode ? img : 1;
          for (int cfg : SWEEP_CFG) for (int sw = 0; sw < 8; ++sw) {
            GemmSwitches w;
            w.gemm_cfg = cfg; w.splitk = sw & 1; w.tailsplit = (sw >> 1) & 1; w.bm192 = (sw >> 2) & 1;
            f(s, w);
          }
        }
      }
    }
  }
}

// The contracts the launch side and gemm16.hip rely on; returns what is broken, or nullptr.
const char* broken_contract(const GemmShape& s, const GemmSwitches& w, const GemmPlan& p) {
  const bool g16 = p.kind == PLAN_G16_TILE || p.kind == PLAN_G16_SPLITK || p.kind == PLAN_G16_TAIL;
  const bool geglu = s.act == 1;
  if (g16 && !(s.bf16 && s.fast)) return "a gemm16 plan without bf16 and the vectorised epilogue";
  if (g16 && !((p.bm == 256 && (p.bn == 128 || p.bn == 256 || p.bn == 320)) || (p.bm == 192 && p.bn == 320))) return "a gemm16 tile that does not exist";
  if (geglu && p.kind == PLAN_TILE && (p.tile == T128x64 || p.tile == T128x320)) return "GEGLU on a 128x64 or 128x320 tile";
  if (geglu && g16 && !(p.kind == PLAN_G16_TILE && p.bm == 256 && p.bn == 256 && !s.post)) return "GEGLU on gemm16 other than the 256x256 tile without post";
  if (p.kind == PLAN_TILE && p.tile == T128x128_POST && s.mode != 0) return "the dense POST instantiation for a conv";
  if (s.mode == 1 && s.up >= 2 && !g16 && p.kind != PLAN_REFUSE) return "up >= 2 off the gemm16 path";
  if (p.kind == PLAN_REFUSE && !(s.mode == 1 && s.up >= 2)) return "a refusal without up >= 2";
  if (p.kind == PLAN_G16_SPLITK) {
    const long tiles = (long)((s.M + 255) / 256) * ((s.N + p.bn - 1) / p.bn);
    if (!(s.batch == 1 && s.act == 0 && p.S >= 2 && p.S <= 8 && (s.K / 64) % p.S == 0 && p.S * tiles <= 256 && s.N % p.bn == 0 && s.N % 8 == 0 && !s.post))
      return "split-K outside batch 1, no activation, S in 2..8, (K / 64) % S == 0, S x tiles <= 256";
    if (w.gemm_cfg != 0 && w.gemm_cfg != 18) return "split-K under a forced gemm_cfg";
    if (!w.splitk) return "split-K with the switch off";
  }
  if (p.kind == PLAN_G16_TAIL) {
    const long tail = (long)((s.M - p.rows_a + 255) / 256) * (s.N / p.bn);
    if (!(p.rows_a > 0 && p.rows_a < s.M && p.rows_a % 256 == 0 && p.rows_a % s.img == 0 && 2 * tail <= 256 && 256 <= 4 * tail && p.S == 2 && (s.K / 64) % 2 == 0 &&
          s.mode == 1 && s.batch == 1 && s.act == 0 && !s.post && s.N % p.bn == 0 && s.N % 8 == 0 && p.bm == 256))
      return "tail split outside 0 < rows_a < M, rows_a % 256 == 0, rows_a % img == 0, 2 tail <= 256 <= 4 tail";
    if (!w.tailsplit) return "tail split with the switch off";
  }
  if (g16 && p.bm == 192 && !w.bm192 && w.gemm_cfg != 19) return "the 192-row tile with the switch off";
  return nullptr;
}

int contracts(long step) {
  long shapes = 0, checked = 0;
  int rc = 0;
  for (int M : sweep_rows()) {
    sweep_rows_of(M, step, shapes, [&](const GemmShape& s, const GemmSwitches& w) {
      if (rc) return;
      ++checked;
      const GemmPlan p = plan_gemm(s, w);
      if (const char* what = broken_contract(s, w, p)) {
        fprintf(stderr, "gemm_plan_host_check: %s\n  ", what);
        print_shape(stderr, s, w);
        fprintf(stderr, "\n  -> ");
        print_plan(stderr, p);
        rc = 1;
      }
    });
    if (rc) return rc;
  }
  printf("%ld cases (every %ld-th of %ld shapes x 96 switch settings) ok\n", checked, step, shapes);
  return 0;
}

int plans(const char* path, const GemmSwitches& w) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "gemm_plan_host_check: cannot open %s\n", path); return 2; }
  int v[14];
  long img;
  for (;;) {
    const int got = fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %ld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11, v + 12, v + 13, &img);
    if (got == EOF) break;
    if (got != 15 || v[2] < 1 || v[3] < 1 || v[4] < 1 || v[5] < 1 || img < 1) { fclose(f); fprintf(stderr, "gemm_plan_host_check: bad shape line\n"); return 2; }
    GemmShape s{};
    s.bf16 = v[0]; s.mode = v[1]; s.M = v[2]; s.N = v[3]; s.K = v[4]; s.batch = v[5]; s.act = v[6]; s.fast = v[7]; s.post = v[8]; s.residual = v[9];
    s.bias_unaligned = v[10]; s.bias_post_unaligned = v[11]; s.up = v[12]; s.ksplit = v[13]; s.img = img;
    print_plan(stdout, plan_gemm(s, w));
  }
  fclose(f);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "contracts")) return contracts(argc >= 3 ? atol(argv[2]) > 0 ? atol(argv[2]) : 1 : 1);
  if ((argc == 3 || argc == 7) && !strcmp(argv[1], "plan")) {
    GemmSwitches w;
    if (argc == 7) { w.gemm_cfg = atoi(argv[3]); w.splitk = atoi(argv[4]); w.tailsplit = atoi(argv[5]); w.bm192 = atoi(argv[6]); }
    return plans(argv[2], w);
  }
  fprintf(stderr, "usage: gemm_plan_host_check plan FILE [gemm_cfg splitk tailsplit bm192] | contracts [STEP]\n");
  return 2;
}
