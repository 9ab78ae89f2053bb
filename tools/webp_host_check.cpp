// The arithmetic of the WebP lossless writer (mmgt_amd/csrc/webp_core.h, the functions csrc/webp.hip's kernels call) run on the host, so that it can
// be built with AddressSanitizer and UBSan and held to the yardstick of tests/webp_ref.py without a GPU (tests/test_webp.py builds and runs it).
//
//   webp_host_check JOB OUT
//   webp_host_check --png-tokens JOB OUT
//
// JOB: int32 n, H, W, strip_rows, then n * H * W * 3 bytes of RGB.  OUT: the modes, n * bh * bw bytes; the residuals, n * H * W uint32 ARGB words;
// then per frame and strip an uint32 count of tokens and per token two uint32: 0 and the literal's word, or a match's length and its prefix symbol |
// extra bits << 8 | extra value << 16.  The loops mirror the kernels': a block's 14 costs summed pixel by pixel, the residuals taken under the
// winning mode, a strip's tokens found position by position from the start of the run that the position lies in.
//
// --png-tokens runs the PNG writer's tokens (csrc/png.hip: csrc/strip_coder.h's closed form at 258, which webp_core.h's wp_token_at uses at 4096) the
// same way (tests/test_png.py).  JOB: int32 len, strip_bytes, then len bytes.  OUT: per strip an uint32 count of tokens and per token one uint32, the
// literal's byte or a match's length | 0x1000.  The end-of-block symbol is not a token of the closed form and is not written.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "webp_core.h"

static int fail(const char* what) {
  std::fprintf(stderr, "webp_host_check: %s\n", what);
  return 2;
}

static int png_tokens(const char* job, const char* result) {
  FILE* in = std::fopen(job, "rb");
  if (!in) return fail("cannot open the job");
  int32_t head[2];
  if (std::fread(head, sizeof(int32_t), 2, in) != 2) return fail("short job");
  const long len = head[0], strip_bytes = head[1];
  if (len < 1 || len > (1l << 26) || strip_bytes < 1) return fail("sizes outside the range");
  std::vector<unsigned char> data((size_t)len);
  if (std::fread(data.data(), 1, data.size(), in) != data.size()) return fail("short job");
  std::fclose(in);
  FILE* out = std::fopen(result, "wb");
  if (!out) return fail("cannot open the output");
  for (long first = 0; first < len; first += strip_bytes) {
    const int n = (int)(len - first < strip_bytes ? len - first : strip_bytes);
    std::vector<unsigned char> strip(data.begin() + first, data.begin() + first + n);                           // its own allocation: ASan sees its ends
    std::vector<uint32_t> toks;
    int run_start = 0;
    for (int p = 0; p < n; ++p) {
      if (p > 0 && strip[(size_t)p] != strip[(size_t)p - 1]) run_start = p;
      const int tok = sc_token_at<258>(ScSameAsBefore<unsigned char>{strip.data()}, p, n, run_start);
      if (tok != SC_NONE) toks.push_back(tok == SC_LITERAL ? (uint32_t)strip[(size_t)p] : (uint32_t)tok | 0x1000u);
    }
    const uint32_t count = (uint32_t)toks.size();
    std::fwrite(&count, sizeof(uint32_t), 1, out);
    std::fwrite(toks.data(), sizeof(uint32_t), toks.size(), out);
  }
  if (std::fclose(out) != 0) return fail("cannot write the output");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "--png-tokens") return png_tokens(argv[2], argv[3]);
  if (argc != 3) return fail("usage: webp_host_check [--png-tokens] JOB OUT");
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return fail("cannot open the job");
  int32_t head[4];
  if (std::fread(head, sizeof(int32_t), 4, in) != 4) return fail("short job");
  const long n = head[0], H = head[1], W = head[2], strip_rows = head[3];
  if (n < 1 || H < 1 || W < 1 || H > 16384 || W > 16384 || strip_rows < 1 || n * H * W > (1l << 26)) return fail("sizes outside the range");
  std::vector<unsigned char> frames((size_t)(n * H * W * 3));
  if (std::fread(frames.data(), 1, frames.size(), in) != frames.size()) return fail("short job");
  std::fclose(in);

  const long B = 1 << WP_PREDICTOR_BITS, bh = (H + B - 1) / B, bw = (W + B - 1) / B;
  std::vector<unsigned char> modes((size_t)(n * bh * bw));
  std::vector<uint32_t> res((size_t)(n * H * W));
  for (long f = 0; f < n; ++f) {
    const unsigned char* frame = frames.data() + f * H * W * 3;
    for (long by = 0; by < bh; ++by)
      for (long bx = 0; bx < bw; ++bx) {
        unsigned cost[WP_MODES] = {};
        for (long y = by * B; y < H && y < by * B + B; ++y)
          for (long x = bx * B; x < W && x < bx * B + B; ++x) {
            const uint32_t cur = wp_pixel(frame, W, y, x);
            const WpNeighbours nb = wp_neighbours(frame, W, y, x);
            for (int m = 0; m < WP_MODES; ++m) cost[m] += wp_cost(wp_sub(cur, wp_predict_at(m, y, x, nb)));
          }
        int mode = 0;
        for (int m = 1; m < WP_MODES; ++m)
          if (cost[m] < cost[mode]) mode = m;
        modes[(size_t)((f * bh + by) * bw + bx)] = (unsigned char)mode;
        for (long y = by * B; y < H && y < by * B + B; ++y)
          for (long x = bx * B; x < W && x < bx * B + B; ++x)
            res[(size_t)(f * H * W + y * W + x)] = wp_sub(wp_pixel(frame, W, y, x), wp_predict_at(mode, y, x, wp_neighbours(frame, W, y, x)));
      }
  }

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return fail("cannot open the output");
  std::fwrite(modes.data(), 1, modes.size(), out);
  std::fwrite(res.data(), sizeof(uint32_t), res.size(), out);
  const long strip_px = strip_rows * W;
  for (long f = 0; f < n; ++f)
    for (long first = 0; first < H * W; first += strip_px) {
      const int len = (int)(H * W - first < strip_px ? H * W - first : strip_px);
      std::vector<uint32_t> strip(res.begin() + (f * H * W + first), res.begin() + (f * H * W + first + len));   // its own allocation: ASan sees its ends
      std::vector<uint32_t> toks;
      int run_start = 0;
      for (int p = 0; p < len; ++p) {
        if (p > 0 && strip[(size_t)p] != strip[(size_t)p - 1]) run_start = p;
        const int tok = wp_token_at(strip.data(), p, len, run_start);
        if (tok == WP_NONE) continue;
        if (tok == WP_LITERAL) {
          toks.push_back(0u);
          toks.push_back(strip[(size_t)p]);
        } else {
          int sym, ebits, eval;
          wp_prefix(tok, &sym, &ebits, &eval);
          toks.push_back((uint32_t)tok);
          toks.push_back((uint32_t)sym | (uint32_t)ebits << 8 | (uint32_t)eval << 16);
        }
      }
      const uint32_t count = (uint32_t)(toks.size() / 2);
      std::fwrite(&count, sizeof(uint32_t), 1, out);
      std::fwrite(toks.data(), sizeof(uint32_t), toks.size(), out);
    }
  if (std::fclose(out) != 0) return fail("cannot write the output");
  return 0;
}
