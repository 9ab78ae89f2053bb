// The arithmetic of the lossy WebP writer (mmgt_amd/csrc/vp8_core.h, the functions csrc/vp8.hip's kernels call) run on the host, so that it can be
// built with AddressSanitizer and UBSan and held to the yardstick of tests/vp8_ref.py without a GPU (tests/test_vp8.py builds and runs it).
//
//   vp8_host_check encode JOB OUT
//   vp8_host_check worst MBH MBW
//
// encode.  JOB: int32 H, W, q, partitions, filter_level, then H * W * 3 bytes of RGB.  OUT: int32 mbh, mbw, skipped; the reconstructed Y, U, V planes;
// the modes, 2 bytes a macroblock; the non-zero masks, uint32 each; the levels, 400 int16 each; then per partition (the first, then the token
// partitions) an int64 byte count and the bytes.  The loops mirror the kernels': colour conversion per chroma sample, macroblocks along the
// anti-diagonals, one coder per partition into a slot of exactly the derived worst-case size (its own allocation, so ASan sees its ends).
//
// worst.  A frame of MBH x MBW macroblocks whose every level is +-2047 is coded into slots of the derived size; then the same frame into slots that
// are far too small.  Prints "tokens BYTES BOUND", "first BYTES BOUND" and "small T F" (the two returns for the small slots, -1 = refused).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vp8_core.h"

static int fail(const char* what) {
  std::fprintf(stderr, "vp8_host_check: %s\n", what);
  return 2;
}

static int worst(int mbh, int mbw) {
  if (mbh < 1 || mbw < 1 || mbh * mbw > 4096) return fail("sizes outside the range");
  const long mbs = (long)mbh * mbw;
  std::vector<short> levels((size_t)(mbs * V8_MB_LEVELS));
  for (size_t i = 0; i < levels.size(); ++i) levels[i] = (short)(i % 3 ? V8_MAX_LEVEL : -V8_MAX_LEVEL);
  std::vector<unsigned> nz((size_t)mbs, 0x1ffffffu);
  std::vector<unsigned char> modes((size_t)(2 * mbs), 3);
  std::vector<unsigned char> tslot((size_t)v8_token_slot_bytes(mbs)), fslot((size_t)v8_first_slot_bytes(mbs)), probs(1056);
  v8_coef_table(probs.data(), 0, 1);
  const long long tb = v8_code_tokens(levels.data(), nz.data(), probs.data(), mbh, mbw, 0, 1, tslot.data(), (long long)tslot.size());
  const long long fb = v8_code_first(nz.data(), modes.data(), mbh, mbw, 127, 0, 63, 0, fslot.data(), (long long)fslot.size());
  std::printf("tokens %lld %zu\nfirst %lld %zu\n", tb, tslot.size(), fb, fslot.size());
  std::vector<unsigned char> small_t(100), small_f(10);
  const long long st = v8_code_tokens(levels.data(), nz.data(), probs.data(), mbh, mbw, 0, 1, small_t.data(), (long long)small_t.size());
  const long long sf = v8_code_first(nz.data(), modes.data(), mbh, mbw, 127, 0, 63, 0, small_f.data(), (long long)small_f.size());
  std::printf("small %lld %lld\n", st, sf);
  return tb >= 0 && fb >= 0 && st == -1 && sf == -1 ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "worst")) return worst(std::atoi(argv[2]), std::atoi(argv[3]));
  if (argc != 4 || std::strcmp(argv[1], "encode")) return fail("usage: vp8_host_check encode JOB OUT | worst MBH MBW");
  FILE* in = std::fopen(argv[2], "rb");
  if (!in) return fail("cannot open the job");
  int32_t head[5];
  if (std::fread(head, sizeof(int32_t), 5, in) != 5) return fail("short job");
  const int H = head[0], W = head[1], q = head[2], parts = head[3], filter_level = head[4];
  if (H < 1 || W < 1 || H > V8_MAX_SIDE || W > V8_MAX_SIDE || (long)H * W > (1l << 22) || q < 0 || q > 127 || filter_level < 0 || filter_level > 63 ||
      !(parts == 1 || parts == 2 || parts == 4 || parts == 8))
    return fail("arguments outside the range");
  std::vector<unsigned char> frame((size_t)H * W * 3);
  if (std::fread(frame.data(), 1, frame.size(), in) != frame.size()) return fail("short job");
  std::fclose(in);

  const int mbh = (H + 15) / 16, mbw = (W + 15) / 16;
  const long mbs = (long)mbh * mbw, ys = 16l * mbw, cs = 8l * mbw;
  std::vector<unsigned char> Y((size_t)(256 * mbs)), U((size_t)(64 * mbs)), V((size_t)(64 * mbs)), ry(Y.size()), ru(U.size()), rv(V.size());
  for (int cy = 0; cy < 8 * mbh; ++cy)
    for (int cx = 0; cx < 8 * mbw; ++cx) {
      for (int k = 0; k < 4; ++k) {
        const int py = 2 * cy + (k >> 1), px = 2 * cx + (k & 1);
        Y[(size_t)(py * ys + px)] = (unsigned char)v8_luma(frame.data(), H, W, py, px);
      }
      int u, v;
      v8_chroma(frame.data(), H, W, cy, cx, &u, &v);
      U[(size_t)(cy * cs + cx)] = (unsigned char)u, V[(size_t)(cy * cs + cx)] = (unsigned char)v;
    }

  std::vector<short> levels((size_t)(mbs * V8_MB_LEVELS));
  std::vector<unsigned char> modes((size_t)(2 * mbs));
  std::vector<unsigned> nz((size_t)mbs);
  const V8Quant m = v8_quant(q);
  int32_t skipped = 0;
  for (int d = 0; d < mbh + mbw - 1; ++d)
    for (int my = d >= mbw ? d - mbw + 1 : 0; my <= (d < mbh ? d : mbh - 1); ++my) {
      const int mx = d - my;
      const long k = (long)my * mbw + mx;
      nz[(size_t)k] = v8_encode_mb(Y.data(), U.data(), V.data(), ry.data(), ru.data(), rv.data(), ys, cs, my, mx, m, levels.data() + k * V8_MB_LEVELS,
                                   modes.data() + 2 * k);
      skipped += nz[(size_t)k] == 0;
    }

  FILE* out = std::fopen(argv[3], "wb");
  if (!out) return fail("cannot open the output");
  const int32_t dims[3] = {mbh, mbw, skipped};
  std::fwrite(dims, sizeof(int32_t), 3, out);
  std::fwrite(ry.data(), 1, ry.size(), out);
  std::fwrite(ru.data(), 1, ru.size(), out);
  std::fwrite(rv.data(), 1, rv.size(), out);
  std::fwrite(modes.data(), 1, modes.size(), out);
  std::fwrite(nz.data(), sizeof(unsigned), nz.size(), out);
  std::fwrite(levels.data(), sizeof(short), levels.size(), out);
  const int log2_parts = parts == 8 ? 3 : parts == 4 ? 2 : parts == 2 ? 1 : 0;
  std::vector<unsigned char> probs(1056);
  v8_coef_table(probs.data(), 0, 1);
  for (int p = 0; p <= parts; ++p) {
    std::vector<unsigned char> slot((size_t)(p == 0 ? v8_first_slot_bytes(mbs) : v8_token_slot_bytes((long long)((mbh + parts - 1) / parts) * mbw)));
    const long long bytes = p == 0 ? v8_code_first(nz.data(), modes.data(), mbh, mbw, q, log2_parts, filter_level, skipped, slot.data(), (long long)slot.size())
                                   : v8_code_tokens(levels.data(), nz.data(), probs.data(), mbh, mbw, p - 1, parts, slot.data(), (long long)slot.size());
    if (bytes < 0) return fail("a partition did not fit its derived slot");
    const int64_t count = bytes;
    std::fwrite(&count, sizeof(int64_t), 1, out);
    std::fwrite(slot.data(), 1, (size_t)bytes, out);
  }
  if (std::fclose(out) != 0) return fail("cannot write the output");
  return 0;
}
