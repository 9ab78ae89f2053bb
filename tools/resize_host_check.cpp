// Host program over mmgt_amd/csrc/resample_core.h: the resize's arithmetic and indexing, exactly as the kernels of csrc/resize.hip call it, without a
// GPU.  Plain C++ (no HIP); tests/test_resize.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it.  Every buffer is
// a heap block of exactly the size the C ABI asks for, so a tap outside [first, first + count), an item past the end of a row or an output index
// outside the result ends the program with an error report.
//
//   resize_host_check JOB OUT    run the passes of JOB the way mmgt_resize_u8 dispatches them, write the result (uint8 interleaved, or float planar) to OUT
//
// JOB (little endian, written by the test): int32 magic 'RSJ1', n, Hs, Ws, Hd, Wd, C, ksize_x, ksize_y, mode (0: uint8, 1: float through the lookup
// table); then, only for an axis that changes, int32 bounds[D * 2] and int32 kk[D * ksize] (x first, then y); for mode 1 float lut[C * 256]; then the
// n * Hs * Ws * C input bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "resample_core.h"

namespace {

template <typename T>
struct Block {                       // exactly `count` elements on the heap (no vector capacity slack)
  T* p = nullptr;
  size_t count = 0;
  bool alloc(size_t n) {
    count = n;
    p = static_cast<T*>(malloc(n * sizeof(T) ? n * sizeof(T) : 1));
    return p != nullptr;
  }
  bool read(FILE* f, size_t n) { return alloc(n) && (n == 0 || fread(p, sizeof(T), n, f) == n); }
  ~Block() { free(p); }
};

int fail(const char* what) {
  fprintf(stderr, "resize_host_check: %s\n", what);
  return 2;
}

template <int V>
void run_vertical(const uint8_t* src, const RsOut& o, int n, int Hs, int Hd, int W, int C, const int* bounds, const int* kk, int ksize) {
  const long items = (long)n * Hd * ((long)W * C / V);
  for (long i = 0; i < items; ++i) rs_v_item<V>(src, o, n, Hs, Hd, W, C, bounds, kk, ksize, i);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: resize_host_check JOB OUT");
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fail("cannot open the job");
  int32_t h[10];
  if (fread(h, sizeof h, 1, f) != 1 || h[0] != 0x314A5352) return fail("not a job file");
  const int n = h[1], Hs = h[2], Ws = h[3], Hd = h[4], Wd = h[5], C = h[6], ksx = h[7], ksy = h[8], mode = h[9];
  if (!rs_shape_ok(n, Hs, Ws, Hd, Wd, C) || n > 64 || (mode != 0 && mode != 1)) return fail("bad shape");
  const bool horiz = Ws != Wd, vert = Hs != Hd;
  if ((horiz && ksx < 1) || (vert && ksy < 1)) return fail("bad ksize");
  Block<int32_t> bx, kx, by, ky;
  Block<float> lut;
  Block<uint8_t> in, tmp, out8, alt8;
  Block<float> outf, altf;
  bool ok = true;
  if (horiz) ok = ok && bx.read(f, (size_t)Wd * 2) && kx.read(f, (size_t)Wd * ksx);
  if (vert) ok = ok && by.read(f, (size_t)Hd * 2) && ky.read(f, (size_t)Hd * ksy);
  if (mode == 1) ok = ok && lut.read(f, (size_t)C * 256);
  ok = ok && in.read(f, (size_t)n * Hs * Ws * C);
  if (!ok || fgetc(f) != EOF) return fail("the job's size does not match its header");
  fclose(f);
  const size_t total = (size_t)n * Hd * Wd * C;
  if (!tmp.alloc((size_t)rs_workspace_bytes(n, Hs, Ws, Hd, Wd, C))) return fail("out of memory");
  if (!(mode ? outf.alloc(total) && altf.alloc(total) : out8.alloc(total) && alt8.alloc(total))) return fail("out of memory");
  const RsOut last{mode ? nullptr : out8.p, mode ? outf.p : nullptr, mode ? lut.p : nullptr};
  const RsOut alt{mode ? nullptr : alt8.p, mode ? altf.p : nullptr, mode ? lut.p : nullptr};

  const uint8_t* src = in.p;
  if (horiz) {
    const RsOut o = vert ? RsOut{tmp.p, nullptr, nullptr} : last;
    const long items = (long)n * Hs * Wd;
    for (long i = 0; i < items; ++i) {
      if (C == 1)
        rs_h_item<1>(src, o, n, Hs, Ws, Wd, bx.p, kx.p, ksx, i);
      else
        rs_h_item<3>(src, o, n, Hs, Ws, Wd, bx.p, kx.p, ksx, i);
    }
    src = tmp.p;
  }
  if (vert) {
    run_vertical<1>(src, last, n, Hs, Hd, Wd, C, by.p, ky.p, ksy);
    if ((long)Wd * C % 4 == 0) {                                    // malloc's blocks are aligned: the 4-byte items are eligible, and must agree
      run_vertical<4>(src, alt, n, Hs, Hd, Wd, C, by.p, ky.p, ksy);
      if (memcmp(mode ? (const void*)outf.p : (const void*)out8.p, mode ? (const void*)altf.p : (const void*)alt8.p, total * (mode ? 4 : 1)))
        return fail("the 4-byte and the 1-byte vertical items disagree");
    }
  }
  if (!horiz && !vert)
    for (long i = 0; i < (long)total; ++i) rs_copy_item(in.p, last, n, Hs, Ws, C, i);

  FILE* g = fopen(argv[2], "wb");
  if (!g) return fail("cannot open the output");
  const size_t wrote = mode ? fwrite(outf.p, 4, total, g) : fwrite(out8.p, 1, total, g);
  fclose(g);
  return wrote == total ? 0 : fail("short write");
}
