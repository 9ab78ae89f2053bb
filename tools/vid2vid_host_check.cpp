// The integer rules of re-voicing a clip (mmgt_amd/csrc/vid2vid_core.h) in a host program: the functions the kernels of csrc/vid2vid.hip
// call, driven by the kernels' own index arithmetic, on buffers of exactly the operands' sizes.  tests/test_vid2vid.py builds it with
// -fsanitize=address,undefined and compares what it writes with tests/vid2vid_ref.py byte for byte.
//
//   vid2vid_host_check mask L H W grow in.u8 out.f32        pixel mask -> latent cell mask
//   vid2vid_host_check feather L h w r in.f32 out.u8        cell mask -> paste-back alpha
//   vid2vid_host_check composite npix gen.u8 orig.u8 alpha.u8 out.u8
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "vid2vid_core.h"

namespace {

template <class T>
std::unique_ptr<T[]> read_exact(const char* path, size_t count) {
  std::unique_ptr<T[]> buf(new T[count]);
  FILE* f = fopen(path, "rb");
  if (!f || fread(buf.get(), sizeof(T), count, f) != count || fgetc(f) != EOF) {
    fprintf(stderr, "%s: expected exactly %zu elements of %zu bytes\n", path, count, sizeof(T));
    exit(2);
  }
  fclose(f);
  return buf;
}

template <class T>
void write_all(const char* path, const T* data, size_t count) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(data, sizeof(T), count, f) != count || fclose(f) != 0) {
    fprintf(stderr, "%s: write failed\n", path);
    exit(2);
  }
}

int usage() {
  fprintf(stderr, "usage: vid2vid_host_check mask L H W grow in out | feather L h w r in out | composite npix gen orig alpha out\n");
  return 64;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return usage();
  const std::string mode = argv[1];
  if (mode == "mask" && argc == 8) {
    const int L = atoi(argv[2]), H = atoi(argv[3]), W = atoi(argv[4]), grow = atoi(argv[5]);
    if (L < 1 || H < 8 || W < 8 || H % V2V_CELL || W % V2V_CELL || grow < 0 || grow > V2V_GROW_MAX) return usage();
    const int h = H / V2V_CELL, w = W / V2V_CELL;
    auto px = read_exact<uint8_t>(argv[6], (size_t)L * H * W);
    std::unique_ptr<float[]> cells(new float[(size_t)L * h * w]);
    const long n = (long)L * h * w, frame_px = (long)H * W;
    for (long i = 0; i < n; ++i) {                              // mask_to_latent_kernel's thread i
      const int cx = (int)(i % w), cy = (int)((i / w) % h);
      const long l = i / ((long)h * w);
      cells[i] = v2v_cell_mask(px.get() + l * frame_px, h, w, cy, cx, grow) ? 1.f : 0.f;
    }
    write_all(argv[7], cells.get(), (size_t)n);
    return 0;
  }
  if (mode == "feather" && argc == 8) {
    const int L = atoi(argv[2]), h = atoi(argv[3]), w = atoi(argv[4]), r = atoi(argv[5]);
    if (L < 1 || h < 1 || w < 1 || r < 0 || r > V2V_FEATHER_MAX) return usage();
    auto cells = read_exact<float>(argv[6], (size_t)L * h * w);
    const int W4 = w * V2V_CELL / 4, H = h * V2V_CELL;
    const long n = (long)L * H * W4;
    std::unique_ptr<uint8_t[]> alpha(new uint8_t[(size_t)n * 4]);
    for (long i = 0; i < n; ++i) {                              // feather_alpha_kernel's thread i: four pixels, one word
      const int x = (int)(i % W4) * 4, y = (int)((i / W4) % H);
      const float* fr = cells.get() + (i / ((long)W4 * H)) * h * w;
      for (int k = 0; k < 4; ++k) alpha[4 * i + k] = v2v_feather_pixel(fr, h, w, y, x + k, r);
    }
    write_all(argv[7], alpha.get(), (size_t)n * 4);
    return 0;
  }
  if (mode == "composite" && argc == 7) {
    const long npix = atol(argv[2]);
    if (npix < 1) return usage();
    auto gen = read_exact<uint8_t>(argv[3], (size_t)npix * 3);
    auto orig = read_exact<uint8_t>(argv[4], (size_t)npix * 3);
    auto alpha = read_exact<uint8_t>(argv[5], (size_t)npix);
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)npix * 3]);
    for (long p = 0; p < npix; ++p)
      for (int c = 0; c < 3; ++c) out[3 * p + c] = (uint8_t)v2v_blend(gen[3 * p + c], orig[3 * p + c], alpha[p]);
    write_all(argv[6], out.get(), (size_t)npix * 3);
    return 0;
  }
  return usage();
}
