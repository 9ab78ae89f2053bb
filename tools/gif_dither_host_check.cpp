// Host program over mmgt_amd/csrc/gif_dither_core.h: the Floyd-Steinberg index map of the device GIF writer, computed twice without a GPU.
//   serial    the rule as the header states it: raster order, one pixel after the other, a full plane of errors;
//   schedule  gif_dither_kernel of csrc/gif.hip as loops: bands of GDI_BAND rows, lane r at x = t - 2 r in step t, the move from the lane above
//             taken from a snapshot of the step before, the carry row between bands, pixels fetched a group ahead through gdi_fetch16 / gdi_align12.
// Both go through gdi_step; the program exits 1 at the first index that differs.  Plain C++ (no HIP).  tests/test_gif_dither.py builds it with
// -fsanitize=address,undefined -fno-sanitize-recover=all, and every buffer has exactly the size the kernel's caller gives it, so a fetch or a store
// outside one ends the program with an error.
//
//   gif_dither_host_check [H W]...      the sizes to run (default: the list of tests/test_gif_dither_gpu.py); per size three frames in one call
//                                       (noise, a colour ramp, a frame of 0 and 255 only), against a colour-cube palette and a two-entry palette
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gif_dither_core.h"

namespace {

struct Exact {                                                     // exactly `bytes` bytes: one byte further is an ASan error
  unsigned char* p = nullptr;
  size_t bytes = 0;
  Exact(size_t n, int fill) : bytes(n) {
    p = static_cast<unsigned char*>(malloc(n ? n : 1));            // 16-byte aligned, and ASan's red zone starts at byte n
    if (!p) abort();
    memset(p, fill, n);
  }
  ~Exact() { free(p); }
  Exact(const Exact&) = delete;
  Exact& operator=(const Exact&) = delete;
};

struct Rng {                                                       // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

struct Tables {
  std::vector<unsigned char> lut;                                  // 32768
  unsigned char palette[768];
  unsigned pal[256];
};

// lut = the entry among the first `used` nearest to each bin centre, the lowest index on a tie (video_out.gif_lut)
void finish(Tables& t, int used) {
  t.lut.resize(32768);
  for (int i = 0; i < 256; ++i) t.pal[i] = t.palette[3 * i] | (unsigned)t.palette[3 * i + 1] << 8 | (unsigned)t.palette[3 * i + 2] << 16;
  for (int bin = 0; bin < 32768; ++bin) {
    const int c[3] = {8 * (bin >> 10) + 4, 8 * ((bin >> 5) & 31) + 4, 8 * (bin & 31) + 4};
    long best = -1;
    int at = 0;
    for (int k = 0; k < used; ++k) {
      long d = 0;
      for (int ch = 0; ch < 3; ++ch) d += (long)(c[ch] - t.palette[3 * k + ch]) * (c[ch] - t.palette[3 * k + ch]);
      if (best < 0 || d < best) best = d, at = k;
    }
    t.lut[bin] = (unsigned char)at;
  }
}

void cube_tables(Tables& t) {                                      // 6 x 7 x 6 = 252 colours
  memset(t.palette, 0, sizeof t.palette);
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int g = 0; g < 7; ++g)
      for (int b = 0; b < 6; ++b, ++k) t.palette[3 * k] = (unsigned char)(r * 51), t.palette[3 * k + 1] = (unsigned char)(g * 255 / 6), t.palette[3 * k + 2] = (unsigned char)(b * 51);
  finish(t, k);
}

void two_tables(Tables& t) {                                       // black and white: both clamps fire on a frame of 0 and 255
  memset(t.palette, 0, sizeof t.palette);
  t.palette[3] = t.palette[4] = t.palette[5] = 255;
  finish(t, 2);
}

void serial(const unsigned char* frames, const Tables& t, unsigned char* idx, int n, int H, int W) {
  std::vector<unsigned> d((size_t)(H + 1) * (W + 2));              // a border of "no error" left, right and above
  for (int f = 0; f < n; ++f) {
    for (auto& v : d) v = GDI_ZERO;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const unsigned char* p = frames + (((size_t)f * H + y) * W + x) * 3;
        unsigned* here = d.data() + (size_t)(y + 1) * (W + 2) + x + 1;
        const unsigned* above = here - (W + 2);
        idx[((size_t)f * H + y) * W + x] = (unsigned char)gdi_step(p[0], p[1], p[2], here[-1], above[-1], above[0], above[1], t.lut.data(), t.pal, here);
      }
  }
}

// csrc/gif.hip's gif_dither_kernel, one frame: every per-lane variable is an array over the lanes, a step is a loop over them
void schedule_frame(const unsigned char* frames, const Tables& t, unsigned char* idx, unsigned* carry, long long frame, int H, int W, long long total) {
  unsigned* cr = carry ? carry + frame * W : nullptr;
  for (int row0 = 0; row0 < H; row0 += GDI_BAND) {
    const int rows = H - row0 < GDI_BAND ? H - row0 : GDI_BAND;
    const bool first = row0 == 0, more = row0 + GDI_BAND < H;
    const long steps = gdi_band_steps(W, rows);
    GdiLane s[GDI_BAND];
    unsigned cur[GDI_BAND][3], raw[GDI_BAND][4], ccur[GDI_GROUP], cnxt[GDI_GROUP], out_before[GDI_BAND];
    long long rowpix[GDI_BAND];
    int shift[GDI_BAND];
    for (int lane = 0; lane < GDI_BAND; ++lane) {
      const bool has_row = lane < rows, reads_carry = lane == 0 && !first;
      rowpix[lane] = (frame * H + row0 + lane) * W;
      gdi_lane_reset(&s[lane], reads_carry ? cr[0] : GDI_ZERO);
      for (int k = 0; k < 4; ++k) raw[lane][k] = 0u;
      shift[lane] = gdi_shift(3 * (rowpix[lane] - 2 * lane));
      if (has_row && lane < 2) gdi_fetch16(frames, 3 * (rowpix[lane] - 2 * lane), total, raw[lane]);
      gdi_align12(raw[lane], shift[lane], cur[lane]);
    }
    for (int k = 0; k < GDI_GROUP; ++k) ccur[k] = cnxt[k] = GDI_ZERO;
    if (!first)
      for (int k = 0; k < GDI_GROUP; ++k)
        if (k + 1 < W) ccur[k] = cr[k + 1];
    unsigned done_idx[GDI_BAND], done_err[GDI_BAND][GDI_GROUP];      // a group's results are stored when the next group begins
    auto store_group = [&](long t) {
      for (int lane = 0; lane < GDI_BAND; ++lane)
        for (int k = 0; k < GDI_GROUP; ++k) {
          const int x = gdi_x(t + k, lane);
          if (lane < rows && x >= 0 && x < W) {
            idx[rowpix[lane] + x] = (unsigned char)(done_idx[lane] >> (8 * k));
            if (more && lane == GDI_BAND - 1) cr[x] = done_err[lane][k];
          }
        }
    };
    for (long t0 = 0; t0 < steps; t0 += GDI_GROUP) {
      if (t0 > 0) store_group(t0 - GDI_GROUP);
      for (int lane = 0; lane < GDI_BAND; ++lane) {
        done_idx[lane] = 0u;
        const long x1 = gdi_x(t0 + GDI_GROUP, lane);
        if (lane < rows && x1 + GDI_GROUP > 0 && x1 < W) gdi_fetch16(frames, 3 * (rowpix[lane] + x1), total, raw[lane]);
      }
      if (!first)
        for (int k = 0; k < GDI_GROUP; ++k) cnxt[k] = t0 + GDI_GROUP + k + 1 < W ? cr[t0 + GDI_GROUP + k + 1] : GDI_ZERO;
      for (int k = 0; k < GDI_GROUP; ++k) {
        for (int lane = 0; lane < GDI_BAND; ++lane) out_before[lane] = s[lane].out;           // the DPP move reads what the step before left
        for (int lane = 0; lane < GDI_BAND; ++lane) {
          const int x = gdi_x(t0 + k, lane);
          const bool active = lane < rows && x >= 0 && x < W;
          const unsigned in = lane == 0 ? ccur[k] : out_before[lane - 1];
          unsigned r, g, b;
          gdi_pixel(cur[lane], k, &r, &g, &b);
          const int i = gdi_lane_step(&s[lane], in, active, r, g, b, t.lut.data(), t.pal);
          done_idx[lane] |= (unsigned)(i & 255) << (8 * k);
          done_err[lane][k] = s[lane].out;
        }
      }
      for (int lane = 0; lane < GDI_BAND; ++lane) gdi_align12(raw[lane], shift[lane], cur[lane]);
      for (int k = 0; k < GDI_GROUP; ++k) ccur[k] = cnxt[k];
    }
    store_group((steps - 1) / GDI_GROUP * GDI_GROUP);
  }
}

void fill_frames(unsigned char* f, int H, int W, uint64_t seed) {
  Rng r{seed};
  const size_t plane = (size_t)H * W * 3;
  for (size_t i = 0; i < plane; ++i) f[i] = (unsigned char)(r.next() >> 56);                 // noise
  for (int y = 0; y < H; ++y)                                                                 // the ramp of the tests, cropped
    for (int x = 0; x < W; ++x) {
      unsigned char* p = f + plane + ((size_t)y * W + x) * 3;
      p[0] = (unsigned char)((x % 128) * 255 / 127), p[1] = (unsigned char)((y % 96) * 255 / 95), p[2] = (unsigned char)(((x % 128) + (y % 96)) * 255 / 222);
    }
  for (size_t i = 0; i < plane; ++i) f[2 * plane + i] = (r.next() >> 63) ? 255 : 0;           // 0 and 255 only
}

bool run(int H, int W) {
  const int n = 3;
  const size_t npix = (size_t)n * H * W;
  Exact frames(3 * npix, 0);
  fill_frames(frames.p, H, W, 20261020u + 65537u * (unsigned)H + (unsigned)W);
  Tables tabs[2];
  cube_tables(tabs[0]);
  two_tables(tabs[1]);
  for (int k = 0; k < 2; ++k) {
    Exact want(npix, 0xA5), got(npix, 0x5A), carry(H > GDI_BAND ? 4 * (size_t)n * W : 0, 0xC3);
    serial(frames.p, tabs[k], want.p, n, H, W);
    for (int f = 0; f < n; ++f)
      schedule_frame(frames.p, tabs[k], got.p, H > GDI_BAND ? reinterpret_cast<unsigned*>(carry.p) : nullptr, f, H, W, (long long)(3 * npix));
    for (size_t i = 0; i < npix; ++i)
      if (want.p[i] != got.p[i]) {
        fprintf(stderr, "%d x %d, palette %d: pixel %zu (frame %zu, y %zu, x %zu) is %d by the schedule, %d by the rule\n", H, W, k, i, i / ((size_t)H * W),
                i / W % H, i % W, got.p[i], want.p[i]);
        return false;
      }
  }
  printf("%d x %d: schedule == rule\n", H, W);
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<int> sizes = {1, 1, 1, 7, 7, 1, 2, 3, 35, 67, 96, 128, 600, 5, GDI_BAND + 1, 9};
  if (argc > 1) {
    if (argc % 2 != 1) {
      fprintf(stderr, "usage: %s [H W]...\n", argv[0]);
      return 2;
    }
    sizes.clear();
    for (int i = 1; i < argc; ++i) {
      const int v = atoi(argv[i]);
      if (v < 1 || v > 65535) return 2;
      sizes.push_back(v);
    }
  }
  for (size_t i = 0; i < sizes.size(); i += 2)
    if (!run(sizes[i], sizes[i + 1])) return 1;
  return 0;
}
