// Host program over mmgt_amd/csrc/gifdec_core.h: the GIF decoder's un-LZW, de-interlace and composition exactly as the kernels call them, without a
// GPU.  Plain C++ (no HIP): the header's per-lane bodies run as loops over lanes 0 .. 63 between the points where the kernels have barriers.
// tests/test_gifdec.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it, so an out-of-range access or undefined
// arithmetic on ANY input ends the program with an error.
//
//   gifdec_host_check decode JOB OUT [CHUNK]   decode the frames of JOB, CHUNK at a time with the carry planes in between (default: all at once), write
//                                              (n, H, W, 3) RGB bytes to OUT; exit 3 with the first status if there is one (nothing is written then)
//   gifdec_host_check fuzz JOB RUNS SEED       RUNS seeded corruptions of JOB's code streams, each decoded to pixels or to a status; prints the tally
//
// JOB (little endian, written by the test from mmgt_amd.video_in.gif_operands): int32 magic 'GDJ1', n, H, W; int64 data_bytes (a multiple of 16),
// idx_bytes; int64 tab[n * 16]; uint8 palette[n * 768]; data[data_bytes].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "gifdec_core.h"

namespace {

struct Exact {                                                     // exactly `bytes` bytes: one byte further is an ASan error
  unsigned char* p = nullptr;
  size_t bytes = 0;
  void reset(size_t n, int fill) {
    free(p);
    bytes = n;
    p = static_cast<unsigned char*>(malloc(n ? n : 1));
    if (!p) abort();
    memset(p, fill, n);
  }
  ~Exact() { free(p); }
};

struct Job {
  int n = 0, H = 0, W = 0;
  long long idx_bytes = 0;
  std::vector<long long> tab;
  std::vector<unsigned char> palette, data;
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

bool load(const char* path, Job& j) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[4];
  long long sizes[2] = {0, 0};
  bool ok = read_exact(f, h, sizeof h) && read_exact(f, sizes, sizeof sizes) && h[0] == 0x314A4447 && h[1] >= 1 && h[1] <= 4096 && h[2] >= 1 &&
            h[2] <= GD_MAX_SIDE && h[3] >= 1 && h[3] <= GD_MAX_SIDE && sizes[0] >= 16 && sizes[0] % 16 == 0 && sizes[0] <= (1ll << 28) && sizes[1] >= 1 &&
            sizes[1] <= (1ll << 28) && (long long)h[1] * h[2] * h[3] <= (1ll << 27);
  if (ok) {
    j.n = h[1], j.H = h[2], j.W = h[3], j.idx_bytes = sizes[1];
    j.tab.resize((size_t)j.n * GD_TAB);
    j.palette.resize((size_t)j.n * 768);
    j.data.resize((size_t)sizes[0]);
    ok = read_exact(f, j.tab.data(), j.tab.size() * 8) && read_exact(f, j.palette.data(), j.palette.size()) && read_exact(f, j.data.data(), j.data.size());
  }
  fclose(f);
  return ok;
}

struct Result {
  int status = 0, frame = 0;
};

// The two launches of csrc/gifdec.hip as loops, buffers sized exactly as the wrapper sizes them.  status 0: rgb is valid.
Result decode(const Job& j, int chunk, std::vector<unsigned char>& rgb) {
  Result r;
  Exact data, idx, carry, out;
  data.reset(j.data.size(), 0);
  memcpy(data.p, j.data.data(), j.data.size());
  idx.reset((size_t)j.idx_bytes, 0xA5);
  auto sh = std::make_unique<GdShared>();
  for (int f = 0; f < j.n; ++f) {
    const long long* t = j.tab.data() + (size_t)f * GD_TAB;
    int st = GD_ST_DESCRIPTOR;
    if (gd_row_ok(t, (long long)data.bytes, j.idx_bytes, GD_MAX_SIDE, GD_MAX_SIDE)) {
      long long rounds = 0;
      st = gd_unlzw_stream(sh.get(), data.p, t[GD_BEGIN], t[GD_END], (int)t[GD_MCS], idx.p + t[GD_IDX], t[GD_W] * t[GD_H], &rounds);
      if (rounds > 8 * (t[GD_END] - t[GD_BEGIN]) / 3 + 2) {         // at least one code (three bits or more) per round: the bound the kernel's loop is held to
        fprintf(stderr, "frame %d: %lld rounds for %lld bytes\n", f, rounds, t[GD_END] - t[GD_BEGIN]);
        abort();
      }
    }
    if (st < 0 || st > GD_ST_LAST) abort();
    if (st && !r.status) r.status = st, r.frame = f;
  }
  if (r.status) return r;
  const long long plane = (long long)j.H * j.W;
  carry.reset((size_t)(2 * 3 * plane), 0xA5);
  out.reset((size_t)(3 * plane * j.n), 0xA5);
  for (int f0 = 0; f0 < j.n; f0 += chunk) {
    const int m = j.n - f0 < chunk ? j.n - f0 : chunk;
    for (long long p = 0; p < plane; ++p)
      gd_compose_pixel(j.tab.data() + (size_t)f0 * GD_TAB, m, idx.p, j.idx_bytes, j.palette.data() + (size_t)f0 * 768, carry.p,
                       out.p + 3 * plane * f0, j.H, j.W, p);
  }
  rgb.assign(out.p, out.p + out.bytes);
  return r;
}

struct Rng {                                                       // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  long long below(long long n) { return n > 0 ? (long long)(next() % (uint64_t)n) : 0; }
};

int fuzz(const Job& clean, int runs, uint64_t seed) {
  Rng r{seed};
  std::vector<unsigned char> rgb;
  int pixels = 0, status = 0, tally[GD_ST_LAST + 1] = {0};
  for (int k = 0; k < runs; ++k) {
    Job j = clean;
    long long* t = j.tab.data() + (size_t)r.below(j.n) * GD_TAB;
    const long long a = t[GD_BEGIN], b = t[GD_END];
    switch (k % 5) {
      case 0:                                                      // byte flips anywhere in the frame's codes
        for (int i = 1 + (int)r.below(8); i > 0 && b > a; --i) j.data[(size_t)(a + r.below(b - a))] ^= (unsigned char)(1 + r.below(255));
        break;
      case 1:                                                      // a shortened (possibly empty) range
        t[GD_END] = a + r.below(b - a);
        break;
      case 2:                                                      // a run of bytes overwritten (0xFF runs and zero runs among them)
        if (b > a) {
          const long long at = a + r.below(b - a), len = 1 + r.below(32);
          const unsigned char v = (k & 8) ? 0xFF : (k & 16) ? 0x00 : (unsigned char)r.below(256);
          for (long long i = at; i < at + len && i < b; ++i) j.data[(size_t)i] = v;
        }
        break;
      case 3:                                                      // another code size, or a falsified row
        if (k & 4) t[GD_MCS] = 2 + r.below(7);
        else t[r.below(GD_MCS + 1)] += r.below(3) - 1 + (r.below(8) ? 0 : (long long)(r.next() >> (8 + r.below(48))));
        break;
      default:                                                     // a single bit
        if (b > a) j.data[(size_t)(a + r.below(b - a))] ^= (unsigned char)(1u << r.below(8));
        break;
    }
    const Result res = decode(j, 1 + (int)r.below(j.n), rgb);
    if (res.status) ++tally[res.status], ++status;
    else ++pixels;
  }
  printf("fuzz: %d runs, %d ended in pixels, %d in a status (by code:", runs, pixels, status);
  for (int i = 1; i <= GD_ST_LAST; ++i) printf(" %d", tally[i]);
  printf(")\n");
  return 0;
}

bool write_file(const char* path, const std::vector<unsigned char>& v) {
  FILE* f = fopen(path, "wb");
  const bool ok = f && fwrite(v.data(), 1, v.size(), f) == v.size();
  if (f) fclose(f);
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  Job j;
  if (argc < 3 || !load(argv[2], j)) {
    fprintf(stderr, "usage: %s decode JOB OUT [CHUNK] | fuzz JOB RUNS SEED (JOB unreadable or malformed)\n", argv[0]);
    return 2;
  }
  if (!strcmp(argv[1], "decode") && (argc == 4 || argc == 5)) {
    const int chunk = argc == 5 ? atoi(argv[4]) : j.n;
    if (chunk < 1) return 2;
    std::vector<unsigned char> rgb;
    const Result r = decode(j, chunk, rgb);
    if (r.status) {
      fprintf(stderr, "status %d in frame %d\n", r.status, r.frame);
      return 3;
    }
    return write_file(argv[3], rgb) ? 0 : 2;
  }
  if (!strcmp(argv[1], "fuzz") && argc == 5) return fuzz(j, atoi(argv[3]), strtoull(argv[4], nullptr, 10));
  return 2;
}
