// Host program over mmgt_amd/csrc/jpegdec_core.h: the decoder's arithmetic and indexing, exactly as the kernels call it, without a GPU.  Plain C++
// (no HIP); tests/test_jpegdec.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it, so an out-of-range access or
// undefined arithmetic on ANY input ends the program with an error.
//
//   jpegdec_host_check decode JOB OUT    decode the batch of JOB, write (n, H, W, 3) RGB bytes to OUT; exit 3 with the first status if one is set
//   jpegdec_host_check fuzz JOB RUNS SEED    RUNS seeded corruptions of JOB, each decoded to pixels or to a status; prints the tally
//
// JOB (little endian, written by the test from mmgt_amd.video_in.batch_operands): int32 magic 'JDJ1', n, H, W, ncomp, hs, vs, nseg, table_ints, 0;
// int64 data_bytes; int32 tables[n * table_ints]; int32 seginfo[nseg * 3]; int64 offsets[nseg + 1]; data[data_bytes].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegdec_core.h"

namespace {

struct Job {
  int n = 0, nseg = 0;
  JdGeom g{};
  std::vector<int32_t> tables, seginfo;
  std::vector<long long> offsets;
  std::vector<unsigned char> data;
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

bool load(const char* path, Job& j) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[10];
  long long bytes = 0;
  bool ok = read_exact(f, h, sizeof h) && read_exact(f, &bytes, sizeof bytes) && h[0] == 0x314A444A && h[8] == JD_TAB_INTS && h[1] >= 1 &&
            h[1] <= 4096 && h[7] >= 1 && h[7] <= (1 << 22) && bytes >= 0 && bytes <= (1ll << 30) && jd_geom(h[2], h[3], h[4], h[5], h[6], &j.g);
  if (ok) {
    j.n = h[1], j.nseg = h[7];
    j.tables.resize((size_t)j.n * JD_TAB_INTS);
    j.seginfo.resize((size_t)j.nseg * 3);
    j.offsets.resize((size_t)j.nseg + 1);
    j.data.resize((size_t)bytes);
    ok = read_exact(f, j.tables.data(), j.tables.size() * 4) && read_exact(f, j.seginfo.data(), j.seginfo.size() * 4) &&
         read_exact(f, j.offsets.data(), j.offsets.size() * 8) && read_exact(f, j.data.data(), j.data.size());
  }
  fclose(f);
  return ok;
}

// the three launches of csrc/jpegdec.hip as loops; buffers sized exactly as the wrapper sizes them.  Returns the first status (0: rgb is valid).
int decode(const Job& j, std::vector<int16_t>& coef, std::vector<unsigned char>& rgb, long long* bad_segment) {
  const long long blocks = (long long)j.n * jd_frame_blocks(j.g), pixels = (long long)j.n * j.g.H * j.g.W;
  coef.assign((size_t)blocks * 64, 0);
  int first = 0;
  for (long long s = 0; s < j.nseg; ++s) {
    const int st = jd_segment(j.data.data(), (long long)j.data.size(), j.offsets.data(), j.seginfo.data(), j.tables.data(), coef.data(), j.g, j.n, s);
    if (st && !first) first = st, *bad_segment = s;
  }
  if (first) return first;
  std::vector<unsigned char> planes((size_t)blocks * 64);
  for (long long b = 0; b < blocks; ++b) jd_block(coef.data(), j.tables.data(), planes.data(), j.g, b);
  rgb.resize((size_t)pixels * 3);
  for (long long p = 0; p < pixels; ++p) jd_output_pixel(planes.data(), rgb.data(), j.g, p);
  return 0;
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
  std::vector<int16_t> coef;
  std::vector<unsigned char> rgb;
  int pixels = 0, status = 0, tally[8] = {0};
  const long long blocks = (long long)clean.n * jd_frame_blocks(clean.g);
  for (int k = 0; k < runs; ++k) {
    Job j = clean;
    long long bad = 0;
    switch (k % 4) {
      case 0:                                                      // byte flips inside the segment range
        for (int i = 1 + (int)r.below(8); i > 0 && !j.data.empty(); --i) j.data[(size_t)r.below((long long)j.data.size())] ^= (unsigned char)(1 + r.below(255));
        break;
      case 1: {                                                    // a shortened (possibly empty) range
        const long long s = r.below(j.nseg);
        j.offsets[(size_t)s + 1] = j.offsets[(size_t)s] + r.below(j.offsets[(size_t)s + 1] - j.offsets[(size_t)s]);
        break;
      }
      case 2:                                                      // a run of bytes overwritten (0xFF runs and zero runs among them)
        if (!j.data.empty()) {
          const long long at = r.below((long long)j.data.size()), len = 1 + r.below(32);
          const unsigned char v = (k & 4) ? 0xFF : (unsigned char)r.below(256);
          for (long long i = at; i < at + len && i < (long long)j.data.size(); ++i) j.data[(size_t)i] = v;
        }
        break;
      default: {                                                   // coefficients and quantisers at their extremes through the inverse DCT
        coef.assign((size_t)blocks * 64, 0);
        for (auto& c : coef) {
          const uint64_t v = r.next();
          c = (v & 3) == 0 ? 2047 : (v & 3) == 1 ? -2047 : (v & 3) == 2 ? (int16_t)(v >> 8) : (v & 4) ? -32768 : 32767;
        }
        for (int f = 0; f < j.n; ++f)
          for (int i = 0; i < 256; ++i) j.tables[(size_t)f * JD_TAB_INTS + JD_TAB_Q + i] = (r.next() & 1) ? 255 : 1 + (int)r.below(255);
        std::vector<unsigned char> planes((size_t)blocks * 64);
        for (long long b = 0; b < blocks; ++b) jd_block(coef.data(), j.tables.data(), planes.data(), j.g, b);
        rgb.resize((size_t)clean.n * j.g.H * j.g.W * 3);
        for (long long p = 0; p < (long long)clean.n * j.g.H * j.g.W; ++p) jd_output_pixel(planes.data(), rgb.data(), j.g, p);
        ++pixels;
        continue;
      }
    }
    const int st = decode(j, coef, rgb, &bad);
    if (st < 0 || st > 7) return 4;
    ++tally[st];
    st ? ++status : ++pixels;
  }
  printf("fuzz: %d runs, %d ended in pixels, %d in a status (by code:", runs, pixels, status);
  for (int i = 1; i < 8; ++i) printf(" %d", tally[i]);
  printf(")\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  Job j;
  if (argc < 3 || !load(argv[2], j)) {
    fprintf(stderr, "usage: %s decode JOB OUT | fuzz JOB RUNS SEED (JOB unreadable or malformed)\n", argv[0]);
    return 2;
  }
  if (!strcmp(argv[1], "decode") && argc == 4) {
    std::vector<int16_t> coef;
    std::vector<unsigned char> rgb;
    long long bad = 0;
    const int st = decode(j, coef, rgb, &bad);
    if (st) {
      fprintf(stderr, "status %d in segment %lld\n", st, bad);
      return 3;
    }
    FILE* f = fopen(argv[3], "wb");
    if (!f || fwrite(rgb.data(), 1, rgb.size(), f) != rgb.size()) return 2;
    fclose(f);
    return 0;
  }
  if (!strcmp(argv[1], "fuzz") && argc == 5) return fuzz(j, atoi(argv[3]), strtoull(argv[4], nullptr, 10));
  return 2;
}
