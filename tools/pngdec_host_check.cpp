// Host program over mmgt_amd/csrc/pngdec_core.h: the PNG decoder's inflate, scanline reconstruction and expansion exactly as the kernels call them,
// without a GPU.  Plain C++ (no HIP): the header's per-lane bodies run as loops over lanes 0 .. 63 between the points where the kernels have
// barriers.  tests/test_pngdec.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it, so an out-of-range access or
// undefined arithmetic on ANY input ends the program with an error.
//
//   pngdec_host_check decode JOB OUT        decode the batch of JOB, write (n, H, W, 3) RGB bytes to OUT; exit 3 with the first status or Adler-32
//                                           mismatch if there is one (nothing is written then)
//   pngdec_host_check filtered JOB OUT      the same, but OUT receives the inflated, still filtered bytes (n, H, stride)
//   pngdec_host_check fuzz JOB RUNS SEED    RUNS seeded corruptions of JOB, each decoded to pixels or to a status within the step bound; prints the tally
//
// JOB (little endian, written by the test from mmgt_amd.video_in.png_batch_operands): int32 magic 'PDJ1', n, H, W, colour type, depth, 0, 0; int64
// data_bytes (a multiple of 16); int64 offsets[n + 1]; uint32 adler[n]; int32 plte_len[n]; uint8 palette[n * 768]; data[data_bytes].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pngdec_core.h"

namespace {

struct Aligned {                                                   // exactly `bytes` bytes at a 16-byte boundary: one byte further is an ASan error
  unsigned char* p = nullptr;
  size_t bytes = 0;
  void reset(size_t n) {
    free(p);
    p = nullptr, bytes = n;
    if (posix_memalign(reinterpret_cast<void**>(&p), 16, n ? n : 1) != 0) abort();
  }
  ~Aligned() { free(p); }
};

struct Job {
  int n = 0;
  PdGeom g{};
  std::vector<long long> offsets;
  std::vector<uint32_t> adler;
  std::vector<int32_t> plte_len;
  std::vector<unsigned char> palette, data;
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

bool load(const char* path, Job& j) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[8];
  long long bytes = 0;
  bool ok = read_exact(f, h, sizeof h) && read_exact(f, &bytes, sizeof bytes) && h[0] == 0x314A4450 && h[1] >= 1 && h[1] <= 4096 && bytes >= 16 &&
            bytes % 16 == 0 && bytes <= (1ll << 28) && pd_geom(h[2], h[3], h[4], h[5], &j.g) && (long long)h[1] * pd_frame_bytes(j.g) <= (1ll << 28);
  if (ok) {
    j.n = h[1];
    j.offsets.resize((size_t)j.n + 1);
    j.adler.resize((size_t)j.n);
    j.plte_len.resize((size_t)j.n);
    j.palette.resize((size_t)j.n * 768);
    j.data.resize((size_t)bytes);
    ok = read_exact(f, j.offsets.data(), j.offsets.size() * 8) && read_exact(f, j.adler.data(), j.adler.size() * 4) &&
         read_exact(f, j.plte_len.data(), j.plte_len.size() * 4) && read_exact(f, j.palette.data(), j.palette.size()) &&
         read_exact(f, j.data.data(), j.data.size());
  }
  fclose(f);
  return ok;
}

uint32_t adler_combine(uint32_t a1, uint32_t a2, long long len2) {  // zlib's adler32_combine
  const uint32_t M = 65521u;
  const uint64_t rem = (uint64_t)(len2 % M);
  uint64_t s1 = a1 & 0xffffu, s2 = (rem * s1) % M;
  s1 += (a2 & 0xffffu) + M - 1;
  s2 += ((a1 >> 16) & 0xffffu) + ((a2 >> 16) & 0xffffu) + M - rem;
  if (s1 >= M) s1 -= M;
  if (s1 >= M) s1 -= M;
  if (s2 >= (uint64_t)M << 1) s2 -= (uint64_t)M << 1;
  if (s2 >= M) s2 -= M;
  return (uint32_t)(s1 | s2 << 16);
}

struct Result {
  int status = 0, frame = 0;
  const char* stage = "";
  long long steps = 0;
};

// The three launches of csrc/pngdec.hip as loops, buffers sized exactly as the wrapper sizes them.  status 0: rgb is valid.  -1: an Adler-32 mismatch.
Result decode(const Job& j, Aligned& filt, std::vector<unsigned char>& rgb, bool keep_filtered, std::vector<unsigned char>* filtered) {
  Result r;
  const long long fb = pd_frame_bytes(j.g);
  Aligned data;
  data.reset(j.data.size());
  memcpy(data.p, j.data.data(), j.data.size());
  filt.reset((size_t)j.n * fb);
  memset(filt.p, 0xA5, filt.bytes);
  auto sh = std::make_unique<PdShared>();
  for (int f = 0; f < j.n; ++f) {
    long long steps = 0;
    const long long at = (long long)f * fb, len = j.offsets[(size_t)f + 1] - j.offsets[(size_t)f];
    const int st = pd_inflate_stream(sh.get(), data.p, (long long)data.bytes, j.offsets[(size_t)f], j.offsets[(size_t)f + 1], filt.p + at, (int)fb,
                                     (int)(at & 15), &steps);
    r.steps += steps;
    if (steps > 8 * (len > 0 ? len : 0) + 1024) {                  // at least one bit per iteration: the bound the kernel's loop is held to
      fprintf(stderr, "frame %d: %lld loop iterations for %lld bytes\n", f, steps, len);
      abort();
    }
    if (st < 0 || st > PD_ST_LAST) abort();
    if (st && !r.status) r.status = st, r.frame = f, r.stage = "inflate";
  }
  if (r.status) return r;
  if (keep_filtered) {
    filtered->assign(filt.p, filt.p + filt.bytes);
    return r;
  }
  std::vector<long long> sums((size_t)j.n * j.g.H * 2);
  for (int f = 0; f < j.n; ++f) {
    const int st = pd_unfilter_frame(filt.p + (size_t)f * fb, sums.data() + (size_t)f * 2 * j.g.H, j.g);
    if (st && !r.status) r.status = st, r.frame = f, r.stage = "unfilter";
  }
  if (r.status) return r;
  for (int f = 0; f < j.n; ++f) {
    uint32_t a = 1;
    for (int y = 0; y < j.g.H; ++y) {
      const long long s1 = sums[((size_t)f * j.g.H + y) * 2], s2 = sums[((size_t)f * j.g.H + y) * 2 + 1];
      a = adler_combine(a, (uint32_t)((j.g.stride + s2) % 65521) << 16 | (uint32_t)((1 + s1) % 65521), j.g.stride);
    }
    if (a != j.adler[(size_t)f]) {
      r.status = -1, r.frame = f, r.stage = "adler";
      return r;
    }
  }
  const long long pixels = (long long)j.n * j.g.H * j.g.W;
  rgb.assign((size_t)pixels * 3, 0xA5);
  for (long long p = 0; p < pixels; ++p) {
    const int st = pd_expand_pixel(filt.p, j.palette.data(), j.plte_len.data(), rgb.data(), j.g, p);
    if (st && !r.status) r.status = st, r.frame = (int)(p / ((long long)j.g.H * j.g.W)), r.stage = "expand";
  }
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
  Aligned filt;
  std::vector<unsigned char> rgb;
  int pixels = 0, status = 0, adler = 0, tally[PD_ST_LAST + 1] = {0};
  const long long used = clean.offsets.back();                     // the streams' bytes; the rest of data is padding
  for (int k = 0; k < runs; ++k) {
    Job j = clean;
    const long long s = r.below(j.n), a = j.offsets[(size_t)s], b = j.offsets[(size_t)s + 1];
    switch (k % 5) {
      case 0:                                                      // byte flips anywhere in the streams
        for (int i = 1 + (int)r.below(8); i > 0 && used > 0; --i) j.data[(size_t)r.below(used)] ^= (unsigned char)(1 + r.below(255));
        break;
      case 1:                                                      // a shortened (possibly empty) range
        j.offsets[(size_t)s + 1] = a + r.below(b - a);
        for (size_t q = (size_t)s + 2; q < j.offsets.size(); ++q) j.offsets[q] = j.offsets[q] < j.offsets[q - 1] ? j.offsets[q - 1] : j.offsets[q];
        break;
      case 2:                                                      // a run of bytes overwritten (0xFF runs and zero runs among them)
        if (used > 0) {
          const long long at = r.below(used), len = 1 + r.below(32);
          const unsigned char v = (k & 8) ? 0xFF : (k & 16) ? 0x00 : (unsigned char)r.below(256);
          for (long long i = at; i < at + len && i < used; ++i) j.data[(size_t)i] = v;
        }
        break;
      case 3:                                                      // falsified code lengths: bit flips where a stream's block header lies
        for (int i = 1 + (int)r.below(3); i > 0 && b > a; --i) j.data[(size_t)(a + r.below(b - a < 48 ? b - a : 48))] ^= (unsigned char)(1u << r.below(8));
        break;
      default:                                                     // a falsified header in mid-stream (a later block's, where there is one)
        if (b > a) j.data[(size_t)(a + r.below(b - a))] ^= (unsigned char)(1u << r.below(8));
        if (j.g.ct == 3) j.plte_len[(size_t)s] = (int)r.below(257);
        break;
    }
    const Result res = decode(j, filt, rgb, false, nullptr);
    if (res.status == -1) ++adler;
    else if (res.status) ++tally[res.status], ++status;
    else ++pixels;
  }
  printf("fuzz: %d runs, %d ended in pixels, %d in a status, %d in an Adler-32 mismatch (by code:", runs, pixels, status, adler);
  for (int i = 1; i <= PD_ST_LAST; ++i) printf(" %d", tally[i]);
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
    fprintf(stderr, "usage: %s decode JOB OUT | filtered JOB OUT | fuzz JOB RUNS SEED (JOB unreadable or malformed)\n", argv[0]);
    return 2;
  }
  const bool filtered = !strcmp(argv[1], "filtered");
  if ((filtered || !strcmp(argv[1], "decode")) && argc == 4) {
    Aligned filt;
    std::vector<unsigned char> rgb, raw;
    const Result r = decode(j, filt, rgb, filtered, &raw);
    if (r.status) {
      if (r.status == -1) fprintf(stderr, "adler mismatch in frame %d\n", r.frame);
      else fprintf(stderr, "status %d in frame %d (%s)\n", r.status, r.frame, r.stage);
      return 3;
    }
    return write_file(argv[3], filtered ? raw : rgb) ? 0 : 2;
  }
  if (!strcmp(argv[1], "fuzz") && argc == 5) return fuzz(j, atoi(argv[3]), strtoull(argv[4], nullptr, 10));
  return 2;
}
