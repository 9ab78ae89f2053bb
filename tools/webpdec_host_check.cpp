// Host program over mmgt_amd/csrc/webpdec_core.h: the WebP lossless decoder's entropy decode, inverse transforms and composition exactly as the
// kernels call them, without a GPU.  Plain C++ (no HIP): the header's per-lane bodies run as loops over lanes 0 .. 63 between the points where the
// kernels have barriers.  tests/test_webpdec.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it, so an
// out-of-range access or undefined arithmetic on ANY input ends the program with an error.
//
//   webpdec_host_check decode JOB OUT       decode the set of frames of JOB, write (n, H, W, 3) RGB bytes to OUT; exit 3 with the first status if
//                                           there is one (nothing is written then)
//   webpdec_host_check argb JOB OUT         the same, but OUT receives the ARGB words of every frame's rectangle, before composition
//   webpdec_host_check scratch JOB OUT      the same, but OUT receives the scratch words as the entropy decode left them
//   webpdec_host_check fuzz JOB RUNS SEED   RUNS seeded corruptions of JOB, each decoded to pixels or to a status within the step bound; prints the tally
//
// JOB (little endian, written by the test from mmgt_amd.video_in.webp_operands): int32 magic 'WDJ1', n, H, W; int64 scratch_words, argb_words,
// data_bytes (a multiple of 16); int64 tab[n * 16]; data[data_bytes].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "webpdec_core.h"

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
  int n = 0, H = 0, W = 0;
  long long scratch_words = 0, argb_words = 0;
  std::vector<long long> tab;
  std::vector<unsigned char> data;
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

bool load(const char* path, Job& j) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[4];
  long long q[3];
  bool ok = read_exact(f, h, sizeof h) && read_exact(f, q, sizeof q) && h[0] == 0x314A4457 && h[1] >= 1 && h[1] <= 4096 && h[2] >= 1 && h[3] >= 1 &&
            h[2] <= WD_MAX_SIDE && h[3] <= WD_MAX_SIDE && q[0] >= WD_HDR && q[0] <= (1ll << 28) && q[1] >= 1 && q[1] <= (1ll << 28) && q[2] >= 16 &&
            q[2] % 16 == 0 && q[2] <= (1ll << 28) && (long long)h[1] * h[2] * h[3] <= (1ll << 28);
  if (ok) {
    j.n = h[1], j.H = h[2], j.W = h[3], j.scratch_words = q[0], j.argb_words = q[1];
    j.tab.resize((size_t)j.n * WD_TAB);
    j.data.resize((size_t)q[2]);
    ok = read_exact(f, j.tab.data(), j.tab.size() * 8) && read_exact(f, j.data.data(), j.data.size());
  }
  fclose(f);
  return ok;
}

struct Result {
  int status = 0, frame = 0;
  const char* stage = "";
};

enum Stop { kScratch, kArgb, kPixels };

// The three launches of csrc/webpdec.hip as loops, buffers sized exactly as the wrapper sizes them and filled with 0xA5 first.
Result decode(const Job& j, Stop stop, std::vector<unsigned char>& result) {
  Result r;
  Aligned data, scratch, argb;
  data.reset(j.data.size());
  memcpy(data.p, j.data.data(), j.data.size());
  scratch.reset((size_t)j.scratch_words * 4);
  memset(scratch.p, 0xA5, scratch.bytes);
  argb.reset((size_t)j.argb_words * 4);
  memset(argb.p, 0xA5, argb.bytes);
  auto sh = std::make_unique<WdShared>();
  uint32_t* const scr = reinterpret_cast<uint32_t*>(scratch.p);
  uint32_t* const px = reinterpret_cast<uint32_t*>(argb.p);
  for (int f = 0; f < j.n; ++f) {
    const long long* t = j.tab.data() + (size_t)f * WD_TAB;
    long long steps = 0;
    const int st = wd_decode_stream(sh.get(), data.p, (long long)data.bytes, t, scr, j.scratch_words, &steps);
    if (st != WD_ST_DESCRIPTOR) {
      const long long len = t[WD_END] - t[WD_BEGIN];
      if (steps > 131 * 8 * len + t[WD_CAP] + 16) {                // the bound the kernel's loops are held to (webpdec_core.h: wd_decode_stream)
        fprintf(stderr, "frame %d: %lld loop iterations for %lld bytes and %lld scratch words\n", f, steps, len, t[WD_CAP]);
        abort();
      }
    }
    if (st > WD_ST_LAST || (st < 0 && -(long long)st <= t[WD_CAP])) abort();     // a negative status asks for more words than the row gave
    if (st && !r.status) r.status = st, r.frame = f, r.stage = "decode";
  }
  if (stop == kScratch && !r.status) result.assign(scratch.p, scratch.p + scratch.bytes);
  if (stop == kScratch) return r;
  uint32_t palette[256];
  for (int f = 0; f < j.n; ++f) {                                   // as on the device, every frame goes through every launch
    const int st = wd_untransform_frame(palette, j.tab.data() + (size_t)f * WD_TAB, scr, j.scratch_words, px, j.argb_words);
    if (st < 0 || st > WD_ST_LAST) abort();
    if (st && !r.status) r.status = st, r.frame = f, r.stage = "untransform";
  }
  if (stop == kArgb && !r.status) result.assign(argb.p, argb.p + argb.bytes);
  if (stop == kArgb) return r;
  const long long pixels = (long long)j.H * j.W;
  std::vector<uint32_t> carry((size_t)pixels, 0xA5A5A5A5u);
  std::vector<unsigned char> rgb((size_t)j.n * pixels * 3, 0xA5);
  for (long long p = 0; p < pixels; ++p) wd_compose_pixel(j.tab.data(), j.n, px, j.argb_words, carry.data(), rgb.data(), j.H, j.W, p);
  if (!r.status) result.swap(rgb);
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
  int pixels = 0, status = 0, tally[WD_ST_LAST + 1] = {0};
  for (int k = 0; k < runs; ++k) {
    Job j = clean;
    long long* t = j.tab.data() + (size_t)r.below(j.n) * WD_TAB;
    const long long a = t[WD_BEGIN], b = t[WD_END];
    switch (k % 6) {
      case 0:                                                      // byte flips anywhere in the frame's stream
        for (int i = 1 + (int)r.below(8); i > 0 && b > a; --i) j.data[(size_t)(a + r.below(b - a))] ^= (unsigned char)(1 + r.below(255));
        break;
      case 1:                                                      // a shortened (possibly empty) payload
        t[WD_END] = a + r.below(b - a);
        break;
      case 2:                                                      // a run of bytes overwritten (0xFF runs and zero runs among them)
        if (b > a) {
          const long long at = a + r.below(b - a), len = 1 + r.below(32);
          const unsigned char v = (k & 8) ? 0xFF : (k & 16) ? 0x00 : (unsigned char)r.below(256);
          for (long long i = at; i < at + len && i < b; ++i) j.data[(size_t)i] = v;
        }
        break;
      case 3:                                                      // falsified code lengths: bit flips where the transforms and first codes lie
        for (int i = 1 + (int)r.below(3); i > 0 && b > a + 5; --i) j.data[(size_t)(a + 5 + r.below(b - a - 5 < 64 ? b - a - 5 : 64))] ^= (unsigned char)(1u << r.below(8));
        break;
      case 4:                                                      // a falsified header: the size, the alpha bit, the version, the first transform bits
        if (b > a) j.data[(size_t)(a + r.below(b - a < 6 ? b - a : 6))] ^= (unsigned char)(1u << r.below(8));
        break;
      default:                                                     // a table row that lies: less scratch than the frame needs, or a range outside the batch
        if (k & 1) t[WD_CAP] = WD_HDR + r.below(t[WD_CAP] - WD_HDR + 1);
        else t[WD_END] = b + r.below(1 << 20);
        break;
    }
    const Result res = decode(j, kPixels, rgb);
    if (res.status) ++tally[res.status < 0 ? WD_ST_SCRATCH : res.status], ++status;
    else ++pixels;
  }
  printf("fuzz: %d runs, %d ended in pixels, %d in a status (by code:", runs, pixels, status);
  for (int i = 1; i <= WD_ST_LAST; ++i) printf(" %d", tally[i]);
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
    fprintf(stderr, "usage: %s decode JOB OUT | argb JOB OUT | scratch JOB OUT | fuzz JOB RUNS SEED (JOB unreadable or malformed)\n", argv[0]);
    return 2;
  }
  const bool scratch = !strcmp(argv[1], "scratch"), argb = !strcmp(argv[1], "argb");
  if ((scratch || argb || !strcmp(argv[1], "decode")) && argc == 4) {
    std::vector<unsigned char> out;
    const Result r = decode(j, scratch ? kScratch : argb ? kArgb : kPixels, out);
    if (r.status) {
      fprintf(stderr, "status %d in frame %d (%s)\n", r.status, r.frame, r.stage);
      return 3;
    }
    return write_file(argv[3], out) ? 0 : 2;
  }
  if (!strcmp(argv[1], "fuzz") && argc == 5) return fuzz(j, atoi(argv[3]), strtoull(argv[4], nullptr, 10));
  return 2;
}
