// Host program over mmgt_amd/csrc/vp8dec_core.h: the lossy WebP (VP8 key frame) decoder's parse, reconstruction, loop filter and output exactly as
// the kernels of csrc/vp8dec.hip call them, without a GPU.  Plain C++ (no HIP): what the kernels' threads do between two barriers runs here as a
// loop, and in the REVERSE of thread order, so that a step which leaned on a neighbour of the same step would show.  tests/test_vp8dec.py builds it
// with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it, so an out-of-range access or undefined arithmetic on ANY input ends the
// program with an error.
//
//   vp8dec_host_check decode JOB OUT        decode the frames of JOB, write the ARGB words of every frame's rectangle to OUT; exit 3 with the first
//                                           status if there is one (nothing is written then)
//   vp8dec_host_check parsed JOB OUT        the same, but OUT receives the scratch words after the parse (header block, modes, coefficients)
//   vp8dec_host_check unfiltered JOB OUT    ... after reconstruction (the planes before the loop filter)
//   vp8dec_host_check filtered JOB OUT      ... after the loop filter
//   vp8dec_host_check fuzz JOB RUNS SEED    RUNS seeded corruptions of JOB, each decoded to pixels or to a status; prints the tally
//
// JOB (little endian, written by the test from mmgt_amd.video_in.webp_operands_lossy): int32 magic 'V8J1', n; int64 scratch_words, argb_words, data_bytes
// (a multiple of 16); int64 tab[n * 8]; data[data_bytes].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vp8dec_core.h"

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
  long long scratch_words = 0, argb_words = 0;
  std::vector<long long> tab;
  std::vector<unsigned char> data;
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

bool load(const char* path, Job& j) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[2];
  long long q[3];
  bool ok = read_exact(f, h, sizeof h) && read_exact(f, q, sizeof q) && h[0] == 0x314A3856 && h[1] >= 1 && h[1] <= 4096 && q[0] >= V8D_HDR &&
            q[0] <= (1ll << 28) && q[1] >= 1 && q[1] <= (1ll << 28) && q[2] >= 16 && q[2] % 16 == 0 && q[2] <= (1ll << 28);
  if (ok) {
    j.n = h[1], j.scratch_words = q[0], j.argb_words = q[1];
    j.tab.resize((size_t)j.n * V8D_TAB);
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

enum Stop { kParsed, kUnfiltered, kFiltered, kArgb };

// The parse launch for one frame: the serial first partition, then the token workers, skewed, one step at a time.
int parse_frame(const long long* t, const unsigned char* data, long long data_bytes, uint32_t* scr, long long scratch_words) {
  V8dFrame f;
  int st = v8d_frame(t, scr, scratch_words, data_bytes, 1ll << 62, &f);
  if (st) return st;
  unsigned char probs[1056];
  v8_coef_table(probs, 0, 1);
  V8dHdr h;
  long long part[16];
  st = v8d_parse_first(&f, data, &h, probs, part);
  if (st) return st;
  V8dWorker w[8];
  for (int p = 0; p < h.parts; ++p) v8d_bool_init(&w[p].br, data, part[2 * p], part[2 * p + 1]), w[p].lnz = w[p].ldc = 0;
  const long long steps = v8d_token_steps(&f, h.parts);
  for (long long s = 0; s < steps; ++s)
    for (int p = h.parts - 1; p >= 0; --p) v8d_token_step(&f, &h, probs, &w[p], p, s);
  for (int p = 0; p < h.parts && p < f.mbh; ++p)                      // a partition without a macroblock row is never read
    if (w[p].br.eof) return V8D_ST_TOKEN_END;
  f.hdr[V8D_H_MAGIC] = V8D_MAGIC;
  return V8D_OK;
}

bool frame_ready(const long long* t, uint32_t* scr, long long scratch_words, long long argb_words, V8dFrame* f) {
  return v8d_frame(t, scr, scratch_words, 1ll << 62, argb_words, f) == V8D_OK && f->hdr[V8D_H_MAGIC] == (uint32_t)V8D_MAGIC;
}

Result decode(const Job& j, Stop stop, std::vector<unsigned char>& result, long long* hev_count = nullptr) {
  Result r;
  Aligned data, scratch, argb;
  data.reset(j.data.size());
  memcpy(data.p, j.data.data(), j.data.size());
  scratch.reset((size_t)j.scratch_words * 4);
  memset(scratch.p, 0xA5, scratch.bytes);
  argb.reset((size_t)j.argb_words * 4);
  memset(argb.p, 0xA5, argb.bytes);
  uint32_t* const scr = reinterpret_cast<uint32_t*>(scratch.p);
  uint32_t* const px = reinterpret_cast<uint32_t*>(argb.p);
  for (int k = 0; k < j.n; ++k) {
    const int st = parse_frame(j.tab.data() + (size_t)k * V8D_TAB, data.p, (long long)data.bytes, scr, j.scratch_words);
    if (st < 0 || st > V8D_ST_LAST) abort();
    if (st && !r.status) r.status = st, r.frame = k, r.stage = "parse";
  }
  if (stop == kParsed) {
    if (!r.status) result.assign(scratch.p, scratch.p + scratch.bytes);
    return r;
  }
  for (int pass = 0; pass < 2; ++pass) {                            // reconstruct, then filter: as on the device, every frame goes through both
    for (int k = 0; k < j.n; ++k) {
      V8dFrame f;
      if (!frame_ready(j.tab.data() + (size_t)k * V8D_TAB, scr, j.scratch_words, 1ll << 62, &f)) {
        if (!r.status) r.status = V8D_ST_UPSTREAM, r.frame = k, r.stage = pass ? "filter" : "reconstruct";
        continue;
      }
      const int fronts = f.mbw + 2 * (f.mbh - 1);
      int count[2] = {0, 0};
      for (int front = 0; front < fronts; ++front)
        for (int my = f.mbh - 1; my >= 0; --my) {
          const int mx = front - 2 * my;
          if (mx < 0 || mx >= f.mbw) continue;
          if (pass == 0) v8d_recon_mb(&f, my, mx);
          else v8d_filter_mb(&f, (int)f.hdr[V8D_H_FILTER], f.hdr + V8D_H_FS, my, mx, count);
        }
      if (hev_count) hev_count[0] += count[0], hev_count[1] += count[1];
    }
    if (stop == (pass ? kFiltered : kUnfiltered)) {
      if (!r.status) result.assign(scratch.p, scratch.p + scratch.bytes);
      return r;
    }
  }
  for (int k = 0; k < j.n; ++k) {
    V8dFrame f;
    if (!frame_ready(j.tab.data() + (size_t)k * V8D_TAB, scr, j.scratch_words, j.argb_words, &f)) {
      if (!r.status) r.status = V8D_ST_UPSTREAM, r.frame = k, r.stage = "output";
      continue;
    }
    for (int y = 0; y < f.H; ++y)
      for (int x = 0; x < f.W; ++x) px[f.pix + (long long)y * f.W + x] = v8d_pixel(&f, y, x);
  }
  if (!r.status) result.assign(argb.p, argb.p + argb.bytes);
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
  std::vector<unsigned char> out;
  int pixels = 0, status = 0, tally[V8D_ST_LAST + 1] = {0};
  for (int k = 0; k < runs; ++k) {
    Job j = clean;
    long long* t = j.tab.data() + (size_t)r.below(j.n) * V8D_TAB;
    const long long a = t[V8D_BEGIN], b = t[V8D_END];
    switch (k % 6) {
      case 0:                                                      // byte flips anywhere in the payload
        for (int i = 1 + (int)r.below(8); i > 0 && b > a; --i) j.data[(size_t)(a + r.below(b - a))] ^= (unsigned char)(1 + r.below(255));
        break;
      case 1:                                                      // a shortened (possibly empty) payload
        t[V8D_END] = a + r.below(b - a);
        break;
      case 2:                                                      // a run of bytes overwritten (0xFF runs and zero runs among them)
        if (b > a) {
          const long long at = a + r.below(b - a), len = 1 + r.below(32);
          const unsigned char v = (k & 8) ? 0xFF : (k & 16) ? 0x00 : (unsigned char)r.below(256);
          for (long long i = at; i < at + len && i < b; ++i) j.data[(size_t)i] = v;
        }
        break;
      case 3:                                                      // falsified header fields: bit flips in the first partition's first bytes
        for (int i = 1 + (int)r.below(3); i > 0 && b > a + 10; --i) j.data[(size_t)(a + 10 + r.below(b - a - 10 < 48 ? b - a - 10 : 48))] ^= (unsigned char)(1u << r.below(8));
        break;
      case 4:                                                      // a falsified frame tag: first-partition size, profile, sizes
        if (b > a) j.data[(size_t)(a + r.below(b - a < 10 ? b - a : 10))] ^= (unsigned char)(1u << r.below(8));
        break;
      default:                                                     // a table row that lies: too few scratch words, a range or a size outside the batch
        if (k % 18 == 5) t[V8D_CAP] = r.below(t[V8D_CAP]);
        else if (k % 18 == 11) t[V8D_END] = b + r.below(1 << 20);
        else t[r.below(2) ? V8D_W : V8D_H] += r.below(64) - 32;
        break;
    }
    const Result res = decode(j, kArgb, out);
    if (res.status) ++tally[res.status], ++status;
    else ++pixels;
  }
  printf("fuzz: %d runs, %d ended in pixels, %d in a status (by code:", runs, pixels, status);
  for (int i = 1; i <= V8D_ST_LAST; ++i) printf(" %d", tally[i]);
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
    fprintf(stderr, "usage: %s decode|parsed|unfiltered|filtered JOB OUT | fuzz JOB RUNS SEED (JOB unreadable or malformed)\n", argv[0]);
    return 2;
  }
  const char* names[4] = {"parsed", "unfiltered", "filtered", "decode"};
  for (int m = 0; m < 4; ++m)
    if (!strcmp(argv[1], names[m]) && argc == 4) {
      std::vector<unsigned char> out;
      long long hev[2] = {0, 0};
      const Result r = decode(j, (Stop)m, out, hev);
      if (r.status) {
        fprintf(stderr, "status %d in frame %d (%s)\n", r.status, r.frame, r.stage);
        return 3;
      }
      printf("hev taken %lld, not taken %lld\n", hev[0], hev[1]);
      return write_file(argv[3], out) ? 0 : 2;
    }
  if (!strcmp(argv[1], "fuzz") && argc == 5) return fuzz(j, atoi(argv[3]), strtoull(argv[4], nullptr, 10));
  return 2;
}
