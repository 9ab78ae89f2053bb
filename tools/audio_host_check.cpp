// Host run of csrc/audio_core.h -- the sample decoding, down-mix, index arithmetic and summation order that csrc/audio.hip runs on the device --
// built by tests/test_audio_in.py under ASan + UBSan.  Stand-alone: its own main, nothing of it is loaded into Python.  Every buffer is a heap
// block of exactly the bytes the routine may touch, so an index off either end is an error, not a wrong number.
//
//   audio_host_check decode   IN OUT    IN: int64 fmt, channels, n_frames, offset; then the frames' bytes.  The frames are placed `offset` bytes
//                                       into a block of offset + bytes; OUT: n_frames floats (audio_frame_mono)
//   audio_host_check resample IN OUT    IN: int64 up, down, half, n_in; then x (n_in floats) and the phase-major table (audio_table_len floats).
//                                       Walks the outputs in the kernel's workgroups of 256: each stages x[lo .. hi] in a block of exactly that
//                                       size (checked against audio_stage_len) and runs audio_resample_one; OUT: n_out floats
//   audio_host_check index up down half n_in j...   prints "j i_lo i_hi tap_lo tap_hi" per j (tap_hi: the tap that goes with i_lo); no arrays
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "audio_core.h"

static std::vector<uint8_t> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  std::vector<uint8_t> b;
  uint8_t tmp[1 << 16];
  size_t n;
  while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) b.insert(b.end(), tmp, tmp + n);
  fclose(f);
  return b;
}

static void spill(const char* path, const float* v, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); exit(2); }
  if (n && fwrite(v, sizeof(float), n, f) != n) { perror(path); exit(2); }
  fclose(f);
}

static void need(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "audio_host_check: %s\n", what); exit(3); }
}

static int run_decode(const char* in, const char* out) {
  const std::vector<uint8_t> b = slurp(in);
  need(b.size() >= 32, "decode: short header");
  int64_t hd[4];
  memcpy(hd, b.data(), 32);
  const int fmt = (int)hd[0], channels = (int)hd[1];
  const int64_t n = hd[2], offset = hd[3];
  need(fmt >= 0 && fmt < AU_FORMATS && channels >= 1 && channels <= AU_MAX_CHANNELS && n >= 1 && offset >= 0, "decode: header out of range");
  const int64_t fb = (int64_t)channels * audio_sample_bytes(fmt);
  need((int64_t)b.size() == 32 + n * fb, "decode: the file does not hold n_frames frames");
  uint8_t* block = (uint8_t*)malloc((size_t)(offset + n * fb));            // exactly sized: the last frame ends at the block's end
  memcpy(block + offset, b.data() + 32, (size_t)(n * fb));
  std::vector<float> y((size_t)n);
  for (int64_t f = 0; f < n; ++f) y[(size_t)f] = audio_frame_mono(block + offset + f * fb, fmt, channels);
  free(block);
  spill(out, y.data(), y.size());
  return 0;
}

static int run_resample(const char* in, const char* out) {
  const std::vector<uint8_t> b = slurp(in);
  need(b.size() >= 32, "resample: short header");
  int64_t hd[4];
  memcpy(hd, b.data(), 32);
  const int up = (int)hd[0], down = (int)hd[1], half = (int)hd[2];
  const int64_t n_in = hd[3];
  need(up >= 1 && down >= 1 && half >= 1 && n_in >= 1, "resample: header out of range");
  const int64_t tl = audio_table_len(up, half);
  need((int64_t)b.size() == 32 + 4 * (n_in + tl), "resample: the file does not hold x and the table");
  float* x = (float*)malloc((size_t)n_in * 4);
  float* taps = (float*)malloc((size_t)tl * 4);
  memcpy(x, b.data() + 32, (size_t)n_in * 4);
  memcpy(taps, b.data() + 32 + n_in * 4, (size_t)tl * 4);
  const int64_t n_out = audio_out_len(n_in, up, down), T = 256, cap = audio_stage_len(T, up, down, half);
  std::vector<float> y((size_t)n_out);
  for (int64_t j0 = 0; j0 < n_out; j0 += T) {
    const int64_t j1 = (j0 + T < n_out ? j0 + T : n_out) - 1;
    const int64_t lo = audio_span(j0, n_in, up, down, half).i_lo, hi = audio_span(j1, n_in, up, down, half).i_hi;
    need(lo >= 0 && hi < n_in && hi >= lo && hi - lo + 1 <= cap, "resample: a workgroup's span leaves x or exceeds audio_stage_len");
    float* stage = (float*)malloc((size_t)(hi - lo + 1) * 4);               // what the workgroup holds in LDS, and no float more
    memcpy(stage, x + lo, (size_t)(hi - lo + 1) * 4);
    for (int64_t j = j0; j <= j1; ++j) y[(size_t)j] = audio_resample_one(stage, lo, taps, j, n_in, up, down, half);
    free(stage);
  }
  free(x);
  free(taps);
  spill(out, y.data(), y.size());
  return 0;
}

static int run_index(int argc, char** argv) {
  need(argc >= 6, "index: up down half n_in j...");
  const int up = atoi(argv[2]), down = atoi(argv[3]), half = atoi(argv[4]);
  const int64_t n_in = atoll(argv[5]);
  for (int k = 6; k < argc; ++k) {
    const int64_t j = atoll(argv[k]);
    const AudioSpan s = audio_span(j, n_in, up, down, half);
    printf("%lld %lld %lld %lld %lld\n", (long long)j, (long long)s.i_lo, (long long)s.i_hi, (long long)s.tap_lo,
           (long long)(s.tap_lo + (s.i_hi - s.i_lo) * up));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "decode")) return run_decode(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "resample")) return run_resample(argv[2], argv[3]);
  if (argc >= 2 && !strcmp(argv[1], "index")) return run_index(argc, argv);
  fprintf(stderr, "usage: audio_host_check decode|resample IN OUT | index up down half n_in j...\n");
  return 2;
}
