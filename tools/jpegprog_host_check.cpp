// Host program over mmgt_amd/csrc/jpegprog_core.h and jpegdec_core.h: the progressive decoder's arithmetic and indexing, exactly as the kernels
// call it, without a GPU.  Plain C++ (no HIP); tests/test_jpegprog.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all and runs
// it, so an out-of-range access or undefined arithmetic on ANY input ends the program with an error.
//
//   jpegprog_host_check decode JOB OUT        decode the batch of JOB (progressive frames, baseline frames or both), write (n, H, W, 3) RGB bytes
//                                             to OUT; exit 3 with the first status if one is set
//   jpegprog_host_check fuzz JOB RUNS SEED    RUNS seeded corruptions of JOB's progressive part (entropy bytes, byte ranges, segment and scan
//                                             descriptors, Huffman blocks), each decoded lane by lane; after every lane the coefficients outside
//                                             that lane's frame, components, blocks and band must be unchanged (exit 5 otherwise)
//   jpegprog_host_check eobrun                synthetic operands: one EOB run of 32767 blocks (EOB14 with all appended bits set), and the same
//                                             run against a segment that is one block too short
//
// JOB (little endian, written by the test from mmgt_amd.video_in.prog_batch_operands / batch_operands): int32 magic 'JPJ1', n, H, W, ncomp, hs, vs,
// np, nb, nseg_p, nscan, nhuff, nlevels, nseg_b, table_ints, 0; int64 bytes_p, bytes_b; int32 frame_p[np], frame_b[nb] (each part's frames as
// indices of the output); the progressive part: int32 tables[np * table_ints], scaninfo[nscan * 16], huff[nhuff * 307], seginfo[nseg_p * 3],
// int64 levels[nlevels + 1], offsets[nseg_p + 1], data[bytes_p]; the baseline part: int32 tables[nb * table_ints], seginfo[nseg_b * 3], int64
// offsets[nseg_b + 1], data[bytes_b].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpegdec_core.h"
#include "jpegprog_core.h"

namespace {

struct Job {
  int n = 0, np = 0, nb = 0, nseg_p = 0, nscan = 0, nhuff = 0, nlevels = 0, nseg_b = 0;
  JdGeom g{};
  std::vector<int32_t> frame_p, frame_b, tables_p, scaninfo, huff, seginfo_p, tables_b, seginfo_b;
  std::vector<long long> levels, offsets_p, offsets_b;
  std::vector<unsigned char> data_p, data_b;
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
  v.resize(count);
  return read_exact(f, v.data(), count * sizeof(T));
}

bool load(const char* path, Job& j) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[16];
  long long bytes[2] = {0, 0};
  auto in = [](long long v, long long lo, long long hi) { return v >= lo && v <= hi; };
  bool ok = read_exact(f, h, sizeof h) && read_exact(f, bytes, sizeof bytes) && h[0] == 0x314A504A && h[14] == JD_TAB_INTS && in(h[1], 1, 4096) &&
            in(h[7], 0, h[1]) && in(h[8], 0, h[1]) && h[7] + h[8] == h[1] && in(h[9], 0, 1 << 22) && in(h[10], 0, 1 << 20) && in(h[11], 0, 1 << 20) &&
            in(h[12], 0, 64) && in(h[13], 0, 1 << 22) && in(bytes[0], 0, 1ll << 30) && in(bytes[1], 0, 1ll << 30) &&
            jd_geom(h[2], h[3], h[4], h[5], h[6], &j.g);
  if (ok) {
    j.n = h[1], j.np = h[7], j.nb = h[8], j.nseg_p = h[9], j.nscan = h[10], j.nhuff = h[11], j.nlevels = h[12], j.nseg_b = h[13];
    ok = read_vec(f, j.frame_p, (size_t)j.np) && read_vec(f, j.frame_b, (size_t)j.nb) && read_vec(f, j.tables_p, (size_t)j.np * JD_TAB_INTS) &&
         read_vec(f, j.scaninfo, (size_t)j.nscan * PJ_SCAN_INTS) && read_vec(f, j.huff, (size_t)j.nhuff * JD_HUFF_INTS) &&
         read_vec(f, j.seginfo_p, (size_t)j.nseg_p * 3) && read_vec(f, j.levels, (size_t)j.nlevels + 1) &&
         read_vec(f, j.offsets_p, (size_t)j.nseg_p + 1) && read_vec(f, j.data_p, (size_t)bytes[0]) &&
         read_vec(f, j.tables_b, (size_t)j.nb * JD_TAB_INTS) && read_vec(f, j.seginfo_b, (size_t)j.nseg_b * 3) &&
         read_vec(f, j.offsets_b, (size_t)j.nseg_b + 1) && read_vec(f, j.data_b, (size_t)bytes[1]);
    for (int k = 0; ok && k < j.np; ++k) ok = j.frame_p[(size_t)k] >= 0 && j.frame_p[(size_t)k] < j.n;
    for (int k = 0; ok && k < j.nb; ++k) ok = j.frame_b[(size_t)k] >= 0 && j.frame_b[(size_t)k] < j.n;
    for (int l = 0; ok && l < j.nlevels; ++l) ok = j.levels[(size_t)l] >= 0 && j.levels[(size_t)l] <= j.levels[(size_t)l + 1] && j.levels[(size_t)l + 1] <= j.nseg_p;
  }
  fclose(f);
  return ok;
}

// One lane of one level's launch, with the operand pointers sliced as mmgt_amd.video_in slices them for the device.
int lane(const Job& j, long long a, long long s, std::vector<int16_t>& coef) {
  alignas(16) int16_t tmp[64];
  return pj_segment(j.data_p.data(), (long long)j.data_p.size(), j.offsets_p.data() + a, j.seginfo_p.data() + 3 * a, j.scaninfo.data(), j.huff.data(),
                    coef.data(), tmp, j.g, j.np, j.nscan, j.nhuff, s - a);
}

// coefficients of `count` frames -> their pixels at the frames `map` of rgb
void finish(const Job& j, const std::vector<int16_t>& coef, const std::vector<int32_t>& tables, const std::vector<int32_t>& map, int count,
            std::vector<unsigned char>& rgb) {
  const long long fb = jd_frame_blocks(j.g), blocks = count * fb, hw = (long long)j.g.H * j.g.W;
  std::vector<unsigned char> planes((size_t)blocks * 64), part((size_t)count * hw * 3);
  for (long long b = 0; b < blocks; ++b) jd_block(coef.data(), tables.data(), planes.data(), j.g, b);
  for (long long p = 0; p < count * hw; ++p) jd_output_pixel(planes.data(), part.data(), j.g, p);
  for (int k = 0; k < count; ++k) memcpy(rgb.data() + (size_t)map[(size_t)k] * hw * 3, part.data() + (size_t)k * hw * 3, (size_t)hw * 3);
}

// The launches as loops: the progressive part level by level, the baseline part as csrc/jpegdec.hip does it.  Returns the first status.
int decode(const Job& j, std::vector<unsigned char>& rgb, long long* bad_segment, int* bad_part) {
  const long long fb = jd_frame_blocks(j.g);
  std::vector<int16_t> cp((size_t)j.np * fb * 64, 0), cb((size_t)j.nb * fb * 64, 0);
  int first = 0;
  for (int l = 0; l < j.nlevels; ++l)
    for (long long s = j.levels[(size_t)l]; s < j.levels[(size_t)l + 1]; ++s) {
      const int st = lane(j, j.levels[(size_t)l], s, cp);
      if (st && !first) first = st, *bad_segment = s, *bad_part = 0;
    }
  for (long long s = 0; s < j.nseg_b; ++s) {
    const int st = jd_segment(j.data_b.data(), (long long)j.data_b.size(), j.offsets_b.data(), j.seginfo_b.data(), j.tables_b.data(), cb.data(), j.g, j.nb, s);
    if (st && !first) first = st, *bad_segment = s, *bad_part = 1;
  }
  if (first) return first;
  rgb.assign((size_t)j.n * j.g.H * j.g.W * 3, 0);
  if (j.np) finish(j, cp, j.tables_p, j.frame_p, j.np, rgb);
  if (j.nb) finish(j, cb, j.tables_b, j.frame_b, j.nb, rgb);
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

// `keep` := `now` at every coefficient the lane s may write, judged from its (possibly corrupted) descriptors alone: the scan's frame, its
// components, the blocks of the units [u0, u1) and the band [Ss, Se].  Descriptors the core refuses allow nothing.
void allow(const Job& j, long long s, int status, const std::vector<int16_t>& now, std::vector<int16_t>& keep) {
  if (status == PJ_ST_DESCRIPTOR) return;
  const int32_t* sc = j.scaninfo.data() + (size_t)j.seginfo_p[(size_t)s * 3] * PJ_SCAN_INTS;
  const long long u0 = j.seginfo_p[(size_t)s * 3 + 1], u1 = j.seginfo_p[(size_t)s * 3 + 2], fb = jd_frame_blocks(j.g);
  const int ns = sc[PJ_SCAN_NS];
  for (int i = 0; i < ns; ++i) {
    const int c = sc[PJ_SCAN_COMP + i];
    const int hs = (ns > 1 && c == 0) ? j.g.hs : 1, vs = (ns > 1 && c == 0) ? j.g.vs : 1, cols = ns > 1 ? j.g.mcu_cols : pj_own_bw(j.g, c);
    for (long long u = u0; u < u1; ++u)
      for (int v = 0; v < vs; ++v)
        for (int h = 0; h < hs; ++h) {
          const long long b = sc[PJ_SCAN_FRAME] * fb + jd_block0(j.g, c) + ((u / cols) * vs + v) * jd_bw(j.g, c) + (u % cols) * hs + h;
          for (int k = sc[PJ_SCAN_SS]; k <= sc[PJ_SCAN_SE]; ++k) keep[(size_t)b * 64 + jd_natural(k)] = now[(size_t)b * 64 + jd_natural(k)];
        }
  }
}

int fuzz(const Job& clean, int runs, uint64_t seed) {
  Rng r{seed};
  if (clean.np < 1 || clean.nseg_p < 1 || clean.nlevels < 1) return 2;
  const long long fb = jd_frame_blocks(clean.g);
  int clean_runs = 0, status_runs = 0, tally[8] = {0};
  for (int k = 0; k < runs; ++k) {
    Job j = clean;
    switch (k % 6) {
      case 0:                                                      // byte flips inside the entropy-coded bytes
        for (int i = 1 + (int)r.below(8); i > 0 && !j.data_p.empty(); --i)
          j.data_p[(size_t)r.below((long long)j.data_p.size())] ^= (unsigned char)(1 + r.below(255));
        break;
      case 1: {                                                    // a shortened (possibly empty) byte range
        const long long s = r.below(j.nseg_p);
        j.offsets_p[(size_t)s + 1] = j.offsets_p[(size_t)s] + r.below(j.offsets_p[(size_t)s + 1] - j.offsets_p[(size_t)s]);
        break;
      }
      case 2:                                                      // a run of bytes overwritten (0xFF runs and zero runs among them)
        if (!j.data_p.empty()) {
          const long long at = r.below((long long)j.data_p.size()), len = 1 + r.below(32);
          const unsigned char v = (k & 1) ? 0xFF : (unsigned char)r.below(256);
          for (long long i = at; i < at + len && i < (long long)j.data_p.size(); ++i) j.data_p[(size_t)i] = v;
        }
        break;
      case 3: {                                                    // a scan descriptor word: small values (legal-looking) or anything
        int32_t& w = j.scaninfo[(size_t)r.below((long long)j.scaninfo.size())];
        w = (r.next() & 1) ? (int32_t)r.below(70) - 2 : (int32_t)r.next();
        break;
      }
      case 4:                                                      // words of a Huffman block
        for (int i = 1 + (int)r.below(6); i > 0; --i) {
          int32_t& w = j.huff[(size_t)r.below((long long)j.huff.size())];
          w = (r.next() & 1) ? (int32_t)r.below(65536) - 1 : (int32_t)r.next();
        }
        break;
      default: {                                                   // a segment descriptor word, or a byte offset
        if (r.next() & 1) {
          int32_t& w = j.seginfo_p[(size_t)r.below((long long)j.seginfo_p.size())];
          w = (r.next() & 1) ? (int32_t)r.below(2 * fb) - 2 : (int32_t)r.next();
        } else {
          j.offsets_p[(size_t)r.below((long long)j.offsets_p.size())] = (r.next() & 1) ? r.below(2 * (long long)j.data_p.size() + 2) - 1 : (long long)r.next();
        }
      }
    }
    std::vector<int16_t> coef((size_t)j.np * fb * 64, 0), keep;
    int first = 0;
    for (int l = 0; l < j.nlevels; ++l)
      for (long long s = j.levels[(size_t)l]; s < j.levels[(size_t)l + 1]; ++s) {
        keep = coef;
        const int st = lane(j, j.levels[(size_t)l], s, coef);
        if (st < 0 || st > 6) return 4;
        allow(j, s, st, coef, keep);
        if (keep != coef) {
          fprintf(stderr, "fuzz run %d: lane %lld (status %d) changed coefficients outside its range\n", k, s, st);
          return 5;
        }
        if (st && !first) first = st;
      }
    ++tally[first];
    first ? ++status_runs : ++clean_runs;
  }
  printf("fuzz: %d runs, %d ended in coefficients, %d in a status (by code:", runs, clean_runs, status_runs);
  for (int i = 1; i < 7; ++i) printf(" %d", tally[i]);
  printf(")\n");
  return 0;
}

// A flat grey frame of 5 x 8191 blocks whose AC scan is two EOB runs: EOB14 with its 14 appended bits set (32767 blocks, the longest a file can
// state) and EOB12 + 4092 for the other 8188.  Then the same bytes against a segment that ends one block before the first run does.
int eobrun() {
  Job j;
  if (!jd_geom(40, 65528, 1, 1, 1, &j.g)) return 2;
  const long long units = pj_scan_units(j.g, 1, 0);
  if (units != 40955) return 2;
  j.n = j.np = 1, j.nscan = 2, j.nhuff = 2, j.nseg_p = 2, j.nlevels = 1;
  j.huff.assign(2 * JD_HUFF_INTS, 0);
  for (int t = 0; t < 2; ++t) {
    int32_t* h = j.huff.data() + t * JD_HUFF_INTS;
    for (int l = 1; l <= 16; ++l) h[JD_HUFF_MAX + l] = -1;
    h[JD_HUFF_MIN + 2] = 0, h[JD_HUFF_MAX + 2] = t ? 1 : 0, h[JD_HUFF_PTR + 2] = 0;        // DC: 00 -> 0; AC: 00 -> EOB14, 01 -> EOB12
    h[JD_HUFF_VAL] = t ? 0xE0 : 0, h[JD_HUFF_VAL + 1] = t ? 0xC0 : 0;
  }
  j.scaninfo.assign(2 * PJ_SCAN_INTS, 0);
  int32_t* ac = j.scaninfo.data() + PJ_SCAN_INTS;
  j.scaninfo[PJ_SCAN_NS] = ac[PJ_SCAN_NS] = 1;
  ac[PJ_SCAN_SS] = 1, ac[PJ_SCAN_SE] = 63, ac[PJ_SCAN_AC] = 1;
  j.data_p.assign((size_t)(units * 2 + 7) / 8, 0);                                         // DC: 2 zero bits per block
  const long long dc_bytes = (long long)j.data_p.size();
  // 00 11111111111111 | 01 111111111100 (4092) -> 0011 1111 1111 1111 0111 1111 1111 00pp, stuffed after each 0xFF
  const unsigned char acb[] = {0x3F, 0xFF, 0x00, 0x7F, 0xF0};
  j.data_p.insert(j.data_p.end(), acb, acb + sizeof acb);
  j.offsets_p = {0, dc_bytes, dc_bytes + (long long)sizeof acb};
  j.seginfo_p = {0, 0, (int32_t)units, 1, 0, (int32_t)units};
  j.levels = {0, 2};
  std::vector<int16_t> coef((size_t)jd_frame_blocks(j.g) * 64, 0);
  const int dc = lane(j, 0, 0, coef), full = lane(j, 0, 1, coef);
  bool zero = true;
  for (int16_t v : coef) zero = zero && v == 0;
  j.seginfo_p[5] = 32766;
  const int cut = lane(j, 0, 1, coef);
  printf("eobrun: DC status %d, AC status %d over %lld blocks, all coefficients zero %d; a segment of 32766 blocks: status %d\n", dc, full, units,
         (int)zero, cut);
  return dc == PJ_OK && full == PJ_OK && zero && cut == PJ_ST_EOBRUN ? 0 : 6;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "eobrun")) return eobrun();
  Job j;
  if (argc < 3 || !load(argv[2], j)) {
    fprintf(stderr, "usage: %s decode JOB OUT | fuzz JOB RUNS SEED | eobrun (JOB unreadable or malformed)\n", argv[0]);
    return 2;
  }
  if (!strcmp(argv[1], "decode") && argc == 4) {
    std::vector<unsigned char> rgb;
    long long bad = 0;
    int part = 0;
    const int st = decode(j, rgb, &bad, &part);
    if (st) {
      if (part == 0) {
        const int scan = j.seginfo_p[(size_t)bad * 3];
        fprintf(stderr, "status %d in progressive segment %lld (scan descriptor %d)\n", st, bad, scan);
      } else {
        fprintf(stderr, "status %d in baseline segment %lld\n", st, bad);
      }
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
