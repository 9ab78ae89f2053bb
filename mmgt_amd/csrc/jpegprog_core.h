// Progressive JPEG entropy decode (ITU T.81 G.2, SOF2, Huffman, 8 bit), written once as plain inline functions on top of
// csrc/jpegdec_core.h: csrc/jpegprog.hip calls them from its kernel and tools/jpegprog_host_check.cpp from a host program.  A progressive file
// fills the coefficient buffer of the baseline decoder in several scans, each a spectral band [Ss, Se] and a bit plane (Ah, Al) of some
// components; the four procedures are those of libjpeg's jdphuff.c (DC first, DC refinement, AC first, AC refinement).  Nothing here touches
// memory outside the ranges its arguments name, whatever the bytes, descriptors and tables hold: bad data ends in a status, not in a write, and
// every loop is bounded by the segment's own units, by Se, by 16 code lengths or by the segment's bytes (past which the reader gives zeros).
//
// One unit of work is a restart segment of one scan: byte-aligned, DC predictors 0, EOBRUN 0.  Its units are
//   * a scan of all the frame's components (DC only): the frame's MCUs, padding blocks included, as in a baseline scan;
//   * a scan of one component: that component's own ceil(w_c / 8) x ceil(h_c / 8) blocks in raster order (T.81 A.2.2), never the blocks
//     that exist only as MCU padding.
// Coefficients go in natural order into the layout jd_decode_segment writes: (n, frame blocks, 64) int16.
//
// Scan descriptor (PJ_SCAN_INTS int32 words): [0] frame, [1] component count, [2..4] component indices, [5] Ss, [6] Se, [7] Ah, [8] Al,
// [9..11] DC table of each scan component and [12] the AC table, as indices into the batch's Huffman blocks (JD_HUFF_INTS words each: MINCODE,
// MAXCODE, VALPTR, HUFFVAL as in a frame's table block); [13..15] unused.
#pragma once
#include "jpegdec_core.h"

enum {
  PJ_SCAN_FRAME = 0,
  PJ_SCAN_NS = 1,
  PJ_SCAN_COMP = 2,
  PJ_SCAN_SS = 5,
  PJ_SCAN_SE = 6,
  PJ_SCAN_AH = 7,
  PJ_SCAN_AL = 8,
  PJ_SCAN_DC = 9,
  PJ_SCAN_AC = 12,
  PJ_SCAN_INTS = 16
};

// per-segment status words
enum {
  PJ_OK = 0,
  PJ_ST_CODE = 1,        // a code longer than 16 bits
  PJ_ST_INDEX = 2,       // a coefficient index past Se
  PJ_ST_CATEGORY = 3,    // a size category outside the scan type's range: above 11 (DC first), above 10 (AC first), not 1 (AC refinement)
  PJ_ST_EOBRUN = 4,      // an EOB run past the segment's last block
  PJ_ST_EXHAUSTED = 5,   // data exhausted before the last block
  PJ_ST_DESCRIPTOR = 6   // the segment's or its scan's descriptor is outside the batch or no legal progression: nothing was read
};

// the real size in blocks of component c's plane: what a scan of that component alone walks
JD_HD int pj_own_bw(const JdGeom& g, int c) { return ((c == 0 ? g.W : (g.W + g.hs - 1) / g.hs) + 7) / 8; }
JD_HD int pj_own_bh(const JdGeom& g, int c) { return ((c == 0 ? g.H : (g.H + g.vs - 1) / g.vs) + 7) / 8; }
// units of a scan of `ns` components (ns > 1: all of the frame's, interleaved), the first being component c
JD_HD long long pj_scan_units(const JdGeom& g, int ns, int c) {
  return ns > 1 ? (long long)g.mcu_rows * g.mcu_cols : (long long)pj_own_bw(g, c) * pj_own_bh(g, c);
}

// T.81 F.2.2.3 DECODE as jd_huff, in unsigned arithmetic: the table words may be anything (they are operands, not trusted)
JD_HD int pj_huff(JdBits& b, const int32_t* h) {
  const int look = (int)(b.acc >> (b.cnt - 16)) & 0xFFFF;
  for (int l = 1; l <= 16; ++l) {
    const int code = look >> (16 - l);
    if (code <= h[JD_HUFF_MAX + l]) {
      b.cnt -= l;
      return h[JD_HUFF_VAL + (((uint32_t)code - (uint32_t)h[JD_HUFF_MIN + l] + (uint32_t)h[JD_HUFF_PTR + l]) & 255u)] & 255;
    }
  }
  return -1;
}
JD_HD int pj_bit(JdBits& b) {
  if (b.cnt < 1) jd_fill(b);
  return jd_receive(b, 1);
}

// A refinement scan reads every coefficient of its band, and each such read would be a dependent 2-byte global load behind the lane's own
// stores to that line.  So such a scan works on a lane-private copy of the block (`tmp`: 64 int16, 16-byte aligned; LDS in the kernel, the
// stack in the host program): 128 bytes fetched at once, reads from the copy, and a changed coefficient stored to both (measured: about a tenth
// off the refinement launches).  The fetch also reads the coefficients outside the band, which another lane of the same launch may be writing;
// they are never used.
JD_HD void pj_fetch_block(int16_t* tmp, const int16_t* blk) {
  __builtin_memcpy(__builtin_assume_aligned(tmp, 16), __builtin_assume_aligned(blk, 16), 64 * sizeof(int16_t));
}
// one already non-zero coefficient passed over in a refinement: its correction bit (jdphuff.c decode_mcu_AC_refine)
JD_HD void pj_correct(JdBits& b, int16_t* blk, int16_t* tmp, int at, int v, int p1, int m1) {
  if (pj_bit(b) && (v & p1) == 0) tmp[at] = blk[at] = (int16_t)(v + (v >= 0 ? p1 : m1));
}
// block `blk`, band [k, Se]: the correction bit of every coefficient that is already non-zero (the EOBRUN tail)
JD_HD void pj_refine_tail(JdBits& b, int16_t* blk, int16_t* tmp, int k, int Se, int p1, int m1) {
  for (; k <= Se; ++k) {
    const int at = jd_natural(k), v = tmp[at];
    if (v != 0) pj_correct(b, blk, tmp, at, v, p1, m1);
  }
}

// One restart segment: the units [u0, u1) of the scan `sc` (checked by the caller) from data[beg, end) into the FRAME's coefficient block.
JD_HD int pj_decode_segment(const unsigned char* data, long long beg, long long end, const int32_t* sc, const int32_t* huff, const JdGeom& g,
                            long long u0, long long u1, int16_t* coef, int16_t* tmp) {
  JdBits b = {data, beg, end, 0, 0, 0};
  const int ns = sc[PJ_SCAN_NS], Ss = sc[PJ_SCAN_SS], Se = sc[PJ_SCAN_SE], Ah = sc[PJ_SCAN_AH], Al = sc[PJ_SCAN_AL];
  const int p1 = 1 << Al, m1 = -(1 << Al);
  if (Ss == 0) {                                                   // ---- DC: every block of every unit
    uint32_t pred[3] = {0, 0, 0};
    for (long long u = u0; u < u1; ++u) {
      for (int i = 0; i < ns; ++i) {
        const int c = sc[PJ_SCAN_COMP + i];
        const int hs = (ns > 1 && c == 0) ? g.hs : 1, vs = (ns > 1 && c == 0) ? g.vs : 1;
        const int cols = ns > 1 ? g.mcu_cols : pj_own_bw(g, c);
        const long long uy = u / cols, ux = u - uy * cols;
        const int32_t* dc = huff + (long long)sc[PJ_SCAN_DC + i] * JD_HUFF_INTS;
        for (int v = 0; v < vs; ++v)
          for (int h = 0; h < hs; ++h) {
            int16_t* blk = coef + (jd_block0(g, c) + (uy * vs + v) * jd_bw(g, c) + (ux * hs + h)) * 64;
            if (Ah == 0) {                                         // first scan: difference, predictor, << Al, int16 wrap
              jd_fill(b);
              const int s = pj_huff(b, dc);
              if (s < 0) return PJ_ST_CODE;
              if (s > 11) return PJ_ST_CATEGORY;
              if (s) pred[i] += (uint32_t)jd_extend(jd_receive(b, s), s);
              blk[0] = (int16_t)(uint16_t)(pred[i] << Al);
            } else if (pj_bit(b)) {                                // refinement: one bit per block
              blk[0] = (int16_t)(blk[0] | p1);
            }
            if (b.cnt < b.pad) return PJ_ST_EXHAUSTED;
          }
      }
    }
    return PJ_OK;
  }
  // ---- AC: one component, one block per unit
  const int c = sc[PJ_SCAN_COMP];
  const int cols = pj_own_bw(g, c);
  const int32_t* ac = huff + (long long)sc[PJ_SCAN_AC] * JD_HUFF_INTS;
  long long eobrun = 0;                                            // blocks still inside an EOB run, this one included
  for (long long u = u0; u < u1; ++u) {
    const long long uy = u / cols, ux = u - uy * cols;
    int16_t* blk = coef + (jd_block0(g, c) + uy * jd_bw(g, c) + ux) * 64;
    int k = Ss;
    if (Ah != 0) pj_fetch_block(tmp, blk);
    if (eobrun == 0) {
      while (k <= Se) {
        jd_fill(b);
        const int rs = pj_huff(b, ac);
        if (rs < 0) return PJ_ST_CODE;
        int r = rs >> 4, s = rs & 15;
        if (s == 0 && r != 15) {                                   // EOBr: 2^r + r appended bits blocks end here, this one included
          eobrun = (1ll << r) + (r ? jd_receive(b, r) : 0);
          if (eobrun > u1 - u) return PJ_ST_EOBRUN;
          break;
        }
        if (Ah == 0) {                                             // first scan (decode_mcu_AC_first)
          if (s == 0) {
            k += 16;                                               // ZRL
            continue;
          }
          if (s > 10) return PJ_ST_CATEGORY;
          k += r;
          if (k > Se) return PJ_ST_INDEX;
          blk[jd_natural(k)] = (int16_t)(uint16_t)((uint32_t)jd_extend(jd_receive(b, s), s) << Al);
          ++k;
        } else {                                                   // refinement (decode_mcu_AC_refine)
          if (s != 0) {
            if (s != 1) return PJ_ST_CATEGORY;
            s = jd_receive(b, 1) ? p1 : m1;
          }
          for (; k <= Se; ++k) {                                   // pass r zero-history coefficients (ZRL: 15, stop on the 16th), correcting the others
            const int at = jd_natural(k), v = tmp[at];
            if (v != 0) {
              pj_correct(b, blk, tmp, at, v, p1, m1);
            } else if (--r < 0) {
              break;
            }
          }
          if (s != 0) {
            if (k > Se) return PJ_ST_INDEX;
            tmp[jd_natural(k)] = blk[jd_natural(k)] = (int16_t)s;
          }
          ++k;
        }
      }
    }
    if (eobrun > 0) {
      if (Ah != 0) pj_refine_tail(b, blk, tmp, k, Se, p1, m1);
      --eobrun;
    }
    if (b.cnt < b.pad) return PJ_ST_EXHAUSTED;                     // some of the bits this block took were zeros past the end
  }
  return PJ_OK;
}

// Segment s of one level's launch over a batch of n frames: data[offsets[s], offsets[s + 1]) holds the units [seginfo[3 s + 1], seginfo[3 s + 2])
// of scan seginfo[3 s].  Segment, scan and table indices are checked against the batch before anything is read or written.  tmp: pj_fetch_block's.
JD_HD int pj_segment(const unsigned char* data, long long data_bytes, const long long* offsets, const int32_t* seginfo, const int32_t* scaninfo,
                     const int32_t* huff, int16_t* coef, int16_t* tmp, const JdGeom& g, int n, int nscan, int nhuff, long long s) {
  const int scan = seginfo[3 * s];
  const long long u0 = seginfo[3 * s + 1], u1 = seginfo[3 * s + 2], beg = offsets[s], end = offsets[s + 1];
  if (scan < 0 || scan >= nscan || beg < 0 || end < beg || end > data_bytes) return PJ_ST_DESCRIPTOR;
  const int32_t* sc = scaninfo + (long long)scan * PJ_SCAN_INTS;
  const int frame = sc[PJ_SCAN_FRAME], ns = sc[PJ_SCAN_NS], Ss = sc[PJ_SCAN_SS], Se = sc[PJ_SCAN_SE], Ah = sc[PJ_SCAN_AH], Al = sc[PJ_SCAN_AL];
  if (frame < 0 || frame >= n || (ns != 1 && ns != g.ncomp) || Ss < 0 || Se < Ss || Se > 63 || (Ss == 0 && Se != 0) || (Ss > 0 && ns != 1) ||
      Al < 0 || Al > 13 || (Ah != 0 && Ah != Al + 1))
    return PJ_ST_DESCRIPTOR;
  for (int i = 0; i < ns; ++i) {
    const int c = sc[PJ_SCAN_COMP + i];
    if (c < 0 || c >= g.ncomp || (ns > 1 && c != i)) return PJ_ST_DESCRIPTOR;
    const int t = Ss == 0 ? sc[PJ_SCAN_DC + i] : sc[PJ_SCAN_AC];
    if (!(Ss == 0 && Ah != 0) && (t < 0 || t >= nhuff)) return PJ_ST_DESCRIPTOR;       // a DC refinement reads no table
  }
  if (u0 < 0 || u1 < u0 || u1 > pj_scan_units(g, ns, sc[PJ_SCAN_COMP])) return PJ_ST_DESCRIPTOR;
  return pj_decode_segment(data, beg, end, sc, huff, g, u0, u1, coef + (long long)frame * jd_frame_blocks(g) * 64, tmp);
}
