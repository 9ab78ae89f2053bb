"""Input path of the sampler from Motion-JPEG / JPEG files with the decode on the device: the counterpart of video_out's .avi writer.

  parse_jpeg           the markers of one baseline JPEG file -> JpegHeader (geometry, tables, the restart segments' byte ranges); refuses on the
                       host, with a ValueError naming the feature, everything the kernels do not decode
  decode_jpeg_frames   a batch of equally sized JPEG files -> (n, H, W, 3) uint8 RGB on the device: Huffman decode, dequantiser + inverse DCT,
                       chroma up-sampling and colour conversion run in csrc/jpegdec.hip, bit for bit libjpeg's (libjpeg-turbo's) default decode;
                       with progressive=True both also take progressive files (SOF2), whose scans fill the same coefficient buffer through
                       csrc/jpegprog.hip, one launch per dependency level of the scan script (scan_levels, prog_batch_operands)
  parse_png            the chunks of one PNG / APNG file -> PngHeader (geometry, palette, every frame's raw deflate bytes and expected Adler-32);
                       refuses on the host, with a ValueError naming the feature, everything the kernels do not decode
  decode_png_frames    PNG / APNG files of one geometry -> (n, H, W, 3) uint8 RGB on the device: inflate, scanline reconstruction and expansion run
                       in csrc/pngdec.hip, byte for byte PIL's Image.open(f).convert("RGB")
  parse_gif            the blocks of one GIF87a / GIF89a file -> GifHeader (screen, and per frame the rectangle, flags, colour table and LZW bytes with
                       the sub-block framing removed); refuses on the host, with a ValueError naming the cause, what the kernels do not decode
                       
  decode_gif_frames    one GIF file -> (n, H, W, 3) uint8 RGB on the device: un-LZW, de-interlace and PIL's frame composition (sub-rectangles, local
                       palettes, transparency, the four disposals) run in csrc/gifdec.hip, byte for byte ImageSequence.Iterator + convert("RGB")
  parse_webp           the chunks of one lossless WebP file, still or animated -> WebpHeader (canvas, loop count, and per frame the rectangle,
                       duration, blend, dispose, alpha flag, key-frame flag and VP8L payload); refuses on the host, with a ValueError naming the
                       cause, what the kernels do not decode
  decode_webp_frames   lossless WebP files of one canvas size -> (n, H, W, 3) uint8 RGB on the device: the VP8L entropy decode, the inverse
                       transforms and libwebp's frame composition run in csrc/webpdec.hip, byte for byte ImageSequence.Iterator + convert("RGB")
  read_frames_device   a Motion-JPEG .avi, a directory of .jpg frames, a directory of .png frames, a directory of .webp frames, one .png / .apng
                       file (animated or not), one .gif file or one .webp file (animated or not) -> the same tensor; anything else raises
                       (inputs.read_frames is the host route)
"""
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from .video_out import _AC_BITS, _AC_VALS, _DC_BITS, _ADLER, PNG_MAX_SIDE, _PNG_SIG

# T.81 figure A.6: zigzag position -> natural index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# the tables a file without any DHT segment means (T.81 Annex K.3; the usual Motion-JPEG frame): (class, id) -> (BITS, HUFFVAL)
ANNEX_K = {(0, 0): (_DC_BITS[0], bytes(range(12))), (0, 1): (_DC_BITS[1], bytes(range(12))),
           (1, 0): (_AC_BITS[0], _AC_VALS[0]), (1, 1): (_AC_BITS[1], _AC_VALS[1])}

_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential", 0xC6: "differential progressive",
              0xC7: "differential lossless", 0xC9: "arithmetic", 0xCA: "arithmetic progressive", 0xCB: "arithmetic lossless",
              0xCD: "arithmetic differential sequential", 0xCE: "arithmetic differential progressive", 0xCF: "arithmetic differential lossless"}

STATUS_TEXT = {1: "a Huffman code longer than 16 bits", 2: "a coefficient index past 63", 3: "a DC category above 11 or an AC category above 10",
               4: "an accumulated DC outside [-2048, 2047]", 5: "data exhausted before the last block", 6: "a segment descriptor outside the batch"}

# layout of a frame's table block: csrc/jpegdec_core.h (checked against the library's table_ints on every call)
_TAB_Q, _HUFF_INTS = 16, 51 + 256
_TAB_HUFF = _TAB_Q + 4 * 64
TAB_INTS = _TAB_HUFF + 4 * _HUFF_INTS


@dataclass
class JpegHeader:
    width: int
    height: int
    ncomp: int                                   # 1 or 3
    hs: int                                      # luma sampling (chroma is 1 x 1); 1, 1 for one component: its scan is not interleaved
    vs: int
    tq: Tuple[int, ...]                          # per component: quantiser table, DC table, AC table
    td: Tuple[int, ...]
    ta: Tuple[int, ...]
    qtables: Dict[int, np.ndarray]               # id -> (64,) in natural order
    huffman: Dict[Tuple[int, int], Tuple[bytes, bytes]]      # (class 0 DC / 1 AC, id) -> (BITS, HUFFVAL); Annex K when the file has no DHT
    restart_interval: int                        # MCUs per restart interval, 0 = none
    scan_offset: int                             # first byte of the entropy-coded data
    segments: List[Tuple[int, int]] = field(default_factory=list)       # [start, end) of every restart segment, markers excluded
    progressive: bool = False                    # SOF2 (parse_jpeg(..., progressive=True)): `scans` holds the file, the five fields above are unused
    scans: List["JpegScan"] = field(default_factory=list)

    @property
    def mcu_rows(self):
        return -(-self.height // (8 * self.vs))

    @property
    def mcu_cols(self):
        return -(-self.width // (8 * self.hs))

    @property
    def mcus(self):
        return self.mcu_rows * self.mcu_cols

    @property
    def geometry(self):
        return self.height, self.width, self.ncomp, self.hs, self.vs


def _check_huffman(bits, vals, what):
    total, code = 0, 0
    for length, n in enumerate(bits, 1):                                  # T.81 Annex C: the codes of each length must fit that length
        code += n
        if code > 1 << length:
            raise ValueError(f"parse_jpeg: {what} has more codes of length {length} than that length holds")
        code <<= 1
        total += n
    if total != len(vals) or total > 256:
        raise ValueError(f"parse_jpeg: {what} counts {total} codes for {len(vals)} values")


def parse_jpeg(data, progressive=False) -> JpegHeader:
    """One baseline JPEG file (bytes; trailing bytes after EOI are ignored) -> JpegHeader.  ValueError for everything outside the decoder's scope.
    With progressive=True a progressive file (SOF2) parses too, into a header with `progressive` set and its `scans`; a baseline file
    parses as without it."""
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise ValueError("parse_jpeg: not a JPEG file (missing SOI)")
    if progressive and _first_sof(data) == 0xC2:
        return _parse_progressive(data)
    pos, n = 2, len(data)
    qtables, huffman, sof, sos, ri, adobe = {}, {}, None, None, 0, None
    while sos is None:
        if pos + 2 > n:
            raise ValueError("parse_jpeg: missing SOS (the file ends in its headers)" if sof else "parse_jpeg: missing SOF (the file ends in its headers)")
        if data[pos] != 0xFF:
            raise ValueError(f"parse_jpeg: expected a marker at byte {pos}")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            continue
        m = data[pos]
        pos += 1
        if m == 0xD9:
            raise ValueError("parse_jpeg: missing SOS (EOI before any scan)" if sof else "parse_jpeg: missing SOF (EOI before any frame header)")
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if pos + 2 > n:
            continue
        length = int.from_bytes(data[pos:pos + 2], "big")
        body = data[pos + 2:pos + length]
        if length < 2 or pos + length > n:
            raise ValueError(f"parse_jpeg: segment {m:#04x} at byte {pos - 2} runs past the end of the file")
        pos += length
        if m == 0xDB:
            k = 0
            while k < len(body):
                pq, tid = body[k] >> 4, body[k] & 15
                if pq != 0:
                    raise ValueError("parse_jpeg: 16-bit quantiser tables are not decoded (8-bit DQT only)")
                if tid > 3 or k + 65 > len(body):
                    raise ValueError("parse_jpeg: bad DQT segment")
                q = np.zeros(64, np.int32)
                q[ZIGZAG] = np.frombuffer(body[k + 1:k + 65], np.uint8)
                qtables[tid] = q
                k += 65
        elif m == 0xC0:
            if sof is not None:
                raise ValueError("parse_jpeg: more than one SOF")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError("parse_jpeg: bad SOF0 segment")
            sof = body
        elif m in _SOF_NAMES:
            raise ValueError(f"parse_jpeg: {_SOF_NAMES[m]} JPEG (SOF{m - 0xC0}) is not decoded (baseline SOF0 only)")
        elif m == 0xC4:
            k = 0
            while k < len(body):
                tc, th = body[k] >> 4, body[k] & 15
                if tc > 1 or th > 1 or k + 17 > len(body):
                    raise ValueError("parse_jpeg: bad DHT segment (baseline: classes 0 - 1, tables 0 - 1)")
                bits = body[k + 1:k + 17]
                cnt = sum(bits)
                vals = body[k + 17:k + 17 + cnt]
                _check_huffman(bits, vals, f"DHT table {tc}/{th}")
                huffman[(tc, th)] = (bits, vals)
                k += 17 + cnt
        elif m == 0xDD:
            if len(body) != 2:
                raise ValueError("parse_jpeg: bad DRI segment")
            ri = int.from_bytes(body, "big")
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            if sof is None:
                raise ValueError("parse_jpeg: missing SOF (SOS before any frame header)")
            sos = body
        # APPn, COM and anything else with a length: skipped
    precision, height, width, ncomp = sof[0], int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    if precision != 8:
        raise ValueError(f"parse_jpeg: {precision}-bit samples are not decoded (8-bit only)")
    if ncomp == 4:
        raise ValueError("parse_jpeg: four components (CMYK / YCCK) are not decoded")
    if ncomp not in (1, 3):
        raise ValueError(f"parse_jpeg: {ncomp} components are not decoded (one or three)")
    if height < 1 or width < 1:
        raise ValueError(f"parse_jpeg: frame size {width} x {height}")
    if adobe == 0 and ncomp == 3:
        raise ValueError("parse_jpeg: Adobe APP14 transform 0 (RGB stored without a colour transform) is not decoded")
    ids = [sof[6 + 3 * c] for c in range(ncomp)]
    samp = [(sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15) for c in range(ncomp)]
    tq = tuple(sof[8 + 3 * c] for c in range(ncomp))
    if ncomp == 1:
        hs, vs = 1, 1
    else:
        hs, vs = samp[0]
        if samp[0] not in ((1, 1), (2, 1), (2, 2)) or samp[1] != (1, 1) or samp[2] != (1, 1):
            raise ValueError(f"parse_jpeg: sampling factors {samp} are not decoded (luma 1x1, 2x1 or 2x2 with chroma 1x1)")
    if len(sos) < 1 or sos[0] != ncomp or len(sos) != 4 + 2 * sos[0]:
        raise ValueError("parse_jpeg: more than one scan (the scan does not interleave all components)")
    if [sos[1 + 2 * c] for c in range(ncomp)] != ids:
        raise ValueError("parse_jpeg: the scan's components are not the frame's in order")
    if tuple(sos[1 + 2 * ncomp:]) != (0, 63, 0):
        raise ValueError("parse_jpeg: the scan is not a full sequential one (Ss 0, Se 63, Ah / Al 0)")
    td = tuple(sos[2 + 2 * c] >> 4 for c in range(ncomp))
    ta = tuple(sos[2 + 2 * c] & 15 for c in range(ncomp))
    if not huffman:
        huffman = dict(ANNEX_K)
    for c in range(ncomp):
        if tq[c] not in qtables:
            raise ValueError(f"parse_jpeg: component {c} names quantiser table {tq[c]}, which no DQT defines")
        if (0, td[c]) not in huffman or (1, ta[c]) not in huffman:
            raise ValueError(f"parse_jpeg: component {c} names Huffman tables DC {td[c]} / AC {ta[c]}, which no DHT defines")
    h = JpegHeader(width, height, ncomp, hs, vs, tq, td, ta, qtables, huffman, ri, pos)

    # restart segments: inside entropy-coded data an 0xFF is followed only by 0x00, a marker or fill 0xFFs
    a = np.frombuffer(data, np.uint8, offset=pos)
    at = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] != 0) & (a[1:] != 0xFF)) if a.size > 1 else np.zeros(0, np.int64)
    marks = a[at + 1]
    eoi = np.flatnonzero(marks == 0xD9)
    other = np.flatnonzero((marks < 0xD0) | (marks > 0xD9))
    if other.size and (eoi.size == 0 or other[0] < eoi[0]):
        m = int(marks[other[0]])
        raise ValueError("parse_jpeg: more than one scan is not decoded" if m in (0xDA, 0xC4, 0xDB, 0xDD) else
                         f"parse_jpeg: unexpected marker {m:#04x} inside the scan")
    if eoi.size == 0:
        raise ValueError("parse_jpeg: missing EOI (the scan is truncated)")
    k = int(eoi[0])
    if k and ri == 0:
        raise ValueError("parse_jpeg: restart marker out of sequence (the file defines no restart interval)")
    if not np.array_equal(marks[:k], 0xD0 + (np.arange(k) & 7)):
        raise ValueError("parse_jpeg: restart marker out of sequence")
    need = -(-h.mcus // ri) if ri else 1
    if k + 1 != need:
        raise ValueError(f"parse_jpeg: the scan has {k + 1} restart intervals, {'fewer' if k + 1 < need else 'more'} than the frame's "
                         f"{h.mcus} MCUs need ({need})")
    starts = np.concatenate([[0], at[:k] + 2]) + pos
    ends = at[:k + 1] + pos
    h.segments = list(zip(starts.tolist(), ends.tolist()))
    return h


# ---- progressive files (SOF2) -----------------------------------------------------------------------------------------------------

# csrc/jpegprog_core.h's status words and scan descriptor
PROG_STATUS_TEXT = {1: "a Huffman code longer than 16 bits", 2: "a coefficient index past the scan's Se",
                    3: "a size category outside the scan type's range", 4: "an EOB run past the segment's last block",
                    5: "data exhausted before the last block", 6: "a segment or scan descriptor outside the batch"}
PROG_SCAN_INTS = 16


@dataclass
class JpegScan:
    comps: Tuple[int, ...]                       # component indices (positions in the frame header), in scan order
    ss: int                                      # spectral band [ss, se] in zigzag positions
    se: int
    ah: int                                      # successive approximation: 0 in a first scan, else the Al the band stood at; al: its new Al
    al: int
    restart_interval: int                        # the DRI in force at this SOS, in MCUs of THIS scan; 0 = none
    td: Tuple[int, ...]                          # per scan component: DC table id, AC table id
    ta: Tuple[int, ...]
    huffman: Dict[Tuple[int, int], Tuple[bytes, bytes]]      # the tables in force at this SOS: (class, id 0..3) -> (BITS, HUFFVAL)
    units: int                                   # MCUs of this scan: the frame's when it interleaves all components, else the component's own blocks
    level: int                                   # dependency level (scan_levels)
    segments: List[Tuple[int, int]] = field(default_factory=list)       # [start, end) of every restart segment, markers excluded


def scan_levels(scans) -> List[int]:
    """Dependency levels of a progressive file's scans, given as (components, Ss, Se) in file order: 0 for a scan that shares no (component,
    coefficient) pair with an earlier one, else 1 + the largest level among the earlier scans that do.  Scans of one level touch disjoint
    coefficients and may run in any order, after all scans of lower levels."""
    last, out = {}, []
    for comps, ss, se in scans:
        pairs = [(c, k) for c in comps for k in range(ss, se + 1)]
        level = 1 + max((last.get(p, -1) for p in pairs), default=-1)
        for p in pairs:
            last[p] = level
        out.append(level)
    return out


def _first_sof(data):
    """The marker of the file's first frame header (0xC0 .. 0xCF without DHT / JPG / DAC), or None: a walk over the header segments only."""
    pos, n = 2, len(data)
    while pos + 4 <= n and data[pos] == 0xFF:
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return None
        m = data[pos]
        pos += 1
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m
        if m in (0xD9, 0xDA):
            return None
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        pos += int.from_bytes(data[pos:pos + 2], "big")
    return None


def _parse_progressive(data) -> JpegHeader:
    """parse_jpeg for a file whose frame header is SOF2: every scan with the tables and restart interval in force at its SOS."""
    n = len(data)
    a = np.frombuffer(data, np.uint8)
    marks_at = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] != 0) & (a[1:] != 0xFF))          # every 0xFF that a marker byte follows
    qtables, huffman, sof, ri, adobe, scans, pos = {}, {}, None, 0, None, [], 2
    geom = None                                                                           # set at the first SOS
    bits_at = {}                                                                          # (component, zigzag position) -> the Al it stands at
    while True:
        if pos + 2 > n:
            raise ValueError("parse_jpeg: missing EOI (the file ends after a scan)" if scans else
                             "parse_jpeg: missing SOS (the file ends in its headers)" if sof else "parse_jpeg: missing SOF (the file ends in its headers)")
        if data[pos] != 0xFF:
            raise ValueError(f"parse_jpeg: expected a marker at byte {pos}")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            continue
        m = data[pos]
        pos += 1
        if m == 0xD9:
            if not scans:
                raise ValueError("parse_jpeg: missing SOS (EOI before any scan)" if sof else "parse_jpeg: missing SOF (EOI before any frame header)")
            break
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            if scans:
                raise ValueError("parse_jpeg: restart marker out of sequence (between two scans)")
            continue
        if pos + 2 > n:
            continue
        length = int.from_bytes(data[pos:pos + 2], "big")
        body = data[pos + 2:pos + length]
        if length < 2 or pos + length > n:
            raise ValueError(f"parse_jpeg: segment {m:#04x} at byte {pos - 2} runs past the end of the file")
        pos += length
        if m == 0xDB:
            if scans:
                raise ValueError("parse_jpeg: a DQT after the first scan of a progressive file is not decoded (the library latches a component's "
                                 "quantiser at that component's first scan)")
            k = 0
            while k < len(body):
                pq, tid = body[k] >> 4, body[k] & 15
                if pq != 0:
                    raise ValueError("parse_jpeg: 16-bit quantiser tables are not decoded (8-bit DQT only)")
                if tid > 3 or k + 65 > len(body):
                    raise ValueError("parse_jpeg: bad DQT segment")
                q = np.zeros(64, np.int32)
                q[ZIGZAG] = np.frombuffer(body[k + 1:k + 65], np.uint8)
                qtables[tid] = q
                k += 65
        elif m == 0xC2:
            if sof is not None:
                raise ValueError("parse_jpeg: more than one SOF")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError("parse_jpeg: bad SOF2 segment")
            sof = body
        elif m == 0xC0:
            raise ValueError("parse_jpeg: more than one SOF")
        elif m in _SOF_NAMES:
            raise ValueError(f"parse_jpeg: {_SOF_NAMES[m]} JPEG (SOF{m - 0xC0}) is not decoded")
        elif m == 0xDC:
            raise ValueError("parse_jpeg: a DNL segment (the number of lines defined after the first scan) is not decoded")
        elif m == 0xC4:
            k = 0
            while k < len(body):
                tc, th = body[k] >> 4, body[k] & 15
                if tc > 1 or th > 3 or k + 17 > len(body):
                    raise ValueError("parse_jpeg: bad DHT segment (classes 0 - 1, tables 0 - 3)")
                bits = body[k + 1:k + 17]
                cnt = sum(bits)
                vals = body[k + 17:k + 17 + cnt]
                _check_huffman(bits, vals, f"DHT table {tc}/{th}")
                huffman[(tc, th)] = (bits, vals)
                k += 17 + cnt
        elif m == 0xDD:
            if len(body) != 2:
                raise ValueError("parse_jpeg: bad DRI segment")
            ri = int.from_bytes(body, "big")
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            if sof is None:
                raise ValueError("parse_jpeg: missing SOF (SOS before any frame header)")
            if geom is None:
                geom = _progressive_frame(sof, adobe, qtables)
            width, height, ncomp, hs, vs, ids, tq = geom
            ns = body[0] if body else 0
            if ns < 1 or len(body) != 4 + 2 * ns:
                raise ValueError("parse_jpeg: bad SOS segment")
            try:
                comps = tuple(ids.index(body[1 + 2 * i]) for i in range(ns))
            except ValueError:
                raise ValueError(f"parse_jpeg: scan {len(scans)} names a component the frame does not have") from None
            td, ta = tuple(body[2 + 2 * i] >> 4 for i in range(ns)), tuple(body[2 + 2 * i] & 15 for i in range(ns))
            ss, se, ah, al = body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns] >> 4, body[3 + 2 * ns] & 15
            what = f"parse_jpeg: scan {len(scans)} (components {list(comps)}, Ss {ss}, Se {se}, Ah {ah}, Al {al})"
            if ss > se or se > 63 or (ss == 0 and se != 0) or al > 13 or (ah != 0 and al != ah - 1):
                raise ValueError(f"{what} is no legal progression (Ss <= Se <= 63, a DC scan has Se 0, Al <= 13, a refinement has Al = Ah - 1)")
            if ss > 0 and ns != 1:
                raise ValueError(f"{what} is no legal progression: an AC scan holds one component")
            if ns > 1 and comps != tuple(range(ncomp)):
                raise ValueError(f"{what}: a scan of several components that are not all of the frame's in order is not decoded")
            for c in comps:
                if ss > 0 and (c, 0) not in bits_at:
                    raise ValueError(f"{what} is no legal progression: an AC scan of component {c} before that component's DC first scan")
                for k in range(ss, se + 1):
                    cur = bits_at.get((c, k))
                    if cur is None and ah != 0:
                        raise ValueError(f"{what} is no legal progression: the first scan of coefficient {k} of component {c} has Ah != 0")
                    if cur is not None and ah == 0:
                        raise ValueError(f"{what} is no legal progression: coefficient {k} of component {c} is sent twice at the same precision")
                    if cur is not None and ah != cur:
                        raise ValueError(f"{what} is no legal progression: a refinement with Ah {ah} of coefficient {k} of component {c}, "
                                         f"which stands at Al {cur}")
                    bits_at[(c, k)] = al
            for i, c in enumerate(comps):
                need = [(0, td[i])] if ss == 0 and ah == 0 else [] if ss == 0 else [(1, ta[i])]
                for key in need:
                    if key[1] > 3 or key not in huffman:
                        raise ValueError(f"{what} names {'AC' if key[0] else 'DC'} Huffman table {key[1]}, which no DHT has defined by that point")
            if ns > 1:
                units = (-(-height // (8 * vs))) * (-(-width // (8 * hs)))
            else:
                wc, hc = (width, height) if comps[0] == 0 else (-(-width // hs), -(-height // vs))
                units = (-(-wc // 8)) * (-(-hc // 8))
            scan = JpegScan(comps, ss, se, ah, al, ri, td, ta, dict(huffman), units, 0)
            # the scan's entropy-coded data: up to the first marker that is no RSTn
            first = int(np.searchsorted(marks_at, pos))
            cand = a[marks_at[first:] + 1]
            stop = np.flatnonzero((cand < 0xD0) | (cand > 0xD7))
            if stop.size == 0:
                raise ValueError("parse_jpeg: missing EOI (a scan is truncated)")
            k = int(stop[0])
            if k and ri == 0:
                raise ValueError(f"{what}: restart marker out of sequence (no restart interval is in force)")
            if not np.array_equal(cand[:k], 0xD0 + (np.arange(k) & 7)):
                raise ValueError(f"{what}: restart marker out of sequence")
            need = -(-units // ri) if ri else 1
            if k + 1 != need:
                raise ValueError(f"{what} has {k + 1} restart intervals, {'fewer' if k + 1 < need else 'more'} than its {units} MCUs need ({need})")
            at = marks_at[first:first + k + 1]
            starts = np.concatenate([[pos], at[:k] + 2])
            scan.segments = list(zip(starts.tolist(), at.tolist()))
            scans.append(scan)
            pos = int(at[k])
        # APPn, COM and anything else with a length: skipped
    if geom is None:
        raise ValueError("parse_jpeg: missing SOS")
    width, height, ncomp, hs, vs, ids, tq = geom
    short = [(c, k, bits_at.get((c, k))) for c in range(ncomp) for k in range(64) if bits_at.get((c, k)) != 0]
    if short:
        c, k, cur = short[0]
        raise ValueError(f"parse_jpeg: the scans do not bring every coefficient to full precision (coefficient {k} of component {c} "
                         f"{'is never sent' if cur is None else f'stops at Al {cur}'}): the library decodes such a file with inter-block "
                         "smoothing of the missing precision, which is not decoded here")
    for s, level in zip(scans, scan_levels([(s.comps, s.ss, s.se) for s in scans])):
        s.level = level
    return JpegHeader(width, height, ncomp, hs, vs, tq, (0,) * ncomp, (0,) * ncomp, qtables, {}, 0, scans[0].segments[0][0], [], True, scans)


def _progressive_frame(sof, adobe, qtables):
    """The frame-level refusals of parse_jpeg on an SOF2 body -> (width, height, ncomp, hs, vs, component ids, quantiser ids)."""
    precision, height, width, ncomp = sof[0], int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big"), sof[5]
    if precision != 8:
        raise ValueError(f"parse_jpeg: {precision}-bit samples are not decoded (8-bit only)")
    if ncomp == 4:
        raise ValueError("parse_jpeg: four components (CMYK / YCCK) are not decoded")
    if ncomp not in (1, 3):
        raise ValueError(f"parse_jpeg: {ncomp} components are not decoded (one or three)")
    if height < 1 or width < 1:
        raise ValueError(f"parse_jpeg: frame size {width} x {height}")
    if adobe == 0 and ncomp == 3:
        raise ValueError("parse_jpeg: Adobe APP14 transform 0 (RGB stored without a colour transform) is not decoded")
    ids = [sof[6 + 3 * c] for c in range(ncomp)]
    if len(set(ids)) != ncomp:
        raise ValueError("parse_jpeg: two components of the frame share an identifier")
    samp = [(sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15) for c in range(ncomp)]
    tq = tuple(sof[8 + 3 * c] for c in range(ncomp))
    if ncomp == 1:
        hs, vs = 1, 1
    else:
        hs, vs = samp[0]
        if samp[0] not in ((1, 1), (2, 1), (2, 2)) or samp[1] != (1, 1) or samp[2] != (1, 1):
            raise ValueError(f"parse_jpeg: sampling factors {samp} are not decoded (luma 1x1, 2x1 or 2x2 with chroma 1x1)")
    for c in range(ncomp):
        if tq[c] not in qtables:
            raise ValueError(f"parse_jpeg: component {c} names quantiser table {tq[c]}, which no DQT defines")
    return width, height, ncomp, hs, vs, ids, tq


def prog_batch_operands(jpegs, headers):
    """Host-side operands of the progressive entropy stage for progressive files of one geometry (csrc/jpegprog_core.h):
    dict(data uint8 (bytes,), offsets int64 (nseg + 1,), seginfo int32 (nseg, 3) = (scan, first unit, end unit), scaninfo int32 (nscan,
    PROG_SCAN_INTS), huff int32 (nhuff, 307), tables int32 (n, TAB_INTS) for the idct launch, levels = the segment index at which each level starts
    (nlevels + 1,), where = per segment (frame, scan of that file, restart segment of that scan)).  The segments are sorted by level, so one
    level's launch takes a slice of offsets, seginfo and status.  Scans whose Huffman tables are equal share a table block."""
    blocks, scaninfo, segs = {}, [], []

    def block(table):
        return blocks.setdefault((bytes(table[0]), bytes(table[1])), len(blocks))

    for f, (j, h) in enumerate(zip(jpegs, headers)):
        for k, s in enumerate(h.scans):
            row = [0] * PROG_SCAN_INTS
            row[0], row[1] = f, len(s.comps)
            row[2:2 + len(s.comps)] = s.comps
            row[5:9] = s.ss, s.se, s.ah, s.al
            for i in range(len(s.comps)):
                if s.ss == 0 and s.ah == 0:
                    row[9 + i] = block(s.huffman[(0, s.td[i])])
            if s.ss > 0:
                row[12] = block(s.huffman[(1, s.ta[0])])
            step = s.restart_interval or s.units
            for r, (a, b) in enumerate(s.segments):
                segs.append((s.level, len(scaninfo), r * step, min((r + 1) * step, s.units), j[a:b], (f, k, r)))
            scaninfo.append(row)
    segs.sort(key=lambda t: t[0])                                             # stable: (frame, scan, segment) order within a level
    nlev = segs[-1][0] + 1
    levels = np.searchsorted(np.asarray([t[0] for t in segs]), np.arange(nlev + 1)).astype(np.int64)
    offsets = np.zeros(len(segs) + 1, np.int64)
    np.cumsum([len(t[4]) for t in segs], out=offsets[1:])
    if not blocks:                                                            # cannot happen for a parsed file (its first scan is a DC first scan)
        blocks[(bytes(16), b"")] = 0
    huff = np.stack([huffman_decode_arrays(bits, vals) for bits, vals in blocks])
    return dict(data=np.frombuffer(b"".join(t[4] for t in segs) or b"\0", np.uint8), offsets=offsets,
                seginfo=np.asarray([t[1:4] for t in segs], np.int32).reshape(-1, 3), scaninfo=np.asarray(scaninfo, np.int32).reshape(-1, PROG_SCAN_INTS),
                huff=huff, tables=np.stack([frame_tables(h) for h in headers]), levels=levels, where=[t[5] for t in segs])


def huffman_decode_arrays(bits, vals) -> np.ndarray:
    """BITS / HUFFVAL -> the int32 block of one table: MINCODE[0..16], MAXCODE[0..16] (-1: none), VALPTR[0..16] (T.81 F.2.2.3), HUFFVAL[0..255]."""
    out = np.zeros(_HUFF_INTS, np.int32)
    out[17:34] = -1
    code, k = 0, 0
    for length in range(1, 17):
        n = bits[length - 1]
        if n:
            out[length] = code
            out[34 + length] = k
            code += n
            k += n
            out[17 + length] = code - 1
        code <<= 1
    out[51:51 + len(vals)] = np.frombuffer(bytes(vals), np.uint8)
    return out


def frame_tables(h: JpegHeader) -> np.ndarray:
    """One frame's table block for the kernels (csrc/jpegdec_core.h)."""
    t = np.zeros(TAB_INTS, np.int32)
    for c in range(h.ncomp):
        t[c], t[3 + c], t[6 + c] = h.tq[c], h.td[c], h.ta[c]
    for tid, q in h.qtables.items():
        t[_TAB_Q + 64 * tid:_TAB_Q + 64 * tid + 64] = q
    for (tc, th), (bits, vals) in h.huffman.items():
        o = _TAB_HUFF + (2 * tc + th) * _HUFF_INTS
        t[o:o + _HUFF_INTS] = huffman_decode_arrays(bits, vals)
    return t


def batch_operands(jpegs, headers=None):
    """Host-side operands of one decode call: (headers, data uint8 (bytes,), offsets int64 (nseg + 1,), seginfo int32 (nseg, 3), tables int32
    (n, TAB_INTS)).  Segment s is data[offsets[s]:offsets[s + 1]] and holds the MCUs [seginfo[s, 1], seginfo[s, 2]) of frame seginfo[s, 0]."""
    jpegs = [bytes(j) for j in jpegs]
    headers = [parse_jpeg(j) for j in jpegs] if headers is None else headers
    if not headers:
        raise ValueError("decode_jpeg_frames: no frames")
    for k, h in enumerate(headers):
        if h.geometry != headers[0].geometry:
            raise ValueError(f"decode_jpeg_frames: frame {k} is {h.width} x {h.height}, {h.ncomp} components, luma sampling {h.hs}x{h.vs}; frame 0 is "
                             f"{headers[0].width} x {headers[0].height}, {headers[0].ncomp}, {headers[0].hs}x{headers[0].vs}: one call decodes one size")
    parts, sizes, info = [], [], []
    for f, (j, h) in enumerate(zip(jpegs, headers)):
        step = h.restart_interval or h.mcus
        for s, (a, b) in enumerate(h.segments):
            parts.append(j[a:b])
            sizes.append(b - a)
            info.append((f, s * step, min((s + 1) * step, h.mcus)))
    data = np.frombuffer(b"".join(parts) or b"\0", np.uint8)
    offsets = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    return headers, data, offsets, np.asarray(info, np.int32).reshape(-1, 3), np.stack([frame_tables(h) for h in headers])


def _same_geometry(headers):
    for k, h in enumerate(headers):
        if h.geometry != headers[0].geometry:
            raise ValueError(f"decode_jpeg_frames: frame {k} is {h.width} x {h.height}, {h.ncomp} components, luma sampling {h.hs}x{h.vs}; frame 0 is "
                             f"{headers[0].width} x {headers[0].height}, {headers[0].ncomp}, {headers[0].hs}x{headers[0].vs}: one call decodes one size")


def _decode_progressive(jpegs, headers, frames, dev, out=None):
    """Progressive files of one geometry -> (n, H, W, 3): one mmgt_jpegprog_entropy call per dependency level, then the baseline decoder's idct and
    colour launches on the same coefficient layout.  `frames`: the files' indices in the caller's batch, for the error text."""
    import torch
    from . import hip
    ops = prog_batch_operands(jpegs, headers)
    H, W, ncomp, hs, vs = headers[0].geometry
    fb, ti = hip.jpegdec_sizes(H, W, ncomp, hs, vs)
    if ti != TAB_INTS:
        raise RuntimeError(f"decode_jpeg_frames: the library's table block has {ti} words, this module builds {TAB_INTS}")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_data, d_offsets, d_seginfo, d_scaninfo, d_huff, d_tables = (up(ops[k].copy()) for k in ("data", "offsets", "seginfo", "scaninfo", "huff", "tables"))
    nseg = len(ops["seginfo"])
    coef = torch.empty((len(headers), fb, 64), device=dev, dtype=torch.int16)
    status = torch.empty((nseg,), device=dev, dtype=torch.int32)
    lv = ops["levels"].tolist()
    for level, (a, b) in enumerate(zip(lv[:-1], lv[1:])):
        hip.jpegprog_entropy(d_data, d_offsets[a:b + 1], d_seginfo[a:b], d_scaninfo, d_huff, coef, status[a:b], H, W, ncomp, hs, vs, zero_fill=level == 0)
    planes = hip.jpegdec_idct(coef, d_tables, H, W, ncomp, hs, vs)
    bad = torch.nonzero(status).flatten()[:1].cpu()                          # the one read of the status words (it also orders the launches)
    if bad.numel():
        s = int(bad[0])
        code = int(status[s])
        f, k, r = ops["where"][s]
        raise RuntimeError(f"decode_jpeg_frames: frame {frames[f]}, scan {k}, restart segment {r}: {PROG_STATUS_TEXT.get(code, f'status {code}')}")
    return hip.jpegdec_color(planes, H, W, ncomp, hs, vs, out=out)


def _decode_mixed(jpegs, dev, out):
    """decode_jpeg_frames(progressive=True): the batch split by kind, both kinds into the one output tensor."""
    import torch
    jpegs = [bytes(j) for j in jpegs]
    headers = [parse_jpeg(j, progressive=True) for j in jpegs]
    if not headers:
        raise ValueError("decode_jpeg_frames: no frames")
    _same_geometry(headers)
    prog = [k for k, h in enumerate(headers) if h.progressive]
    base = [k for k, h in enumerate(headers) if not h.progressive]
    if not prog:
        return _decode_baseline(batch_operands(jpegs, headers), dev, out)
    if not base:
        return _decode_progressive(jpegs, headers, prog, dev, out)
    H, W = headers[0].height, headers[0].width
    shape = (len(headers), H, W, 3)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"decode_jpeg_frames: out must be contiguous uint8 {shape} on {dev}")
    a = _decode_baseline(batch_operands([jpegs[k] for k in base], [headers[k] for k in base]), dev, None, base)
    b = _decode_progressive([jpegs[k] for k in prog], [headers[k] for k in prog], prog, dev)
    out[torch.as_tensor(base, device=dev)] = a
    out[torch.as_tensor(prog, device=dev)] = b
    return out


def decode_jpeg_frames(jpegs, device="cuda", out=None, progressive=False):
    """n baseline JPEG files of one size and sampling (quantiser and Huffman tables may differ per frame) -> (n, H, W, 3) uint8 RGB on `device`,
    contiguous; a greyscale file gives Y in all three channels (what Image.convert("RGB") gives).  `out`: a tensor of that shape to write into.
    Out-of-scope files raise ValueError before anything is launched; entropy-coded data that does not decode raises RuntimeError naming the
    first bad frame and segment (the status words are read once per call), and no pixels are returned.  With progressive=True the batch may hold
    progressive files (SOF2), baseline files or both: a progressive file's scans fill the same coefficient buffer through csrc/jpegprog.hip, one
    launch per dependency level of its scan script, and the rest of the decode is the baseline one."""
    import torch
    if progressive:
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return _decode_mixed(jpegs, dev, out)
    return _decode_baseline(batch_operands(jpegs), torch.device(device), out)


def _decode_baseline(operands, dev, out, frames=None):
    import torch
    from . import hip
    headers, data, offsets, seginfo, tables = operands
    H, W, ncomp, hs, vs = headers[0].geometry
    fb, ti = hip.jpegdec_sizes(H, W, ncomp, hs, vs)
    if ti != TAB_INTS:
        raise RuntimeError(f"decode_jpeg_frames: the library's table block has {ti} words, this module builds {TAB_INTS}")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_data, d_tables = up(data.copy()), up(tables)
    coef, status = hip.jpegdec_entropy(d_data, up(offsets), up(seginfo), d_tables, len(headers), H, W, ncomp, hs, vs)
    planes = hip.jpegdec_idct(coef, d_tables, H, W, ncomp, hs, vs)
    bad = torch.nonzero(status).flatten()[:1].cpu()                          # the one read of the status words (it also orders the launches)
    if bad.numel():
        s = int(bad[0])
        code = int(status[s])
        f = int(seginfo[s, 0])
        raise RuntimeError(f"decode_jpeg_frames: frame {f if frames is None else frames[f]}, restart segment {s - int(np.searchsorted(seginfo[:, 0], f))}: "
                           f"{STATUS_TEXT.get(code, f'status {code}')}")
    return hip.jpegdec_color(planes, H, W, ncomp, hs, vs, out=out)


# ---------------------------------------------------------------------------------------------------------------- PNG / APNG

PNGDEC_SCRATCH_BYTES = 256 << 20    # decode_png_frames holds at most this much filtered rows and row sums per set of launches

# csrc/pngdec_core.h's status words
PNG_STATUS_TEXT = {1: "an over-subscribed Huffman code", 2: "an incomplete Huffman code", 3: "an invalid symbol", 4: "a distance beyond the bytes produced",
                   5: "a stored block whose LEN and NLEN do not match", 6: "data exhausted before the final block's end",
                   7: "more image data than the frame holds (output too long)", 8: "less image data than the frame holds (output too short)",
                   9: "a bad code-length repeat", 10: "more than 286 literal/length or 30 distance codes", 11: "a code without an end-of-block symbol",
                   12: "block type 3", 13: "a stream descriptor outside the batch", 14: "a scanline filter type above 4",
                   15: "a palette index beyond PLTE"}

_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


@dataclass
class PngHeader:
    width: int
    height: int
    colour_type: int                             # 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA
    bit_depth: int
    palette: Optional[np.ndarray]                # (entries, 3) uint8 for colour type 3
    streams: List[bytes] = field(default_factory=list)       # per frame: the raw deflate bytes (IDAT / fdAT payloads joined, zlib header and trailer cut)
    adlers: List[int] = field(default_factory=list)          # per frame: the zlib trailer, the Adler-32 its filtered bytes must have
    animated: bool = False                       # acTL present: the frames are the animation's
    plays: int = 0

    @property
    def geometry(self):
        return self.height, self.width, self.colour_type, self.bit_depth

    @property
    def stride(self):
        """Bytes of one filtered scanline: the filter type and ceil(W * bits per pixel / 8)."""
        return 1 + (self.width * _PNG_CHANNELS[self.colour_type] * self.bit_depth + 7) // 8


def _zlib_range(stream: bytes, what: str):
    """One frame's zlib stream -> (raw deflate bytes, expected Adler-32)."""
    if len(stream) < 6:
        raise ValueError(f"parse_png: bad zlib header ({what} holds {len(stream)} bytes: no room for header and trailer)")
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31 or flg & 0x20:
        raise ValueError(f"parse_png: bad zlib header {cmf:#04x} {flg:#04x} in {what} (CM 8, CINFO <= 7, no FDICT, FCHECK)")
    return stream[2:-4], int.from_bytes(stream[-4:], "big")


def parse_png(data) -> PngHeader:
    """One PNG / APNG file (bytes) -> PngHeader.  Every chunk's CRC-32 is verified.  ValueError for everything outside the decoder's scope: bit depth
    16, Adam7 interlace, APNG frames that are not full size at (0, 0) or that blend OVER where the image has transparency, a default image outside
    the animation, missing IHDR / PLTE / IDAT / IEND, a bad CRC, a bad zlib header, an unknown critical chunk."""
    import zlib
    data = bytes(data)
    if data[:8] != _PNG_SIG:
        raise ValueError("parse_png: not a PNG file (bad signature)")
    pos, n = 8, len(data)
    ihdr = palette = actl = None
    idat, frames, ctl, seq, trns, ended = [], [], [], 0, False, False          # frames: [fcTL or None, [payloads]]
    while pos < n:
        if pos + 12 > n:
            raise ValueError(f"parse_png: a chunk header at byte {pos} runs past the end of the file" + ("" if ihdr else " (missing IHDR)"))
        length, kind = int.from_bytes(data[pos:pos + 4], "big"), data[pos + 4:pos + 8]
        if pos + 12 + length > n:
            raise ValueError(f"parse_png: chunk {kind!r} at byte {pos} runs past the end of the file (missing IEND)")
        body = data[pos + 8:pos + 8 + length]
        if zlib.crc32(data[pos + 4:pos + 8 + length]) != int.from_bytes(data[pos + 8 + length:pos + 12 + length], "big"):
            raise ValueError(f"parse_png: bad CRC in chunk {kind!r} at byte {pos}")
        pos += 12 + length
        if ihdr is None and kind != b"IHDR":
            raise ValueError(f"parse_png: missing IHDR (the first chunk is {kind!r})")
        if kind == b"IHDR":
            if ihdr is not None or length != 13:
                raise ValueError("parse_png: bad IHDR chunk")
            ihdr = body
        elif kind == b"PLTE":
            if length % 3 or not 3 <= length <= 768 or idat:
                raise ValueError("parse_png: bad PLTE chunk")
            palette = np.frombuffer(body, np.uint8).reshape(-1, 3).copy()
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            break
        elif kind == b"tRNS":
            trns = True                                                           # ignored, as Image.convert("RGB") ignores it
        elif kind == b"acTL" and length == 8 and not idat:
            actl = (int.from_bytes(body[:4], "big"), int.from_bytes(body[4:], "big"))
        elif kind == b"fcTL" and actl is not None:
            if length != 26 or int.from_bytes(body[:4], "big") != seq:
                raise ValueError("parse_png: bad fcTL chunk (its length or sequence number)")
            seq += 1
            if not frames and idat:
                raise ValueError("parse_png: an APNG whose default image is not its first frame is not decoded")
            frames.append([body, idat if not frames else []])
        elif kind == b"fdAT" and actl is not None:
            if length < 4 or int.from_bytes(body[:4], "big") != seq or not frames or frames[-1][1] is idat:
                raise ValueError("parse_png: bad fdAT chunk (its sequence number or place)")
            seq += 1
            frames[-1][1].append(body[4:])
        elif not kind[0] & 0x20:
            raise ValueError(f"parse_png: unknown critical chunk {kind!r}")
        # every other ancillary chunk: skipped
    if ihdr is None:
        raise ValueError("parse_png: missing IHDR")
    if not ended:
        raise ValueError("parse_png: missing IEND")
    W, H = int.from_bytes(ihdr[:4], "big"), int.from_bytes(ihdr[4:8], "big")
    depth, ct, comp, filt, lace = ihdr[8:13]
    if lace == 1:
        raise ValueError("parse_png: Adam7 interlace is not decoded")
    if depth == 16 and ct in _PNG_CHANNELS:
        raise ValueError("parse_png: bit depth 16 is not decoded (1, 2, 4 or 8 bits)")
    if ct not in _PNG_CHANNELS or depth not in ((1, 2, 4, 8) if ct in (0, 3) else (8,)) or comp or filt or lace:
        raise ValueError(f"parse_png: bad IHDR (colour type {ct}, bit depth {depth}, compression {comp}, filter {filt}, interlace {lace})")
    if not (1 <= W <= PNG_MAX_SIDE and 1 <= H <= PNG_MAX_SIDE):
        raise ValueError(f"parse_png: a frame is 1 .. {PNG_MAX_SIDE} pixels a side, got {W} x {H}")
    if ct == 3 and palette is None:
        raise ValueError("parse_png: a palette image without PLTE")
    if not idat:
        raise ValueError("parse_png: missing IDAT")
    h = PngHeader(W, H, ct, depth, palette if ct == 3 else None)
    if actl is None:
        frames = [[None, idat]]
    else:
        h.animated, h.plays = True, actl[1]
        if not frames or frames[0][1] is not idat:
            raise ValueError("parse_png: an APNG whose default image is not its first frame is not decoded")
        if len(frames) != actl[0]:
            raise ValueError(f"parse_png: acTL announces {actl[0]} frames, the file holds {len(frames)}")
    for k, (fctl, parts) in enumerate(frames):
        if fctl is not None:
            fw, fh, fx, fy = (int.from_bytes(fctl[4 + 4 * i:8 + 4 * i], "big") for i in range(4))
            dispose, blend = fctl[24], fctl[25]
            if (fw, fh, fx, fy) != (W, H, 0, 0):
                raise ValueError(f"parse_png: APNG sub-rectangle frames are not decoded (frame {k} is {fw} x {fh} at ({fx}, {fy}) of {W} x {H})")
            if dispose > 2 or blend > 1:
                raise ValueError(f"parse_png: bad fcTL chunk (dispose {dispose}, blend {blend})")
            if blend == 1 and k > 0 and (ct in (4, 6) or trns):
                raise ValueError(f"parse_png: APNG blend OVER on an image with transparency is not decoded (frame {k}): the frame shown is composed "
                                 "from the one before")
        if not parts:
            raise ValueError(f"parse_png: missing IDAT (frame {k} has no image data)")
        raw, adler = _zlib_range(b"".join(parts), f"frame {k}" if h.animated else "IDAT")
        h.streams.append(raw)
        h.adlers.append(adler)
    return h


def png_batch_operands(pngs, headers=None):
    """Host-side operands of one decode call: (headers, geometry (H, W, colour type, depth), data uint8 (bytes,) padded to a multiple of 16, offsets int64
    (n + 1,), adlers (n,), palette uint8 (n, 256, 3) or None, plte_len int32 (n,)).  Every frame of every file counts: n = all frames in order."""
    headers = [parse_png(b) for b in pngs] if headers is None else headers
    if not headers:
        raise ValueError("decode_png_frames: no frames")
    g0 = headers[0]
    for k, h in enumerate(headers):
        if h.geometry != g0.geometry:
            raise ValueError(f"decode_png_frames: file {k} is {h.width} x {h.height}, colour type {h.colour_type} at {h.bit_depth} bits; file 0 is "
                             f"{g0.width} x {g0.height}, colour type {g0.colour_type} at {g0.bit_depth} bits: one call decodes one geometry")
    streams = [s for h in headers for s in h.streams]
    adlers = np.asarray([a for h in headers for a in h.adlers], np.int64)
    offsets = np.zeros(len(streams) + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=offsets[1:])
    blob = b"".join(streams)
    data = np.frombuffer(blob + bytes(16 + (-len(blob)) % 16), np.uint8)
    palette = plte_len = None
    if g0.colour_type == 3:
        palette = np.zeros((len(streams), 256, 3), np.uint8)
        plte_len = np.zeros(len(streams), np.int32)
        f = 0
        for h in headers:
            for _ in h.streams:
                palette[f, :len(h.palette)] = h.palette
                plte_len[f] = len(h.palette)
                f += 1
    return headers, g0.geometry, data, offsets, adlers, palette, plte_len


def adler32_of_row_sums(sums, stride) -> np.ndarray:
    """sums (n, H, 2) = per filtered scanline { sum d[i], sum (stride - i) d[i] } -> (n,) the Adler-32 of each frame's H * stride bytes: what folding
    video_out.adler32_combine over the rows' own Adler-32s gives, in one numpy expression."""
    s = np.asarray(sums, np.int64) % _ADLER
    n, H, _ = s.shape
    after = (np.arange(H - 1, -1, -1, dtype=np.int64) * (stride % _ADLER)) % _ADLER           # bytes behind each row, mod 65521
    a = (1 + s[:, :, 0].sum(axis=1)) % _ADLER
    b = ((H * stride) % _ADLER + ((s[:, :, 1] + after[None] * s[:, :, 0]) % _ADLER).sum(axis=1)) % _ADLER
    return b << 16 | a


def decode_png_frames(pngs, device="cuda", out=None):
    """PNG / APNG files (bytes each) of one size, colour type and bit depth (palettes may differ per file) -> (n, H, W, 3) uint8 RGB on `device`,
    contiguous, n = all frames of all files in order: byte for byte Image.open(f).convert("RGB") (grey of 1 / 2 / 4 bits scaled to 0 .. 255, alpha
    dropped, tRNS ignored, palette entries copied).  `out`: a tensor of that shape to write into.  Out-of-scope files raise ValueError before
    anything is launched.  Image data that does not inflate, a filter type above 4, an Adler-32 that differs from the stream's trailer or a palette
    index beyond PLTE raise RuntimeError naming the first bad frame (the status words and row sums are read once per call); no pixels are returned."""
    return _decode_png_operands(png_batch_operands(pngs), device, out)


def _decode_png_operands(operands, device, out=None):
    import torch
    from . import hip
    headers, (H, W, ct, depth), data, offsets, adlers, palette, plte_len = operands
    n, stride = len(adlers), headers[0].stride
    dev = torch.device(device)
    if out is None:
        out = torch.empty((n, H, W, 3), device=dev, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError(f"decode_png_frames: out must be contiguous uint8 ({n}, {H}, {W}, 3) on the device")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_data, d_off = up(data.copy()), up(offsets)
    d_pal, d_len = (up(palette), up(plte_len)) if ct == 3 else (None, None)
    status = torch.empty((3, n), device=dev, dtype=torch.int32)
    sums = torch.empty((n, H, 2), device=dev, dtype=torch.int64)
    per_call = max(1, PNGDEC_SCRATCH_BYTES // (H * stride + 16 * H))
    for f0 in range(0, n, per_call):
        f1 = min(n, f0 + per_call)
        filt, _ = hip.png_inflate(d_data, d_off[f0:f1 + 1], H * stride, out=(None, status[0, f0:f1]))
        hip.png_unfilter(filt, H, W, ct, depth, out=(sums[f0:f1], status[1, f0:f1]))
        hip.png_expand(filt, H, W, ct, depth, d_pal[f0:f1] if ct == 3 else None, d_len[f0:f1] if ct == 3 else None, out=(out[f0:f1], status[2, f0:f1]))
    st = status.cpu().numpy()                                                  # the one read of the status words (it also orders the launches)
    for stage, name in ((0, "image data"), (1, "scanlines")):
        bad = np.flatnonzero(st[stage])
        if bad.size:
            f = int(bad[0])
            raise RuntimeError(f"decode_png_frames: frame {f}, {name}: {PNG_STATUS_TEXT.get(int(st[stage, f]), f'status {int(st[stage, f])}')}")
    got = adler32_of_row_sums(sums.cpu().numpy(), stride)
    bad = np.flatnonzero(got != adlers)
    if bad.size:
        f = int(bad[0])
        raise RuntimeError(f"decode_png_frames: frame {f}: the image data's Adler-32 is {int(got[f]):#010x}, the stream's trailer says {int(adlers[f]):#010x}")
    bad = np.flatnonzero(st[2])
    if bad.size:
        f = int(bad[0])
        raise RuntimeError(f"decode_png_frames: frame {f}, pixels: {PNG_STATUS_TEXT.get(int(st[2, f]), f'status {int(st[2, f])}')}")
    return out


# ---------------------------------------------------------------------------------------------------------------- GIF

GIFDEC_SCRATCH_BYTES = 256 << 20    # decode_gif_frames holds at most this many palette indices per set of launches (one frame at least)
GIF_MAX_SIDE = 16384

# csrc/gifdec_core.h's status words
GIF_STATUS_TEXT = {1: "a code above the next free one", 2: "a first code after a clear that is not a literal",
                   3: "the image data ends before the frame's pixels are complete", 4: "a frame descriptor outside the batch"}

# csrc/gifdec_core.h's table row (checked against the binding's GIFDEC_TAB on every call)
_GD_X, _GD_Y, _GD_W, _GD_H, _GD_IDX, _GD_BEGIN, _GD_END, _GD_MCS, _GD_LACE, _GD_TRANS, _GD_MODE, _GD_COLOUR, _GD_FIRST, _GD_FILL = range(14)
GIF_TAB = 16


@dataclass
class GifFrame:
    x: int
    y: int
    width: int
    height: int
    interlace: bool
    min_code_size: int                           # 2 .. 8
    transparent: Optional[int]                   # the graphic control extension's transparent index, or None
    disposal: int                                # the graphic control extension's disposal bits as they stand in the file (0 without one)
    palette: np.ndarray                          # (256, 3) uint8: the local colour table, else the global one, zero padded
    colours: int                                 # entries of that table
    lzw: bytes                                   # the code stream, sub-block framing removed


@dataclass
class GifHeader:
    width: int                                   # the logical screen
    height: int
    background: int                              # the screen descriptor's background index; 0 in a file without a global colour table
    frames: List[GifFrame] = field(default_factory=list)


def parse_gif(data) -> GifHeader:
    """One GIF87a / GIF89a file (bytes) -> GifHeader.  Graphic control extensions are read, every other extension is skipped; bytes that open no
    block are skipped as PIL skips them, and a file that ends without a trailer after its last complete image is taken as PIL takes it.  ValueError
    for everything outside the decoder's scope: a bad signature, a block or sub-block that runs past the end of the file, a missing trailer before
    any image, a frame without a colour table, a frame rectangle that is empty or leaves the logical screen, a minimum code size outside 2 .. 8, a
    screen outside 1 .. 16384 a side, no frames."""
    data = bytes(data)
    n = len(data)
    if data[:6] not in (b"GIF87a", b"GIF89a"):
        raise ValueError("parse_gif: not a GIF file (bad signature)")
    if n < 13:
        raise ValueError("parse_gif: the logical screen descriptor runs past the end of the file")
    W, H = int.from_bytes(data[6:8], "little"), int.from_bytes(data[8:10], "little")
    packed = data[10]
    background = data[11] if packed & 0x80 else 0                             # PIL reads the background index only beside a global colour table
    if not (1 <= W <= GIF_MAX_SIDE and 1 <= H <= GIF_MAX_SIDE):
        raise ValueError(f"parse_gif: a screen is 1 .. {GIF_MAX_SIDE} pixels a side, got {W} x {H}")
    pos = 13

    def table(flags, what):
        nonlocal pos
        entries = 2 << (flags & 7)
        if pos + 3 * entries > n:
            raise ValueError(f"parse_gif: {what} runs past the end of the file")
        t = np.zeros((256, 3), np.uint8)
        t[:entries] = np.frombuffer(data, np.uint8, 3 * entries, pos).reshape(entries, 3)
        pos += 3 * entries
        return t, entries

    def sub_blocks(what):
        nonlocal pos
        parts = []
        while True:
            if pos >= n:
                raise ValueError(f"parse_gif: a sub-block of {what} runs past the end of the file (no block terminator)")
            size = data[pos]
            if pos + 1 + size > n:
                raise ValueError(f"parse_gif: a sub-block of {what} runs past the end of the file")
            parts.append(data[pos + 1:pos + 1 + size])
            pos += 1 + size
            if size == 0:
                return parts[:-1]

    gtable = table(packed, "the global colour table") if packed & 0x80 else None
    h = GifHeader(W, H, background)
    control, ended = None, False                                              # the graphic control extension waiting for its image
    while pos < n:
        kind = data[pos]
        pos += 1
        if kind == 0x3B:
            ended = True
            break
        if kind == 0x21:
            if pos >= n:
                raise ValueError("parse_gif: an extension block runs past the end of the file")
            label = data[pos]
            pos += 1
            parts = sub_blocks(f"extension {label:#04x}")
            if label == 0xF9 and parts and len(parts[0]) >= 4:
                control = ((parts[0][0] >> 2) & 7, parts[0][3] if parts[0][0] & 1 else None)
        elif kind == 0x2C:
            k = len(h.frames)
            if pos + 9 > n:
                raise ValueError(f"parse_gif: the image descriptor of frame {k} runs past the end of the file")
            x, y, w, hh = (int.from_bytes(data[pos + 2 * i:pos + 2 * i + 2], "little") for i in range(4))
            flags = data[pos + 8]
            pos += 9
            ltable = table(flags, f"the local colour table of frame {k}") if flags & 0x80 else gtable
            if ltable is None:
                raise ValueError(f"parse_gif: frame {k} has neither a local nor a global colour table (a greyscale GIF is not decoded)")
            if w == 0 or hh == 0:
                raise ValueError(f"parse_gif: frame {k} has an empty rectangle ({w} x {hh})")
            if x + w > W or y + hh > H:
                raise ValueError(f"parse_gif: the rectangle of frame {k} ({w} x {hh} at ({x}, {y})) leaves the logical screen ({W} x {H}): a canvas "
                                 "that grows is not decoded")
            if pos >= n:
                raise ValueError(f"parse_gif: the image data of frame {k} runs past the end of the file")
            mcs = data[pos]
            pos += 1
            if not 2 <= mcs <= 8:
                raise ValueError(f"parse_gif: frame {k} has minimum code size {mcs} (2 .. 8)")
            lzw = b"".join(sub_blocks(f"the image data of frame {k}"))
            disposal, transparent = control if control is not None else (0, None)
            h.frames.append(GifFrame(x, y, w, hh, bool(flags & 0x40), mcs, transparent, disposal, ltable[0], ltable[1], lzw))
            control = None
        # any other byte: skipped
    if not h.frames:
        raise ValueError("parse_gif: no frames" if ended else "parse_gif: missing trailer (the file ends before any image)")
    return h


def gif_operands(h: GifHeader, limit: Optional[int] = None, scratch_bytes: Optional[int] = None):
    """Host-side operands of one decode: (tab int64 (n, 16), palette uint8 (n, 256, 3), data uint8 (bytes,) padded to a multiple of 16, chunks
    [(f0, f1, idx_bytes)]).  n = the file's first `limit` frames; the chunks are runs of frames whose palette indices together fit scratch_bytes (one
    frame at least), and a row's index offset counts from its chunk's start.  The composition rules that need more than the frame itself (the sticky
    disposal, the colours of the first frame's canvas and of a restore to background) are resolved here."""
    frames = h.frames if limit is None else h.frames[:max(0, int(limit))]
    if not frames:
        raise ValueError("decode_gif_frames: no frames")
    budget = GIFDEC_SCRATCH_BYTES if scratch_bytes is None else int(scratch_bytes)
    rgb = lambda c: int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16
    tab = np.zeros((len(frames), GIF_TAB), np.int64)
    palette = np.stack([f.palette for f in frames])
    chunks, begin, sticky, f0, at = [], 0, 0, 0, 0
    for k, f in enumerate(frames):
        npix = f.width * f.height
        if k > f0 and at + npix > budget:
            chunks.append((f0, k, at))
            f0, at = k, 0
        sticky = f.disposal or sticky                                         # bits 0 inherit the last disposal the file named
        t = tab[k]
        t[_GD_X], t[_GD_Y], t[_GD_W], t[_GD_H], t[_GD_IDX] = f.x, f.y, f.width, f.height, at
        t[_GD_BEGIN], t[_GD_END], t[_GD_MCS], t[_GD_LACE] = begin, begin + len(f.lzw), f.min_code_size, int(f.interlace)
        t[_GD_TRANS] = -1 if f.transparent is None else f.transparent
        t[_GD_FIRST] = int(k == 0)
        if k == 0:
            t[_GD_FILL] = rgb(f.palette[f.transparent if f.transparent is not None else 0])
        if sticky == 2:
            index = f.transparent if f.transparent is not None else h.background
            t[_GD_MODE], t[_GD_COLOUR] = 2, rgb(f.palette[index if k == 0 or index < f.colours else 0])
        elif sticky >= 3:
            if k > 0:
                t[_GD_MODE] = 3
            elif f.transparent is not None:                                   # the first frame has no earlier canvas: its transparent colour, else nothing
                t[_GD_MODE], t[_GD_COLOUR] = 2, rgb(f.palette[f.transparent])
        at += npix
        begin += len(f.lzw)
    chunks.append((f0, len(frames), at))
    blob = b"".join(f.lzw for f in frames)
    data = np.frombuffer(blob + bytes(16 + (-len(blob)) % 16), np.uint8)
    return tab, palette, data, chunks


def decode_gif_frames(data, device="cuda", out=None, limit=None):
    """One GIF file (bytes) -> (n, H, W, 3) uint8 RGB on `device`, contiguous, n = its frames (the first `limit` of them; later ones are neither
    un-LZW'd nor composed): byte for byte what PIL's ImageSequence.Iterator(Image.open(f)) gives after convert("RGB") -- sub-rectangles, local
    palettes, transparency, interlace and the four disposals composed as PIL composes them.  `out`: a tensor of that shape to write into.  Out-of-scope
    files raise ValueError before anything is launched; a code stream that does not decode raises RuntimeError naming the first bad frame (the
    status words are read once per call), and no pixels are returned."""
    import torch
    from . import hip
    h = parse_gif(data)
    tab, palette, blob, chunks = gif_operands(h, limit)
    if hip.GIFDEC_TAB != GIF_TAB:
        raise RuntimeError(f"decode_gif_frames: the binding's table row has {hip.GIFDEC_TAB} words, this module builds {GIF_TAB}")
    n, H, W = len(tab), h.height, h.width
    dev = torch.device(device)
    if out is None:
        out = torch.empty((n, H, W, 3), device=dev, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError(f"decode_gif_frames: out must be contiguous uint8 ({n}, {H}, {W}, 3) on the device")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_data, d_tab, d_pal = up(blob.copy()), up(tab), up(palette)
    status = torch.empty((n,), device=dev, dtype=torch.int32)
    idx = torch.empty((max(c[2] for c in chunks),), device=dev, dtype=torch.uint8)
    carry = torch.empty((2, H, W, 3), device=dev, dtype=torch.uint8)          # canvas and pending restore, from one chunk to the next
    for f0, f1, idx_bytes in chunks:
        hip.gif_unlzw(d_data, d_tab[f0:f1], idx_bytes, out=(idx[:idx_bytes], status[f0:f1]))
        hip.gif_compose(d_tab[f0:f1], idx[:idx_bytes], d_pal[f0:f1], carry, H, W, out=out[f0:f1])
    st = status.cpu().numpy()                                                  # the one read of the status words (it also orders the launches)
    bad = np.flatnonzero(st)
    if bad.size:
        f = int(bad[0])
        raise RuntimeError(f"decode_gif_frames: frame {f}, image data: {GIF_STATUS_TEXT.get(int(st[f]), f'status {int(st[f])}')}")
    return out

# ---------------------------------------------------------------------------------------------------------------- WebP lossless

WEBPDEC_SCRATCH_BYTES = 256 << 20   # decode_webp_frames holds at most this much scratch and ARGB words per set of launches (one frame at least)
WEBPDEC_GROUP_BYTES = 1 << 20       # of a frame's scratch, at most this much is set aside AT FIRST for prefix-code groups beyond the first; a frame
                                    # that needs more says how much, and the call is run again with exactly that
WEBP_MAX_SIDE = 16384

# csrc/webpdec_core.h's status words
WEBP_STATUS_TEXT = {1: "a VP8L signature other than 0x2f or a version other than 0", 2: "a VP8L size that differs from the frame's rectangle",
                    3: "a transform read twice", 4: "a prefix code that is over-subscribed, incomplete or empty",
                    5: "a symbol outside its alphabet, or bits that are no code", 6: "a code-length repeat or max_symbol past the alphabet",
                    7: "colour-cache bits outside 1 .. 11", 8: "a distance beyond the pixels produced", 9: "a copy that runs past the image",
                    10: "data exhausted before the last pixel", 11: "more sub-images or prefix-code groups than the frame's scratch holds",
                    12: "a frame descriptor outside the batch", 13: "no decoded image to undo the transforms of"}

# csrc/webpdec_core.h's table row (checked against the binding's WEBPDEC_TAB on every call)
_WD_X, _WD_Y, _WD_W, _WD_H, _WD_BEGIN, _WD_END, _WD_SCR, _WD_CAP, _WD_PIX, _WD_FLAGS, _WD_PX, _WD_PY, _WD_PW, _WD_PH = range(14)
_WD_BLEND, _WD_KEY, _WD_FIRST, _WD_PREV_DISPOSED = 1, 2, 4, 8
WEBP_TAB = 16
_WD_HDR_WORDS = 32


@dataclass
class WebpFrame:
    x: int
    y: int
    width: int
    height: int
    duration: int                                # milliseconds; 0 for a still
    blend: bool                                  # ANMF flag bit 1 clear
    dispose: bool                                # ANMF flag bit 0: the rectangle is zeroed before the next frame draws
    alpha_is_used: bool                          # the VP8L header's bit
    key: bool                                    # libwebp's key frame: the canvas is zeroed before it draws, and it does not blend
    payload: bytes                               # the VP8L chunk's body (of a lossy frame: the `VP8 ` chunk's, with its padding byte if it has one)
    lossy: bool = False                          # a VP8 key frame (parse_webp(lossy=True) only)


@dataclass
class WebpHeader:
    width: int                                   # the canvas
    height: int
    loop: int
    animated: bool
    frames: List[WebpFrame] = field(default_factory=list)


def _vp8l_header(payload, what):
    if len(payload) < 5:
        raise ValueError(f"parse_webp: the VP8L chunk of {what} holds {len(payload)} bytes: no room for its header")
    v = int.from_bytes(payload[:5], "little")
    if v & 255 != 0x2F:
        raise ValueError(f"parse_webp: bad VP8L signature {v & 255:#04x} in {what} (0x2f)")
    if v >> 37 & 7:
        raise ValueError(f"parse_webp: bad VP8L version {v >> 37 & 7} in {what} (0)")
    return (v >> 8 & 0x3FFF) + 1, (v >> 22 & 0x3FFF) + 1, bool(v >> 36 & 1)


def _vp8_header(payload, what):
    """The 10-byte frame header of a `VP8 ` chunk -> (width, height); everything libwebp refuses there is refused here."""
    if len(payload) < 10:
        raise ValueError(f"parse_webp: the VP8 chunk of {what} holds {len(payload)} bytes: no room for its frame header")
    tag = int.from_bytes(payload[:3], "little")
    if tag & 1:
        raise ValueError(f"parse_webp: the VP8 chunk of {what} is not a key frame (inter frames are not decoded)")
    if tag >> 1 & 7 > 3:
        raise ValueError(f"parse_webp: bad VP8 profile {tag >> 1 & 7} in {what} (0 .. 3)")
    if not tag >> 4 & 1:
        raise ValueError(f"parse_webp: the VP8 frame of {what} is not shown")
    if payload[3:6] != b"\x9d\x01\x2a":
        raise ValueError(f"parse_webp: bad VP8 start code {bytes(payload[3:6]).hex()} in {what} (9d012a)")
    if (tag >> 5) > len(payload) - 10:
        raise ValueError(f"parse_webp: the first partition of {what} ({tag >> 5} bytes) runs past its VP8 chunk ({len(payload) - 10} bytes behind "
                         "the frame header)")
    w, h = int.from_bytes(payload[6:8], "little") & 0x3FFF, int.from_bytes(payload[8:10], "little") & 0x3FFF
    if not w or not h:
        raise ValueError(f"parse_webp: the VP8 frame of {what} has an empty size ({w} x {h})")
    return w, h


def parse_webp(data, lossy=False) -> WebpHeader:
    """One WebP file (bytes), still or animated -> WebpHeader.  With lossy=False (the default) only lossless files are taken, as described below;
    with lossy=True a `VP8 ` chunk (a lossy key frame) is taken as a still and as the image of an ANMF frame, a file may mix `VP8 ` and
    VP8L frames, and the further refusals are: an ALPH chunk (named as such), a VP8 payload that is not a shown key frame of profile 0 .. 3, a bad
    start code, a first partition that runs past the chunk, a VP8 size that differs from the ANMF rectangle or the VP8X canvas.

    lossy=False: one lossless WebP file (bytes), still or animated -> WebpHeader.  ICCP, EXIF, XMP and unknown chunks are skipped, bytes behind the RIFF size
    are ignored.  ValueError for everything outside the decoder's scope: not a RIFF/WEBP file, a RIFF size or a chunk that runs past the file, a
    lossy `VP8 ` or an ALPH chunk, a VP8L signature other than 0x2f or a version other than 0, a frame whose VP8L size differs from its ANMF size,
    a frame rectangle that leaves the canvas, a VP8X canvas that differs from a still's VP8L size, image data on the wrong side of the VP8X
    animation flag, frames without an ANIM chunk before them, a canvas above 16384 a side, no frames."""
    data = bytes(data)
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WEBP":
        raise ValueError("parse_webp: not a RIFF/WEBP file")
    end = 8 + int.from_bytes(data[4:8], "little")
    if end > len(data):
        raise ValueError(f"parse_webp: the RIFF size ({end - 8}) runs past the end of the file ({len(data)} bytes)")

    def chunks(pos, stop, where):
        while pos < stop:
            if pos + 8 > stop:
                raise ValueError(f"parse_webp: a chunk header at byte {pos} runs past the end of {where}")
            kind, ln = data[pos:pos + 4], int.from_bytes(data[pos + 4:pos + 8], "little")
            if pos + 8 + ln > stop:
                raise ValueError(f"parse_webp: chunk {kind!r} at byte {pos} runs past the end of {where}")
            if kind in (b"VP8 ", b"ALPH") and not lossy:
                raise ValueError(f"parse_webp: lossy WebP (VP8) is not decoded (chunk {kind!r} at byte {pos}; VP8L only)")
            if kind == b"ALPH":
                raise ValueError(f"parse_webp: an ALPH chunk (the alpha plane of a lossy frame) is not decoded (at byte {pos}); such a file goes "
                                 "through the host route")
            yield kind, pos + 8, ln
            pos += 8 + ln + (ln & 1)

    u24 = lambda at: int.from_bytes(data[at:at + 3], "little")
    canvas, flags, loop, stills, frames, still_lossy = None, 0, None, [], [], False
    for kind, at, ln in chunks(12, end, "the file"):
        if kind == b"VP8X":
            if ln < 10 or canvas is not None or stills or frames:
                raise ValueError("parse_webp: bad VP8X chunk (its length or place)")
            flags, canvas = data[at], (u24(at + 4) + 1, u24(at + 7) + 1)
        elif kind == b"ANIM":
            if ln < 6 or canvas is None or frames:
                raise ValueError("parse_webp: bad ANIM chunk (its length or place)")
            loop = int.from_bytes(data[at + 4:at + 6], "little")
        elif kind == b"VP8L" or (lossy and kind == b"VP8 "):
            still_lossy = kind == b"VP8 "
            stills.append(data[at:min(at + ln + (ln & 1), end)] if still_lossy else data[at:at + ln])   # libwebp reads a VP8 chunk with its padding byte
        elif kind == b"ANMF":
            k = len(frames)
            if loop is None:
                raise ValueError("parse_webp: an ANMF chunk before any ANIM chunk")
            if ln < 16:
                raise ValueError(f"parse_webp: the ANMF chunk of frame {k} holds {ln} bytes: no room for its header")
            payload, frame_lossy = None, False
            for sub, sat, sln in chunks(at + 16, at + ln, f"the ANMF chunk of frame {k}"):
                if (sub == b"VP8L" or (lossy and sub == b"VP8 ")) and payload is None:
                    payload, frame_lossy = data[sat:sat + sln], sub == b"VP8 "
                    if frame_lossy:                                           # libwebp reads a VP8 chunk with its padding byte
                        payload = data[sat:min(sat + sln + (sln & 1), at + ln)]
            if payload is None:
                raise ValueError(f"parse_webp: frame {k} has no VP8L chunk" + (" and no VP8 chunk" if lossy else ""))
            w, h, alpha = (*_vp8_header(payload, f"frame {k}"), False) if frame_lossy else _vp8l_header(payload, f"frame {k}")
            x, y, fw, fh = 2 * u24(at), 2 * u24(at + 3), u24(at + 6) + 1, u24(at + 9) + 1
            if (w, h) != (fw, fh):
                raise ValueError(f"parse_webp: the {'VP8' if frame_lossy else 'VP8L'} size of frame {k} ({w} x {h}) differs from its ANMF size "
                                 f"({fw} x {fh})")
            frames.append(WebpFrame(x, y, w, h, u24(at + 12), not data[at + 15] & 2, bool(data[at + 15] & 1), alpha, False, payload, frame_lossy))
        # ICCP, EXIF, XMP and unknown chunks: skipped
    animated = bool(flags & 2)
    if (frames and not animated) or (stills and animated):
        raise ValueError("parse_webp: image data on the wrong side of the VP8X animation flag (ANMF without it, or VP8L beside it)")
    if len(stills) > 1:
        raise ValueError("parse_webp: more than one VP8L chunk in a still" if not lossy else "parse_webp: more than one image chunk in a still")
    if stills:
        w, h, alpha = (*_vp8_header(stills[0], "the still"), False) if still_lossy else _vp8l_header(stills[0], "the still")
        if canvas is not None and canvas != (w, h):
            raise ValueError(f"parse_webp: the VP8X canvas ({canvas[0]} x {canvas[1]}) differs from the still's {'VP8' if still_lossy else 'VP8L'} "
                             f"size ({w} x {h})")
        canvas = (w, h)
        frames = [WebpFrame(0, 0, w, h, 0, False, False, alpha, True, stills[0], still_lossy)]
    if not frames:
        raise ValueError("parse_webp: no frames")
    W, H = canvas
    if W > WEBP_MAX_SIDE or H > WEBP_MAX_SIDE:
        raise ValueError(f"parse_webp: a canvas is 1 .. {WEBP_MAX_SIDE} pixels a side, got {W} x {H}")
    for k, f in enumerate(frames):
        if f.x + f.width > W or f.y + f.height > H:
            raise ValueError(f"parse_webp: the rectangle of frame {k} ({f.width} x {f.height} at ({f.x}, {f.y})) leaves the canvas ({W} x {H})")
        covers = (f.x, f.y, f.width, f.height) == (0, 0, W, H)
        before = frames[k - 1] if k else None
        f.key = (k == 0 or (covers and (not f.alpha_is_used or not f.blend))
                 or (before.dispose and (before.key or (before.x, before.y, before.width, before.height) == (0, 0, W, H))))
    return WebpHeader(W, H, loop or 0, animated, frames)


def webp_frame_scratch_words(f: WebpFrame) -> int:
    """Scratch words of one frame as first given: the header block, the main image, three sub-images at the finest block size (predictor,
    cross-colour, entropy image), a palette, and room for the prefix-code groups beyond the first: no more of them than entropy-image pixels or
    than the payload has bits for (a group's five codes take 20 bits at least), and no more than WEBPDEC_GROUP_BYTES.  The number of groups is
    known only once the entropy image is decoded: a frame with more than fit here ends with minus the words it needs as its status."""
    from . import hip
    sub = -(-f.width // 4) * -(-f.height // 4)
    groups = min(sub, 8 * len(f.payload) // 20)
    area = min(groups * hip.WEBPDEC_GROUP_WORDS, WEBPDEC_GROUP_BYTES // 4) if groups > 1 else 0
    return (_WD_HDR_WORDS + f.width * f.height + 3 * sub + 256 + 32 + area + 3) & ~3


def webp_operands(headers, limit: Optional[int] = None, scratch_bytes: Optional[int] = None, caps: Optional[Dict[int, int]] = None):
    """Host-side operands of one decode: (tab int64 (n, 16), data uint8 (bytes,) padded to a multiple of 16, chunks [(f0, f1, scratch words, ARGB
    words)]).  n = the files' first `limit` frames in order; the chunks are runs of frames whose scratch and ARGB words together fit scratch_bytes
    (one frame at least), and a row's offsets count from its chunk's start.  caps: frame -> the scratch words it asked for in an earlier run."""
    if not headers:
        raise ValueError("decode_webp_frames: no frames")
    for k, h in enumerate(headers):
        if (h.width, h.height) != (headers[0].width, headers[0].height):
            raise ValueError(f"decode_webp_frames: file {k} has a canvas of {h.width} x {h.height}; file 0 has {headers[0].width} x "
                             f"{headers[0].height}: one call decodes one canvas size")
    frames = [(f, k == 0, h.frames[k - 1] if k else None) for h in headers for k, f in enumerate(h.frames)]
    frames = frames if limit is None else frames[:max(0, int(limit))]
    if not frames:
        raise ValueError("decode_webp_frames: no frames")
    budget = (WEBPDEC_SCRATCH_BYTES if scratch_bytes is None else int(scratch_bytes)) // 4
    tab = np.zeros((len(frames), WEBP_TAB), np.int64)
    chunks, begin, f0, scr, pix = [], 0, 0, 0, 0
    for k, (f, first, before) in enumerate(frames):
        cap, npix = max(webp_frame_scratch_words(f), ((caps or {}).get(k, 0) + 3) & ~3), f.width * f.height
        if k > f0 and scr + cap + pix + npix > budget:
            chunks.append((f0, k, scr, pix))
            f0, scr, pix = k, 0, 0
        t = tab[k]
        t[_WD_X], t[_WD_Y], t[_WD_W], t[_WD_H] = f.x, f.y, f.width, f.height
        t[_WD_BEGIN], t[_WD_END], t[_WD_SCR], t[_WD_CAP], t[_WD_PIX] = begin, begin + len(f.payload), scr, cap, pix
        t[_WD_FLAGS] = _WD_BLEND * f.blend | _WD_KEY * f.key | _WD_FIRST * first
        if before is not None and before.dispose:
            t[_WD_FLAGS] |= _WD_PREV_DISPOSED
            t[_WD_PX], t[_WD_PY], t[_WD_PW], t[_WD_PH] = before.x, before.y, before.width, before.height
        scr += cap
        pix += npix
        begin += len(f.payload)
    chunks.append((f0, len(frames), scr, pix))
    blob = b"".join(f.payload for f, _, _ in frames)
    data = np.frombuffer(blob + bytes(16 + (-len(blob)) % 16), np.uint8)
    return tab, data, chunks


def decode_webp_frames(files, device="cuda", out=None, limit=None, lossy=False):
    """lossy=True: as below, and lossy frames (`VP8 ` chunks: key frames of any profile, partition count, segment, filter and mode use)
    are decoded too, alone or mixed with VP8L frames in one file or one call; byte for byte PIL's frames again.  What parse_webp(lossy=True)
    refuses (ALPH, inter frames, a bad frame header) is a ValueError before any launch; a VP8 stream that does not decode is a RuntimeError naming
    the frame and the cause (VP8_STATUS_TEXT).  lossy=False (the default) is the lossless decoder unchanged:

    Lossless WebP files (a list of bytes; one bytes object is a list of one), still or animated, all of one canvas size -> (n, H, W, 3) uint8
    RGB on `device`, contiguous, n = all frames of all files in order (the first `limit` of them; later ones are neither decoded nor composed):
    byte for byte what PIL's ImageSequence.Iterator(Image.open(f)) gives after convert("RGB") -- the whole of VP8L, and sub-rectangles, blend and
    dispose composed as libwebp's WebPAnimDecoder composes them, anew at each file.  `out`: a tensor of that shape to write into.  Out-of-scope
    files raise ValueError before anything is launched; a stream that does not decode raises RuntimeError naming the first bad frame and the
    cause, and no pixels are returned.  The status words are read once per call; a frame with more prefix-code groups than its first scratch
    allowance holds (WEBPDEC_GROUP_BYTES) says so in its status, and the call's launches are then run once more with what such frames need."""
    if isinstance(files, (bytes, bytearray, memoryview)):
        files = [files]
    if lossy:
        return _decode_webp_headers_lossy([parse_webp(b, lossy=True) for b in files], device, out, limit)
    headers = [parse_webp(b) for b in files]
    return _decode_webp_headers(headers, device, out, limit)


def _decode_webp_headers(headers, device, out=None, limit=None, caps=None):
    import torch
    from . import hip
    tab, blob, chunks = webp_operands(headers, limit, caps=caps)
    if hip.WEBPDEC_TAB != WEBP_TAB:
        raise RuntimeError(f"decode_webp_frames: the binding's table row has {hip.WEBPDEC_TAB} words, this module builds {WEBP_TAB}")
    n, H, W = len(tab), headers[0].height, headers[0].width
    dev = torch.device(device)
    if out is None:
        out = torch.empty((n, H, W, 3), device=dev, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError(f"decode_webp_frames: out must be contiguous uint8 ({n}, {H}, {W}, 3) on the device")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_data, d_tab = up(blob.copy()), up(tab)
    status = torch.empty((2, n), device=dev, dtype=torch.int32)
    scratch = torch.empty((max(c[2] for c in chunks),), device=dev, dtype=torch.int32)
    argb = torch.empty((max(c[3] for c in chunks),), device=dev, dtype=torch.int32)
    carry = torch.empty((H, W), device=dev, dtype=torch.int32)                # the RGBA canvas, from one chunk to the next
    for f0, f1, scr_words, argb_words in chunks:
        hip.webp_decode(d_data, d_tab[f0:f1], scratch[:scr_words], out=status[0, f0:f1])
        hip.webp_untransform(d_tab[f0:f1], scratch[:scr_words], out=(argb[:argb_words], status[1, f0:f1]))
        hip.webp_compose(d_tab[f0:f1], argb[:argb_words], carry, H, W, out=out[f0:f1])
    st = status.cpu().numpy()                                                  # the one read of the status words (it also orders the launches)
    bad = np.flatnonzero(st[0])
    if bad.size and st[0, bad[0]] < 0 and caps is None:                        # more groups than the first allowance: once more, with what they need
        del scratch, argb, carry
        return _decode_webp_headers(headers, device, out, limit, {int(f): -int(st[0, f]) for f in np.flatnonzero(st[0] < 0)})
    for stage, name in ((0, "image data"), (1, "transforms")):
        bad = np.flatnonzero(st[stage])
        if bad.size:
            f = int(bad[0])
            code = 11 if st[stage, f] < 0 else int(st[stage, f])
            raise RuntimeError(f"decode_webp_frames: frame {f}, {name}: {WEBP_STATUS_TEXT.get(code, f'status {code}')}")
    return out


# ------------------------------------------------------------------------------------------------------------------ WebP lossy

# csrc/vp8dec_core.h's status words
VP8_STATUS_TEXT = {1: "a frame descriptor outside the batch", 2: "a frame header that is no shown key frame of profile 0 .. 3 and the frame's size",
                   3: "a first partition that runs past the payload", 4: "a partition table that runs past the payload, or an empty last partition",
                   5: "a first partition that ends inside the header or the macroblock modes",
                   6: "a token partition that ends inside its macroblocks", 7: "no parsed frame to reconstruct, filter or convert"}

# csrc/vp8dec_core.h's table row (checked against the binding's VP8DEC_TAB on every call)
_V8D_BEGIN, _V8D_END, _V8D_SCR, _V8D_CAP, _V8D_PIX, _V8D_W, _V8D_H = range(7)
VP8_TAB = 8
_V8D_HDR_WORDS, _V8D_MB_BYTES = 64, 32 + 384 * 2 + 384


def vp8_frame_scratch_words(f: WebpFrame) -> int:
    """Scratch words of one lossy frame: the header block and, per macroblock, its modes (32 bytes), 384 int16 coefficients and 384 plane bytes."""
    return _V8D_HDR_WORDS + -(-f.width // 16) * -(-f.height // 16) * _V8D_MB_BYTES // 4


def webp_operands_lossy(headers, limit: Optional[int] = None, scratch_bytes: Optional[int] = None, caps: Optional[Dict[int, int]] = None):
    """webp_operands for files that may hold lossy frames: (tab int64 (n, 16), the composition rows of ALL frames; ltab int64 (nl, 16), the rows of
    the VP8L frames; vtab int64 (nv, 8), the rows of the VP8 frames (csrc/vp8dec_core.h); lidx, vidx, each row's frame number; data; chunks
    [(f0, f1, l0, l1, v0, v1, scratch words, ARGB words)]).  A frame's scratch and ARGB offsets count from its chunk's start, and both kinds of
    frame share the two buffers."""
    if not headers:
        raise ValueError("decode_webp_frames: no frames")
    for k, h in enumerate(headers):
        if (h.width, h.height) != (headers[0].width, headers[0].height):
            raise ValueError(f"decode_webp_frames: file {k} has a canvas of {h.width} x {h.height}; file 0 has {headers[0].width} x "
                             f"{headers[0].height}: one call decodes one canvas size")
    frames = [(f, k == 0, h.frames[k - 1] if k else None) for h in headers for k, f in enumerate(h.frames)]
    frames = frames if limit is None else frames[:max(0, int(limit))]
    if not frames:
        raise ValueError("decode_webp_frames: no frames")
    budget = (WEBPDEC_SCRATCH_BYTES if scratch_bytes is None else int(scratch_bytes)) // 4
    tab = np.zeros((len(frames), WEBP_TAB), np.int64)
    lrows, vrows, lidx, vidx = [], [], [], []
    chunks, begin, f0, l0, v0, scr, pix = [], 0, 0, 0, 0, 0, 0
    for k, (f, first, before) in enumerate(frames):
        cap = vp8_frame_scratch_words(f) if f.lossy else max(webp_frame_scratch_words(f), ((caps or {}).get(k, 0) + 3) & ~3)
        npix = f.width * f.height
        if k > f0 and scr + cap + pix + npix > budget:
            chunks.append((f0, k, l0, len(lrows), v0, len(vrows), scr, pix))
            f0, l0, v0, scr, pix = k, len(lrows), len(vrows), 0, 0
        t = tab[k]
        t[_WD_X], t[_WD_Y], t[_WD_W], t[_WD_H] = f.x, f.y, f.width, f.height
        t[_WD_BEGIN], t[_WD_END], t[_WD_SCR], t[_WD_CAP], t[_WD_PIX] = begin, begin + len(f.payload), scr, cap, pix
        t[_WD_FLAGS] = _WD_BLEND * f.blend | _WD_KEY * f.key | _WD_FIRST * first
        if before is not None and before.dispose:
            t[_WD_FLAGS] |= _WD_PREV_DISPOSED
            t[_WD_PX], t[_WD_PY], t[_WD_PW], t[_WD_PH] = before.x, before.y, before.width, before.height
        if f.lossy:
            vrows.append([begin, begin + len(f.payload), scr, cap, pix, f.width, f.height, 0])
            vidx.append(k)
        else:
            lrows.append(t.copy())
            lidx.append(k)
        scr += cap
        pix += npix
        begin += len(f.payload)
    chunks.append((f0, len(frames), l0, len(lrows), v0, len(vrows), scr, pix))
    blob = b"".join(f.payload for f, _, _ in frames)
    data = np.frombuffer(blob + bytes(16 + (-len(blob)) % 16), np.uint8)
    ltab = np.array(lrows, np.int64).reshape(len(lrows), WEBP_TAB)
    vtab = np.array(vrows, np.int64).reshape(len(vrows), VP8_TAB)
    return tab, ltab, vtab, np.array(lidx, np.int64), np.array(vidx, np.int64), data, chunks


def _decode_webp_headers_lossy(headers, device, out=None, limit=None, caps=None):
    """_decode_webp_headers for headers of parse_webp(lossy=True): per set of launches, the VP8L frames go through decode and untransform, the VP8
    frames through parse, reconstruct, filter and output, all into one ARGB buffer, and one compose draws them in file order."""
    import torch
    from . import hip
    tab, ltab, vtab, lidx, vidx, blob, chunks = webp_operands_lossy(headers, limit, caps=caps)
    if hip.WEBPDEC_TAB != WEBP_TAB or hip.VP8DEC_TAB != VP8_TAB:
        raise RuntimeError(f"decode_webp_frames: the binding's table rows have {hip.WEBPDEC_TAB} and {hip.VP8DEC_TAB} words, this module builds "
                           f"{WEBP_TAB} and {VP8_TAB}")
    n, H, W = len(tab), headers[0].height, headers[0].width
    dev = torch.device(device)
    if out is None:
        out = torch.empty((n, H, W, 3), device=dev, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W, 3) or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError(f"decode_webp_frames: out must be contiguous uint8 ({n}, {H}, {W}, 3) on the device")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_data, d_tab = up(blob.copy()), up(tab)
    d_ltab, d_vtab = (up(ltab) if len(ltab) else None), (up(vtab) if len(vtab) else None)
    lstatus = torch.zeros((2, max(1, len(ltab))), device=dev, dtype=torch.int32)
    vstatus = torch.zeros((4, max(1, len(vtab))), device=dev, dtype=torch.int32)
    scratch = torch.empty((max(c[6] for c in chunks),), device=dev, dtype=torch.int32)
    argb = torch.empty((max(c[7] for c in chunks),), device=dev, dtype=torch.int32)
    carry = torch.empty((H, W), device=dev, dtype=torch.int32)                # the RGBA canvas, from one chunk to the next
    for f0, f1, l0, l1, v0, v1, scr_words, argb_words in chunks:
        if l1 > l0:
            hip.webp_decode(d_data, d_ltab[l0:l1], scratch[:scr_words], out=lstatus[0, l0:l1])
            hip.webp_untransform(d_ltab[l0:l1], scratch[:scr_words], out=(argb[:argb_words], lstatus[1, l0:l1]))
        if v1 > v0:
            hip.vp8dec_parse(d_data, d_vtab[v0:v1], scratch[:scr_words], out=vstatus[0, v0:v1])
            hip.vp8dec_reconstruct(d_vtab[v0:v1], scratch[:scr_words], out=vstatus[1, v0:v1])
            hip.vp8dec_filter(d_vtab[v0:v1], scratch[:scr_words], out=vstatus[2, v0:v1])
            hip.vp8dec_output(d_vtab[v0:v1], scratch[:scr_words], argb[:argb_words], int((vtab[v0:v1, _V8D_W] * vtab[v0:v1, _V8D_H]).max()),
                              out=vstatus[3, v0:v1])
        hip.webp_compose(d_tab[f0:f1], argb[:argb_words], carry, H, W, out=out[f0:f1])
    st = torch.cat([lstatus.reshape(-1), vstatus.reshape(-1)]).cpu().numpy()   # the one read of the status words (it also orders the launches)
    lst, vst = st[:lstatus.numel()].reshape(2, -1)[:, :len(ltab)], st[lstatus.numel():].reshape(4, -1)[:, :len(vtab)]
    if len(ltab) and (lst[0] < 0).any() and caps is None:                      # more prefix-code groups than the first allowance: once more
        del scratch, argb, carry
        return _decode_webp_headers_lossy(headers, device, out, limit, {int(lidx[r]): -int(lst[0, r]) for r in np.flatnonzero(lst[0] < 0)})
    found = []                                                                 # (frame, text) of the first failure of each kind
    for stage, name in ((0, "image data"), (1, "transforms")):
        bad = np.flatnonzero(lst[stage]) if len(ltab) else np.zeros(0, np.int64)
        if bad.size and not any(x[1] == "l" for x in found):
            code = 11 if lst[stage, bad[0]] < 0 else int(lst[stage, bad[0]])
            found.append((int(lidx[bad[0]]), "l", f"{name}: {WEBP_STATUS_TEXT.get(code, f'status {code}')}"))
    for stage, name in ((0, "VP8 parse"), (1, "VP8 reconstruction"), (2, "VP8 loop filter"), (3, "VP8 output")):
        bad = np.flatnonzero(vst[stage]) if len(vtab) else np.zeros(0, np.int64)
        if bad.size and not any(x[1] == "v" for x in found):
            code = int(vst[stage, bad[0]])
            found.append((int(vidx[bad[0]]), "v", f"{name}: {VP8_STATUS_TEXT.get(code, f'status {code}')}"))
    if found:
        f, _, text = min(found)
        raise RuntimeError(f"decode_webp_frames: frame {f}, {text}")
    return out


def read_frames_device(path, limit: Optional[int] = None, device="cuda", webp_lossy=False, jpeg_progressive=False):
    """(L, H, W, 3) uint8 RGB frames of `path` on `device`, decoded there: a Motion-JPEG .avi (what video_out.write_avi writes, or any stock
    tool's `-c:v mjpeg`), a directory whose images are all .jpg / .jpeg, all .png or all .webp (sorted by name; a .png or .webp file gives its
    first frame), one .png / .apng file, animated or not (what video_out.write_apng / write_png write), one .gif file (what video_out.write_gif
    or PIL writes), or one lossless .webp file, animated or not (what video_out.write_webp or PIL's lossless=True writes).  With webp_lossy=True a
    .webp file or a directory of .webp files may also hold lossy frames (`VP8 ` chunks: video_out.write_webp(webp_quality=Q), PIL's default), alone
    or beside lossless ones; without it such a file raises as before.  With jpeg_progressive=True the .jpg / .jpeg files of a directory and the
    frames of a Motion-JPEG .avi may be progressive (SOF2), alone or beside baseline ones; without it they raise as before.  Everything else raises: inputs.read_frames is the host route, and the
    caller chooses it."""
    from .inputs import IMAGE_SUFFIXES, mjpeg_avi_frames
    p = Path(path)
    if not p.exists():
        raise FileNotFoundError(f"read_frames_device: {p} does not exist")
    if p.is_dir():
        files = sorted(f for f in p.iterdir() if f.is_file() and f.suffix.lower() in IMAGE_SUFFIXES)
        if {f.suffix.lower() for f in files} == {".png"}:
            heads = [parse_png(f.read_bytes()) for f in (files if limit is None else files[:limit])]
            for h in heads:                                                   # a file of a directory is one frame, as for inputs.read_frames
                h.streams, h.adlers = h.streams[:1], h.adlers[:1]
            return _decode_png_operands(png_batch_operands(None, heads), device)
        if {f.suffix.lower() for f in files} == {".webp"}:
            heads = [parse_webp(f.read_bytes(), **({"lossy": True} if webp_lossy else {})) for f in (files if limit is None else files[:limit])]
            for h in heads:                                                   # a file of a directory is one frame, as for inputs.read_frames
                h.frames = h.frames[:1]
            if not heads:
                raise RuntimeError(f"read_frames_device: no frames in {p}")
            if len({(h.width, h.height) for h in heads}) > 1:
                raise RuntimeError(f"read_frames_device: the .webp frames of {p} differ in size; use inputs.read_frames for such a directory")
            return _decode_webp_headers_lossy(heads, device) if webp_lossy else _decode_webp_headers(heads, device)
        other = [f.name for f in files if f.suffix.lower() not in (".jpg", ".jpeg")]
        if not files or other:
            raise RuntimeError(f"read_frames_device: {p} must hold .jpg / .jpeg frames only, .png frames only or .webp frames only "
                               f"({'found ' + other[0] if other else 'no images'}); use inputs.read_frames for other inputs")
        jpegs = [f.read_bytes() for f in (files if limit is None else files[:limit])]
    elif p.suffix.lower() in (".png", ".apng"):
        h = parse_png(p.read_bytes())
        if limit is not None:
            h.streams, h.adlers = h.streams[:limit], h.adlers[:limit]
        if not h.streams:
            raise RuntimeError(f"read_frames_device: no frames in {p}")
        return _decode_png_operands(png_batch_operands(None, [h]), device)
    elif p.suffix.lower() == ".gif":
        if limit is not None and limit < 1:
            raise RuntimeError(f"read_frames_device: no frames in {p}")
        return decode_gif_frames(p.read_bytes(), device, limit=limit)
    elif p.suffix.lower() == ".webp":
        if limit is not None and limit < 1:
            raise RuntimeError(f"read_frames_device: no frames in {p}")
        return decode_webp_frames(p.read_bytes(), device, limit=limit, **({"lossy": True} if webp_lossy else {}))
    else:
        jpegs = mjpeg_avi_frames(p, limit) if p.suffix.lower() == ".avi" else None
        if jpegs is None:
            raise RuntimeError(f"read_frames_device: {p.name} is neither a Motion-JPEG .avi, a .png / .apng file, a .webp file, a .gif file nor a "
                               "directory of .jpg, .png or .webp frames; use inputs.read_frames for other inputs")
    if not jpegs:
        raise RuntimeError(f"read_frames_device: no frames in {p}")
    return decode_jpeg_frames(jpegs, device, **({"progressive": True} if jpeg_progressive else {}))
