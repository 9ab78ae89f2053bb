"""The progressive JPEG streams the decoder tests share (tests/test_jpegprog.py against PIL on the host, tests/test_jpegprog_gpu.py against
tests/jpegprog_ref.py on the device): name -> bytes, built once per process, everything seeded.

PIL writes one scan script only, so this file also holds a small TRANSCODER: the quantised coefficients of a baseline file (as
jpegdec_ref.coefficients decodes them) written out as a progressive file under any scan script and any restart interval per scan, by the
procedures of T.81 G.1 (as libjpeg's jcphuff.c).  Its Huffman tables are the simplest that are valid: in a DC table the size categories 0 .. 15
as 5-bit codes, in an AC table the symbols 0 .. 254 as 9-bit codes (symbol v is code v, so no code is all ones), defined anew before every scan
under a changing table id.  A transcoded file counts only if PIL decodes it to
the pixels of its baseline source: tests/test_jpegprog.py asserts that for every one, so a writer bug cannot hide a decoder bug."""
import functools
import struct

import numpy as np

from tests import jpegdec_ref as R
from tests import mjpeg_ref as M
from tests.jpegdec_cases import pil_jpeg

# PIL's (libjpeg's jpeg_simple_progression) script for three components and for one: (components, Ss, Se, Ah, Al)
A = (0, 1, 2)
PIL_SCRIPT = [(A, 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
              (A, 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
PIL_SCRIPT_GREY = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]

SCRIPTS = {
    "spectral": [(A, 0, 0, 0, 0)] + [((c,), 1, 63, 0, 0) for c in A],
    "dc_split": [((c,), 0, 0, 0, 0) for c in A] + [((c,), 1, 63, 0, 0) for c in A],
    "bands": [(A, 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for c in A for a, b in ((1, 1), (2, 7), (8, 63))],
    "deep": [(A, 0, 0, 0, 3)] + [((c,), 1, 63, 0, 3) for c in A]
            + [s for ah in (3, 2, 1) for s in [(A, 0, 0, ah, ah - 1)] + [((c,), 1, 63, ah, ah - 1) for c in A]],
    "chroma_first": [(A, 0, 0, 0, 1)] + [((c,), 1, 63, 0, 1) for c in A] + [((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), (A, 0, 0, 1, 0),
                                                                          ((0,), 1, 63, 1, 0)],
    "restarts": PIL_SCRIPT,
}
RESTARTS = {"restarts": [2, 1, 3, 0, 4, 1, 5, 2, 1, 7]}                # per scan, in MCUs of that scan; 0 = none


class _BitWriter:
    def __init__(self, code_bits):
        self.acc, self.n, self.out, self.code_bits = 0, 0, bytearray(), code_bits

    def put(self, value, bits):
        self.acc, self.n = (self.acc << bits) | (value & ((1 << bits) - 1)), self.n + bits
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def symbol(self, v):
        self.put(v, self.code_bits)                                      # the fixed tables: symbol v is the code v

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)                # pad with ones
        out, self.out = bytes(self.out), bytearray()
        return out


def _seg(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def _scan_blocks(p, coef, comps):
    """The scan's units: a list, per unit, of the (scan component position, block) pairs it holds, in coding order."""
    ncomp, hs, vs, rows, cols = R.geometry(p)
    if len(comps) > 1:
        samp = [(hs, vs)] + [(1, 1)] * (ncomp - 1)
        return [[(i, coef[c][my * samp[c][1] + by, mx * samp[c][0] + bx]) for i, c in enumerate(comps) for by in range(samp[c][1])
                 for bx in range(samp[c][0])] for my in range(rows) for mx in range(cols)]
    c = comps[0]
    w, h = (p["W"], p["H"]) if c == 0 else (-(-p["W"] // hs), -(-p["H"] // vs))
    return [[(0, coef[c][y, x])] for y in range(-(-h // 8)) for x in range(-(-w // 8))]


def _encode_segment(units, ss, se, ah, al, ns):
    """One restart interval of a scan -> its entropy-coded bytes (T.81 G.1.2)."""
    w, zz = _BitWriter(9 if ss else 5), R.ZIGZAG.tolist()
    pred = [0] * ns
    eobrun, held = 0, []                                                 # held: correction bits that follow the pending EOB run

    def emit_eobrun():
        nonlocal eobrun, held
        if eobrun:
            nbits = eobrun.bit_length() - 1
            w.symbol(nbits << 4)
            if nbits:
                w.put(eobrun, nbits)
            eobrun = 0
        for bit in held:
            w.put(bit, 1)
        held = []

    for unit in units:
        for i, blk in unit:
            blk = [int(v) for v in blk]
            if ss == 0 and ah == 0:
                v = blk[0] >> al
                d, pred[i] = v - pred[i], v
                s = abs(d).bit_length()
                w.symbol(s)
                if s:
                    w.put(d if d >= 0 else d - 1, s)
            elif ss == 0:
                w.put((blk[0] >> al) & 1, 1)
            elif ah == 0:
                r = 0
                for k in range(ss, se + 1):
                    v = blk[zz[k]]
                    a = abs(v) >> al
                    if a == 0:
                        r += 1
                        continue
                    emit_eobrun()
                    while r > 15:
                        w.symbol(0xF0)
                        r -= 16
                    s = a.bit_length()
                    w.symbol((r << 4) | s)
                    w.put(a if v >= 0 else ~a, s)
                    r = 0
                if r:
                    eobrun += 1
                    if eobrun == 0x7FFF:
                        emit_eobrun()
            else:
                absv = [abs(blk[zz[k]]) >> al for k in range(ss, se + 1)]
                last_new = max((k for k, a in zip(range(ss, se + 1), absv) if a == 1), default=-1)
                r, bits = 0, []
                for k, a in zip(range(ss, se + 1), absv):
                    if a == 0:
                        r += 1
                        continue
                    while r > 15 and k <= last_new:
                        emit_eobrun()
                        w.symbol(0xF0)
                        r -= 16
                        for bit in bits:
                            w.put(bit, 1)
                        bits = []
                    if a > 1:
                        bits.append(a & 1)
                        continue
                    emit_eobrun()
                    w.symbol((r << 4) | 1)
                    w.put(0 if blk[zz[k]] < 0 else 1, 1)
                    for bit in bits:
                        w.put(bit, 1)
                    r, bits = 0, []
                if r or bits:
                    eobrun += 1
                    held += bits
                    if eobrun == 0x7FFF:
                        emit_eobrun()
    emit_eobrun()
    return w.flush()


def transcode(baseline, script, restarts=None):
    """A baseline JPEG file -> a progressive file holding the same quantised coefficients under `script` [(components, Ss, Se, Ah, Al)], with
    `restarts[k]` MCUs of scan k per restart interval (0 or no list: none)."""
    p = R.parse(baseline)
    coef = R.coefficients(p)
    out = bytearray(b"\xff\xd8")
    for tid, q in sorted(p["q"].items()):
        out += _seg(0xDB, bytes([tid]) + bytes(int(v) for v in q[R.ZIGZAG]))
    comps = p["comps"]
    out += _seg(0xC2, struct.pack(">BHHB", 8, p["H"], p["W"], len(comps)) + b"".join(bytes([cid, (h << 4) | v, tq]) for cid, h, v, tq in comps))
    dc_table = bytes([0] * 4 + [16] + [0] * 11) + bytes(range(16))       # sixteen 5-bit codes
    ac_table = bytes([0] * 8 + [255] + [0] * 7) + bytes(range(255))      # 255 nine-bit codes; symbol 255 is never used
    ri_now = 0
    for k, (sc, ss, se, ah, al) in enumerate(script):
        ri = restarts[k] if restarts else 0
        if ri != ri_now:
            out += _seg(0xDD, struct.pack(">H", ri))
            ri_now = ri
        tid = k % 4
        out += _seg(0xC4, bytes([0x10 | tid]) + ac_table if ss else bytes([tid]) + dc_table)
        out += _seg(0xDA, bytes([len(sc)]) + b"".join(bytes([comps[c][0], (tid << 4) | tid]) for c in sc) + bytes([ss, se, (ah << 4) | al]))
        units = _scan_blocks(p, coef, sc)
        step = ri or len(units)
        for n, at in enumerate(range(0, len(units), step)):
            if n:
                out += bytes([0xFF, 0xD0 + ((n - 1) & 7)])
            out += _encode_segment(units[at:at + step], ss, se, ah, al, len(sc))
    return bytes(out + b"\xff\xd9")


def one_bright_pixel():
    """128 x 128 grey, flat but for one bright pixel in the first block: the other 255 blocks of every AC scan are one EOB run."""
    f = np.full((128, 128), 90, np.uint8)
    f[3, 5] = 250
    return f


def mask_frame(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.zeros((H, W, 3), np.uint8)
    f[(xx - 0.45 * W) ** 2 + (yy - 0.5 * H) ** 2 < (H / 3.2) ** 2] = 255
    return f


@functools.lru_cache(maxsize=None)
def sources():
    """The baseline files the transcoded streams are made from, and the arrays / settings the PIL-written pairs are made from."""
    return {"21x37_420_smooth": pil_jpeg(M.smooth_frame(21, 37, 301), quality=85, subsampling=2),
            "16x16_444_noise": pil_jpeg(M.noise_frame(16, 16, 302), quality=100, subsampling=0)}


@functools.lru_cache(maxsize=None)
def pil_pairs():
    """name -> (progressive file, its baseline twin): the same array, quality and subsampling, written by PIL both ways."""
    cases = {"pil_8x8_grey": (M.smooth_frame(8, 8, 310)[..., 1], dict(quality=75)),
             "pil_16x16_444_noise_q100": (M.noise_frame(16, 16, 302), dict(quality=100, subsampling=0)),
             "pil_21x37_420_smooth": (M.smooth_frame(21, 37, 301), dict(quality=85, subsampling=2)),
             "pil_33x17_422": (M.smooth_frame(33, 17, 311, sigma=10.0), dict(quality=90, subsampling=1)),
             "pil_48x64_420_restart_rows1": (M.smooth_frame(48, 64, 312), dict(quality=75, subsampling=2, restart_marker_rows=1)),
             "pil_48x64_mask": (mask_frame(48, 64), dict(quality=90, subsampling=2)),
             "pil_128x128_grey_one_pixel": (one_bright_pixel(), dict(quality=75))}
    return {k: (pil_jpeg(f, progressive=True, **kw), pil_jpeg(f, **kw)) for k, (f, kw) in cases.items()}


@functools.lru_cache(maxsize=None)
def transcoded():
    """name -> (progressive file, the baseline file it was transcoded from, script name)."""
    out = {}
    for src, data in sources().items():
        for script in SCRIPTS:
            out[f"tc_{src}_{script}"] = (transcode(data, SCRIPTS[script], RESTARTS.get(script)), data, script)
    return out


@functools.lru_cache(maxsize=None)
def streams():
    return {k: v[0] for k, v in pil_pairs().items()} | {k: v[0] for k, v in transcoded().items()}


@functools.lru_cache(maxsize=None)
def twins():
    """name -> the baseline file holding the same quantised coefficients."""
    return {k: v[1] for k, v in pil_pairs().items()} | {k: v[1] for k, v in transcoded().items()}


def names():
    return sorted(streams())
