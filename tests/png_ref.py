"""CPU yardstick of the device PNG encoder (csrc/png.hip, mmgt_amd/video_out.py): the stream definition restated in numpy / plain
Python, with nothing imported from the product.  Truecolour, 8 bit, no alpha, no interlace.

 1. filter   per scanline, bpp = 3, the row above row 0 is zeros; of the five PNG filter types the one with the smallest sum of min(v, 256 - v) over
             the row's filtered bytes, the lowest type on a tie.  (n, H, 1 + 3 W): type byte, filtered row.
 2. strips   strip_rows scanlines each (the last may be shorter), every strip one dynamic-Huffman deflate block, BFINAL on the frame's last, blocks
             joined bit by bit.
 3. tokens   within a strip, distance-1 matches only: at p >= 1 with r = bytes from p on that equal byte p - 1 (at most 258), r >= 3 is a match of
             length r, else a literal; position 0 is a literal; symbol 256 ends the block.
 4. codes    package-merge, limit 15 (literal/length) and 7 (code-length code); the order that decides ties is stated at code_lengths.
 5. packing  LSB-first, Huffman codes bit-reversed.
 6. zlib     header 0x78 0x01, the blocks, Adler-32 of the filtered bytes."""
import struct
import zlib
from fractions import Fraction

import numpy as np

ZLIB_HEADER = b"\x78\x01"           # CM = 8, CINFO = 7 (32 KB window), FLEVEL = 0, FCHECK makes 0x7801 a multiple of 31
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5: (first length, extra bits) of the length symbols 257 .. 285
LENGTH_TABLE = ((3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1), (19, 2), (23, 2), (27, 2),
                (31, 2), (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4), (115, 4), (131, 5), (163, 5), (195, 5), (227, 5), (258, 0))


# ---- test inputs -----------------------------------------------------------------------------------------------------------------------------------
def smooth_frames(n, H, W, seed=0):
    """(n, H, W, 3) uint8 whose row bands each favour another filter type: a horizontal ramp (Sub on row 0), repeated noisy rows (Up), rows built as
    the mean of left and above (Average), staggered flat blocks (Paeth), faint noise about zero (None), then a two-way ramp for whatever is left."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, H, W, 3), np.int64)
    xx = np.arange(W)[:, None] + np.zeros((1, 3), np.int64)
    for f in range(n):
        img = out[f]
        for y in range(H):
            band, k = divmod(y, 6)
            band %= 6
            if band == 0:
                img[y] = 40 + 3 * xx + 17 * y + np.array([0, 30, 60]) + 11 * f
            elif band == 1:
                img[y] = rng.integers(0, 256, (W, 3)) if k == 0 else img[y - 1]
            elif band == 2:
                if k == 0:
                    img[y] = rng.integers(0, 256, (W, 3))
                else:
                    for x in range(W):
                        left = img[y, x - 1] if x else rng.integers(0, 256, 3)
                        img[y, x] = (left + img[y - 1, x]) >> 1
            elif band == 3:
                cell = (np.arange(W) // 5 + ((y + 3 * ((np.arange(W) // 5) % 2)) // 6) * 7 + f) % 11
                img[y] = (cell[:, None] * np.array([23, 51, 87]) + 9) % 256
            elif band == 4:
                img[y] = rng.integers(-2, 3, (W, 3)) * (rng.random((W, 3)) < 0.5)
            else:
                img[y] = 2 * xx + 3 * y + 5 * f
    return (out % 256).astype(np.uint8)


def pose_frames(n, H, W):
    """Lines of a few colours on black, as a pose frame has them."""
    out = np.zeros((n, H, W, 3), np.uint8)
    colours = np.array([[255, 0, 0], [0, 255, 85], [0, 85, 255], [255, 170, 0]], np.uint8)
    for f in range(n):
        for k in range(4):
            for t in np.linspace(0.0, 1.0, 4 * max(H, W)):
                y = int(round((0.1 + 0.2 * k + 0.05 * f) * (H - 1) * (1 - t) + (0.9 - 0.15 * k) * (H - 1) * t))
                x = int(round((0.15 * k) * (W - 1) * (1 - t) + (0.95 - 0.2 * k + 0.03 * f) * (W - 1) * t))
                out[f, min(max(y, 0), H - 1), min(max(x, 0), W - 1)] = colours[k]
    return out


# ---- 1. filter --------------------------------------------------------------------------------------------------------------------------------------
def filter_frames(frames):
    """(n, H, W, 3) uint8 -> (n, H, 1 + 3 W) uint8."""
    x = np.asarray(frames)
    n, H, W, _ = x.shape
    raw = x.reshape(n, H, 3 * W).astype(np.int64)
    out = np.zeros((n, H, 1 + 3 * W), np.uint8)
    for f in range(n):
        for y in range(H):
            cur = raw[f, y]
            up = raw[f, y - 1] if y else np.zeros_like(cur)
            left = np.concatenate([np.zeros(3, np.int64), cur[:-3]])
            upleft = np.concatenate([np.zeros(3, np.int64), up[:-3]])
            p = left + up - upleft
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
            paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
            cands = [cur, cur - left, cur - up, cur - ((left + up) >> 1), cur - paeth]
            cands = [c % 256 for c in cands]
            costs = [int(np.minimum(c, 256 - c).sum()) for c in cands]
            t = costs.index(min(costs))                                  # index() returns the first minimum: the lowest type on a tie
            out[f, y, 0] = t
            out[f, y, 1:] = cands[t]
    return out


# ---- 3. tokens --------------------------------------------------------------------------------------------------------------------------------------
def tokens(data):
    """bytes of one strip -> list of ("lit", byte) / ("len", length), without the end-of-block symbol."""
    d = bytes(data)
    out, p = [("lit", d[0])], 1
    while p < len(d):
        r = 0
        while r < 258 and p + r < len(d) and d[p + r] == d[p - 1]:
            r += 1
        if r >= 3:
            out.append(("len", r))
            p += r
        else:
            out.append(("lit", d[p]))
            p += 1
    return out


def length_symbol(length):
    """match length 3 .. 258 -> (symbol, extra bits, extra value)."""
    if length == 258:
        return 285, 0, 0
    for k in range(27, -1, -1):
        base, eb = LENGTH_TABLE[k]
        if length >= base:
            return 257 + k, eb, length - base
    raise ValueError(length)


# ---- 4. codes ---------------------------------------------------------------------------------------------------------------------------------------
def code_lengths(hist, max_bits):
    """Package-merge (Larmore / Hirschberg).  The used symbols are the leaves, sorted by (count, symbol).  List 1 is the leaves; list k + 1 is the
    leaves merged with the packages of list k (its items paired in order, an odd last item dropped), ordered by weight, at equal weight every leaf
    before every package and otherwise in the order they already had.  A symbol's length is the number of times it occurs in the first 2 m - 2
    items of list max_bits (m = used symbols).  One used symbol gets length 1, none gives all zeros."""
    hist = [int(h) for h in hist]
    used = sorted((h, s) for s, h in enumerate(hist) if h > 0)
    lengths = [0] * len(hist)
    if len(used) == 1:
        lengths[used[0][1]] = 1
    if len(used) < 2:
        return lengths
    if len(used) > (1 << max_bits):
        raise ValueError("more symbols than codes of that length")
    leaves = [(h, (s,)) for h, s in used]
    cur = list(leaves)
    for _ in range(max_bits - 1):
        packages = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + packages, key=lambda it: it[0])            # stable: leaves stand before packages in the list that is sorted
    for _, syms in cur[:2 * len(used) - 2]:
        for s in syms:
            lengths[s] += 1
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2."""
    lengths = list(lengths)
    count = [0] * 17
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lengths)
    for s, ln in enumerate(lengths):
        if ln:
            codes[s] = nxt[ln]
            nxt[ln] += 1
    return codes


class BitWriter:
    """LSB-first."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits

    def huff(self, code, length):
        self.put(int(format(code, f"0{length}b")[::-1], 2) if length else 0, length)      # Huffman codes go in most significant bit first

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def rle_code_lengths(seq):
    """The code lengths as symbols of the code-length alphabet: list of (symbol, extra bits, extra value).  A run of zeros: 18 for min(run, 138)
    while 11 or more are left, then 17 for 3 .. 10, then single zeros.  A run of a non-zero length: the length once, then 16 for min(rest, 6)
    while 3 or more are left, then the length itself."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, 7, k - 11))
                run -= k
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, 2, k - 3))
                run -= k
            out += [(v, 0, 0)] * run
        i = j
    return out


def deflate_block(bw, data, final):
    """One strip -> one dynamic-Huffman block appended to bw."""
    toks = tokens(data)
    hist = [0] * 286
    for kind, v in toks:
        hist[v if kind == "lit" else length_symbol(v)[0]] += 1
    hist[256] = 1
    matches = any(kind == "len" for kind, _ in toks)
    ll = code_lengths(hist, 15)
    dl = [1] if matches else [0]
    nll = max(257, max(s for s in range(286) if ll[s]) + 1)
    cl_syms = rle_code_lengths(ll[:nll] + dl)
    cl_hist = [0] * 19
    for s, _, _ in cl_syms:
        cl_hist[s] += 1
    cl = code_lengths(cl_hist, 7)
    ncl = max(4, max(k for k in range(19) if cl[CL_ORDER[k]]) + 1)
    ll_codes, cl_codes = canonical_codes(ll), canonical_codes(cl)
    bw.put(1 if final else 0, 1)
    bw.put(2, 2)
    bw.put(nll - 257, 5)
    bw.put(0, 5)                                                         # HDIST = 1 code
    bw.put(ncl - 4, 4)
    for k in range(ncl):
        bw.put(cl[CL_ORDER[k]], 3)
    for s, eb, ev in cl_syms:
        bw.huff(cl_codes[s], cl[s])
        bw.put(ev, eb)
    for kind, v in toks:
        if kind == "lit":
            bw.huff(ll_codes[v], ll[v])
        else:
            s, eb, ev = length_symbol(v)
            bw.huff(ll_codes[s], ll[s])
            bw.put(ev, eb)
            bw.put(0, 1)                                                 # the one distance code, length 1: distance 1, no extra bits
    bw.huff(ll_codes[256], ll[256])


def deflate_strips(data, strip_bytes):
    """Any byte string cut into strips of strip_bytes -> raw deflate stream (no zlib wrapper): what the low-level device path produces."""
    data = bytes(data)
    bw = BitWriter()
    starts = list(range(0, len(data), strip_bytes))
    for s in starts:
        deflate_block(bw, data[s:s + strip_bytes], s == starts[-1])
    return bw.bytes()


def adler32(data):
    a, b = 1, 0
    for v in bytes(data):
        a = (a + v) % 65521
        b = (b + a) % 65521
    return b << 16 | a


def encode_frames(frames, strip_rows):
    """(n, H, W, 3) uint8 -> one zlib stream per frame."""
    filt = filter_frames(frames)
    n, H, rowlen = filt.shape
    return [ZLIB_HEADER + deflate_strips(filt[f].tobytes(), strip_rows * rowlen) + struct.pack(">I", zlib.adler32(filt[f].tobytes())) for f in range(n)]


# ---- containers -------------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_file(blob, W, H):
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", blob) + chunk(b"IEND", b"")


def parse_chunks(data):
    """PNG / APNG file -> list of (type, body); checks the signature and every CRC."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, p = [], 8
    while p < len(data):
        (ln,) = struct.unpack(">I", data[p:p + 4])
        kind, body = data[p + 4:p + 8], data[p + 8:p + 8 + ln]
        (crc,) = struct.unpack(">I", data[p + 8 + ln:p + 12 + ln])
        assert crc == zlib.crc32(kind + body), kind
        out.append((kind, body))
        p += 12 + ln
    assert p == len(data) and out[-1][0] == b"IEND"
    return out


def delay_fraction(fps):
    fr = Fraction(1 / fps).limit_denominator(65535)
    return fr.numerator, fr.denominator
