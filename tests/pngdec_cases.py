"""Shared inputs of the PNG decoder's tests (tests/test_pngdec.py, tests/test_pngdec_gpu.py): PNG files built chunk by chunk around
hand-chosen filtered rows, a fixed-Huffman token writer for the deflate streams zlib never emits, a numpy unfilter, and the list of well-formed
streams both test files decode.  Nothing here imports the product except write_job, which lays out the host program's input."""
import functools
import io
import struct
import zlib

import numpy as np
from PIL import Image

from tests import png_ref as P

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
SIZES = ((1, 1), (300, 1), (1, 300), (37, 29), (21, 37), (150, 150))                      # (W, H)
LEVELS = (0, 1, 6, 9)
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "rle": zlib.Z_RLE, "huffman": zlib.Z_HUFFMAN_ONLY, "filtered": zlib.Z_FILTERED}
FILTERS = (0, 1, 2, 3, 4, "mixed")
DEPTHS = ((0, 1), (0, 2), (0, 4), (0, 8), (3, 1), (3, 2), (3, 4), (3, 8), (2, 8), (4, 8), (6, 8))     # (colour type, bit depth)


def rowbytes(W, ct, depth):
    return (W * CHANNELS[ct] * depth + 7) // 8


def filter_bpp(ct, depth):
    return max(1, CHANNELS[ct] * depth // 8)


# ---- pixels ------------------------------------------------------------------------------------------------------------------------------------------
def raw_rows(W, H, ct, depth, seed=0):
    """(H, rowbytes) uint8 of packed samples: smooth ramps, flat runs and noise in bands, so that every filter type and long and short matches occur.
    Palette images only use indices below palette_for(depth, seed)'s length."""
    rng = np.random.default_rng(1000 * seed + 10 * ct + depth)
    ch = CHANNELS[ct]
    top = (1 << depth) - 1 if ct != 3 else len(palette_for(depth, seed)) - 1
    yy, xx = np.mgrid[0:H, 0:W]
    s = np.zeros((H, W, ch), np.int64)
    for c in range(ch):
        ramp = (3 * xx + 5 * yy + 40 * c + seed) // max(1, 256 >> depth if depth < 8 else 1)
        noise = rng.integers(0, top + 1, (H, W))
        flat = ((xx // 7 + yy // 5 + c) * 37)
        band = (yy // 4) % 3
        s[..., c] = np.where(band == 0, ramp, np.where(band == 1, noise, flat)) % (top + 1)
    s = s.reshape(H, W * ch)
    if depth == 8:
        return s.astype(np.uint8)
    per = 8 // depth
    pad = (-s.shape[1]) % per
    s = np.concatenate([s, np.zeros((H, pad), np.int64)], axis=1).reshape(H, -1, per)
    shifts = np.arange(per - 1, -1, -1) * depth                                            # first sample in the high bits
    return (s << shifts).sum(axis=2).astype(np.uint8)


def palette_for(depth, seed=0):
    """A PLTE shorter than 2^depth allows where that is possible (so that the length matters): (entries, 3) uint8."""
    n = {1: 2, 2: 3, 4: 13, 8: 200}[depth]
    rng = np.random.default_rng(77 + seed)
    return rng.integers(0, 256, (n, 3)).astype(np.uint8)


# ---- filters -----------------------------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(raw, bpp, types):
    """(H, rowbytes) uint8 and a filter type per row -> (H, 1 + rowbytes) filtered bytes."""
    raw = np.asarray(raw).astype(np.int64)
    H, n = raw.shape
    out = np.zeros((H, 1 + n), np.uint8)
    for y in range(H):
        cur, up = raw[y], raw[y - 1] if y else np.zeros(n, np.int64)
        a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]])[:n] if n > bpp else np.zeros(n, np.int64)
        c = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]])[:n] if n > bpp else np.zeros(n, np.int64)
        t = types[y]
        pred = [np.zeros(n, np.int64), a, up, (a + up) >> 1, _paeth(a, up, c)][t]
        out[y, 0], out[y, 1:] = t, (cur - pred) % 256
    return out


def unfilter_ref(filtered, bpp):
    """(H, 1 + rowbytes) filtered bytes -> (H, rowbytes) reconstructed: the PNG specification's five filter types, byte by byte."""
    f = np.asarray(filtered).astype(np.int64)
    H, n = f.shape[0], f.shape[1] - 1
    out = np.zeros((H, n), np.int64)
    for y in range(H):
        t, up = f[y, 0], out[y - 1] if y else np.zeros(n, np.int64)
        for i in range(n):
            a = out[y, i - bpp] if i >= bpp else 0
            b = up[i]
            c = up[i - bpp] if i >= bpp else 0
            p = a + b - c
            paeth = a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else (b if abs(p - b) <= abs(p - c) else c)
            out[y, i] = (f[y, 1 + i] + (0, a, b, (a + b) >> 1, paeth)[t]) % 256
    return out.astype(np.uint8)


def filter_types(H, choice, seed=0):
    if choice == "mixed":
        return [int(v) for v in np.random.default_rng(5 + seed).integers(0, 5, H)]
    return [int(choice)] * H


# ---- containers ----------------------------------------------------------------------------------------------------------------------------------------
def zcompress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9 if level else 8, strategy)
    return c.compress(bytes(data)) + c.flush()


def make_png(filtered_bytes, W, H, colour_type, depth, compress=None, idat_split=None, plte=None, trns=None, extra=()):
    """Filtered rows (bytes, H * (1 + rowbytes)) -> a PNG file.  compress: None (zlib level 6), a (level, strategy) pair, or the finished zlib stream
    as bytes.  idat_split: cut the stream into IDAT chunks of that many bytes (an empty IDAT in front as well).  extra: (type, body) chunks put
    before the first IDAT."""
    data = bytes(filtered_bytes)
    blob = compress if isinstance(compress, (bytes, bytearray)) else zcompress(data, *(compress or (6, zlib.Z_DEFAULT_STRATEGY)))
    out = [SIG, P.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour_type, 0, 0, 0))]
    if plte is not None:
        out.append(P.chunk(b"PLTE", np.asarray(plte, np.uint8).tobytes()))
    if trns is not None:
        out.append(P.chunk(b"tRNS", bytes(trns)))
    out += [P.chunk(k, b) for k, b in extra]
    if idat_split:
        out.append(P.chunk(b"IDAT", b""))
        out += [P.chunk(b"IDAT", blob[i:i + idat_split]) for i in range(0, len(blob), idat_split)]
    else:
        out.append(P.chunk(b"IDAT", blob))
    out.append(P.chunk(b"IEND", b""))
    return b"".join(out)


def make_apng(blobs, W, H, colour_type, depth, plte=None, trns=None, dispose=0, blend=0, rect=None):
    """zlib streams, one per frame -> an APNG whose frames are all full size at (0, 0) (rect = (w, h, x, y) for the frames after the first)."""
    out = [SIG, P.chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour_type, 0, 0, 0)), P.chunk(b"acTL", struct.pack(">II", len(blobs), 0))]
    if plte is not None:
        out.append(P.chunk(b"PLTE", np.asarray(plte, np.uint8).tobytes()))
    if trns is not None:
        out.append(P.chunk(b"tRNS", bytes(trns)))
    seq = 0
    for k, b in enumerate(blobs):
        w, h, x, y = (W, H, 0, 0) if k == 0 or rect is None else rect
        out.append(P.chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, x, y, 1, 10, dispose, blend)))
        seq += 1
        if k == 0:
            out.append(P.chunk(b"IDAT", b))
        else:
            out.append(P.chunk(b"fdAT", struct.pack(">I", seq) + b))
            seq += 1
    out.append(P.chunk(b"IEND", b""))
    return b"".join(out)


def pil_rgb(data, frame=0):
    im = Image.open(io.BytesIO(data))
    if frame:
        im.seek(frame)
    return np.asarray(im.convert("RGB"))


def pil_frames(data):
    im = Image.open(io.BytesIO(data))
    out = []
    for k in range(getattr(im, "n_frames", 1)):
        im.seek(k)
        out.append(np.asarray(im.convert("RGB")))
    return np.stack(out)


def case_png(W, H, ct, depth, level=6, strategy="default", filt="mixed", seed=0, **kw):
    raw = raw_rows(W, H, ct, depth, seed)
    f = filter_rows(raw, filter_bpp(ct, depth), filter_types(H, filt, seed))
    return make_png(f.tobytes(), W, H, ct, depth, compress=(level, STRATEGIES[strategy]), plte=palette_for(depth, seed) if ct == 3 else None, **kw)


# ---- a fixed-Huffman token writer ---------------------------------------------------------------------------------------------------------------------
DIST_TABLE = tuple((1 + ((2 + (d & 1)) << ((d >> 1) - 1)) if d >= 4 else 1 + d, (d >> 1) - 1 if d >= 4 else 0) for d in range(30))     # (first, extra bits)


class FixedTokens:
    """Literals and (length, distance) pairs on the fixed codes of RFC 1951 3.2.6, in one final block; tracks the bytes it stands for."""

    def __init__(self):
        self.bw = P.BitWriter()
        self.bw.put(1, 1)
        self.bw.put(1, 2)
        self.out = bytearray()

    def _sym(self, s):
        if s < 144:
            self.bw.huff(0x30 + s, 8)
        elif s < 256:
            self.bw.huff(0x190 + s - 144, 9)
        elif s < 280:
            self.bw.huff(s - 256, 7)
        else:
            self.bw.huff(0xC0 + s - 280, 8)

    def lit(self, *values):
        for v in values:
            self._sym(v)
            self.out.append(v)
        return self

    def match(self, length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(self.out)
        s, eb, ev = P.length_symbol(length)
        self._sym(s)
        self.bw.put(ev, eb)
        d = max(k for k in range(30) if DIST_TABLE[k][0] <= dist)
        self.bw.huff(d, 5)
        self.bw.put(dist - DIST_TABLE[d][0], DIST_TABLE[d][1])
        for _ in range(length):
            self.out.append(self.out[-dist])
        return self

    def zlib_stream(self):
        """(zlib stream, the bytes it decompresses to)."""
        bw = P.BitWriter()
        bw.acc, bw.n = self.bw.acc, self.bw.n
        bw.huff(0, 7)                                                # symbol 256
        return P.ZLIB_HEADER + bw.bytes() + struct.pack(">I", zlib.adler32(bytes(self.out))), bytes(self.out)


def token_streams():
    """name -> (zlib stream, W, H) of grey 8-bit images whose FILTERED bytes are the stream's output (every row begins with filter type 0 .. 4 only
    where the test decodes past the inflate; the inflate alone takes any bytes).  What zlib never emits but must be decoded."""
    out = {}
    rng = np.random.default_rng(9)

    def finish(t, W, H):
        need = H * (1 + W) - len(t.out)
        assert need >= 0
        t.lit(*([7] * need))
        z, data = t.zlib_stream()
        assert zlib.decompress(z) == data and len(data) == H * (1 + W)
        return z, W, H

    t = FixedTokens().lit(*rng.integers(0, 256, 300).tolist())
    for k in range(29):                                              # every length code at both ends of its extra-bit range
        base, eb = P.LENGTH_TABLE[k]
        t.match(base, 1 + k)
        t.match(258 if k == 28 else min(base + (1 << eb) - 1, 257), 300 - k)
    out["every_length_code"] = finish(t, 8191, 1)
    t = FixedTokens().lit(*rng.integers(0, 256, 64).tolist())
    while len(t.out) < 33000:
        t.lit(*rng.integers(0, 256, 50).tolist()).match(258, 1 + int(rng.integers(0, min(len(t.out), 32768))))
    for d in range(30):                                              # all 30 distance codes at both ends
        first, eb = DIST_TABLE[d]
        t.match(3 + d, first)
        t.match(4 + d, first + (1 << eb) - 1)
    t.match(258, 32768).match(5, 32768).lit(1, 2).match(7, 2).match(258, 1).match(258, 1).lit(9).match(3, 1)
    out["every_distance_code"] = finish(t, 16383, 3)
    return out


# ---- the well-formed files both test files decode -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cross_batches():
    """(W, H) -> list of RGB files of that size: zlib levels x strategies x the five filter types forced per row and mixed (120 files a size)."""
    out = {}
    for W, H in SIZES:
        out[(W, H)] = [case_png(W, H, 2, 8, lv, st, ft, seed=lv + 3 * k) for lv in LEVELS for k, st in enumerate(STRATEGIES) for ft in FILTERS]
    return out


@functools.lru_cache(maxsize=None)
def depth_batches():
    """(W, H, colour type, depth) -> list of files: every accepted colour type / depth at every size, mixed filters, level 6 and level 0 (stored
    blocks), the second one cut into IDAT chunks of 1000 bytes."""
    out = {}
    for W, H in SIZES:
        for ct, depth in DEPTHS:
            out[(W, H, ct, depth)] = [case_png(W, H, ct, depth, 6, "default", "mixed", seed=1), case_png(W, H, ct, depth, 0, "default", "mixed", seed=2, idat_split=1000),
                                      case_png(W, H, ct, depth, 9, "rle", 4, seed=3)]
    return out


def palette_batch():
    """Five 21 x 37 palette files at 4 bits whose palettes differ."""
    return [case_png(21, 37, 3, 4, 6, "default", "mixed", seed=20 + k) for k in range(5)]


def write_job(path, pngs=None, headers=None):
    """The host program's input (tools/pngdec_host_check.cpp states the layout) -> (n, H, W, stride)."""
    from mmgt_amd import video_in
    headers, (H, W, ct, depth), data, offsets, adlers, palette, plte_len = video_in.png_batch_operands(pngs, headers)
    n = len(adlers)
    if palette is None:
        palette, plte_len = np.zeros((n, 256, 3), np.uint8), np.zeros(n, np.int32)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<8i", 0x314A4450, n, H, W, ct, depth, 0, 0))
        fh.write(struct.pack("<q", data.size))
        for a in (offsets.astype("<i8"), adlers.astype("<u4"), plte_len.astype("<i4"), palette, data):
            fh.write(np.ascontiguousarray(a).tobytes())
    return n, H, W, headers[0].stride
