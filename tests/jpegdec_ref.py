"""Test-side restatement of a baseline JPEG decode as libjpeg (libjpeg-turbo) does it by default, in numpy and plain Python: marker parse, Huffman
decode from BITS / HUFFVAL, dequantiser + the slow-integer inverse DCT (jidctint.c), "fancy" chroma up-sampling (jdsample.c) and the 16-bit
fixed-point YCbCr -> RGB (jdcolor.c).  Test infrastructure (like tests/mjpeg_ref.py): it imports nothing of the package, and the package never
imports it.  tests/test_jpegdec.py holds it to PIL byte for byte; the GPU tests then compare the kernels with it, so the PIL build of the GPU box
does not matter.

Scope: SOF0, 8 bit, one or three components, luma 1x1 / 2x1 / 2x2 with chroma 1x1, one interleaved scan, any restart interval; a file without DHT
means the T.81 Annex K.3 tables."""
import re

import numpy as np


def _zigzag():
    order = []
    for s in range(15):
        diag = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        order += diag if s % 2 else diag[::-1]
    return np.array([y * 8 + x for y, x in order])


ZIGZAG = _zigzag()                                                      # zigzag position -> natural index

K3_DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
K3_AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
K3_AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7"
    "b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5"
    "b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def annex_k_tables():
    return {(0, t): (bytes(K3_DC_BITS[t]), bytes(range(12))) for t in range(2)} | {(1, t): (bytes(K3_AC_BITS[t]), K3_AC_VALS[t]) for t in range(2)}


def parse(data):
    """-> dict(H, W, comps=[(id, h, v, tq)], scan=[(td, ta)], q={id: (64,) natural}, huff={(class, id): (BITS, HUFFVAL)}, ri, segments=[bytes])."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    pos, out = 2, dict(q={}, huff={}, ri=0)
    while True:
        assert data[pos] == 0xFF, f"no marker at {pos}"
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        length = int.from_bytes(data[pos:pos + 2], "big")
        body = data[pos + 2:pos + length]
        pos += length
        if m == 0xDB:
            while body:
                assert body[0] >> 4 == 0, "16-bit DQT"
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = list(body[1:65])
                out["q"][body[0] & 15] = q
                body = body[65:]
        elif m == 0xC0:
            assert body[0] == 8
            out["H"], out["W"] = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            out["comps"] = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])]
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise AssertionError(f"SOF{m - 0xC0} is out of scope")
        elif m == 0xC4:
            while body:
                n = sum(body[1:17])
                out["huff"][(body[0] >> 4, body[0] & 15)] = (bytes(body[1:17]), bytes(body[17:17 + n]))
                body = body[17 + n:]
        elif m == 0xDD:
            out["ri"] = int.from_bytes(body, "big")
        elif m == 0xDA:
            assert body[0] == len(out["comps"]) and tuple(body[-3:]) == (0, 63, 0)
            out["scan"] = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(body[0])]
            break
    if not out["huff"]:
        out["huff"] = annex_k_tables()
    # entropy-coded data: cut at every marker (0xFF followed by neither 0x00 nor 0xFF) up to EOI
    segs, start, i = [], pos, pos
    while True:
        i = data.index(b"\xff", i)
        nxt = data[i + 1]
        if nxt == 0 or nxt == 0xFF:
            i += 1
            continue
        segs.append(data[start:i])
        if nxt == 0xD9:
            break
        assert nxt == 0xD0 + ((len(segs) - 1) & 7), f"marker {nxt:#x} in the scan"
        i = start = i + 2
    out["segments"] = segs
    return out


def _lookup(bits, vals):
    """16-bit look -> (code length, symbol); length 0 where no code matches."""
    ln, sym = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            ln[lo:lo + (1 << (16 - length))] = length
            sym[lo:lo + (1 << (16 - length))] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return ln.tolist(), sym.tolist()


class _Bits:
    def __init__(self, seg):
        raw = re.split(b"\xff(?!\x00)", seg, maxsplit=1, flags=re.S)[0].replace(b"\xff\x00", b"\xff")       # fill bytes before a marker end the data
        self.n = 8 * len(raw)
        self.v = int.from_bytes(raw + bytes(8), "big")                  # zeros past the end
        self.total = self.n + 64
        self.pos = 0

    def peek16(self):
        assert self.pos <= self.n, "segment exhausted"
        return (self.v >> (self.total - self.pos - 16)) & 0xFFFF

    def take(self, n):
        self.pos += n
        assert self.pos <= self.n, "segment exhausted"
        return (self.v >> (self.total - self.pos)) & ((1 << n) - 1)


def _extend(v, s):
    return v - (1 << s) + 1 if v < 1 << (s - 1) else v


def geometry(p):
    """(ncomp, hs, vs, mcu_rows, mcu_cols) with the one-component case normalised to 1 x 1 (its scan is not interleaved)."""
    ncomp = len(p["comps"])
    hs, vs = (1, 1) if ncomp == 1 else p["comps"][0][1:3]
    if ncomp == 3:
        assert (hs, vs) in ((1, 1), (2, 1), (2, 2)) and all(c[1:3] == (1, 1) for c in p["comps"][1:]), "sampling out of scope"
    return ncomp, hs, vs, -(-p["H"] // (8 * vs)), -(-p["W"] // (8 * hs))


def coefficients(p):
    """-> one int64 array (block_rows, block_cols, 64) in natural order per component."""
    ncomp, hs, vs, R, C = geometry(p)
    samp = [(hs, vs)] + [(1, 1)] * (ncomp - 1)
    coef = [np.zeros((R * v, C * h, 64), np.int64) for h, v in samp]
    look = {k: _lookup(*bv) for k, bv in p["huff"].items()}
    mcus = R * C
    ri = p["ri"] or mcus
    assert len(p["segments"]) == -(-mcus // ri), "segment count"
    zz = ZIGZAG.tolist()
    for s, seg in enumerate(p["segments"]):
        b = _Bits(seg)
        pred = [0] * ncomp
        for m in range(s * ri, min((s + 1) * ri, mcus)):
            my, mx = divmod(m, C)
            for c in range(ncomp):
                (dl, dsym), (al, asym) = look[(0, p["scan"][c][0])], look[(1, p["scan"][c][1])]
                h, v = samp[c]
                for by in range(v):
                    for bx in range(h):
                        blk = coef[c][my * v + by, mx * h + bx]
                        w = b.peek16()
                        assert dl[w], "bad DC code"
                        b.pos += dl[w]
                        cat = dsym[w]
                        if cat:
                            pred[c] += _extend(b.take(cat), cat)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            w = b.peek16()
                            assert al[w], "bad AC code"
                            b.pos += al[w]
                            r, cat = asym[w] >> 4, asym[w] & 15
                            if cat == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[zz[k]] = _extend(b.take(cat), cat)
                            k += 1
        assert b.pos <= b.n, "segment exhausted"
    return coef


def _wrap32(x):
    return ((x + (1 << 31)) % (1 << 32)) - (1 << 31)


def _fix(x):
    return int(x * 8192 + 0.5)


def _idct_1d(d, shift):
    """jpeg_idct_islow's butterfly over d[0..7] (int64 arrays); every output descaled by `shift` with round half up, in 32-bit wrap."""
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * _fix(0.541196100)
    tmp2 = z1 - z3 * _fix(1.847759065)
    tmp3 = z1 + z2 * _fix(0.765366865)
    tmp0, tmp1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * _fix(1.175875602)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * _fix(0.298631336), tmp1 * _fix(2.053119869), tmp2 * _fix(3.072711026), tmp3 * _fix(1.501321110)
    z1, z2, z3, z4 = -z1 * _fix(0.899976223), -z2 * _fix(2.562915447), -z3 * _fix(1.961570560) + z5, -z4 * _fix(0.390180644) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    outs = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return [_wrap32(_wrap32(o) + (1 << (shift - 1))) >> shift for o in outs]


def idct_plane(coef, q):
    """(bh, bw, 64) coefficients, (64,) quantiser -> (bh * 8, bw * 8) uint8 samples."""
    bh, bw, _ = coef.shape
    d = _wrap32(coef * q).reshape(bh, bw, 8, 8)
    ws = np.stack(_idct_1d([d[:, :, y, :] for y in range(8)], 11), axis=2)              # columns: over y, per x
    px = np.stack(_idct_1d([ws[:, :, :, x] for x in range(8)], 18), axis=3)             # rows: over x, per y
    px = np.clip(px + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample(p, hs, vs, H, W):
    """One chroma plane (MCU-padded) -> (>= H, >= W) ints at luma resolution; the edges are those of the plane's real size."""
    if hs == 1:
        return p.astype(np.int64)
    cw, ch = -(-W // hs), -(-H // vs)
    p = p[:ch, :cw].astype(np.int64)
    if cw <= 2:                                                         # libjpeg replicates planes of 1 or 2 columns
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)
    out = np.empty((ch * vs, 2 * cw), np.int64)
    if vs == 1:
        left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
        return out
    up, down = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    s = np.empty((2 * ch, cw), np.int64)
    s[0::2], s[1::2] = 3 * p + up, 3 * p + down
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out[:, 0::2] = (3 * s + left + 8) >> 4                              # at column 0 `left` is s itself: (4 s + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out


def colour(y, cb, cr):
    F = lambda x: int(x * 65536 + 0.5)
    y, cb, cr = y.astype(np.int64), cb - 128, cr - 128
    r = y + ((F(1.402) * cr + 32768) >> 16)
    g = y + ((-F(0.34414) * cb + 32768 - F(0.71414) * cr) >> 16)
    b = y + ((F(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    """One JPEG file -> (H, W, 3) uint8 RGB; a one-component file gives Y in all three channels."""
    p = parse(data)
    ncomp, hs, vs, _, _ = geometry(p)
    H, W = p["H"], p["W"]
    planes = [idct_plane(c, p["q"][p["comps"][k][3]]) for k, c in enumerate(coefficients(p))]
    if ncomp == 1:
        return np.repeat(planes[0][:H, :W, None], 3, axis=2)
    cb, cr = (upsample(planes[k], hs, vs, H, W)[:H, :W] for k in (1, 2))
    return colour(planes[0][:H, :W], cb, cr)
