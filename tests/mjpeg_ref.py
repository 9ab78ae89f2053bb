"""Test-side restatement of baseline JPEG (ITU T.81, JFIF 1.01) as mmgt_amd's Motion-JPEG path defines it, in numpy fp64 and plain Python:
colour, sampling, DCT, quantiser -> coefficients, and an entropy coder -> bytes.  Test infrastructure (like tests/wavlm_ref.py): the package
never imports it, and it imports nothing of the package -- tables, headers and coder are written out again here from the standard.

Definition shared with csrc/mjpeg.hip: JFIF full-range BT.601 without rounding to 8 bits, level shift -128, 4:2:0 = 2x2 box average of Cb / Cr,
the frame extended to the MCU multiple by edge replication, orthonormal DCT-II, sign(c) floor(|c| / q + 0.5) with the Annex K tables under the IJG
quality rule, DC clamped to [-1024, 1023] and AC to [-1023, 1023], the Annex K Huffman tables, a restart interval of one MCU row."""
import struct

import numpy as np

BASE_Q = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32])


def _zigzag():
    """zigzag position -> natural index, walked along the anti-diagonals (T.81 figure A.6)."""
    order = []
    for s in range(15):
        diag = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        order += diag if s % 2 else diag[::-1]
    return np.array([y * 8 + x for y, x in order])


ZIGZAG = _zigzag()

DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa])
DC_VALS = list(range(12))


def _codes(bits, vals):
    """symbol -> (code, length): T.81 Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [_codes(DC_BITS[c], DC_VALS) for c in range(2)]
AC_CODES = [_codes(AC_BITS[c], AC_VALS[c]) for c in range(2)]


def qtables(quality):
    """(2, 64) ints, natural order: the IJG rule."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE_Q * s + 50) // 100, 1, 255)


def geometry(H, W, subsampling):
    side, bpm = (16, 6) if subsampling == "4:2:0" else (8, 3)
    return -(-H // side), -(-W // side), bpm


def _dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    c[0] = 1.0 / np.sqrt(8.0)
    return c


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)                # (h / 8, w / 8, 8, 8)


def coefficients(frame, quality=90, subsampling="4:2:0", with_ratio=False):
    """(H, W, 3) uint8 -> int (mcu_rows, mcu_cols, blocks per MCU, 64) in zigzag order; with_ratio also returns |c| / q in fp64, the number whose
    distance from a rounding tie defines the band in which an fp32 implementation may differ by one."""
    assert subsampling in ("4:2:0", "4:4:4")
    H, W, _ = frame.shape
    R, C, bpm = geometry(H, W, subsampling)
    side = 16 if bpm == 6 else 8
    x = np.pad(frame.astype(np.float64), ((0, R * side - H), (0, C * side - W), (0, 0)), mode="edge")
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b - 128.0
    cb = -0.168736 * r - 0.331264 * g + 0.5 * b
    cr = 0.5 * r - 0.418688 * g - 0.081312 * b
    if bpm == 6:
        cb = cb.reshape(R * 8, 2, C * 8, 2).mean(axis=(1, 3))
        cr = cr.reshape(R * 8, 2, C * 8, 2).mean(axis=(1, 3))
    D = _dct_matrix()
    dct = lambda p: np.einsum("uy,rcyx,vx->rcuv", D, _blocks(p), D)                 # F[u][v] = sum C[u][y] s[y][x] C[v][x]
    fy, fcb, fcr = dct(y), dct(cb), dct(cr)
    if bpm == 6:
        fy = fy.reshape(R, 2, C, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(R, C, 4, 8, 8)         # Y00 Y01 Y10 Y11
    else:
        fy = fy[:, :, None]
    f = np.concatenate([fy, fcb[:, :, None], fcr[:, :, None]], axis=2).reshape(R, C, bpm, 64)
    q = qtables(quality)
    qq = np.stack([q[0]] * (bpm - 2) + [q[1], q[1]])[None, None]                     # (1, 1, bpm, 64)
    ratio = np.abs(f) / qq
    c = (np.sign(f) * np.floor(ratio + 0.5)).astype(np.int64)
    lo = np.full(64, -1023)
    lo[0] = -1024
    c = np.clip(c, lo, 1023)
    c, ratio = c[..., ZIGZAG], ratio[..., ZIGZAG]
    return (c, ratio) if with_ratio else c


def tie_band(ratio, width=1e-3):
    """True where the fp64 quotient lies within `width` of a rounding tie: the only places where an fp32 kernel may land on the other side."""
    return np.abs(ratio - np.floor(ratio) - 0.5) < width


def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, cat):
    v = int(v)
    return v if v >= 0 else v + (1 << cat) - 1


def entropy_segment(row):
    """One MCU row of coefficients (mcu_cols, bpm, 64) -> its entropy-coded segment: DC predictors start at 0, 1-bit padding to the byte,
    0xFF -> 0xFF 0x00."""
    C, bpm, _ = row.shape
    bits = []
    pred = [0, 0, 0]
    for m in range(C):
        for k in range(bpm):
            comp = 0 if k < bpm - 2 else k - (bpm - 2) + 1
            t = 0 if comp == 0 else 1
            blk = row[m, k]
            d = int(blk[0]) - pred[comp]
            pred[comp] = int(blk[0])
            cat = _category(d)
            code, ln = DC_CODES[t][cat]
            bits.append(format(code, f"0{ln}b"))
            if cat:
                bits.append(format(_value_bits(d, cat), f"0{cat}b"))
            run = 0
            for v in blk[1:]:
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    code, ln = AC_CODES[t][0xF0]
                    bits.append(format(code, f"0{ln}b"))
                    run -= 16
                cat = _category(v)
                code, ln = AC_CODES[t][run << 4 | cat]
                bits.append(format(code, f"0{ln}b"))
                bits.append(format(_value_bits(v, cat), f"0{cat}b"))
                run = 0
            if run:
                code, ln = AC_CODES[t][0x00]
                bits.append(format(code, f"0{ln}b"))
    s = "".join(bits)
    s += "1" * (-len(s) % 8)
    raw = int(s, 2).to_bytes(len(s) // 8, "big") if s else b""
    return raw.replace(b"\xff", b"\xff\x00")


def _seg(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def headers(W, H, quality, subsampling):
    q = qtables(quality)
    C, bpm = geometry(H, W, subsampling)[1:]
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += _seg(0xDB, bytes([t]) + bytes(int(v) for v in q[t][ZIGZAG]))
    out += _seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22 if bpm == 6 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t in range(2):
        out += _seg(0xC4, bytes([t]) + bytes(DC_BITS[t]) + bytes(DC_VALS))
        out += _seg(0xC4, bytes([0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t]))
    out += _seg(0xDD, struct.pack(">H", C))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def file_from_coefficients(coef, W, H, quality, subsampling):
    """Coefficients of one frame (mcu_rows, mcu_cols, bpm, 64) -> the complete JFIF file."""
    coef = np.asarray(coef)
    out = [headers(W, H, quality, subsampling)]
    R = coef.shape[0]
    for r in range(R):
        out.append(entropy_segment(coef[r]))
        out.append(b"\xff\xd9" if r == R - 1 else bytes([0xFF, 0xD0 + (r & 7)]))
    return b"".join(out)


def encode(frame, quality=90, subsampling="4:2:0"):
    H, W, _ = frame.shape
    return file_from_coefficients(coefficients(frame, quality, subsampling), W, H, quality, subsampling)


def psnr(a, b):
    mse = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


# ---- seeded test frames --------------------------------------------------------------------------------------------------------------------------
def smooth_frame(H, W, seed, sigma=6.0):
    """A smooth synthetic picture (low-frequency waves per channel) with sigma-6 Gaussian noise: the kind of frame the tie-band condition was
    checked on."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((H, W, 3))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.01, 0.06, 2).tolist() + [rng.uniform(0, 6.28)]
        out[..., c] = 128 + 80 * np.sin(fx * xx + ph) * np.cos(fy * yy + 0.5 * ph) + 30 * np.sin(0.11 * (xx + yy) + c)
    out += rng.normal(0.0, sigma, out.shape)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def noise_frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
