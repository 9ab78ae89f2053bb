"""The yardstick of the lossy WebP writer: a plain numpy / Python encoder of the VP8 key-frame stream that csrc/vp8.hip writes, and a
restatement of libwebp's default YUV -> RGB output path (fancy chroma upsampling, fixed-point conversion) as PIL's decoder applies it.

The stream: key frames only; 16 x 16 luma modes DC / V / H / TM (numbered 0 .. 3) and the same four for chroma; no segments, no filter deltas, no
probability updates; mb_no_coeff_skip = 1; one quantiser index; 1, 2, 4 or 8 token partitions (macroblock row r in partition r mod P).  The format
fixes the inverse transforms, dequantisation, prediction edges, trees and tables; the colour conversion, forward transforms, quantiser rounding,
mode choice and quality map are this project's, all in integers, and are restated here independently of csrc/vp8_core.h.

encode_frame(rgb, quality, partitions, filter_level) -> dict(payload, parts, recon=(Y, U, V) padded, modes (mbh, mbw, 2), levels (mbh, mbw, 25, 16)
in scan order, nz (mbh, mbw) bit masks, skipped)."""
import struct

import numpy as np

MAX_SIDE = 16383
MAX_LEVEL = 2047
HEADER_SYMBOLS = 1100          # bool symbols of a first partition before its macroblocks (29 header bits, 1056 flags, 9 for the skip probability)
MB_MODE_SYMBOLS = 7            # skip flag, three for the luma mode, three for the chroma mode
MB_TOKEN_SYMBOLS = 384 * 19    # 16 * 15 + 8 * 16 + 16 coefficients, each at most 7 tree bits, 11 extra bits and a sign
FLUSH_BYTES = 4                # 32 closing symbols of one bit each

DC_Q = (4,5,6,7,8,9,10,10,11,12,13,14,15,16,17,17,18,19,20,20,21,21,22,22,23,23,24,25,25,26,27,28,
        29,30,31,32,33,34,35,36,37,37,38,39,40,41,42,43,44,45,46,46,47,48,49,50,51,52,53,54,55,56,57,58,
        59,60,61,62,63,64,65,66,67,68,69,70,71,72,73,74,75,76,76,77,78,79,80,81,82,83,84,85,86,87,88,89,
        91,93,95,96,98,100,101,102,104,106,108,110,112,114,116,118,122,124,126,128,130,132,134,136,138,140,143,145,148,151,154,157)
AC_Q = (4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,34,35,
        36,37,38,39,40,41,42,43,44,45,46,47,48,49,50,51,52,53,54,55,56,57,58,60,62,64,66,68,70,72,74,76,
        78,80,82,84,86,88,90,92,94,96,98,100,102,104,106,108,110,112,114,116,119,122,125,128,131,134,137,140,143,146,149,152,
        155,158,161,164,167,170,173,177,181,185,189,193,197,201,205,209,213,217,221,225,229,234,239,245,249,254,259,264,269,274,279,284)
ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)
BANDS = (0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0)
CAT3, CAT4, CAT5 = (173, 148, 140), (176, 155, 140, 135), (180, 157, 141, 134, 130)
CAT6 = (254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129)
# default coefficient probabilities and the probabilities of their update flags, [type 4][band 8][context 3][node 11]
COEF_PROBS = np.frombuffer(bytes.fromhex(
    "808080808080808080808080808080808080808080808080808080808080808080fd88feffe4db8080808080bd81f2ffe3d5ffdb8080806a7ee3fcd6d1ffff8080800162f8ffece2"
    "ffff808080b585eefeddeaff9a8080804e86caf7c6b4ffdb80808001b9f9fff3ff8080808080b896f7ffece080808080804d6ed8ffece680808080800165fbfff1ff8080808080aa"
    "8bf1fcecd1ffff8080802574c4f3e4ffffff80808001ccfefff5ff8080808080cfa0faffee8080808080806667e7ffd3ab80808080800198fcfff0ff8080808080b187f3ffeae180"
    "808080805081d3ffc2e080808080800101ff8080808080808080f601ff8080808080808080ff80808080808080808080c623eddfc1bba2a0919b3e832dc6ddacb0dc9dfcdd01442f"
    "92d095a7dda2ffdf800195f1ffdde0ffff808080b88deafddedcffc78080805163b5f2b0bef9caffff800181e8fdd6c5f2c4ffff806379d2fac9c6ffca808080175ba3f2aabbf7d2"
    "ffff8001c8f6ffeaff80808080806db2f1ffe7f5ffff8080802c82c9fdcdc0ffff8080800184effbdbd1ffa58080805e88e1fbdabeffff8080801664aef5baa1ffc780808001b6f9"
    "ffe8eb80808080807c8ff1ffe3ea8080808080234db5fbc1d3ffcd808080019df7ffece7ffff808080798debffe1e3ffff8080802d63bcfbc3d9ffe08080800101fbffd5ff808080"
    "8080cb01f8ffff8080808080808901b1ffe0ff8080808080fd09f8fbcfd0ffc0808080af0de0f3c1b9f9c6ffff804911abdda1b3eca7ffea80015ff7fdd4b7ffff808080ef5af4fa"
    "d3d1ffff8080809b4dc3f8bcc3ffff8080800118effbdadbffcd808080c933dbffc4ba8080808080452ebeefc9daffe480808001bffbffff808080808080dfa5f9ffd5ff80808080"
    "808d7cf8ffff8080808080800110f8ffff808080808080be24e6ffecff80808080809501ff808080808080808001e2ff8080808080808080f7c0ff8080808080808080f080ff8080"
    "8080808080800186fcffff808080808080d53efaffff808080808080375dff8080808080808080808080808080808080808080808080808080808080808080808080808080808080ca"
    "18d5ebbabfdca0f0afff7e26b6e8a9b8e4aeffbb803d2e8adb97b2f0aaffd8800170e6fac7bff79fffff80a66de4fcd3d7ffae808080274da2e8acb4f5b2ffff800134dcf6c6c7f9"
    "dcffff807c4abff3b7c1faddffff80184782db9aaaf3b6ffff8001b6e1f9dbf0ffe08080809596e2fcd8cdffab8080801c6caaf2b7c2fedfffff800151e6fccccbffc08080807b66"
    "d1f7bcc4ffe9808080145f99f3a4adffcb80808001def8ffd8d58080808080a8aff6fcebcdffff8080802f74d7ffd3d4ffff8080800179ecfdd4d6ffff8080808d54d5fcc9caffdb"
    "8080802a50a0f0a2b9ffcd8080800101ff8080808080808080f401ff8080808080808080ee01ff8080808080808080"), np.uint8).reshape(4, 8, 3, 11)
_UPDATE_NOT_255 = {                                                             # flat index: value; the other 898 entries are 255
    33: 176, 34: 246, 44: 223, 45: 241, 46: 252, 55: 249, 56: 253, 57: 253, 67: 244, 68: 252, 77: 234, 78: 254, 79: 254, 88: 253, 100: 246,
    101: 254, 110: 239, 111: 253, 112: 254, 121: 254, 123: 254, 133: 248, 134: 254, 143: 251, 145: 254, 166: 253, 167: 254, 176: 251, 177: 254,
    178: 254, 187: 254, 189: 254, 199: 254, 200: 253, 202: 254, 209: 250, 211: 254, 213: 254, 220: 254, 264: 217, 275: 225, 276: 252, 277: 241,
    278: 253, 281: 254, 286: 234, 287: 250, 288: 241, 289: 250, 290: 253, 292: 253, 293: 254, 298: 254, 308: 223, 309: 254, 310: 254, 319: 238,
    320: 253, 321: 254, 322: 254, 331: 248, 332: 254, 341: 249, 342: 254, 364: 253, 374: 247, 375: 254, 397: 253, 398: 254, 407: 252, 430: 254,
    431: 254, 440: 253, 463: 254, 464: 253, 473: 250, 484: 254, 528: 186, 529: 251, 530: 250, 539: 234, 540: 251, 541: 244, 542: 254, 550: 251,
    551: 251, 552: 243, 553: 253, 554: 254, 556: 254, 562: 253, 563: 254, 572: 236, 573: 253, 574: 254, 583: 251, 584: 253, 585: 253, 586: 254,
    587: 254, 595: 254, 596: 254, 605: 254, 606: 254, 607: 254, 628: 254, 638: 254, 639: 254, 649: 254, 671: 254, 792: 248, 803: 250, 804: 254,
    805: 252, 806: 254, 814: 248, 815: 254, 816: 249, 817: 253, 826: 253, 827: 253, 836: 246, 837: 253, 838: 253, 847: 252, 848: 254, 849: 251,
    850: 254, 851: 254, 859: 254, 860: 252, 869: 248, 870: 254, 871: 253, 880: 253, 882: 254, 883: 254, 892: 251, 893: 254, 902: 245, 903: 251,
    904: 254, 913: 253, 914: 253, 915: 254, 925: 251, 926: 253, 935: 252, 936: 253, 937: 254, 947: 254, 958: 252, 968: 249, 970: 254, 981: 254,
    992: 253, 1001: 250, 1034: 254}
UPDATE_PROBS = np.full(1056, 255, np.uint8)
for _i, _v in _UPDATE_NOT_255.items():
    UPDATE_PROBS[_i] = _v
assert COEF_PROBS.size == 1056 and len(_UPDATE_NOT_255) == 158
UPDATE_PROBS = UPDATE_PROBS.reshape(4, 8, 3, 11)

# default loop filter level by quantiser index / 8 (chosen from profiles/vp8/filter_level.jsonl; 0 is a legal entry)
FILTER_LEVELS = (0, 8, 12, 16, 16, 16, 24, 24, 24, 32, 32, 32, 48, 48, 48, 48)


def quality_to_q(quality):
    quality = int(quality)
    if not 0 <= quality <= 100:
        raise ValueError(f"quality must be 0 .. 100, got {quality}")
    return (100 - quality) * 127 // 100


def default_filter_level(q):
    return FILTER_LEVELS[q >> 3]


def default_partitions(H):
    rows = (H + 15) // 16
    return 8 if rows >= 8 else 4 if rows >= 4 else 2 if rows >= 2 else 1


def quantisers(q):
    """(y dc, y ac, y2 dc, y2 ac, uv dc, uv ac) of index q, all deltas 0."""
    return (DC_Q[q], AC_Q[q], DC_Q[q] * 2, max(8, AC_Q[q] * 101581 >> 16), DC_Q[min(q, 117)], AC_Q[q])


# ---- colour -------------------------------------------------------------------------------------------------------------------------------------------
def rgb_to_yuv420(rgb):
    """(H, W, 3) uint8 -> Y (16 mbh, 16 mbw), U, V (8 mbh, 8 mbw): the frame padded to whole macroblocks by edge replication, studio range, chroma
    from the sum of a 2 x 2 cell."""
    H, W, _ = rgb.shape
    ph, pw = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    p = rgb[np.minimum(np.arange(ph), H - 1)][:, np.minimum(np.arange(pw), W - 1)].astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (16839 * r + 33059 * g + 6420 * b + (16 << 16) + 32768) >> 16
    s = p.reshape(ph // 2, 2, pw // 2, 2, 3).sum((1, 3))
    r, g, b = s[..., 0], s[..., 1], s[..., 2]
    u = (-9719 * r - 19081 * g + 28800 * b + (128 << 18) + (1 << 17)) >> 18
    v = (28800 * r - 24116 * g - 4684 * b + (128 << 18) + (1 << 17)) >> 18
    return tuple(np.clip(a, 0, 255).astype(np.uint8) for a in (y, u, v))


def _clip8(v):
    return np.where((v & ~16383) == 0, v >> 6, np.where(v < 0, 0, 255))


def yuv_to_rgb(y, u, v):
    y, u, v = (np.asarray(a, np.int64) for a in (y, u, v))
    yy = y * 19077 >> 8
    r = _clip8(yy + (v * 26149 >> 8) - 14234)
    g = _clip8(yy - (u * 6419 >> 8) - (v * 13320 >> 8) + 8708)
    b = _clip8(yy + (u * 33050 >> 8) - 17685)
    return np.stack([r, g, b], -1).astype(np.uint8)


def _upsample(c, H, W):
    """libwebp's fancy upsampler: a pixel takes 9 : 3 : 3 : 1 of the four chroma samples around it, the nearest first, rounded in two steps; the
    frame's edges repeat."""
    c = np.asarray(c, np.int64)
    ch, cw = c.shape
    r, x = np.arange(H), np.arange(W)
    rn = np.where(r & 1, (r - 1) // 2, r // 2)
    rf = np.clip(np.where(r & 1, rn + 1, rn - 1), 0, ch - 1)
    xn = np.where(x & 1, (x - 1) // 2, x // 2)
    xf = np.clip(np.where(x & 1, xn + 1, xn - 1), 0, cw - 1)
    nn, nf, fn, ff = c[rn][:, xn], c[rn][:, xf], c[rf][:, xn], c[rf][:, xf]
    out = (((nn + 3 * nf + 3 * fn + ff + 8) >> 3) + nn) >> 1
    edge = xn == xf                                                             # the first column, and the last of an even width
    out[:, edge] = ((3 * nn + fn + 2) >> 2)[:, edge]
    return out


def decoded_rgb(recon, H, W):
    """The reconstructed planes as PIL shows them: cropped to the true size, chroma upsampled, converted."""
    y, u, v = recon
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return yuv_to_rgb(y[:H, :W], _upsample(u[:ch, :cw], H, W), _upsample(v[:ch, :cw], H, W))


# ---- transforms ---------------------------------------------------------------------------------------------------------------------------------------
def fdct(d):
    """(4, 4) differences -> 16 coefficients in raster order (ours)."""
    d = d.astype(np.int64)
    a0, a1, a2, a3 = d[:, 0] + d[:, 3], d[:, 1] + d[:, 2], d[:, 1] - d[:, 2], d[:, 0] - d[:, 3]
    t = np.stack([(a0 + a1) * 8, (a2 * 2217 + a3 * 5352 + 1812) >> 9, (a0 - a1) * 8, (a3 * 2217 - a2 * 5352 + 937) >> 9], 1)
    a0, a1, a2, a3 = t[0] + t[3], t[1] + t[2], t[1] - t[2], t[0] - t[3]
    return np.stack([(a0 + a1 + 7) >> 4, ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0), (a0 - a1 + 7) >> 4,
                     (a3 * 2217 - a2 * 5352 + 51000) >> 16]).reshape(16)


def fwht(dc):
    """16 DC terms in block order -> 16 coefficients in raster order (ours)."""
    m = np.asarray(dc, np.int64).reshape(4, 4)
    a0, a1, a2, a3 = m[:, 0] + m[:, 2], m[:, 1] + m[:, 3], m[:, 1] - m[:, 3], m[:, 0] - m[:, 2]
    t = np.stack([a0 + a1, a3 + a2, a3 - a2, a0 - a1], 1)
    a0, a1, a2, a3 = t[0] + t[2], t[1] + t[3], t[1] - t[3], t[0] - t[2]
    return np.stack([(a0 + a1) >> 1, (a3 + a2) >> 1, (a3 - a2) >> 1, (a0 - a1) >> 1]).reshape(16)


def idct_add(c, pred):
    """The format's inverse transform of 16 raster coefficients added to a (4, 4) prediction."""
    m = np.asarray(c, np.int64).reshape(4, 4)
    mul1 = lambda a: ((a * 20091) >> 16) + a
    mul2 = lambda a: (a * 35468) >> 16
    a, b = m[0] + m[2], m[0] - m[2]
    cc, d = mul2(m[1]) - mul1(m[3]), mul1(m[1]) + mul2(m[3])
    t = np.stack([a + d, b + cc, b - cc, a - d], 1)                             # t[i] = the vertical pass of column i
    dc = t[0] + 4
    a, b = dc + t[2], dc - t[2]
    cc, d = mul2(t[1]) - mul1(t[3]), mul1(t[1]) + mul2(t[3])
    res = np.stack([a + d, b + cc, b - cc, a - d], 0) >> 3                      # res[x][row]
    return np.clip(pred.astype(np.int64) + res.T, 0, 255).astype(np.uint8)


def iwht(c):
    """The format's inverse Walsh-Hadamard transform: 16 raster coefficients -> the 16 blocks' DC terms."""
    m = np.asarray(c, np.int64).reshape(4, 4)
    a0, a1, a2, a3 = m[0] + m[3], m[1] + m[2], m[1] - m[2], m[0] - m[3]
    t = np.stack([a0 + a1, a3 + a2, a0 - a1, a3 - a2])
    dc = t[:, 0] + 3
    a0, a1, a2, a3 = dc + t[:, 3], t[:, 1] + t[:, 2], t[:, 1] - t[:, 2], dc - t[:, 3]
    return (np.stack([a0 + a1, a3 + a2, a0 - a1, a3 - a2], 1) >> 3).reshape(16)


def quantise(c, q, bias):
    """level = sign(c) * min(2047, (|c| + (q * bias >> 3)) // q): bias 4 rounds to nearest, 3 leaves a small dead zone."""
    c = np.asarray(c, np.int64)
    return np.sign(c) * np.minimum(MAX_LEVEL, (np.abs(c) + (q * bias >> 3)) // q)


# ---- prediction ---------------------------------------------------------------------------------------------------------------------------------------
def predictions(rec, mby, mbx, n):
    """The four predictions (DC, V, H, TM) of the n x n block at macroblock (mby, mbx) from the reconstructed plane."""
    y0, x0 = mby * n, mbx * n
    top = rec[y0 - 1, x0:x0 + n].astype(np.int64) if mby else np.full(n, 127, np.int64)
    left = rec[y0:y0 + n, x0 - 1].astype(np.int64) if mbx else np.full(n, 129, np.int64)
    tl = int(rec[y0 - 1, x0 - 1]) if mby and mbx else 127 if not mby else 129
    shift = 3 if n == 8 else 4
    if mby and mbx:
        dc = (top.sum() + left.sum() + n) >> (shift + 1)
    elif mby or mbx:
        dc = ((top.sum() if mby else left.sum()) * 2 + n) >> (shift + 1)
    else:
        dc = 128
    return [np.full((n, n), dc, np.int64), np.repeat(top[None], n, 0), np.repeat(left[:, None], n, 1),
            np.clip(left[:, None] + top[None] - tl, 0, 255)]


def _best(cost):
    return int(np.argmin(cost))                                                 # the first minimum: ties to the lower mode number


# ---- the boolean coder --------------------------------------------------------------------------------------------------------------------------------
class BoolCoder:
    def __init__(self):
        self.out, self.range, self.bottom, self.count = bytearray(), 255, 0, 24

    def put(self, bit, prob):
        split = 1 + (((self.range - 1) * int(prob)) >> 8)
        if bit:
            self.bottom += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            if self.bottom & (1 << 31):
                k = len(self.out) - 1
                while self.out[k] == 255:
                    self.out[k] = 0
                    k -= 1
                self.out[k] += 1
            self.bottom = (self.bottom << 1) & 0xFFFFFFFF
            self.count -= 1
            if not self.count:
                self.out.append(self.bottom >> 24)
                self.bottom &= (1 << 24) - 1
                self.count = 8
        return bit

    def bits(self, value, n):
        for k in range(n - 1, -1, -1):
            self.put(value >> k & 1, 128)

    def finish(self):
        for _ in range(32):
            self.put(0, 128)
        return bytes(self.out)


def put_coeffs(bw, kind, ctx, lv, first):
    """One block's levels (scan order) as tokens; returns whether any is non-zero."""
    last = max((n for n in range(first, 16) if lv[n]), default=-1)
    probs = COEF_PROBS[kind]
    n = first
    p = probs[BANDS[n]][ctx]
    if not bw.put(last >= 0, p[0]):
        return 0
    while n < 16:
        c = int(lv[n])
        n += 1
        v = abs(c)
        if not bw.put(v != 0, p[1]):
            p = probs[BANDS[n]][0]
            continue
        if not bw.put(v > 1, p[2]):
            p = probs[BANDS[n]][1]
        else:
            if not bw.put(v > 4, p[3]):
                if bw.put(v != 2, p[4]):
                    bw.put(v == 4, p[5])
            elif not bw.put(v > 10, p[6]):
                if not bw.put(v > 6, p[7]):
                    bw.put(v == 6, 159)
                else:
                    bw.put(v >= 9, 165)
                    bw.put(not v & 1, 145)
            else:
                if v < 19:
                    bw.put(0, p[8]), bw.put(0, p[9])
                    e, tab = v - 11, CAT3
                elif v < 35:
                    bw.put(0, p[8]), bw.put(1, p[9])
                    e, tab = v - 19, CAT4
                elif v < 67:
                    bw.put(1, p[8]), bw.put(0, p[10])
                    e, tab = v - 35, CAT5
                else:
                    bw.put(1, p[8]), bw.put(1, p[10])
                    e, tab = v - 67, CAT6
                for k, pr in enumerate(tab):
                    bw.put(e >> (len(tab) - 1 - k) & 1, pr)
            p = probs[BANDS[n]][2]
        bw.put(c < 0, 128)
        if n == 16 or not bw.put(n <= last, p[0]):
            return 1
    return 1


# ---- a frame ------------------------------------------------------------------------------------------------------------------------------------------
def analyse(rgb, q):
    """Predict, transform, quantise and reconstruct every macroblock in raster order."""
    H, W, _ = rgb.shape
    Y, U, V = rgb_to_yuv420(rgb)
    mbh, mbw = Y.shape[0] // 16, Y.shape[1] // 16
    ydc, yac, y2dc, y2ac, uvdc, uvac = quantisers(q)
    rec = [np.zeros_like(Y), np.zeros_like(U), np.zeros_like(V)]
    modes = np.zeros((mbh, mbw, 2), np.uint8)
    levels = np.zeros((mbh, mbw, 25, 16), np.int16)
    nz = np.zeros((mbh, mbw), np.uint32)
    zz = np.array(ZIGZAG)
    for my in range(mbh):
        for mx in range(mbw):
            src = Y[my * 16:my * 16 + 16, mx * 16:mx * 16 + 16].astype(np.int64)
            preds = predictions(rec[0], my, mx, 16)
            mode = _best([((src - p) ** 2).sum() for p in preds])
            pred = preds[mode]
            coef = np.stack([fdct(src[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] - pred[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4])
                             for by in range(4) for bx in range(4)])
            y2 = fwht(coef[:, 0])
            y2l = np.concatenate([quantise(y2[:1], y2dc, 4), quantise(y2[1:], y2ac, 3)])
            dcs = iwht(y2l * np.array([y2dc] + [y2ac] * 15))
            lv = levels[my, mx]
            lv[24] = y2l[zz]
            for b in range(16):
                by, bx = divmod(b, 4)
                l = quantise(coef[b], yac, 3)
                l[0] = 0
                lv[b] = l[zz]
                deq = l * yac
                deq[0] = dcs[b]
                rec[0][my * 16 + by * 4:my * 16 + by * 4 + 4, mx * 16 + bx * 4:mx * 16 + bx * 4 + 4] = \
                    idct_add(deq, pred[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4])
            srcs = [P[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8].astype(np.int64) for P in (U, V)]
            preds = [predictions(rec[k], my, mx, 8) for k in (1, 2)]
            uvmode = _best([((srcs[0] - preds[0][m]) ** 2).sum() + ((srcs[1] - preds[1][m]) ** 2).sum() for m in range(4)])
            for k in range(2):
                pred = preds[k][uvmode]
                for b in range(4):
                    by, bx = divmod(b, 2)
                    c = fdct(srcs[k][by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] - pred[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4])
                    l = np.concatenate([quantise(c[:1], uvdc, 4), quantise(c[1:], uvac, 3)])
                    lv[16 + 4 * k + b] = l[zz]
                    deq = l * np.array([uvdc] + [uvac] * 15)
                    rec[1 + k][my * 8 + by * 4:my * 8 + by * 4 + 4, mx * 8 + bx * 4:mx * 8 + bx * 4 + 4] = \
                        idct_add(deq, pred[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4])
            modes[my, mx] = mode, uvmode
            nz[my, mx] = sum(1 << b for b in range(25) if lv[b].any())
    return tuple(rec), modes, levels, nz


def skip_prob(mbs, skipped):
    """The probability (of 256) that a macroblock is NOT skipped, from the frame's own count, kept inside 1 .. 255."""
    return min(255, max(1, (mbs - skipped) * 255 // mbs))


def first_partition(q, partitions, filter_level, modes, nz):
    mbh, mbw = nz.shape
    bw = BoolCoder()
    bw.bits(0, 2)                                                               # colour space, clamping
    bw.bits(0, 1)                                                               # no segments
    bw.bits(0, 1), bw.bits(filter_level, 6), bw.bits(0, 3)                      # the normal filter, its level, sharpness 0
    bw.bits(0, 1)                                                               # no filter deltas
    bw.bits({1: 0, 2: 1, 4: 2, 8: 3}[partitions], 2)
    bw.bits(q, 7), bw.bits(0, 5)                                                # the index; no delta
    bw.bits(0, 1)                                                               # refresh_entropy_probs
    for pr in UPDATE_PROBS.reshape(-1):
        bw.put(0, int(pr))
    prob = skip_prob(mbh * mbw, int((nz == 0).sum()))
    bw.bits(1, 1), bw.bits(prob, 8)
    for my in range(mbh):
        for mx in range(mbw):
            bw.put(nz[my, mx] == 0, prob)
            ym, uvm = (int(m) for m in modes[my, mx])
            bw.put(1, 145)                                                      # a 16 x 16 mode
            if bw.put(ym in (2, 3), 156):
                bw.put(ym == 3, 128)
            else:
                bw.put(ym == 1, 163)
            if bw.put(uvm != 0, 142):
                if bw.put(uvm != 1, 114):
                    bw.put(uvm != 2, 183)
    return bw.finish()


def token_partition(levels, nz, part, partitions):
    mbh, mbw = nz.shape
    bw = BoolCoder()
    bit = lambda my, mx, b: int(nz[my, mx] >> b & 1) if my >= 0 and mx >= 0 else 0
    for my in range(part, mbh, partitions):
        for mx in range(mbw):
            if nz[my, mx] == 0:
                continue
            lv = levels[my, mx]
            put_coeffs(bw, 1, bit(my - 1, mx, 24) + bit(my, mx - 1, 24), lv[24], 0)
            for b in range(16):
                by, bx = divmod(b, 4)
                top = bit(my, mx, b - 4) if by else bit(my - 1, mx, b + 12)
                left = bit(my, mx, b - 1) if bx else bit(my, mx - 1, b + 3)
                put_coeffs(bw, 0, top + left, lv[b], 1)
            for b in range(16, 24):
                by, bx = divmod(b & 3, 2)
                top = bit(my, mx, b - 2) if by else bit(my - 1, mx, b + 2)
                left = bit(my, mx, b - 1) if bx else bit(my, mx - 1, b + 1)
                put_coeffs(bw, 2, top + left, lv[b], 0)
    return bw.finish()


def assemble(W, H, parts):
    """The first partition and the token partitions -> the 'VP8 ' payload."""
    first = parts[0]
    tag = 0 | 0 << 1 | 1 << 4 | len(first) << 5                                 # a key frame, profile 0, shown
    out = struct.pack("<I", tag)[:3] + b"\x9d\x01\x2a" + struct.pack("<HH", W, H) + first
    out += b"".join(struct.pack("<I", len(p))[:3] for p in parts[1:-1])
    return out + b"".join(parts[1:])


def encode_frame(rgb, quality=75, partitions=None, filter_level=None):
    rgb = np.asarray(rgb)
    H, W, _ = rgb.shape
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"a frame is 1 .. {MAX_SIDE} pixels a side, got {W} x {H}")
    q = quality_to_q(quality)
    partitions = default_partitions(H) if partitions is None else int(partitions)
    filter_level = default_filter_level(q) if filter_level is None else int(filter_level)
    if partitions not in (1, 2, 4, 8) or not 0 <= filter_level <= 63:
        raise ValueError("partitions must be 1, 2, 4 or 8 and filter_level 0 .. 63")
    recon, modes, levels, nz = analyse(rgb, q)
    parts = [first_partition(q, partitions, filter_level, modes, nz)] + [token_partition(levels, nz, p, partitions) for p in range(partitions)]
    return dict(payload=assemble(W, H, parts), parts=parts, recon=recon, modes=modes, levels=levels, nz=nz, skipped=int((nz == 0).sum()), q=q,
                filter_level=filter_level)


def _chunk(fourcc, body):
    return fourcc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def webp_file(payloads, W, H, duration=125, loop=0):
    """'VP8 ' payloads -> a still (one) or an animation (several), laid out as mmgt_amd.video_out.write_webp does."""
    u24 = lambda v: struct.pack("<I", v)[:3]
    if len(payloads) == 1:
        body = b"WEBP" + _chunk(b"VP8 ", payloads[0])
    else:
        size = u24(W - 1) + u24(H - 1)
        body = b"WEBP" + _chunk(b"VP8X", b"\x02\0\0\0" + size) + _chunk(b"ANIM", struct.pack("<IH", 0, loop))
        body += b"".join(_chunk(b"ANMF", u24(0) + u24(0) + size + u24(duration) + b"\x02" + _chunk(b"VP8 ", p)) for p in payloads)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def psnr(a, b):
    mse = ((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean()
    return 99.0 if mse == 0 else float(10 * np.log10(255 ** 2 / mse))


def case_image(kind, W, H):
    """The test inputs: noise, mask and photo are webpdec_cases.kind_image's; flat, black and smooth are defined here."""
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "flat":
        return np.broadcast_to(np.array([200, 90, 40], np.uint8), (H, W, 3)).copy()
    if kind == "black":
        return np.zeros((H, W, 3), np.uint8)
    if kind == "smooth":
        return np.stack([64 + (xx * 160) // max(1, W - 1), 32 + (yy * 190) // max(1, H - 1), 128 + ((xx + yy) * 100) // max(1, W + H - 2)],
                        -1).astype(np.uint8)
    from tests.webpdec_cases import kind_image
    return kind_image(kind, W, H)
