"""CPU yardstick of the device WebP lossless writer (csrc/webp.hip, mmgt_amd/video_out.py): the stream definition restated in numpy /
plain Python, with nothing imported from the product (the package-merge, the canonical codes and the bit writer are those of tests/png_ref.py).
One VP8L bitstream per frame, RGB in, alpha 255 throughout.

 1. transforms  subtract green, then the predictor transform with blocks of 16 x 16 pixels over the subtract-green pixels (255, r - g, g, b - g), per
                channel mod 256; of the 14 modes a block takes the one with the smallest sum of min(v, 256 - v) over its residuals' r, g, b, the
                lowest mode on a tie.
 2. strips      strip_rows rows each (the last may be shorter); they bound the matches and change nothing else.
 3. tokens      within a strip over whole residual pixels, the left pixel only: at p >= 1 with r = pixels from p on that equal pixel p - 1 (at most
                4096), r >= 3 is a match of length r, else a literal; position 0 is a literal.
 4. codes       one group of five prefix codes per frame from the sums of the strips' histograms: package-merge, limit 15 and 7 (code-length
                code); an alphabet with one used symbol (or none) is a simple code and its symbol costs no bits.
 5. packing     LSB-first, prefix codes bit-reversed; header, mode sub-image, codes, the strips' tokens back to back, zero bits up to a byte."""
import struct

import numpy as np

from tests.png_ref import BitWriter, canonical_codes, code_lengths

PREDICTOR_BITS = 4
MAX_LENGTH = 4096
CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
BLACK = (255, 0, 0, 0)                # a, r, g, b


# ---- 1. transforms ----------------------------------------------------------------------------------------------------------------------------------
def subtract_green(frame):
    """(H, W, 3) uint8 RGB -> (H, W, 4) int64 in the order a, r, g, b."""
    x = np.asarray(frame).astype(np.int64)
    out = np.empty(x.shape[:2] + (4,), np.int64)
    out[..., 0] = 255
    out[..., 1] = (x[..., 0] - x[..., 1]) & 255
    out[..., 2] = x[..., 1]
    out[..., 3] = (x[..., 2] - x[..., 1]) & 255
    return out


def add_green(px):
    """The inverse: (H, W, 4) a, r, g, b -> (H, W, 3) uint8 RGB."""
    px = np.asarray(px)
    return np.stack([(px[..., 1] + px[..., 2]) & 255, px[..., 2], (px[..., 3] + px[..., 2]) & 255], axis=-1).astype(np.uint8)


def predict_pixel(mode, L, T, TL, TR):
    """One pixel, 4-tuples of channels, no forced cases."""
    avg = lambda p, q: tuple((a + b) >> 1 for a, b in zip(p, q))
    clamp = lambda v: 0 if v < 0 else 255 if v > 255 else v
    if mode == 0:
        return BLACK
    if mode in (1, 2, 3, 4):
        return (L, T, TR, TL)[mode - 1]
    if mode == 5:
        return avg(avg(L, TR), T)
    if mode in (6, 7, 8, 9):
        return avg(*((L, TL), (L, T), (TL, T), (T, TR))[mode - 6])
    if mode == 10:
        return avg(avg(L, TL), avg(T, TR))
    if mode == 11:
        return L if sum(abs(t - c) for t, c in zip(T, TL)) < sum(abs(l - c) for l, c in zip(L, TL)) else T
    if mode == 12:
        return tuple(clamp(l + t - c) for l, t, c in zip(L, T, TL))
    if mode == 13:
        a = avg(L, T)
        return tuple(clamp(v + int((v - c) / 2)) for v, c in zip(a, TL))            # int(): toward zero, as C divides
    raise ValueError(mode)


def predictions(px):
    """(H, W, 4) -> (14, H, W, 4): every mode's prediction of every pixel, the forced ones included."""
    px = np.asarray(px, np.int64)
    H, W, _ = px.shape
    L, T, TL, TR = (np.zeros_like(px) for _ in range(4))
    L[:, 1:] = px[:, :-1]
    T[1:] = px[:-1]
    TL[1:, 1:] = px[:-1, :-1]
    TR[1:, :-1] = px[:-1, 1:]
    TR[1:, W - 1] = px[1:, 0]                                                           # the pixel after the row above's last one
    avg = lambda p, q: (p + q) >> 1
    out = np.empty((14,) + px.shape, np.int64)
    out[0] = BLACK
    out[1], out[2], out[3], out[4] = L, T, TR, TL
    out[5] = avg(avg(L, TR), T)
    out[6], out[7], out[8], out[9] = avg(L, TL), avg(L, T), avg(TL, T), avg(T, TR)
    out[10] = avg(avg(L, TL), avg(T, TR))
    pick_l = np.abs(T - TL).sum(-1) < np.abs(L - TL).sum(-1)
    out[11] = np.where(pick_l[..., None], L, T)
    out[12] = np.clip(L + T - TL, 0, 255)
    a = avg(L, T)
    d = a - TL
    out[13] = np.clip(a + np.sign(d) * (np.abs(d) // 2), 0, 255)
    out[:, 0, 1:] = L[0, 1:]
    out[:, 1:, 0] = T[1:, 0]
    out[:, 0, 0] = BLACK
    return out


def predictor_transform(px):
    """(H, W, 4) -> (modes (bh, bw), residuals (H, W, 4), costs (bh, bw, 14))."""
    H, W, _ = px.shape
    B = 1 << PREDICTOR_BITS
    res = (px[None] - predictions(px)) & 255
    cost = np.minimum(res, 256 - res)[..., 1:].sum(-1)                                  # (14, H, W)
    bh, bw = -(-H // B), -(-W // B)
    modes, costs = np.zeros((bh, bw), np.int64), np.zeros((bh, bw, 14), np.int64)
    out = np.empty_like(px)
    for by in range(bh):
        for bx in range(bw):
            ys, xs = slice(by * B, min(H, by * B + B)), slice(bx * B, min(W, bx * B + B))
            c = [int(cost[m, ys, xs].sum()) for m in range(14)]
            costs[by, bx] = c
            modes[by, bx] = c.index(min(c))                                            # index(): the lowest mode on a tie
            out[ys, xs] = res[modes[by, bx], ys, xs]
    return modes, out, costs


def inverse_predictor(modes, residuals):
    """What a decoder does: (bh, bw) modes and (H, W, 4) residuals -> (H, W, 4) pixels, one after the other."""
    res = np.asarray(residuals, np.int64)
    H, W, _ = res.shape
    px = np.zeros_like(res)
    for y in range(H):
        for x in range(W):
            if y == 0:
                pred = BLACK if x == 0 else tuple(px[0, x - 1])
            elif x == 0:
                pred = tuple(px[y - 1, 0])
            else:
                tr = px[y - 1, x + 1] if x + 1 < W else px[y, 0]
                pred = predict_pixel(int(modes[y >> PREDICTOR_BITS, x >> PREDICTOR_BITS]), tuple(int(v) for v in px[y, x - 1]),
                                     tuple(int(v) for v in px[y - 1, x]), tuple(int(v) for v in px[y - 1, x - 1]), tuple(int(v) for v in tr))
            px[y, x] = (res[y, x] + np.array(pred)) & 255
    return px


def words(px):
    """(..., 4) a, r, g, b -> ARGB words."""
    px = np.asarray(px, np.int64)
    return px[..., 0] << 24 | px[..., 1] << 16 | px[..., 2] << 8 | px[..., 3]


# ---- 3. tokens --------------------------------------------------------------------------------------------------------------------------------------
def tokens(strip):
    """ARGB words of one strip -> list of ("lit", word) / ("len", length)."""
    d = [int(v) for v in strip]
    out, p = [("lit", d[0])], 1
    while p < len(d):
        r = 0
        while r < MAX_LENGTH and p + r < len(d) and d[p + r] == d[p - 1]:
            r += 1
        if r >= 3:
            out.append(("len", r))
            p += r
        else:
            out.append(("lit", d[p]))
            p += 1
    return out


def prefix_value(v):
    """A length or distance value >= 1 -> (prefix symbol, extra bits, extra value)."""
    if v <= 4:
        return v - 1, 0, 0
    d = v - 1
    hb = d.bit_length() - 1
    sb = (d >> (hb - 1)) & 1
    return 2 * hb + sb, hb - 1, d & ((1 << (hb - 1)) - 1)


def strip_histograms(strip):
    """-> (green + length [280], red [256], blue [256], matches)."""
    g, r, b, m = [0] * 280, [0] * 256, [0] * 256, 0
    for kind, v in tokens(strip):
        if kind == "lit":
            g[v >> 8 & 255] += 1
            r[v >> 16 & 255] += 1
            b[v & 255] += 1
        else:
            g[256 + prefix_value(v)[0]] += 1
            m += 1
    return g, r, b, m


# ---- 4. codes ---------------------------------------------------------------------------------------------------------------------------------------
def rle_code_lengths(seq):
    """The code lengths as (symbol, extra bits, extra value) of the code-length alphabet.  `prev` starts at 8 and only a length written as itself
    changes it: a non-zero length equal to prev with 3 or more equal lengths from here on is 16 for min(run, 6) of them."""
    out, i, prev = [], 0, 8
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
            i = j
        elif v == prev and run >= 3:
            k = min(run, 6)
            out.append((16, 2, k - 3))
            i += k
        else:
            out.append((v, 0, 0))
            prev = v
            i += 1
    return out


def prefix_code(bw, counts):
    """Writes the code of one alphabet and returns (lengths, canonical codes) as the pixels are coded with them: all zero for a simple code."""
    counts = [int(c) for c in counts]
    used = [s for s, c in enumerate(counts) if c]
    if len(used) <= 1:
        s = used[0] if used else 0
        assert s < 256
        bw.put(1, 1)
        bw.put(0, 1)
        if s < 2:
            bw.put(0, 1)
            bw.put(s, 1)
        else:
            bw.put(1, 1)
            bw.put(s, 8)
        return [0] * len(counts), [0] * len(counts)
    lengths = code_lengths(counts, 15)
    syms = rle_code_lengths(lengths)
    cl_hist = [0] * 19
    for s, _, _ in syms:
        cl_hist[s] += 1
    cl = code_lengths(cl_hist, 7)
    cl_codes = canonical_codes(cl)
    ncl = max(4, max(k for k in range(19) if cl[CL_ORDER[k]]) + 1)
    one = sum(1 for v in cl if v) == 1                                                  # a one-symbol code is read with zero bits
    bw.put(0, 1)
    bw.put(ncl - 4, 4)
    for k in range(ncl):
        bw.put(cl[CL_ORDER[k]], 3)
    bw.put(0, 1)                                                                        # max_symbol is not used
    for s, eb, ev in syms:
        if not one:
            bw.huff(cl_codes[s], cl[s])
        bw.put(ev, eb)
    return lengths, canonical_codes(lengths)


# ---- 5. the frame -----------------------------------------------------------------------------------------------------------------------------------
def frame_parts(frame, strip_rows):
    """(H, W, 3) uint8 -> dict of everything a test compares: modes, residual words, per-strip histograms, header bits, per-strip bits, payload."""
    frame = np.asarray(frame)
    H, W, _ = frame.shape
    modes, res, costs = predictor_transform(subtract_green(frame))
    w = words(res)
    strips = [w[y:y + strip_rows].reshape(-1) for y in range(0, H, strip_rows)]
    hists = [strip_histograms(s) for s in strips]
    g = [sum(h[0][k] for h in hists) for k in range(280)]
    r = [sum(h[1][k] for h in hists) for k in range(256)]
    b = [sum(h[2][k] for h in hists) for k in range(256)]
    matches = sum(h[3] for h in hists)
    alpha = [0] * 256
    alpha[0] = sum(g[:256])
    dist = [0] * 40
    dist[1] = matches

    bw = BitWriter()
    bw.put(0x2F, 8)
    bw.put(W - 1, 14)
    bw.put(H - 1, 14)
    bw.put(0, 1)
    bw.put(0, 3)
    bw.put(1, 1)
    bw.put(2, 2)                                                                        # subtract green
    bw.put(1, 1)
    bw.put(0, 2)                                                                        # predictor
    bw.put(PREDICTOR_BITS - 2, 3)
    bw.put(0, 1)                                                                        # the sub-image: no colour cache
    mg, zero, a255 = [0] * 280, [0] * 256, [0] * 256
    for m in modes.reshape(-1):
        mg[int(m)] += 1
    zero[0] = a255[255] = modes.size
    ml, mc = prefix_code(bw, mg)
    for counts in (zero, zero, a255, [0] * 40):
        prefix_code(bw, counts)
    for m in modes.reshape(-1):
        bw.huff(mc[int(m)], ml[int(m)])
    bw.put(0, 1)                                                                        # no further transform
    bw.put(0, 1)                                                                        # no colour cache
    bw.put(0, 1)                                                                        # no meta prefix codes
    (gl, gc), (rl, rc), (bl, bc), _, _ = [prefix_code(bw, c) for c in (g, r, b, alpha, dist)]
    header_bits = bw.n
    strip_bits = []
    for s in strips:
        n0 = bw.n
        for kind, v in tokens(s):
            if kind == "lit":
                bw.huff(gc[v >> 8 & 255], gl[v >> 8 & 255])
                bw.huff(rc[v >> 16 & 255], rl[v >> 16 & 255])
                bw.huff(bc[v & 255], bl[v & 255])                                      # alpha: the one-symbol code, no bits
            else:
                sym, eb, ev = prefix_value(v)
                bw.huff(gc[256 + sym], gl[256 + sym])
                bw.put(ev, eb)                                                          # the distance: the one-symbol code, no bits
        strip_bits.append(bw.n - n0)
    return {"modes": modes, "costs": costs, "words": w, "hist": hists, "header_bits": header_bits, "strip_bits": strip_bits, "payload": bw.bytes(),
            "tokens": [tokens(s) for s in strips]}


def encode_frames(frames, strip_rows):
    """(n, H, W, 3) uint8 -> one VP8L payload per frame."""
    return [frame_parts(f, strip_rows)["payload"] for f in np.asarray(frames)]


# ---- containers -------------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, body):
    return kind + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def u24(v):
    return struct.pack("<I", v)[:3]


def duration_ms(fps):
    return max(1, int(1000 / fps + 0.5))


def webp_file(blobs, W, H, fps, loop=0):
    if len(blobs) == 1:
        body = b"WEBP" + chunk(b"VP8L", blobs[0])
    else:
        body = b"WEBP" + chunk(b"VP8X", b"\x02\0\0\0" + u24(W - 1) + u24(H - 1)) + chunk(b"ANIM", struct.pack("<IH", 0, loop))
        for b in blobs:
            body += chunk(b"ANMF", u24(0) + u24(0) + u24(W - 1) + u24(H - 1) + u24(duration_ms(fps)) + b"\x02" + chunk(b"VP8L", b))
    return b"RIFF" + struct.pack("<I", len(body)) + body


def parse_chunks(data):
    """WebP file -> list of (fourcc, body); checks the RIFF size and the padding."""
    assert data[:4] == b"RIFF" and data[8:12] == b"WEBP" and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    out, p = [], 12
    while p < len(data):
        kind, (ln,) = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])
        out.append((kind, data[p + 8:p + 8 + ln]))
        p += 8 + ln + (ln & 1)
    assert p == len(data)
    return out


# ---- test inputs ------------------------------------------------------------------------------------------------------------------------------------
def mask_frames(n, H, W):
    """Flat white shapes on black, as a hands or face mask has them."""
    out = np.zeros((n, H, W, 3), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(n):
        out[f][(yy - H * 0.4 - f) ** 2 * 4 + (xx - W * 0.5) ** 2 < (min(H, W) * 0.3) ** 2] = 255
        out[f][(yy > H * 0.7) & (abs(xx - W * 0.3 - 2 * f) < W * 0.12)] = 255
    return out


def gradient_frames(n):
    """(n, 1, 256, 3): one row whose steps from pixel to pixel take every value of red and of blue exactly once (a one-row frame is mode 0
    throughout, so the steps are the residuals).  All 256 red lengths and all 256 blue lengths are then 8, and with `prev` starting at 8 each is
    written with the ONE code-length symbol 16: the code-length code that is read with zero bits."""
    out = np.empty((n, 1, 256, 3), np.uint8)
    x = np.arange(256)
    for f in range(n):
        res = np.stack([0 * x, x, (5 * x + f) & 255, ((3 + 2 * f) * x) & 255], axis=-1)[None]
        out[f] = add_green(inverse_predictor(np.zeros((1, 16), np.int64), res))
    return out


def run_frame(runs, W):
    """A black frame of width W with one marker pixel after every run of black of the given lengths, behind a first row (and one more pixel) of
    black: under mode 0 the residual of a pixel is the pixel, and a marker makes every other mode dearer, so the residuals are these runs.
    -> ((H, W, 3) uint8, the run lengths as they are in the residuals)."""
    pos, at = [], W + 1
    for k in runs:
        at += k
        pos.append(at)
        at += 1
    H = -(-(at + 3) // W)
    img = np.zeros((H * W, 3), np.uint8)
    for k, p in enumerate(pos):
        assert p % W != 0, "a marker in column 0 is predicted from above whatever the mode"
        img[p] = (200, 10, 30) if k & 1 else (90, 250, 40)
    return img.reshape(H, W, 3), [W + 1 + runs[0]] + list(runs[1:]) + [H * W - at]
