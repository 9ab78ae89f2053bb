"""CPU yardstick of the device WebP lossless decoder (csrc/webpdec.hip, mmgt_amd/video_in.py): the VP8L stream definition and libwebp's
animation composition restated in numpy and plain loops, with nothing imported from the product.  tests/test_webpdec.py holds it to PIL on every
byte; the product is then held to it stage by stage (entropy-coded words, ARGB words, composed canvases).

`decode_vp8l` keeps counters of the features a stream used, so that a test can say what its corpus reached."""
import struct

import numpy as np

CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
DISTANCE_MAP = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3),
                (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4),
                (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2),
                (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2),
                (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1),
                (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7), (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5),
                (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7),
                (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7)]
assert len(DISTANCE_MAP) == 120 and len(set(DISTANCE_MAP)) == 120


class Bad(ValueError):
    """A stream that does not decode."""


class _Probe(Exception):
    """count_groups has what it came for."""


class Bits:
    def __init__(self, data):
        self.v, self.n, self.pos = int.from_bytes(data, "little"), 8 * len(data), 0

    def read(self, k):
        out = (self.v >> self.pos) & ((1 << k) - 1)
        self.pos += k
        if self.pos > self.n:
            raise Bad("data exhausted")
        return out

    def peek(self, k):
        return (self.v >> self.pos) & ((1 << k) - 1)


class Code:
    """A canonical prefix code from its lengths; the stream holds a code's bits most significant first."""
    FAST = 10

    def __init__(self, lengths):
        used = [(l, s) for s, l in enumerate(lengths) if l]
        self.one = used[0][1] if len(used) == 1 else None
        if not used:
            raise Bad("a prefix code without symbols")
        if self.one is not None:
            return
        used.sort()
        if sum(1 << (15 - l) for l, _ in used) != 1 << 15:
            raise Bad("a prefix code that is not complete")
        self.fast, self.slow, code, prev = {}, {}, 0, used[0][0]
        for l, s in used:
            code <<= l - prev
            prev = l
            rev = int(format(code, f"0{l}b")[::-1], 2)
            if l <= self.FAST:
                for hi in range(1 << (self.FAST - l)):
                    self.fast[rev | hi << l] = (s, l)
            else:
                self.slow[(l, rev)] = s
            code += 1

    def read(self, br):
        if self.one is not None:
            return self.one
        hit = self.fast.get(br.peek(self.FAST))
        if hit:
            br.read(hit[1])
            return hit[0]
        for l in range(self.FAST + 1, 16):
            s = self.slow.get((l, br.peek(l)))
            if s is not None:
                br.read(l)
                return s
        raise Bad("bits that are no code")


def read_code(br, alphabet, c):
    lengths = [0] * alphabet
    if br.read(1):
        two = br.read(1)
        syms = [br.read(8 if br.read(1) else 1)]
        if two:
            syms.append(br.read(8))
        for s in syms:
            if s >= alphabet:
                raise Bad("a symbol outside the alphabet")
            lengths[s] = 1
        c["simple_codes"] += 1
    else:
        ncl = br.read(4) + 4
        cl = [0] * 19
        for k in range(ncl):
            cl[CL_ORDER[k]] = br.read(3)
        clc = Code(cl)
        tokens = alphabet
        if br.read(1):
            nb = 2 + 2 * br.read(3)
            tokens = 2 + br.read(nb)
            c["max_symbol"] += 1
            if tokens > alphabet:
                raise Bad("max_symbol above the alphabet")
        n, prev = 0, 8
        while n < alphabet and tokens > 0:
            tokens -= 1
            s = clc.read(br)
            if s < 16:
                lengths[n] = s
                n += 1
                prev = s or prev
            else:
                rep = (3 + br.read(2)) if s == 16 else (3 + br.read(3)) if s == 17 else (11 + br.read(7))
                if n + rep > alphabet:
                    raise Bad("a repeat past the alphabet")
                if s == 16:
                    lengths[n:n + rep] = [prev] * rep
                n += rep
        if sum(1 for l in lengths if l) == 1:
            c["one_symbol_normal_codes"] += 1
    return Code(lengths)


def prefix_value(br, p):
    if p < 4:
        return p + 1
    e = (p - 2) >> 1
    return ((2 + (p & 1)) << e) + br.read(e) + 1


def coded_image(br, w, h, main, c):
    """-> list of w * h ARGB words."""
    cache_bits = 0
    if br.read(1):
        cache_bits = br.read(4)
        if not 1 <= cache_bits <= 11:
            raise Bad("colour-cache bits outside 1 .. 11")
        c["cache_bits"].add(cache_bits)
    ent, pb, ew, groups = None, 0, 0, 1
    if main and br.read(1):
        pb = br.read(3) + 2
        ew = -(-w // (1 << pb))
        ent = [(p >> 8) & 0xffff for p in coded_image(br, ew, -(-h // (1 << pb)), False, c)]
        groups = max(ent) + 1
        c["groups"] = max(c["groups"], groups)
    if main and c.get("stop_after_groups"):
        raise _Probe(groups)
    green = 280 + ((1 << cache_bits) if cache_bits else 0)
    codes = [[read_code(br, a, c) for a in (green, 256, 256, 256, 40)] for _ in range(groups)]
    cache = [0] * (1 << cache_bits) if cache_bits else None
    shift = 32 - cache_bits
    out, n, pos = [0] * (w * h), w * h, 0
    while pos < n:
        g = codes[ent[(pos // w >> pb) * ew + (pos % w >> pb)]] if ent else codes[0]
        s = g[0].read(br)
        if s < 256:
            r = g[1].read(br)
            b = g[2].read(br)
            a = g[3].read(br)
            px = a << 24 | r << 16 | s << 8 | b
        elif s < 280:
            length = prefix_value(br, s - 256)
            v = prefix_value(br, g[4].read(br))
            if v > 120:
                dist = v - 120
                c["far_distances"] += 1
            else:
                xi, yi = DISTANCE_MAP[v - 1]
                dist = max(1, xi + yi * w)
                c["short_distance_codes"].add(v)
            if dist > pos:
                raise Bad("a distance beyond the pixels produced")
            if pos + length > n:
                raise Bad("a copy past the image")
            if dist < length:
                c["overlapping_copies"] += 1
            for i in range(length):
                px = out[pos + i - dist]
                out[pos + i] = px
                if cache is not None:
                    cache[(0x1e35a7bd * px & 0xffffffff) >> shift] = px
            pos += length
            continue
        else:
            px = cache[s - 280]
            c["cache_hits"] += 1
        out[pos] = px
        if cache is not None:
            cache[(0x1e35a7bd * px & 0xffffffff) >> shift] = px
        pos += 1
    return out


# ---- inverse transforms -------------------------------------------------------------------------------------------------------------------------------
def _avg(a, b):
    return (((a ^ b) & 0xfefefefe) >> 1) + (a & b)


def _channels(p):
    return p >> 24, (p >> 16) & 255, (p >> 8) & 255, p & 255


def _pack(ch):
    return ch[0] << 24 | ch[1] << 16 | ch[2] << 8 | ch[3]


def _clamp(v):
    return 0 if v < 0 else 255 if v > 255 else v


def predict(mode, L, T, TL, TR):
    if mode in (0, 14, 15):
        return 0xff000000
    if mode < 5:
        return (L, T, TR, TL)[mode - 1]
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode < 10:
        return _avg(*((L, TL), (L, T), (TL, T), (T, TR))[mode - 6])
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    l, t, c = _channels(L), _channels(T), _channels(TL)
    if mode == 11:
        return L if sum(abs(a - b) for a, b in zip(t, c)) < sum(abs(a - b) for a, b in zip(l, c)) else T
    if mode == 12:
        return _pack([_clamp(a + b - d) for a, b, d in zip(l, t, c)])
    a = _channels(_avg(L, T))
    return _pack([_clamp(v + int((v - d) / 2)) for v, d in zip(a, c)])      # int(): toward zero


def add_pixels(a, b):
    return ((a & 0xff00ff00) + (b & 0xff00ff00)) & 0xff00ff00 | ((a & 0x00ff00ff) + (b & 0x00ff00ff)) & 0x00ff00ff


def inverse_predictor(px, w, h, sub, bits, c):
    bw = -(-w // (1 << bits))
    for y in range(h):
        row = y * w
        for x in range(w):
            if y == 0:
                pred = 0xff000000 if x == 0 else px[x - 1]
            elif x == 0:
                pred = px[row - w]
            else:
                mode = (sub[(y >> bits) * bw + (x >> bits)] >> 8) & 15
                c["modes"].add(mode)
                tr = px[row - w + x + 1] if x + 1 < w else px[row]
                pred = predict(mode, px[row + x - 1], px[row - w + x], px[row - w + x - 1], tr)
            px[row + x] = add_pixels(px[row + x], pred)


def _i8(v):
    v = np.asarray(v, np.int64) & 255
    return v - ((v & 128) << 1)


def inverse_cross_colour(px, w, h, sub, bits):
    a = np.asarray(px, np.int64).reshape(h, w)
    bw = -(-w // (1 << bits))
    m = np.asarray(sub, np.int64).reshape(-1, bw)[np.arange(h)[:, None] >> bits, np.arange(w)[None] >> bits]
    g = (a >> 8) & 255
    r = ((a >> 16) + ((_i8(m) * _i8(g)) >> 5)) & 255
    b = (a + ((_i8(m >> 8) * _i8(g)) >> 5) + ((_i8(m >> 16) * _i8(r)) >> 5)) & 255
    return ((a & 0xff00ff00) | r << 16 | b).reshape(-1).tolist()


def add_green(px):
    a = np.asarray(px, np.int64)
    g = (a >> 8) & 255
    return ((a & 0xff00ff00) | (((a >> 16) + g) & 255) << 16 | ((a + g) & 255)).tolist()


def expand_palette(px, w, h, sub, k):
    pal, acc = [], 0
    for e in sub:
        acc = add_pixels(acc, e)
        pal.append(acc)
    pal = np.asarray(pal + [0] * (256 - len(pal)), np.int64)
    pw, per = -(-w // (1 << k)), 8 >> k
    a = np.asarray(px, np.int64).reshape(h, pw)
    x = np.arange(w)
    idx = ((a[:, x >> k] >> 8) & 255) >> ((x & ((1 << k) - 1)) * per)[None] & ((1 << per) - 1)
    return pal[idx].reshape(-1).tolist()


def new_counters():
    return {"transforms": set(), "modes": set(), "cache_bits": set(), "groups": 1, "max_symbol": 0, "simple_codes": 0, "one_symbol_normal_codes": 0,
            "far_distances": 0, "short_distance_codes": set(), "overlapping_copies": 0, "cache_hits": 0, "palette_overflow": 0}


def decode_vp8l(data, counters=None):
    """One VP8L payload -> dict: width, height, alpha_is_used, argb (H, W) uint32, and the decoder's stages: `transforms`, in the order read, as
    (type, bits, sub-image words, width it was read at, palette entries), and `main`, the entropy-coded image (H, main_width) uint32."""
    c = counters if counters is not None else new_counters()
    br = Bits(data)
    if br.read(8) != 0x2f:
        raise Bad("bad signature")
    W, H, alpha, version = br.read(14) + 1, br.read(14) + 1, br.read(1), br.read(3)
    if version:
        raise Bad("bad version")
    xs, transforms = W, []
    while br.read(1):
        t = br.read(2)
        if any(t == u[0] for u in transforms):
            raise Bad("a transform read twice")
        c["transforms"].add(t)
        if t in (0, 1):
            bits = br.read(3) + 2
            transforms.append((t, bits, coded_image(br, -(-xs // (1 << bits)), -(-H // (1 << bits)), False, c), xs, 0))
        elif t == 3:
            n = br.read(8) + 1
            k = 3 if n <= 2 else 2 if n <= 4 else 1 if n <= 16 else 0
            transforms.append((t, k, coded_image(br, n, 1, False, c), xs, n))
            xs = -(-xs // (1 << k))
        else:
            transforms.append((t, 0, [], xs, 0))
    main = coded_image(br, xs, H, True, c)
    px = list(main)
    for t, bits, sub, w, n in reversed(transforms):
        if t == 0:
            inverse_predictor(px, w, H, sub, bits, c)
        elif t == 1:
            px = inverse_cross_colour(px, w, H, sub, bits)
        elif t == 2:
            px = add_green(px)
        else:
            packed = np.asarray(px, np.int64).reshape(H, -1)
            per = 8 >> bits
            x = np.arange(w)
            idx = ((packed[:, x >> bits] >> 8) & 255) >> ((x & ((1 << bits) - 1)) * per)[None] & ((1 << per) - 1)
            c["palette_overflow"] += int((idx >= n).sum())
            px = expand_palette(px, w, H, sub, bits)
    return {"width": W, "height": H, "alpha_is_used": alpha, "argb": np.asarray(px, np.uint32).reshape(H, W), "transforms": transforms,
            "main": np.asarray(main, np.uint32).reshape(H, xs), "counters": c, "bits_used": br.pos}


def count_groups(data):
    """The number of prefix-code groups of one VP8L payload's main image, without decoding its pixels."""
    c = new_counters()
    c["stop_after_groups"] = True
    try:
        decode_vp8l(data, c)
    except _Probe as p:
        return p.args[0]
    raise AssertionError("unreachable")


# ---- container and composition ------------------------------------------------------------------------------------------------------------------------
def chunks(data, pos, end):
    while pos + 8 <= end:
        kind, (ln,) = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])
        yield kind, data[pos + 8:pos + 8 + ln]
        pos += 8 + ln + (ln & 1)


def _u24(b, at):
    return b[at] | b[at + 1] << 8 | b[at + 2] << 16


def file_frames(data):
    """A lossless WebP file -> (canvas W, H, [dict(x, y, w, h, blend, dispose, payload)])."""
    assert data[:4] == b"RIFF" and data[8:12] == b"WEBP"
    top = list(chunks(data, 12, len(data)))
    frames, canvas = [], None
    for kind, body in top:
        if kind == b"VP8X":
            canvas = (_u24(body, 4) + 1, _u24(body, 7) + 1)
        elif kind == b"VP8L":
            frames.append({"x": 0, "y": 0, "w": None, "h": None, "blend": False, "dispose": False, "payload": body})
        elif kind == b"ANMF":
            sub = dict(chunks(body, 16, len(body)))
            frames.append({"x": 2 * _u24(body, 0), "y": 2 * _u24(body, 3), "w": _u24(body, 6) + 1, "h": _u24(body, 9) + 1,
                           "blend": not body[15] & 2, "dispose": bool(body[15] & 1), "payload": sub[b"VP8L"]})
    if canvas is None:
        bits = Bits(frames[0]["payload"][:5])
        bits.read(8)
        canvas = (bits.read(14) + 1, bits.read(14) + 1)
    return canvas[0], canvas[1], frames


def compose(W, H, frames, decoded, stats=None):
    """libwebp's WebPAnimDecoder: frames as file_frames gives them, decoded[k] = decode_vp8l's dict -> list of (H, W, 4) uint8 RGBA canvases."""
    stats = stats if stats is not None else {}
    canvas = np.zeros((H, W, 4), np.int64)
    out, prev, prev_key = [], None, False
    for k, (f, d) in enumerate(zip(frames, decoded)):
        w, h = d["width"], d["height"]
        full = (f["x"], f["y"], w, h) == (0, 0, W, H)
        if k == 0:
            key, why = True, "first"
        elif full and (not d["alpha_is_used"] or not f["blend"]):
            key, why = True, "covers"
        elif prev["dispose"] and (prev["full"] or prev_key):
            key, why = True, "after a disposed key frame"
        else:
            key, why = False, None
        stats.setdefault("keys", []).append(key)
        if key:
            stats[f"key: {why}"] = stats.get(f"key: {why}", 0) + 1
        before = canvas.copy()
        hole = np.zeros((H, W), bool)
        if key:
            canvas[:] = 0
        elif prev["dispose"]:
            hole[prev["y"]:prev["y"] + prev["h"], prev["x"]:prev["x"] + prev["w"]] = True
            canvas[hole] = 0
            before = canvas.copy()
        a = d["argb"].astype(np.int64)
        src = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], -1)
        ys, xs = slice(f["y"], f["y"] + h), slice(f["x"], f["x"] + w)
        canvas[ys, xs] = src
        if f["blend"] and not key:
            dst = before[ys, xs]
            sa, da = src[..., 3], dst[..., 3]
            todo = (sa != 255) & ~hole[ys, xs]
            stats["inside the disposed rectangle"] = stats.get("inside the disposed rectangle", 0) + int(((sa != 255) & hole[ys, xs]).sum())
            stats["partial-alpha blends"] = stats.get("partial-alpha blends", 0) + int((todo & (sa > 0) & (da > 0)).sum())
            fd = (da * (256 - sa)) >> 8
            alpha = sa + fd
            scale = (1 << 24) // np.maximum(alpha, 1)
            mixed = np.concatenate([((src[..., :3] * sa[..., None] + dst[..., :3] * fd[..., None]) * scale[..., None]) >> 24, alpha[..., None]], -1)
            mixed = np.where((sa == 0)[..., None], dst, mixed)
            canvas[ys, xs] = np.where(todo[..., None], mixed, src)
        out.append(canvas.astype(np.uint8).copy())
        prev, prev_key = {"x": f["x"], "y": f["y"], "w": w, "h": h, "dispose": f["dispose"], "full": full}, key
    return out


def decode_file(data, counters=None, stats=None):
    """A lossless WebP file, still or animated -> list of (H, W, 4) uint8 RGBA canvases, one per frame."""
    W, H, frames = file_frames(data)
    decoded = [decode_vp8l(f["payload"], counters) for f in frames]
    return compose(W, H, frames, decoded, stats)
