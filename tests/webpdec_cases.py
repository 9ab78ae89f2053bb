"""Inputs of the WebP lossless decoder's tests: PIL-written stills and animations, hand-assembled animation containers, and a small
token-level VP8L writer for streams that no stock writer emits.  PIL (libwebp) is the decoder of record: `pil_rgb` / `pil_rgba` give what a file
must decode to.  Everything is seeded and computed once per process."""
import functools
import io
import struct

import numpy as np
from PIL import Image, ImageSequence

from tests import webp_ref as E
from tests import webpdec_ref as R
from tests.png_ref import BitWriter

METHODS, QUALITIES = (0, 2, 4, 6), (0, 50, 100)
SIZES = ((1, 1), (300, 1), (1, 300), (16, 17), (17, 16), (13, 29), (21, 131))           # (W, H)


def pil_rgb(data):
    return np.stack([np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(data)))])


def pil_rgba(data):
    return np.stack([np.asarray(f.convert("RGBA")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(data)))])


def save(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="WEBP", lossless=True, **kw)
    return b.getvalue()


# ---- PIL-written stills -------------------------------------------------------------------------------------------------------------------------------
def kind_image(kind, W, H, seed=0):
    rng = np.random.default_rng([seed, W, H, sum(kind.encode())])
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "ramps":
        return np.stack([xx * 3 + yy, yy * 5, xx + 2 * yy], -1).astype(np.uint8)
    if kind == "mask":
        return np.repeat(((((yy - H * 0.4) ** 2 * 4 + (xx - W * 0.5) ** 2 < (min(H, W) * 0.3) ** 2) | ((yy > H * 0.7) & (abs(xx - W * 0.3) < W * 0.12)))
                          * 255).astype(np.uint8)[..., None], 3, -1)
    if kind.startswith("palette"):
        n = int(kind[7:])
        return rng.integers(0, 256, (n, 3)).astype(np.uint8)[rng.integers(0, n, (H, W))]
    if kind == "tiles":
        tile = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
        return np.tile(tile, (-(-H // 5), -(-W // 7), 1))[:H, :W].copy()
    if kind == "photo":
        return np.clip(np.stack([xx * 3 + yy, 255 - yy * 4, 90 + xx - yy], -1) + rng.integers(-5, 6, (H, W, 3)), 0, 255).astype(np.uint8)
    if kind == "rgba":
        return rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    raise KeyError(kind)


KINDS = ("noise", "ramps", "mask", "palette2", "palette3", "palette12", "palette40", "tiles", "photo", "rgba")


def mixed_frame(W=200, H=135):
    """Smooth, noise and a repeated band in one frame."""
    rng = np.random.default_rng(7)
    a = kind_image("ramps", W, H)
    a[40:80, 30:120] = rng.integers(0, 256, (40, 90, 3))
    band = rng.integers(0, 256, (6, W, 3)).astype(np.uint8)
    for y in range(90, 126, 6):
        a[y:y + 6] = band
    return a


@functools.lru_cache(None)
def stills():
    """{name: file bytes}: every kind at 67 x 45 over methods x qualities; three kinds at the odd sizes; the mixed frame; a frame of eight prefix-code groups; two flat frames."""
    out = {}
    for kind in KINDS:
        a = kind_image(kind, 67, 45)
        for m in METHODS:
            for q in QUALITIES:
                out[f"{kind}-67x45-m{m}-q{q}"] = save(a, method=m, quality=q, **({"exact": True} if kind == "rgba" else {}))
    for W, H in SIZES:
        for kind in ("photo", "palette3", "mask"):
            for m in (0, 4):
                out[f"{kind}-{W}x{H}-m{m}-q50"] = save(kind_image(kind, W, H), method=m, quality=50)
    for m in (0, 6):
        out[f"mixed-200x135-m{m}-q100"] = save(mixed_frame(), method=m, quality=100)
    out["photo-160x120-m4-q75"] = save(kind_image("photo", 160, 120), method=4, quality=75)      # eight prefix-code groups
    for W, H, m in ((256, 256, 4), (300, 300, 2)):                                      # one flat colour: a group whose only green symbol is a length
        out[f"flat-{W}x{H}-m{m}-q0"] = save(np.full((H, W, 3), 77, np.uint8), method=m, quality=0)
    return out


def textured_frame(W, H, tile=16, seed=3):
    """Tiles of differing texture (ramps, products, noise of differing strength): libwebp gives such a frame many prefix-code groups."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.zeros((H, W, 3), np.int64)
    for ty in range(0, H, tile):
        for tx in range(0, W, tile):
            k, base, amp = rng.integers(0, 6), rng.integers(0, 200, 3), int(rng.integers(2, 60))
            y, x = yy[ty:ty + tile, tx:tx + tile], xx[ty:ty + tile, tx:tx + tile]
            t = [x * 3, y * 5, (x ^ y) * 2, (x * y) % 64, rng.integers(0, amp, x.shape), (x // 4 + y // 3) * 9][k]
            a[ty:ty + tile, tx:tx + tile] = base + np.stack([t % (amp + 1), (t * 2) % (amp + 3), rng.integers(0, amp, x.shape)], -1)
    return np.clip(a, 0, 255).astype(np.uint8)


@functools.lru_cache(None)
def many_groups():
    """A PIL-written 640 x 480 still of 89 prefix-code groups: more than a frame's first scratch allowance holds."""
    return save(textured_frame(640, 480), method=4, quality=100)


def vp8l_of(data):
    """The first VP8L payload of a still."""
    return next(body for kind, body in E.parse_chunks(data) if kind == b"VP8L")


# ---- a token-level VP8L writer ------------------------------------------------------------------------------------------------------------------------
def _coded_image(bw, w, tokens, cache_bits=0, main=False):
    """tokens: ("px", argb) | ("copy", length, distance code value).  A pixel that the colour cache holds at its key goes out as a cache symbol."""
    bw.put(1 if cache_bits else 0, 1)
    if cache_bits:
        bw.put(cache_bits, 4)
    if main:
        bw.put(0, 1)
    key = lambda p: (0x1e35a7bd * p & 0xffffffff) >> (32 - cache_bits)
    cache, out, ops = [0] * (1 << cache_bits), [], []
    for t in tokens:
        if t[0] == "px":
            p = t[1]
            if cache_bits and cache[key(p)] == p and out:
                ops.append(("cache", key(p)))
            else:
                ops.append(("lit", p))
            out.append(p)
            if cache_bits:
                cache[key(p)] = p
        else:
            _, length, v = t
            if v > 120:
                dist = v - 120
            else:
                xi, yi = R.DISTANCE_MAP[v - 1]
                dist = max(1, xi + yi * w)
            assert dist <= len(out)
            for _ in range(length):
                p = out[-dist]
                out.append(p)
                if cache_bits:
                    cache[key(p)] = p
            ops.append(("copy", E.prefix_value(length), E.prefix_value(v)))
    green = [0] * (280 + ((1 << cache_bits) if cache_bits else 0))
    red, blue, alpha, dist_h = [0] * 256, [0] * 256, [0] * 256, [0] * 40
    for op in ops:
        if op[0] == "lit":
            p = op[1]
            green[p >> 8 & 255] += 1
            red[p >> 16 & 255] += 1
            blue[p & 255] += 1
            alpha[p >> 24] += 1
        elif op[0] == "cache":
            green[280 + op[1]] += 1
        else:
            green[256 + op[1][0]] += 1
            dist_h[op[2][0]] += 1
    (gl, gc), (rl, rc), (bl, bc), (al, ac), (dl, dc) = [E.prefix_code(bw, c) for c in (green, red, blue, alpha, dist_h)]
    for op in ops:
        if op[0] == "lit":
            p = op[1]
            bw.huff(gc[p >> 8 & 255], gl[p >> 8 & 255])
            bw.huff(rc[p >> 16 & 255], rl[p >> 16 & 255])
            bw.huff(bc[p & 255], bl[p & 255])
            bw.huff(ac[p >> 24], al[p >> 24])
        elif op[0] == "cache":
            bw.huff(gc[280 + op[1]], gl[280 + op[1]])
        else:
            (ls, leb, lev), (ds, deb, dev) = op[1], op[2]
            bw.huff(gc[256 + ls], gl[256 + ls])
            bw.put(lev, leb)
            bw.huff(dc[ds], dl[ds])
            bw.put(dev, deb)
    return out, ops


def vp8l_stream(W, H, tokens, transforms=(), cache_bits=0, alpha=1):
    """transforms: ("predictor", bits, [modes]) | ("palette", [entries as stored, i.e. differences]) | ("green",) in the order written; the tokens
    are those of the image as the transforms leave it (residuals, or packed indices in green)."""
    bw = BitWriter()
    bw.put(0x2F, 8)
    bw.put(W - 1, 14)
    bw.put(H - 1, 14)
    bw.put(alpha, 1)
    bw.put(0, 3)
    xs = W
    for t in transforms:
        bw.put(1, 1)
        if t[0] == "predictor":
            bw.put(0, 2)
            bw.put(t[1] - 2, 3)
            _coded_image(bw, -(-xs // (1 << t[1])), [("px", 0xff000000 | m << 8) for m in t[2]])
        elif t[0] == "palette":
            n = len(t[1])
            bw.put(3, 2)
            bw.put(n - 1, 8)
            _coded_image(bw, n, [("px", e) for e in t[1]])
            xs = -(-xs // (1 << (3 if n <= 2 else 2 if n <= 4 else 1 if n <= 16 else 0)))
        else:
            bw.put(2, 2)
    bw.put(0, 1)
    out, ops = _coded_image(bw, xs, tokens, cache_bits, main=True)
    assert len(out) == xs * H, (len(out), xs, H)
    return bw.bytes()


def still_file(payload):
    return b"RIFF" + struct.pack("<I", 4 + len(E.chunk(b"VP8L", payload))) + b"WEBP" + E.chunk(b"VP8L", payload)


def _rand_px(rng, n, colours=None):
    if colours is not None:
        return [int(colours[i]) for i in rng.integers(0, len(colours), n)]
    return [int(v) for v in rng.integers(0, 1 << 32, n, dtype=np.uint64)]


@functools.lru_cache(None)
def crafted():
    """{name: (file bytes, W, H)}: streams no stock writer emits."""
    rng = np.random.default_rng(11)
    out = {}
    for W in (20, 3):                                                                   # each of the 120 short distance codes
        tokens = [("px", p) for p in _rand_px(rng, 160)]
        for v in range(1, 121):
            tokens += [("copy", 2, v), ("px", _rand_px(rng, 1)[0])]
        tokens += [("px", p) for p in _rand_px(rng, (-520) % W)]
        H = (520 + (-520) % W) // W
        out[f"short-distances-w{W}"] = (still_file(vp8l_stream(W, H, tokens)), W, H)
    modes = [m % 16 for m in range(3 * 5)]                                              # modes 0 .. 15 on 4 x 4 blocks
    modes[0], modes[1] = 14, 15
    out["modes-14-15"] = (still_file(vp8l_stream(17, 11, [("px", p) for p in _rand_px(rng, 17 * 11)], [("predictor", 2, modes)])), 17, 11)
    for n in (2, 3, 5, 20):                                                             # a palette index at or past n
        k = 3 if n <= 2 else 2 if n <= 4 else 1 if n <= 16 else 0
        W, H = 13, 9
        pw = -(-W // (1 << k))
        tokens = [("px", 0xff000000 | int(g) << 8) for g in rng.integers(0, 256, pw * H)]
        out[f"palette-overflow-n{n}"] = (still_file(vp8l_stream(W, H, tokens, [("palette", _rand_px(rng, n))])), W, H)
    tokens, total = [("px", p) for p in _rand_px(rng, 7)], 7                          # every length prefix at both ends of its extra bits
    for p in range(24):
        e = 0 if p < 4 else (p - 2) >> 1
        lo = p + 1 if p < 4 else ((2 + (p & 1)) << e) + 1
        for length in (lo, lo + (1 << e) - 1):
            v = (2, 121 + 2, 121 + 5)[(p + length) % 3]                                 # distance 1, 3 and 6: below the length wherever it is longer
            tokens += [("copy", length, v), ("px", _rand_px(rng, 1)[0])]
            total += length + 1
    W = 64
    tokens += [("px", p) for p in _rand_px(rng, (-total) % W)]
    out["length-prefixes"] = (still_file(vp8l_stream(W, (total + (-total) % W) // W, tokens)), W, (total + (-total) % W) // W)
    for bits in (1, 11):                                                                # the smallest and the largest colour cache
        colours = rng.integers(0, 1 << 32, 2 if bits == 1 else 900, dtype=np.uint64)
        tokens = [("px", p) for p in _rand_px(rng, 40 * 25 - 30, colours)] + [("copy", 30, 121 + 400)]
        out[f"cache-bits-{bits}"] = (still_file(vp8l_stream(40, 25, tokens, cache_bits=bits)), 40, 25)
    frames = np.concatenate([E.mask_frames(1, 37, 21), np.random.default_rng(5).integers(0, 256, (1, 37, 21, 3)).astype(np.uint8)])
    for rows in (1, 5, 64):                                                             # the writer's own yardstick streams
        for k, payload in enumerate(E.encode_frames(frames, rows)):
            out[f"writer-rows{rows}-{k}"] = (still_file(payload), 21, 37)
    return out


# ---- corruptions that reach the GPU -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def corrupt():
    """{name: ([good file, bad file], the status word the bad one ends in)}: a short fixed list, each ended with that status by the host program
    (tests/test_webpdec.py) before a GPU test feeds it to the kernels."""
    good = stills()["photo-67x45-m4-q50"]
    p = vp8l_of(good)
    bad = {"truncated": (p[:len(p) // 2], 10), "zeros": (p[:9] + bytes(len(p) - 9), 4), "ones": (p[:9] + b"\xff" * (len(p) - 9), 4),
           "falsified code lengths": (p[:7] + bytes([p[7] ^ 0x55]) + p[8:], 4)}
    return {name: ([good, still_file(q)], code) for name, (q, code) in bad.items()}


# ---- animations ---------------------------------------------------------------------------------------------------------------------------------------
def anmf(payload, x, y, w, h, blend, dispose, ms=40):
    return E.chunk(b"ANMF", E.u24(x // 2) + E.u24(y // 2) + E.u24(w - 1) + E.u24(h - 1) + E.u24(ms) + bytes([(0 if blend else 2) | (1 if dispose else 0)])
                   + E.chunk(b"VP8L", payload))


def animation_file(W, H, frames, loop=0, background=0x80402010):
    """frames: (payload, x, y, w, h, blend, dispose)."""
    body = b"WEBP" + E.chunk(b"VP8X", b"\x12\0\0\0" + E.u24(W - 1) + E.u24(H - 1)) + E.chunk(b"ANIM", struct.pack("<IH", background, loop))
    body += b"".join(anmf(*f) for f in frames)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def random_animation(seed, W=30, H=22, n=5):
    rng = np.random.default_rng([seed, 4242])
    frames = []
    for k in range(n):
        if rng.random() < 0.35:
            x, y, w, h = 0, 0, W, H
        else:
            x, y = 2 * int(rng.integers(0, W // 2)), 2 * int(rng.integers(0, H // 2))
            w, h = int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))
        style = int(rng.integers(0, 3))
        if style == 0:
            a = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            payload = vp8l_of(save(a, method=int(rng.integers(0, 3))))
        else:
            a = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
            a[..., 3] = rng.choice([0, 255] if style == 1 else [0, 255, 1, 77, 128, 254], (h, w))
            payload = vp8l_of(save(a, method=int(rng.integers(0, 3)), exact=True))
        frames.append((payload, x, y, w, h, bool(rng.random() < 0.6), bool(rng.random() < 0.45)))
    return animation_file(W, H, frames)


@functools.lru_cache(None)
def animations():
    return {f"random-{s}": random_animation(s) for s in range(40)}


def shapes_clip(n=6, W=48, H=36):
    out = np.zeros((n, H, W, 3), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(n):
        out[f, ..., 1] = 40
        out[f][(yy - 12 - 2 * f) ** 2 + (xx - 10 - 5 * f) ** 2 < 60] = (250, 200, 30)
        out[f][(abs(yy - 28) < 4) & (abs(xx - 40 + 4 * f) < 6)] = (30, 60, 240)
    return out


def noise_patch_clip(n=5, W=48, H=36):
    rng = np.random.default_rng(9)
    out = np.repeat(rng.integers(0, 256, (1, H, W, 3)).astype(np.uint8), n, 0)
    for f in range(1, n):
        out[f:, 4 + 5 * f:14 + 5 * f, 6 * f:6 * f + 12] = rng.integers(0, 256, (10, 12, 3))
    return out


@functools.lru_cache(None)
def pil_animations():
    out = {}
    for name, clip in (("shapes", shapes_clip()), ("noise-patch", noise_patch_clip())):
        for minimize in (False, True):
            b = io.BytesIO()
            ims = [Image.fromarray(f) for f in clip]
            ims[0].save(b, format="WEBP", save_all=True, append_images=ims[1:], lossless=True, duration=40, minimize_size=minimize)
            out[f"{name}-minimize{int(minimize)}"] = b.getvalue()
    return out


# ---- the host program's job file ------------------------------------------------------------------------------------------------------------------------
def write_job(path, headers, limit=None, caps=None):
    """headers: mmgt_amd.video_in.WebpHeader of files of one canvas -> the job file of tools/webpdec_host_check.cpp, one set of launches."""
    from mmgt_amd import video_in
    tab, data, chunks = video_in.webp_operands(headers, limit, 1 << 40, caps=caps)
    assert len(chunks) == 1
    with open(path, "wb") as f:
        f.write(struct.pack("<4i3q", 0x314A4457, len(tab), headers[0].height, headers[0].width, chunks[0][2], chunks[0][3], data.size))
        f.write(tab.tobytes())
        f.write(data.tobytes())
    return tab, chunks[0]
