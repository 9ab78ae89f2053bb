"""PIL's 8-bit Image.resize (BILINEAR / BICUBIC / LANCZOS) restated in numpy: the yardstick of the device resize on the GPU side, held to
PIL itself byte for byte by tests/test_resize.py.  Independent of mmgt_amd.conditioning.pil_resample_tables: its own filter functions, its own
coefficient loop and its own two passes.  Also the list of shapes and the test images both test files use."""
import math

import numpy as np

BITS = 22

# (Hs, Ws) -> (Hd, Wd)
SHAPES = [
    ((37, 53), (16, 24)),       # general downscale
    ((64, 48), (64, 20)),       # vertical pass skipped
    ((20, 30), (45, 30)),       # horizontal pass skipped, upscale
    ((9, 7), (23, 31)),         # upscale
    ((135, 240), (64, 64)),     # 16:9 frame
    ((5, 300), (8, 8)),         # 227 taps
    ((1, 1), (4, 4)),           # single pixel
    ((17, 19), (17, 19)),       # identity
    ((270, 480), (32, 32)),     # large downscale
]
FILTERS = ("bilinear", "bicubic", "lanczos")
KINDS = ("noise", "edges")


def shape_id(shape):
    (hs, ws), (hd, wd) = shape
    return f"{hs}x{ws}-{hd}x{wd}"


def image(hs, ws, c, kind, seed=0):
    """(hs, ws, c) uint8: uniform noise, or 0 / 255 regions with straight edges at odd angles (the clamp at both ends, Lanczos over- and undershoot)."""
    rng = np.random.default_rng([hs, ws, c, seed, KINDS.index(kind)])
    if kind == "noise":
        return rng.integers(0, 256, (hs, ws, c), dtype=np.uint8)
    yy, xx = np.mgrid[0:hs, 0:ws]
    out = np.zeros((hs, ws, c), np.uint8)
    for ch in range(c):
        a, b = rng.uniform(-1, 1, 2)
        t = rng.uniform(0.2, 0.8)
        out[..., ch] = np.where(a * (xx - ws * t) + b * (yy - hs * t) + 0.25 * ((xx // 3 + yy // 5) % 2) > 0, 255, 0)
    return out


def frames(n, hs, ws, c, kind):
    """n frames with different content."""
    return np.stack([image(hs, ws, c, kind, seed=k) for k in range(n)])


def pil_resize(img, hd, wd, filt):
    """PIL's own answer for one (h, w, c) uint8 image, c = 1 ("L") or 3 ("RGB")."""
    from PIL import Image
    f = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[filt]
    pil = Image.fromarray(img[..., 0]) if img.shape[2] == 1 else Image.fromarray(img)
    out = np.asarray(pil.resize((wd, hd), f))
    return out[..., None] if img.shape[2] == 1 else out


def _triangle(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _cubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


KERNELS = {"bilinear": (_triangle, 1.0), "bicubic": (_cubic, 2.0), "lanczos": (_lanczos, 3.0)}


def coefficients(in_size, out_size, filt):
    """[(first tap, int64 weights)] per output sample: Resample.c's precompute_coeffs and normalize_coeffs_8bpc."""
    kernel, support = KERNELS[filt]
    scale = in_size / out_size
    filterscale = scale if scale > 1.0 else 1.0
    support = support * filterscale
    inv = 1.0 / filterscale
    rows = []
    for o in range(out_size):
        center = (o + 0.5) * scale
        lo = int(center - support + 0.5)
        lo = lo if lo > 0 else 0
        hi = int(center + support + 0.5)
        hi = hi if hi < in_size else in_size
        w = [kernel((x - center + 0.5) * inv) for x in range(lo, hi)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        rows.append((lo, np.array([int(v * (1 << BITS) + (0.5 if v >= 0 else -0.5)) for v in w], np.int64)))
    return rows


def _pass(img, out_size, filt, axis):
    """One pass along `axis` of (..., H, W, C): clip8((2^21 + sum u8 * k) >> 22)."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((out_size,) + src.shape[1:], np.int64)
    for o, (lo, k) in enumerate(coefficients(src.shape[0], out_size, filt)):
        out[o] = (np.tensordot(k, src[lo:lo + len(k)], axes=(0, 0)) + (1 << (BITS - 1))) >> BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize(img, hd, wd, filt):
    """(..., H, W, C) uint8 -> (..., hd, wd, C): the horizontal pass first, then the vertical; a pass whose size does not change is skipped."""
    assert img.dtype == np.uint8 and img.ndim >= 3
    if img.shape[-2] != wd:
        img = _pass(img, wd, filt, img.ndim - 2)
    if img.shape[-3] != hd:
        img = _pass(img, hd, filt, img.ndim - 3)
    return img
