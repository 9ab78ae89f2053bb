"""The yardstick of re-voicing an existing clip (csrc/vid2vid.hip, scheduler.set_timesteps(strength=), Pose2VideoPipeline's init
arguments): numpy / plain torch, nothing imported from the code under test.

  kept_timesteps      diffusers' img2img get_timesteps on the trailing list: the last min(int(N strength), N) entries
  known_reference     sa x0 + sb z in fp64 and the bound one fp32 evaluation may differ by
  mask_to_latent_ref  a cell is 1 iff a pixel >= 128 lies in a cell within Chebyshev distance grow; cells outside the frame do not exist
  feather_ref         the cell mask x 8 (nearest), box sum over (2r + 1)^2 with edge replication, (255 count + area // 2) // area
  composite_ref       (g a + o (255 - a) + 127) // 255
  loop_from           sampler_ref.gaussian_loop's chain over a given list of steps, from a given start
and the cases the CPU host program and the GPU kernels are both held to (`MASK_SHAPES`, `mask_cases`, `FEATHER_CASES`, `composite_triples`)."""
import math

import numpy as np
import torch

from tests import sampler_ref as R

F64 = torch.float64


# ---- the strength rule ----------------------------------------------------------------------------------------------------------------------------------

def kept_timesteps(n, strength):
    ts = R.trailing_timesteps(n)
    init = min(int(n * strength), n)
    return ts[max(n - init, 0):]


def scalars(alpha_bar):
    """(sqrt(abar), sqrt(1 - abar)) as the fp32 kernel arguments"""
    return R.f32(math.sqrt(alpha_bar)), R.f32(math.sqrt(1 - alpha_bar))


def ddim_pairs_of(table, ts, n):
    return [(R.a_of(table, t), R.a_of(table, t - len(table) // n)) for t in ts]


def dpm_triples_of(table, ts):
    """the solver on a (shortened) list: its first entry has no earlier point"""
    return [(R.a_of(table, ts[i - 1]) if i else None, R.a_of(table, ts[i]), R.a_of(table, ts[i + 1]) if i + 1 < len(ts) else 1.0) for i in range(len(ts))]


# ---- known = sa x0 + sb z ---------------------------------------------------------------------------------------------------------------------------------

def ulp32(v):
    """the spacing of fp32 at magnitude v (fp64 tensor), 2^-149 at and below the subnormals"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 23)


def known_reference(x0, z, sa, sb):
    """-> (ref fp64, bound).  The bound is ONE ulp of fp32 at the magnitude |sa x0| + |sb z|: the terms and the result all lie at or below it, so a
    fused evaluation (the product sb z rounded, then one fma: half an ulp each) stays inside, and so does any single rounding; the result's own
    ulp cannot serve, because where the two terms cancel the rounding of a term is many ulps of the small result."""
    sa, sb = R.f32(sa), R.f32(sb)
    a, b = sa * x0.double(), sb * z.double()
    return a + b, ulp32(a.abs() + b.abs())


# ---- the integer rules ------------------------------------------------------------------------------------------------------------------------------------

def mask_to_latent_ref(mask, grow):
    L, H, W = mask.shape
    h, w = H // 8, W // 8
    cells = (mask.reshape(L, h, 8, w, 8) >= 128).any(axis=(2, 4))
    pad = np.zeros((L, h + 2 * grow, w + 2 * grow), bool)
    pad[:, grow:grow + h, grow:grow + w] = cells
    out = np.zeros((L, h, w), bool)
    for dy in range(2 * grow + 1):
        for dx in range(2 * grow + 1):
            out |= pad[:, dy:dy + h, dx:dx + w]
    return out.astype(np.float32)


def feather_ref(cells, r):
    up = np.repeat(np.repeat(cells >= 0.5, 8, axis=1), 8, axis=2).astype(np.int64)
    L, H, W = up.shape
    p = np.pad(up, ((0, 0), (r, r), (r, r)), mode="edge")
    rows = sum(p[:, :, dx:dx + W] for dx in range(2 * r + 1))
    count = sum(rows[:, dy:dy + H] for dy in range(2 * r + 1))
    area = (2 * r + 1) ** 2
    return ((255 * count + area // 2) // area).astype(np.uint8)


def composite_ref(gen, orig, alpha):
    g, o, a = gen.astype(np.uint32), orig.astype(np.uint32), alpha.astype(np.uint32)[..., None]
    return ((g * a + o * (255 - a) + 127) // 255).astype(np.uint8)


MASK_SHAPES = [(1, 8, 8), (2, 64, 64), (3, 64, 128), (2, 24, 40)]
GROWS = [0, 1, 2, 8]


def mask_cases(L, H, W):
    """{name: uint8 (L, H, W)}: empty, full, a pixel in each corner (one corner per frame, all four in the last), a 127 beside a 128, sparse random"""
    rng = np.random.default_rng(L * 1000003 + H * 1009 + W)
    z = lambda: np.zeros((L, H, W), np.uint8)
    corners = z()
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for l in range(L):
        y, x = spots[l % 4]
        corners[l, y, x] = 255
    for y, x in spots:
        corners[L - 1, y, x] = 128
    edge = z()
    edge[:, H // 2, W // 2 - 1] = 127
    edge[0, H // 2, W // 2] = 128                             # frame 0 has the 128; the others only the 127
    sparse = np.where(rng.random((L, H, W)) < 0.002, rng.integers(0, 256, (L, H, W)), rng.integers(0, 128, (L, H, W))).astype(np.uint8)
    return {"empty": z(), "full": np.full((L, H, W), 255, np.uint8), "corners": corners, "127-beside-128": edge, "sparse": sparse}


FEATHER_RADII = [0, 1, 8, 32]
FEATHER_GRIDS = [(2, 8, 8), (2, 3, 5)]                        # the second: r = 32 reaches past the 24 x 40 frame on every side


def feather_cells(L, h, w):
    """a cell mask with a block, an isolated cell, a corner cell and one fractional value on each side of 0.5; frame 1 is another pattern"""
    rng = np.random.default_rng(h * 31 + w)
    c = np.zeros((L, h, w), np.float32)
    c[0, h // 3:h // 3 + 2, w // 3:w // 3 + 2] = 1
    c[0, h - 1, w - 1] = 1
    c[0, 0, w - 1] = 0.5
    c[0, h - 1, 0] = 0.49
    c[1:] = (rng.random((L - 1, h, w)) < 0.3).astype(np.float32)
    return c


def composite_triples():
    """every (g, o, a) of 256^3 once, as gen / orig (256, 256, 256, 3) and alpha (256, 256, 256): pixel (g, o, a); channel c of gen holds g, o and
    255 - g, of orig o, g and o, so every channel position of the kernel's words sees other data"""
    g, o, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    gen = np.stack([g, o, 255 - g], axis=-1)
    orig = np.stack([o, g, o], axis=-1)
    return np.ascontiguousarray(gen), np.ascontiguousarray(orig), np.ascontiguousarray(a)


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------------------------

def loop_from(x_start, steps, rule, g, s_u, s_c, eta=0.0, noises=None):
    """sampler_ref.gaussian_loop (mean 0, no rescale) over the given steps -- (a_t, a_s) pairs for "ddim", (a_prev, a_t, a_s) triples for "dpm" --
    from `x_start`, taken as exact.  -> (latents fp64, bound)"""
    x = x_start.double()
    d_x = torch.zeros_like(x)
    x0p, d_xp = None, 0.0
    one = torch.ones((x.shape[2],), dtype=torch.float32, device=x.device)
    for i, st in enumerate(steps):
        a_t = st[-2]
        rows, errs = [], []
        for s in (s_u, s_c):
            c = R.f32(R.gaussian_v_gain(a_t, s))
            e = c * x
            rows.append(e)
            errs.append(abs(c) * d_x + 2 * R.U * e.abs())
        co = R.f32s(R.ddim_k(*st, eta) if rule == "ddim" else R.dpm_k(*st))
        x, x0, d_x, d_x0 = R.step_reference(torch.cat(rows), one, x, g, 0.0, co, x0_prev=x0p, z=None if noises is None else noises[i], d_x=d_x,
                                            d_xp=d_xp, d_eu=errs[0], d_ec=errs[1])
        x0p, d_xp = x0, d_x0
    return x, d_x
