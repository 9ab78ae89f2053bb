"""The inputs of the lossy WebP decoder's tests, all small: PIL-written stills and animations, the project's own writer's streams
(tests/vp8_ref.py), and crafted streams from a small header- and mode-level writer for what neither writer emits.  PIL is the judge of every one."""
import functools
import io
import struct

import numpy as np
from PIL import Image, ImageSequence

from tests import vp8_ref as E

KINDS = ("noise", "smooth", "half", "photo", "mask")
SETTINGS = ((75, 4), (75, 0), (10, 6), (50, 2), (100, 4))                                  # (quality, method)
SIZES = ((1, 1), (16, 16), (17, 16), (16, 17), (33, 47), (1, 300), (300, 1))               # (W, H)
BASE = (80, 48)


def pil_rgb(data):
    return np.stack([np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(io.BytesIO(data)))])


def kind_image(kind, W, H, seed=0):
    rng = np.random.default_rng([seed, W, H, sum(kind.encode())])
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "smooth":
        return E.case_image("smooth", W, H)
    if kind == "half":
        a = E.case_image("smooth", W, H)
        a[:, :max(1, W // 2)] = rng.integers(0, 256, (H, max(1, W // 2), 3))
        return a
    if kind == "photo":
        base = np.stack([128 + 90 * np.sin(xx / 7.0 + yy / 11.0), 128 + 80 * np.cos(yy / 5.0), 60 + xx * 2 + yy], -1)
        base[(yy // 9 + xx // 13) % 3 == 0] *= 0.6
        return np.clip(base + rng.integers(-9, 10, (H, W, 3)), 0, 255).astype(np.uint8)
    if kind == "mask":
        m = (((yy - H * 0.4) ** 2 * 4 + (xx - W * 0.5) ** 2 < (min(H, W) * 0.3) ** 2) | ((yy > H * 0.7) & (abs(xx - W * 0.3) < W * 0.12)))
        return np.repeat((m * 255).astype(np.uint8)[..., None], 3, -1)
    raise KeyError(kind)


def save(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="WEBP", **kw)
    return b.getvalue()


@functools.lru_cache(None)
def stills():
    """name -> file bytes: every kind at the base size under every setting, every kind at every edge size, one at 144 x 136."""
    out = {}
    for kind in KINDS:
        for q, m in SETTINGS:
            out[f"{kind}-{BASE[0]}x{BASE[1]}-q{q}-m{m}"] = save(kind_image(kind, *BASE), quality=q, method=m)
        for W, H in SIZES:
            out[f"{kind}-{W}x{H}-q75-m4"] = save(kind_image(kind, W, H), quality=75, method=4)
    out["photo-144x136-q60-m4"] = save(kind_image("photo", 144, 136), quality=60, method=4)
    return out


@functools.lru_cache(None)
def own_streams():
    """name -> file bytes from the project's own writer's yardstick: 1 / 2 / 8 partitions on 144 x 136 and 2 / 4 on 33 x 47, unfiltered and with the
    default filter level."""
    out = {}
    for (W, H), parts in (((144, 136), (1, 2, 8)), ((33, 47), (2, 4))):
        rgb = kind_image("photo", W, H)
        for p in parts:
            for level in (0, None):
                enc = E.encode_frame(rgb, quality=60, partitions=p, filter_level=level)
                out[f"own-{W}x{H}-p{p}-f{'default' if level is None else level}"] = E.webp_file([enc["payload"]], W, H)
    return out


def clip_frames(kind, n=6, W=80, H=48):
    rng = np.random.default_rng([n, W, H, sum(kind.encode())])
    if kind == "noise":
        return [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)]
    if kind == "smooth":
        return [np.roll(E.case_image("smooth", W, H), 3 * k, 1) for k in range(n)]
    if kind == "static":                                                                # mostly static: a photo with a small moving patch
        base = kind_image("photo", W, H)
        out = []
        for k in range(n):
            a = base.copy()
            a[10 + 2 * k:22 + 2 * k, 8 + 5 * k:24 + 5 * k] = rng.integers(0, 256, (12, 16, 3))
            out.append(a)
        return out
    if kind == "tiles":                                                                 # photo-like frames between few-colour ones: allow_mixed
        out = []                                                                        # codes the latter as VP8L
        for k in range(n):
            pal = rng.integers(0, 256, (4, 3)).astype(np.uint8)
            out.append(kind_image("photo", W, H, seed=k) if k % 2 == 0 else pal[rng.integers(0, 4, (H // 8, W // 8))].repeat(8, 0).repeat(8, 1))
        return out
    if kind == "patch":                                                                 # a flat patch moving over a photo, some frames shifted
        base = kind_image("photo", W, H)
        out = []
        for k in range(n):
            a = base.copy() if k % 3 else np.roll(base, 7 * k, 1)
            if k % 3:
                a[10 + 2 * k:22 + 2 * k, 8 + 5 * k:24 + 5 * k] = (200, 30, 30)
            out.append(a)
        return out
    if kind == "mask":
        out = []
        for k in range(n):
            a = np.zeros((H, W, 3), np.uint8)
            a[8 + k:28 + k, 6 + 7 * k:30 + 7 * k] = 255
            out.append(a)
        return out
    raise KeyError(kind)


def save_clip(frames, **kw):
    b = io.BytesIO()
    ims = [Image.fromarray(f) for f in frames]
    ims[0].save(b, format="WEBP", save_all=True, append_images=ims[1:], duration=40, **kw)
    return b.getvalue()


def chunk_kinds(data):
    """The four-character codes of the image chunks of a file, ANMF sub-chunks included, in order."""
    out, pos = [], 12
    end = 8 + int.from_bytes(data[4:8], "little")
    while pos + 8 <= end:
        kind, ln = data[pos:pos + 4], int.from_bytes(data[pos + 4:pos + 8], "little")
        if kind == b"ANMF":
            sub = pos + 8 + 16
            while sub + 8 <= pos + 8 + ln:
                out.append(data[sub:sub + 4])
                sl = int.from_bytes(data[sub + 4:sub + 8], "little")
                sub += 8 + sl + (sl & 1)
        elif kind in (b"VP8 ", b"VP8L", b"ALPH"):
            out.append(kind)
        pos += 8 + ln + (ln & 1)
    return out


def anmf(payload, x, y, w, h, blend, dispose, ms=40):
    u24 = lambda v: struct.pack("<I", v)[:3]
    body = u24(x // 2) + u24(y // 2) + u24(w - 1) + u24(h - 1) + u24(ms) + bytes([(0 if blend else 2) | (1 if dispose else 0)]) + E._chunk(b"VP8 ", payload)
    return E._chunk(b"ANMF", body)


def hand_animation(seed, W=80, H=48, n=5):
    """Lossy sub-rectangles at even offsets, some disposing to the background, assembled by hand from the own writer's payloads."""
    rng = np.random.default_rng(seed)
    u24 = lambda v: struct.pack("<I", v)[:3]
    body = b"WEBP" + E._chunk(b"VP8X", b"\x02\0\0\0" + u24(W - 1) + u24(H - 1)) + E._chunk(b"ANIM", struct.pack("<IH", 0, 0))
    for k in range(n):
        if k == 0:
            x, y, w, h = 0, 0, W, H
        else:
            w, h = int(rng.integers(1, W // 2)), int(rng.integers(1, H // 2))
            x, y = 2 * int(rng.integers(0, (W - w) // 2 + 1)), 2 * int(rng.integers(0, (H - h) // 2 + 1))
        rgb = kind_image(("photo", "noise", "smooth")[k % 3], w, h, seed=seed + k)
        enc = E.encode_frame(rgb, quality=int(rng.integers(30, 95)), partitions=(1, 2, 4)[k % 3])
        body += anmf(enc["payload"], x, y, w, h, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)) or k == 1)
    return b"RIFF" + struct.pack("<I", len(body)) + body


@functools.lru_cache(None)
def animations():
    """name -> file bytes, every one free of ALPH chunks (asserted by the tests): PIL's lossy save_all of three kinds under three settings, and two
    hand-assembled ones."""
    out = {}
    for kind in ("noise", "smooth", "static"):
        fr = clip_frames(kind)
        out[f"{kind}-default"] = save_clip(fr, quality=75)
        out[f"{kind}-minimize"] = save_clip(fr, quality=75, minimize_size=True)
        out[f"{kind}-mixed"] = save_clip(fr, quality=75, allow_mixed=True)
    out["tiles-mixed"] = save_clip(clip_frames("tiles"), quality=75, allow_mixed=True)       # VP8 and VP8L frames in one file
    out["patch-mixed"] = save_clip(clip_frames("patch"), quality=75, allow_mixed=True, minimize_size=True)
    out["hand-1"], out["hand-2"] = hand_animation(1), hand_animation(2)
    return out


def mask_animation():
    return save_clip(clip_frames("mask"), quality=75)


def vp8_of(data):
    at = data.find(b"VP8 ")
    return data[at + 8:at + 8 + int.from_bytes(data[at + 4:at + 8], "little")]


def write_job(path, headers, limit=None):
    """The host program's job file for the VP8 frames of `headers` (tools/vp8dec_host_check.cpp); returns (vtab, vidx, tab)."""
    from mmgt_amd import video_in
    tab, ltab, vtab, lidx, vidx, data, chunks = video_in.webp_operands_lossy(headers, limit, scratch_bytes=1 << 40)
    assert len(chunks) == 1 and len(vtab)
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", 0x314A3856, len(vtab)) + struct.pack("<qqq", chunks[0][6], chunks[0][7], len(data)))
        f.write(vtab.tobytes() + data.tobytes())
    return vtab, vidx, tab


# ---- crafted streams: a header- and mode-level writer on tests/vp8_ref.BoolCoder ------------------------------------------------------------------------
def _bmode_paths():
    from tests.vp8dec_ref import BMODE_TREE
    paths = {}

    # the tree's nodes are pairs (2k, 2k + 1); a positive entry v points at pair 2v
    def walk(pair, path):
        for bit in (0, 1):
            nxt = BMODE_TREE[pair + bit]
            node = pair // 2
            if nxt <= 0:
                paths[-nxt] = path + [(node, bit)]
            else:
                walk(2 * nxt, path + [(node, bit)])
    walk(0, [])
    return paths


def craft_frame(W, H, mb_fn, *, profile=0, colour=0, clamp=0, segments=None, simple=0, level=20, sharpness=0, lf_delta=None, parts=1, base_q=40,
                dq=(0, 0, 0, 0, 0), use_skip=1, skip_p=180, scale=(0, 0)):
    """A VP8 key-frame payload.  mb_fn(my, mx) -> dict(segment, skip, i4x4, modes (16 sub-modes, or [mode] for 16 x 16), uvmode, levels (25, 16) in
    scan order: blocks 0 .. 15 luma, 16 .. 23 chroma, 24 the Y2 block (unused when i4x4)); modes are the format's numbers (DC TM VE HE RD VR LD VL
    HD HU).  segments: dict(update_map, update_data, absolute, quant, strength, probs); lf_delta: dict(update, ref, mode)."""
    from tests.vp8dec_ref import BMODE_PROBS
    paths = _bmode_paths()
    mbw, mbh = (W + 15) // 16, (H + 15) // 16
    bw = E.BoolCoder()
    bw.bits(colour, 1), bw.bits(clamp, 1)
    put_signed = lambda v, n: (bw.bits(abs(v), n), bw.bits(v < 0, 1))
    put_opt = lambda v, n: (bw.bits(1, 1), put_signed(v, n)) if v else bw.bits(0, 1)
    seg_probs = [255, 255, 255]
    bw.bits(1 if segments else 0, 1)
    if segments:
        bw.bits(segments["update_map"], 1), bw.bits(segments["update_data"], 1)
        if segments["update_data"]:
            bw.bits(segments["absolute"], 1)
            for v in segments["quant"]:
                put_opt(v, 7)
            for v in segments["strength"]:
                put_opt(v, 6)
        if segments["update_map"]:
            seg_probs = list(segments["probs"])
            for p in seg_probs:
                if p == 255:
                    bw.bits(0, 1)
                else:
                    bw.bits(1, 1), bw.bits(p, 8)
    bw.bits(simple, 1), bw.bits(level, 6), bw.bits(sharpness, 3)
    bw.bits(1 if lf_delta else 0, 1)
    if lf_delta:
        bw.bits(lf_delta["update"], 1)
        if lf_delta["update"]:
            for v in list(lf_delta["ref"]) + list(lf_delta["mode"]):
                if v is None:
                    bw.bits(0, 1)
                else:
                    bw.bits(1, 1), put_signed(v, 6)
    bw.bits({1: 0, 2: 1, 4: 2, 8: 3}[parts], 2)
    bw.bits(base_q, 7)
    for v in dq:
        put_opt(v, 4)
    bw.bits(0, 1)
    for pr in E.UPDATE_PROBS.reshape(-1):
        bw.put(0, int(pr))
    bw.bits(use_skip, 1)
    if use_skip:
        bw.bits(skip_p, 8)
    tokens = [E.BoolCoder() for _ in range(parts)]
    tops = [dict(nz=[0] * 8, dc=0, modes=[0] * 4) for _ in range(mbw)]
    for my in range(mbh):
        left = dict(nz=[0] * 8, dc=0, modes=[0] * 4)
        tw = tokens[my % parts]
        for mx in range(mbw):
            mb, top = mb_fn(my, mx), tops[mx]
            if segments and segments["update_map"]:
                s = mb["segment"]
                if bw.put(s >= 2, seg_probs[0]):
                    bw.put(s & 1, seg_probs[2])
                else:
                    bw.put(s & 1, seg_probs[1])
            if use_skip:
                bw.put(mb["skip"], skip_p)
            bw.put(not mb["i4x4"], 145)
            if not mb["i4x4"]:
                m = mb["modes"][0]
                if bw.put(m in (1, 3), 156):                                       # TM or HE
                    bw.put(m == 1, 128)
                else:
                    bw.put(m == 2, 163)
                top["modes"], left["modes"] = [m] * 4, [m] * 4
            else:
                cur = list(mb["modes"])
                for y in range(4):
                    for x in range(4):
                        t = cur[4 * y - 4 + x] if y else top["modes"][x]
                        l = cur[4 * y + x - 1] if x else left["modes"][y]
                        for node, bit in paths[cur[4 * y + x]]:
                            bw.put(bit, int(BMODE_PROBS[t][l][node]))
                top["modes"], left["modes"] = cur[12:16], [cur[3], cur[7], cur[11], cur[15]]
            u = mb["uvmode"]
            if bw.put(u != 0, 142):
                if bw.put(u != 2, 114):
                    bw.put(u == 1, 183)
            lv = mb["levels"]
            if use_skip and mb["skip"]:
                assert not np.any(lv)
                top["nz"], left["nz"] = [0] * 8, [0] * 8
                if not mb["i4x4"]:
                    top["dc"] = left["dc"] = 0
                continue
            if not mb["i4x4"]:
                top["dc"] = left["dc"] = E.put_coeffs(tw, 1, top["dc"] + left["dc"], lv[24], 0)
            kind, first = (3, 0) if mb["i4x4"] else (0, 1)
            for y in range(4):
                for x in range(4):
                    top["nz"][x] = left["nz"][y] = E.put_coeffs(tw, kind, top["nz"][x] + left["nz"][y], lv[4 * y + x], first)
            for ch in (0, 1):
                for y in range(2):
                    for x in range(2):
                        a, b = 4 + 2 * ch + x, 4 + 2 * ch + y
                        top["nz"][a] = left["nz"][b] = E.put_coeffs(tw, 2, top["nz"][a] + left["nz"][b], lv[16 + 4 * ch + 2 * y + x], 0)
    first_part = bw.finish()
    bodies = [t.finish() for t in tokens]
    tag = 0 | profile << 1 | 1 << 4 | len(first_part) << 5
    out = struct.pack("<I", tag)[:3] + b"\x9d\x01\x2a" + struct.pack("<HH", W | scale[0] << 14, H | scale[1] << 14) + first_part
    out += b"".join(struct.pack("<I", len(p))[:3] for p in bodies[:-1])
    return out + b"".join(bodies)


def random_mb_fn(seed, i4x4_share=0.5, skip_share=0.2, segments=False, modes4=None, dense=0.08):
    """Seeded macroblocks: a share 4 x 4-predicted, a share flagged skipped, a share coded with every level zero, the rest with a few small levels."""
    cache = {}

    def fn(my, mx):
        if (my, mx) not in cache:
            rng = np.random.default_rng([seed, my, mx])
            i4 = bool(rng.random() < i4x4_share)
            lv = np.zeros((25, 16), np.int64)
            skip = bool(rng.random() < skip_share)
            if not skip and rng.random() > 0.25:
                mask = rng.random((25, 16)) < dense * np.linspace(2.0, 0.2, 16)[None]
                lv = np.where(mask, rng.integers(-3, 4, (25, 16)), 0)
                big = rng.integers(0, 25)
                lv[big, rng.integers(1, 4)] = int(rng.choice([5, -7, 12, -20, 40, -70]))
                if i4:
                    lv[24] = 0
                else:
                    lv[:16, 0] = 0
                    lv[24, 0] = int(rng.integers(-12, 13))
            modes = ([int(v) for v in rng.integers(0, 10, 16)] if modes4 is None else modes4(my, mx)) if i4 else [int(rng.integers(0, 4))]
            cache[(my, mx)] = dict(segment=int(rng.integers(0, 4)) if segments else 0, skip=skip, i4x4=i4, modes=modes, uvmode=int(rng.integers(0, 4)),
                                   levels=lv)
        return cache[(my, mx)]
    return fn


@functools.lru_cache(None)
def crafted():
    """name -> file bytes of what neither PIL's writer nor ours emits; each is judged by PIL."""
    W, H = 48, 48
    out = {}
    add = lambda name, w=W, h=H, **kw: out.__setitem__(name, E.webp_file([craft_frame(w, h, kw.pop("mb", random_mb_fn(len(out))), **kw)], w, h))
    seg = lambda **kw: dict(dict(update_map=1, update_data=1, absolute=1, quant=(30, 50, 70, 90), strength=(10, 25, 40, 63), probs=(120, 200, 80)), **kw)
    add("simple-filter", simple=1, level=30)
    add("simple-filter-strong", simple=1, level=63, parts=2)
    for k in range(1, 8):
        add(f"sharpness-{k}", level=(12, 25, 40, 50, 63, 33, 18)[k - 1], sharpness=k)
    add("lf-delta-update", level=30, lf_delta=dict(update=1, ref=(12, None, -5, 3), mode=(-20, 7, None, None)))
    add("lf-delta-update-negative", level=10, lf_delta=dict(update=1, ref=(-30, None, None, None), mode=(25, None, None, None)))
    add("lf-delta-no-update", level=30, lf_delta=dict(update=0))
    add("segments-delta", mb=random_mb_fn(101, segments=True), level=20, base_q=50,
        segments=seg(absolute=0, quant=(-20, 0, 15, 60), strength=(-20, 0, 12, 40)))
    add("segments-absolute", mb=random_mb_fn(102, segments=True), level=20, segments=seg(), parts=4)
    add("segments-no-map", mb=random_mb_fn(103, segments=True), level=20, segments=seg(update_map=0))
    add("segments-no-data", mb=random_mb_fn(104, segments=True), level=20, base_q=30, segments=seg(update_data=0))
    add("segments-map-defaults", mb=random_mb_fn(105, segments=True), level=20, segments=seg(probs=(255, 128, 255)))
    add("skip-off", use_skip=0, level=25)
    add("skip-off-simple", use_skip=0, level=25, simple=1, parts=8)
    for p in (1, 2, 3):
        add(f"profile-{p}", profile=p, level=28, simple=p & 1)
    add("colour-clamp-bits", colour=1, clamp=1, level=20)
    add("scale-bits", scale=(1, 2), level=20)
    add("quant-deltas", dq=(-7, 9, -15, 15, -3), level=20, base_q=5)
    add("level0-beside-filtering-segment", mb=random_mb_fn(106, segments=True), level=0, segments=seg(strength=(0, 40, 63, 20)))
    add("segment-level0-beside-filtering", mb=random_mb_fn(107, segments=True), level=30, segments=seg(strength=(0, 40, 0, 20)))
    for f in range(10):                                                             # every sub-block mode in every block position of 3 x 3 macroblocks
        add(f"bmodes-{f}", mb=random_mb_fn(200 + f, i4x4_share=1.0, skip_share=0.1, modes4=lambda my, mx, f=f: [(3 * my + mx + n + f) % 10 for n in range(16)]),
            level=(0 if f & 1 else 22))
    add("odd-size", w=33, h=47, level=35, parts=2)
    return out
