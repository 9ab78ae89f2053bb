"""GIF files for the decoder's tests (tests/test_gifdec.py without a GPU, tests/test_gifdec_gpu.py with one): a writer that emits what no stock writer
does (code streams without the initial clear or the end-of-information code, deferred clears, surplus pixels, any minimum code size), a seeded
generator of random files over sub-rectangles, local palettes, transparency, the disposals and interlace, the files PIL itself writes, PIL's reading of
a file as the yardstick, and the job file of tools/gifdec_host_check.cpp."""
import functools
import io
import struct

import numpy as np
from PIL import Image, ImageSequence

SIZES = [(1, 1), (16, 1), (5, 7), (37, 53), (40, 56), (120, 150)]             # (W, H): the issue's 1x1, 1x16, 7x5, 53x37, 56x40, 150x120 as H x W


def lzw_encode(indices, mcs, initial_clear=True, eoi=True, defer_clear=False, clear_every=None, tail=b""):
    """Palette indices -> code stream bytes (LSB first).  The widths follow the decoder's rule (a code is written at the width the decoder has when it
    reads it).  defer_clear: a full table is kept and 12-bit codes go on; otherwise a clear follows the code that fills it.  clear_every: a clear
    after every that many codes as well."""
    clear, end = 1 << mcs, (1 << mcs) + 1
    codes = [clear] if initial_clear else []
    table, nxt, since = {}, end + 1, 0
    data = [int(v) for v in np.asarray(indices).reshape(-1)]
    assert data and max(data) < clear
    prefix = data[0]
    for c in data[1:]:
        if (prefix, c) in table:
            prefix = table[(prefix, c)]
            continue
        codes.append(prefix)
        since += 1
        if nxt < 4096:
            table[(prefix, c)] = nxt
            nxt += 1
        prefix = c
        if (nxt == 4096 and not defer_clear) or (clear_every and since >= clear_every):
            codes.append(clear)
            table, nxt, since = {}, end + 1, 0
    codes.append(prefix)
    if eoi:
        codes.append(end)
    return pack_codes(codes, mcs) + tail


def pack_codes(codes, mcs):
    """Codes -> bytes at the widths a decoder reads them with."""
    clear, end = 1 << mcs, (1 << mcs) + 1
    acc = nacc = 0
    width, nxt, prev = mcs + 1, end + 1, False
    for code in codes:
        acc |= code << nacc
        nacc += width
        if code == clear:
            width, nxt, prev = mcs + 1, end + 1, False
        elif code != end:
            if prev and nxt < 4096:
                nxt += 1
                if nxt == 1 << width and width < 12:
                    width += 1
            prev = True
    return acc.to_bytes((nacc + 7) // 8, "little")


def sub_blocks(stream, size=255):
    out = b""
    for k in range(0, len(stream), size):
        part = stream[k:k + size]
        out += bytes([len(part)]) + part
    return out + b"\0"


def interlace_rows(idx):
    h = idx.shape[0]
    order = list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))
    return idx[order]


def make_gif(W, H, frames, gtable=None, background=0, version=b"GIF89a", trailer=True, extra=b""):
    """frames: dicts of idx ((h, w) uint8), x, y, table ((entries, 3) or None), transparent (or None), disposal (None: no graphic control extension),
    interlace, mcs (default: what the table needs), lzw (keyword arguments of lzw_encode), stream (ready code stream bytes instead of idx's),
    block (sub-block size)."""
    bits = lambda t: max(0, int(np.ceil(np.log2(len(t)))) - 1)
    out = [version, struct.pack("<HHBBB", W, H, (0x80 | 0x70 | bits(gtable)) if gtable is not None else 0x70, background, 0)]
    if gtable is not None:
        assert len(gtable) == 2 << bits(gtable)
        out.append(np.asarray(gtable, np.uint8).tobytes())
    out.append(extra)
    for f in frames:
        idx = np.asarray(f["idx"], np.uint8)
        h, w = idx.shape
        table = f.get("table")
        if f.get("disposal") is not None or f.get("transparent") is not None:
            t = f.get("transparent")
            out.append(b"\x21\xf9\x04" + struct.pack("<BHB", (f.get("disposal") or 0) << 2 | (t is not None), 4, t or 0) + b"\0")
        flags = (0x40 if f.get("interlace") else 0) | ((0x80 | bits(table)) if table is not None else 0)
        out.append(b"\x2c" + struct.pack("<HHHHB", f.get("x", 0), f.get("y", 0), w, h, flags))
        if table is not None:
            assert len(table) == 2 << bits(table)
            out.append(np.asarray(table, np.uint8).tobytes())
        use = table if table is not None else gtable
        mcs = f.get("mcs") or max(2, bits(use) + 1)
        rows = interlace_rows(idx) if f.get("interlace") else idx
        stream = f["stream"] if "stream" in f else lzw_encode(rows, mcs, **f.get("lzw", {}))
        out.append(bytes([mcs]) + sub_blocks(stream, f.get("block", 255)))
    if trailer:
        out.append(b"\x3b")
    return b"".join(out)


def random_table(rng, entries):
    return rng.integers(0, 256, (entries, 3), dtype=np.uint8)


def random_gif(seed):
    """One seeded file: 1 .. 5 frames on a small screen; sub-rectangles, local palettes of 2 .. 256 entries, transparency, disposal bits 0 .. 3 or no
    control extension, interlace, a background index anywhere in 0 .. 255, flat or noisy indices."""
    rng = np.random.default_rng(seed)
    W, H = [(1, 1), (16, 1), (5, 7), (37, 53), (40, 56), (23, 9)][int(rng.integers(0, 6))]
    gtable = random_table(rng, 2 << int(rng.integers(0, 8))) if rng.random() < 0.8 else None
    frames = []
    for k in range(int(rng.integers(1, 6))):
        if rng.random() < 0.4:
            x, y, w, h = 0, 0, W, H
        else:
            w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
            x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        table = random_table(rng, 2 << int(rng.integers(0, 8))) if gtable is None or rng.random() < 0.4 else None
        entries = len(table if table is not None else gtable)
        if rng.random() < 0.5:
            idx = rng.integers(0, entries, (h, w))
        else:                                                                 # flat areas: long strings
            idx = np.full((h, w), int(rng.integers(0, entries)))
            idx[h // 3:, w // 2:] = int(rng.integers(0, entries))
        f = dict(idx=idx.astype(np.uint8), x=x, y=y, table=table, interlace=bool(rng.random() < 0.4))
        if rng.random() < 0.8:
            f["disposal"] = int(rng.integers(0, 4))
            if rng.random() < 0.6:
                f["transparent"] = int(idx[int(rng.integers(0, h)), int(rng.integers(0, w))]) if rng.random() < 0.8 else int(rng.integers(0, 256))
        frames.append(f)
    return make_gif(W, H, frames, gtable, int(rng.integers(0, 256)) if rng.random() < 0.5 else 0)


@functools.lru_cache(maxsize=None)
def random_gifs(n=240):
    return [random_gif(1000 + s) for s in range(n)]


def _save(frames, **kw):
    b = io.BytesIO()
    frames[0].save(b, format="GIF", save_all=len(frames) > 1, append_images=frames[1:], **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def pil_written():
    """name -> the bytes PIL's own writer gives: RGB frames (a palette per frame), "L" masks whose frames PIL stores as delta rectangles with
    transparency, a shared palette, disposal 2 and 3, transparency=, interlace, a single frame."""
    rng = np.random.default_rng(11)
    W, H = 56, 40
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = [Image.fromarray(np.stack([(xx * 4 + 9 * k) % 256, (yy * 6 + 5 * k) % 256, (xx + yy + 31 * k) % 256], axis=2).astype(np.uint8)) for k in range(4)]
    masks = [Image.fromarray((((xx - 10 - 6 * k) ** 2 + (yy - 20) ** 2 < 90) * 255).astype(np.uint8)) for k in range(5)]
    pal = rng.integers(0, 256, 768).astype(np.uint8).tobytes()
    shared = []
    for k in range(3):
        im = Image.fromarray(((xx // 7 + yy // 5 + k) % 16).astype(np.uint8), "P")
        im.putpalette(pal)
        shared.append(im)
    noise = [Image.fromarray(rng.integers(0, 256, (120, 150, 3), dtype=np.uint8)) for _ in range(2)]
    return {"rgb": _save(rgb, duration=40, loop=0), "masks": _save(masks, duration=40), "shared": _save(shared), "dispose2": _save(shared, disposal=2),
            "dispose3": _save(masks, disposal=3), "dispose_mixed": _save(shared + shared, disposal=[0, 2, 3, 1, 3, 2]),
            "transparency": _save(shared, transparency=3, disposal=2), "interlace": _save(shared, interlace=True), "single": _save(rgb[:1]),
            "single_L": _save(masks[:1]), "noise": _save(noise)}


def pil_frames(data):
    """(n, H, W, 3) uint8: PIL's frames of the file, the decoder's definition."""
    with Image.open(io.BytesIO(data)) as im:
        return np.stack([np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(im)])


def one_frame(stream=None, W=37, H=53, mcs=8, seed=0, idx=None, **lzw):
    """A one-frame file around a code stream made here; -> (file bytes, the indices)."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 1 << mcs, (H, W)).astype(np.uint8) if idx is None else np.asarray(idx, np.uint8)
    table = random_table(np.random.default_rng(seed + 1), 1 << mcs)
    f = dict(idx=idx, mcs=mcs, lzw=lzw)
    if stream is not None:
        f["stream"] = stream
    return make_gif(idx.shape[1], idx.shape[0], [f], table), idx


@functools.lru_cache(maxsize=None)
def stream_cases():
    """name -> file bytes: what the un-LZW must take although stock writers rarely write it.  Every file decodes (PIL agrees)."""
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (120, 150)).astype(np.uint8)                 # 18000 noisy indices fill the 4096-entry table several times
    flat = np.full((120, 150), 7, np.uint8)
    out = {"no_initial_clear": one_frame(initial_clear=False)[0],
           "deferred_clear": one_frame(idx=noise, defer_clear=True)[0],
           "full_table_clears": one_frame(idx=noise)[0],
           "no_eoi": one_frame(eoi=False)[0],
           "bytes_after_eoi": one_frame(tail=bytes(range(1, 40)))[0],
           "clear_every_7": one_frame(clear_every=7)[0],
           "constant_kwkwk": one_frame(idx=flat)[0],
           "constant_mcs2": one_frame(idx=np.full((150, 120), 0, np.uint8), mcs=2)[0],
           "mcs2": one_frame(mcs=2, seed=2)[0], "mcs3": one_frame(mcs=3, seed=3)[0], "mcs8_one_pixel": one_frame(W=1, H=1, seed=4)[0]}
    idx = rng.integers(0, 256, (54, 37)).astype(np.uint8)                     # one row more than the rectangle holds
    table = random_table(rng, 256)
    out["surplus_pixels"] = make_gif(37, 53, [dict(idx=idx[:53], stream=lzw_encode(idx, 8))], table)
    return out


def corrupt_cases():
    """name -> (file bytes, status of csrc/gifdec_core.h, frame): streams that must end in a status."""
    good, idx = one_frame(seed=6)
    full = lzw_encode(idx, 8)
    table = random_table(np.random.default_rng(7), 256)
    two = lambda stream: make_gif(37, 53, [dict(idx=idx), dict(idx=idx, stream=stream)], table)
    return {"truncated": (two(full[:len(full) // 2]), 3, 1),
            "eoi_too_early": (two(lzw_encode(idx[:20], 8)), 3, 1),
            "empty": (two(b""), 3, 1),
            "code_above_next": (two(pack_codes([256, 5, 6, 300, 7], 8)), 1, 1),
            "first_code_not_literal": (two(pack_codes([256, 258, 6], 8)), 2, 1),
            "first_code_after_a_later_clear": (two(pack_codes([256, 5, 6, 256, 259, 7], 8)), 2, 1)}


def write_job(path, data, limit=None):
    """The job file of tools/gifdec_host_check.cpp from mmgt_amd.video_in's operands (all frames in one chunk) -> (n, H, W)."""
    from mmgt_amd import video_in
    h = video_in.parse_gif(data)
    tab, palette, blob, chunks = video_in.gif_operands(h, limit, scratch_bytes=1 << 40)
    assert len(chunks) == 1
    with open(path, "wb") as f:
        f.write(struct.pack("<iiiiqq", 0x314A4447, len(tab), h.height, h.width, blob.size, chunks[0][2]))
        f.write(tab.tobytes() + palette.tobytes() + blob.tobytes())
    return len(tab), h.height, h.width
