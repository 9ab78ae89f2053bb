"""The GIF decoder's yardstick in plain loops: a file walker, a textbook LZW decoder with prefix chains, the interlace row order and PIL's
frame composition restated rule by rule.  tests/test_gifdec.py holds decode() to PIL's ImageSequence.Iterator(Image.open(f)) + convert("RGB") on every
byte; nothing here is shared with mmgt_amd.video_in or csrc/gifdec_core.h."""
import numpy as np


def walk(data):
    """-> (W, H, background index, frames): a frame is a dict of rect (x, y, w, h), interlace, mcs, transparent (or None), disposal bits, table
    ((entries, 3) uint8) and lzw (the sub-blocks joined)."""
    assert data[:6] in (b"GIF87a", b"GIF89a")
    W, H = int.from_bytes(data[6:8], "little"), int.from_bytes(data[8:10], "little")
    packed, background = data[10], data[11]
    pos = 13
    gtable = None
    if not packed & 0x80:
        background = 0                                                        # PIL takes the background index only from a file with a global table
    if packed & 0x80:
        size = 3 * (2 << (packed & 7))
        gtable = np.frombuffer(data[pos:pos + size], np.uint8).reshape(-1, 3)
        pos += size

    def blocks():
        nonlocal pos
        out = b""
        while data[pos]:
            out += data[pos + 1:pos + 1 + data[pos]]
            pos += 1 + data[pos]
        pos += 1
        return out

    frames, control = [], (0, None)
    while pos < len(data):
        kind = data[pos]
        pos += 1
        if kind == 0x3B:
            break
        if kind == 0x21:
            label = data[pos]
            first = data[pos + 1:pos + 1 + data[pos + 1] + 1]
            pos += 1
            blocks()
            if label == 0xF9:
                control = ((first[1] >> 2) & 7, first[4] if first[1] & 1 else None)
        elif kind == 0x2C:
            x, y, w, h = (int.from_bytes(data[pos + 2 * i:pos + 2 * i + 2], "little") for i in range(4))
            flags = data[pos + 8]
            pos += 9
            table = gtable
            if flags & 0x80:
                size = 3 * (2 << (flags & 7))
                table = np.frombuffer(data[pos:pos + size], np.uint8).reshape(-1, 3)
                pos += size
            mcs = data[pos]
            pos += 1
            frames.append(dict(rect=(x, y, w, h), interlace=bool(flags & 0x40), mcs=mcs, transparent=control[1], disposal=control[0], table=table,
                               lzw=blocks()))
            control = (0, None)
    return W, H, background, frames


def lzw_decode(stream, mcs, npix):
    """Code stream -> npix indices (a list).  ValueError for a code above the next free one, a first code after a clear that is no literal, or data
    that ends (or says end-of-information) before npix indices.  Whatever follows the npix-th index is ignored."""
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    prefix, last = {}, {}                                                     # code -> the code of its string without the last byte, and that byte
    out, pos, width, nxt, prev = [], 0, mcs + 1, eoi + 1, None
    big, total = int.from_bytes(stream, "little"), 8 * len(stream)

    def string(code):
        s = []
        while code >= clear:
            s.append(last[code])
            code = prefix[code]
        s.append(code)
        return s[::-1]

    while len(out) < npix:
        if pos + width > total:
            raise ValueError("truncated")
        code = (big >> pos) & ((1 << width) - 1)
        pos += width
        if code == clear:
            prefix, last, width, nxt, prev = {}, {}, mcs + 1, eoi + 1, None
            continue
        if code == eoi:
            raise ValueError("truncated")
        if prev is None:
            if code > clear:
                raise ValueError("first code")
            out.append(code)
            prev = code
            continue
        if code > nxt:
            raise ValueError("code above next")
        if code == nxt:
            s = string(prev)
            s = s + s[:1]
        else:
            s = string(code)
        if nxt < 4096:
            prefix[nxt], last[nxt] = prev, s[0]
            nxt += 1
            if nxt == 1 << width and width < 12:
                width += 1
        out.extend(s)
        prev = code
    return out[:npix]


def row_order(h, interlace):
    """Stream row -> rectangle row."""
    if not interlace:
        return list(range(h))
    return list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))


def decode(data, limit=None):
    """-> (n, H, W, 3) uint8: what PIL shows for every frame after convert("RGB")."""
    W, H, background, frames = walk(data)
    frames = frames if limit is None else frames[:limit]
    out = np.zeros((len(frames), H, W, 3), np.uint8)
    canvas = np.zeros((H, W, 3), np.uint8)
    pending = None                                                            # (x, y, w, h, what): a colour (3,), or the saved pixels (h, w, 3)
    sticky = 0
    for k, f in enumerate(frames):
        x0, y0, w, h = f["rect"]
        table = np.zeros((256, 3), np.uint8)
        table[:len(f["table"])] = f["table"]
        entries, trans = len(f["table"]), f["transparent"]
        idx = lzw_decode(f["lzw"], f["mcs"], w * h)
        rows = row_order(h, f["interlace"])
        if k == 0:
            canvas[:, :] = table[trans if trans is not None else 0]
        elif pending is not None:
            px, py, pw, ph, what = pending
            for yy in range(ph):
                for xx in range(pw):
                    canvas[py + yy, px + xx] = what if what.ndim == 1 else what[yy, xx]
        before = canvas[y0:y0 + h, x0:x0 + w].copy()
        for s, r in enumerate(rows):
            for xx in range(w):
                v = idx[s * w + xx]
                if k == 0 or v != trans:
                    canvas[y0 + r, x0 + xx] = table[v]
        sticky = f["disposal"] or sticky
        pending = None
        if sticky == 2:
            index = trans if trans is not None else background
            colour = table[index] if k == 0 or index < entries else table[0]
            pending = (x0, y0, w, h, colour.copy())
        elif sticky >= 3:
            if k > 0:
                pending = (x0, y0, w, h, before)
            elif trans is not None:
                pending = (x0, y0, w, h, table[trans].copy())
        out[k] = canvas
    return out
