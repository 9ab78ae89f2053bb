"""The host side of the opt-in device GIF writer (mmgt_amd.video_out: gif_palette, gif_lut, write_gif, the argument checks) without a GPU, and
the yardstick of tests/test_gif_gpu.py: a plain GIF LZW encoder and decoder (minimum code size 8), checked here against PIL's decoder."""
import struct

import numpy as np
import pytest
from PIL import Image

from mmgt_amd import video_out
from mmgt_amd.video_out import gif_lut, gif_palette, write_gif

CLEAR, EOI, FIRST, LIMIT = 256, 257, 258, 4096


# ---- the yardstick: GIF LZW in the plainest form -----------------------------------------------------------------------------------------------
def lzw_encode(indices, strip_len=None):
    """uint8 indices -> (code stream bytes, LSB-first; number of Clears written because the dictionary was full).  A code is written at the current
    width; then, if the code about to be defined equals 2^width, the width grows (that is when the decoder, one definition behind, grows);
    when code 4095 has been defined, Clear follows at once.  `strip_len`: start a fresh dictionary every strip_len indices, the Clear between two
    strips written at the width the stream then has (the scheme of csrc/gif.hip)."""
    data = [int(v) for v in np.asarray(indices).reshape(-1)]
    strip_len = len(data) if strip_len is None else strip_len
    acc = nacc = full_clears = 0
    out = bytearray()

    def put(code, width):
        nonlocal acc, nacc
        acc |= code << nacc
        nacc += width
        while nacc >= 8:
            out.append(acc & 255)
            acc >>= 8
            nacc -= 8

    put(CLEAR, 9)
    for s0 in range(0, len(data), strip_len):
        table, width, nxt = {}, 9, FIRST
        strip = data[s0:s0 + strip_len]
        prefix = strip[0]
        for c in strip[1:]:
            if (prefix, c) in table:
                prefix = table[(prefix, c)]
                continue
            put(prefix, width)
            table[(prefix, c)] = nxt
            if nxt == 1 << width and width < 12:
                width += 1
            nxt += 1
            prefix = c
            if nxt == LIMIT:
                put(CLEAR, width)
                table, width, nxt = {}, 9, FIRST
                full_clears += 1
        put(prefix, width)
        if nxt == 1 << width and width < 12:
            width += 1
        put(EOI if s0 + strip_len >= len(data) else CLEAR, width)
    if nacc:
        out.append(acc & 255)
    return bytes(out), full_clears


def lzw_decode(stream, npix):
    """Code stream bytes -> npix uint8 indices; raises if the stream is malformed, ends early or holds more than npix indices."""
    out = []
    pos, width, nxt, prev = 0, 9, FIRST, None
    table = {}
    total = 8 * len(stream)
    big = int.from_bytes(stream, "little")
    while True:
        assert pos + width <= total, "stream ends without End-of-Information"
        code = (big >> pos) & ((1 << width) - 1)
        pos += width
        if code == CLEAR:
            table, width, nxt, prev = {}, 9, FIRST, None
            continue
        if code == EOI:
            break
        if prev is None:
            assert code < 256, "a literal must follow Clear"
            entry = (code,)
        else:
            if code < 256:
                entry = (code,)
            elif code in table:
                entry = table[code]
            else:
                assert code == nxt and nxt < LIMIT, f"code {code} is not defined (next is {nxt})"
                entry = prev + prev[:1]                        # the code that refers to the entry being defined
            if nxt < LIMIT:
                table[nxt] = prev + entry[:1]
                nxt += 1
                if nxt == 1 << width and width < 12:
                    width += 1
        out.extend(entry)
        prev = entry
    assert len(out) == npix, f"{len(out)} indices decoded, {npix} expected"
    assert total - pos < 8, "bytes after End-of-Information"
    return np.array(out, np.uint8)


def sub_blocks(stream):
    """Code stream -> GIF data sub-blocks with the terminator: what write_gif takes per frame."""
    return b"".join(bytes([len(stream[i:i + 255])]) + stream[i:i + 255] for i in range(0, len(stream), 255)) + b"\0"


def unblock(blob):
    """The inverse of sub_blocks; every block must hold 1 .. 255 bytes and the terminator must end the blob."""
    out, p = b"", 0
    while blob[p]:
        out += blob[p + 1:p + 1 + blob[p]]
        assert len(blob[p + 1:p + 1 + blob[p]]) == blob[p]
        p += 1 + blob[p]
    assert p == len(blob) - 1
    return out


def distinct_palette(seed=0):
    """256 different colours, so that a decoded RGB frame gives its indices back."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256), rng.permutation(256), np.arange(256)], axis=1).astype(np.uint8)


def read_gif_indices(path, palette):
    """Every frame of a GIF as palette indices (through RGB: PIL converts the later frames of a file itself), plus the image object's info."""
    inv = {tuple(int(v) for v in c): k for k, c in enumerate(palette)}
    assert len(inv) == 256
    img = Image.open(path)
    frames = []
    for k in range(img.n_frames):
        img.seek(k)
        rgb = np.asarray(img.convert("RGB"))
        frames.append(np.array([inv[tuple(p)] for p in rgb.reshape(-1, 3).tolist()], np.uint8).reshape(rgb.shape[:2]))
    return np.stack(frames), img


def random_indices():
    return np.random.default_rng(5).integers(0, 256, (96, 128), dtype=np.uint8)


def test_yardstick_encoder_is_read_back_exactly_by_pil_and_by_the_yardstick_decoder(tmp_path):
    idx = random_indices()
    pal = distinct_palette()
    stream, full_clears = lzw_encode(idx)
    assert full_clears >= 1, "12288 random pixels must fill the 3838 free codes at least once"
    assert np.array_equal(lzw_decode(stream, idx.size).reshape(idx.shape), idx)
    path = tmp_path / "one.gif"
    n = write_gif(str(path), pal, [sub_blocks(stream)], 128, 96, 25)
    assert n == path.stat().st_size
    img = Image.open(path)
    assert img.mode == "P" and img.size == (128, 96) and img.n_frames == 1
    assert np.array_equal(np.asarray(img), idx)
    assert np.array_equal(np.array(img.getpalette()[:768], np.uint8).reshape(256, 3), pal)


@pytest.mark.parametrize("strip_len", [128 * 8, 128 * 96, 1000])
def test_strips_with_their_own_dictionaries_join_into_one_stream(tmp_path, strip_len):
    """The strip scheme of the device coder, restated: PIL and the yardstick decoder read the joined stream as one image."""
    idx = random_indices()
    flat = np.concatenate([idx[:48].reshape(-1), np.repeat(np.arange(48, dtype=np.uint8), 128)])     # random rows, then long runs
    stream, _ = lzw_encode(flat, strip_len)
    assert np.array_equal(lzw_decode(stream, flat.size), flat)
    write_gif(str(tmp_path / "s.gif"), distinct_palette(), [sub_blocks(stream)], 128, 96, 25)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "s.gif")).reshape(-1), flat)


def test_yardstick_on_runs_and_tiny_inputs():
    for flat in (np.zeros(64, np.uint8), np.array([7], np.uint8), np.tile(np.array([1, 2], np.uint8), 3000), np.arange(256, dtype=np.uint8)):
        stream, _ = lzw_encode(flat)
        assert np.array_equal(lzw_decode(stream, flat.size), flat)


# ---- palette and lookup table --------------------------------------------------------------------------------------------------------------------
def _hist(bins_counts):
    h = np.zeros(32768, np.uint32)
    for b, c in bins_counts:
        h[b] = c
    return h


def _bin(r, g, b):
    return r << 10 | g << 5 | b


def palette_by_the_rule(hist):
    """DESIGN 4d's rule restated with plain loops (no numpy): the second implementation the rule is written for."""
    bins = [(b >> 10, b >> 5 & 31, b & 31, int(hist[b])) for b in range(32768) if hist[b]]
    if len(bins) <= 256:
        return [[8 * v + 4 for v in b[:3]] for b in bins] + [[0, 0, 0]] * (256 - len(bins))
    boxes = [bins]
    while len(boxes) < 256:
        best, best_score, best_axis = None, -1, None
        for k, box in enumerate(boxes):
            if len(box) < 2:
                continue
            sides = [max(b[a] for b in box) - min(b[a] for b in box) + 1 for a in range(3)]
            axis = 0
            for a in (1, 2):
                if sides[a] > sides[axis]:                    # strictly longer: R before G before B on a tie
                    axis = a
            s = sum(b[3] for b in box) * sides[axis]
            if s > best_score:                                # strictly larger: the lowest box index on a tie
                best, best_score, best_axis = k, s, axis
        box, a = boxes[best], best_axis
        lo, hi = min(b[a] for b in box), max(b[a] for b in box)
        total = sum(b[3] for b in box)
        m = lo
        while 2 * sum(b[3] for b in box if b[a] <= m) < total:
            m += 1
        m = min(m, hi - 1)
        boxes[best] = [b for b in box if b[a] <= m]
        boxes.append([b for b in box if b[a] > m])
    pal = []
    for box in boxes:
        tot = sum(b[3] for b in box)
        pal.append([(2 * sum(b[3] * (8 * b[a] + 4) for b in box) + tot) // (2 * tot) for a in range(3)])
    return pal


def test_palette_of_one_bin_and_of_three_bins():
    p = gif_palette(_hist([(_bin(3, 0, 31), 99)]))
    assert p.dtype == np.uint8 and p.shape == (256, 3)
    assert p[0].tolist() == [28, 4, 252] and not p[1:].any()
    p = gif_palette(_hist([(_bin(31, 31, 31), 1), (_bin(0, 0, 1), 500), (_bin(1, 2, 3), 7)]))          # ascending bin order, whatever the counts
    assert p[:3].tolist() == [[4, 4, 12], [12, 20, 28], [252, 252, 252]] and not p[3:].any()


def test_palette_of_exactly_256_bins_gives_every_bin_its_own_entry():
    bins = [_bin(r, g, 5) for r in range(16) for g in range(16)]
    p = gif_palette(_hist([(b, 1 + (b % 7)) for b in bins]))
    assert p.tolist() == [[8 * (b >> 10) + 4, 8 * (b >> 5 & 31) + 4, 44] for b in sorted(bins)]
    lut = gif_lut(p)
    assert [int(lut[b]) for b in sorted(bins)] == list(range(256))


def test_palette_of_257_bins_merges_exactly_two():
    """257 bins: 255 splits leave one box of two bins.  A 16 x 16 sheet of bins (b = 0) of one pixel each and a 257th bin next to its corner in B:
    box 0's longest side is R (16, tie with G: R wins), every cut is a count-weighted median, and the pair left together at the end is decided by
    the tie rules.  The result must be the rule's, restated below with plain loops; two entries of the sheet are missing, their mean is there."""
    bins = [_bin(r, g, 0) for r in range(16) for g in range(16)] + [_bin(0, 0, 1)]
    h = _hist([(b, 1) for b in bins])
    p = gif_palette(h)
    assert p.tolist() == palette_by_the_rule(h)
    centres = {(8 * (b >> 10) + 4, 8 * (b >> 5 & 31) + 4, 8 * (b & 31) + 4) for b in bins}
    entries = {tuple(e) for e in p.tolist()}
    assert len(entries) == 256 and len(centres - entries) == 2 and len(entries - centres) == 1
    a, b = sorted(centres - entries)
    merged, = entries - centres
    assert merged == tuple((2 * (x + y) + 2) // 4 for x, y in zip(a, b))                                 # mean of two, rounded half up


def test_palette_tie_rules():
    """A 7 x 7 x 7 cube of bins with equal counts: every side ties at the first split (R must be cut), the two halves' scores tie after cuts (the
    lower box index goes first), and medians fall between coordinates.  Then the same cube with the counts permuted among the axes."""
    cube = [(_bin(r, g, b), 3) for r in range(7) for g in range(7) for b in range(7)]
    h = _hist(cube)
    p = gif_palette(h)
    assert p.tolist() == palette_by_the_rule(h)
    # the first cut is along R at the median m = 3 (2 * 4 * 49 >= 343): box 0 keeps r <= 3, so the palette is NOT symmetric under swapping R and B
    assert sorted(map(tuple, p[:, ::-1].tolist())) != sorted(map(tuple, p.tolist()))
    rng = np.random.default_rng(11)
    h2 = np.zeros(32768, np.uint32)
    h2[rng.choice(32768, 900, replace=False)] = rng.integers(1, 4, 900)                                 # small counts: many equal scores
    assert gif_palette(h2).tolist() == palette_by_the_rule(h2)


def test_palette_and_lut_are_deterministic_and_lut_is_the_nearest_entry():
    rng = np.random.default_rng(3)
    h = np.zeros(32768, np.uint32)
    h[rng.choice(32768, 5000, replace=False)] = rng.integers(1, 100000, 5000)
    p1, p2 = gif_palette(h), gif_palette(h.copy())
    assert np.array_equal(p1, p2) and p1.tolist() == palette_by_the_rule(h)
    l1, l2 = gif_lut(p1), gif_lut(p1.copy())
    assert l1.dtype == np.uint8 and l1.shape == (32768,) and np.array_equal(l1, l2)
    for pal in (p1, np.repeat(p1[:64], 4, axis=0), gif_palette(_hist([(5, 1), (700, 2)]))):             # the last two have duplicate entries: ties
        b = np.arange(32768)
        centre = np.stack([8 * (b >> 10) + 4, 8 * (b >> 5 & 31) + 4, 8 * (b & 31) + 4], axis=1).astype(np.int64)
        dist = ((centre[:, None, :] - pal[None].astype(np.int64)) ** 2).sum(2)
        want = np.array([int(np.flatnonzero(row == row.min())[0]) for row in dist], np.uint8)
        assert np.array_equal(gif_lut(pal), want)


# ---- container -----------------------------------------------------------------------------------------------------------------------------------
def _walk(buf):
    """A GIF89a file -> (screen (W, H, flags, background, aspect), global table bytes, [(kind, payload)] in file order), checking every block."""
    assert buf[:6] == b"GIF89a"
    W, H, flags, bg, aspect = struct.unpack("<HHBBB", buf[6:13])
    assert flags & 0x80
    n = 3 << ((flags & 7) + 1)
    table = buf[13:13 + n]
    p = 13 + n
    items = []

    def blocks(p):
        data = b""
        while buf[p]:
            assert 1 <= buf[p] <= 255
            data += buf[p + 1:p + 1 + buf[p]]
            p += 1 + buf[p]
        return data, p + 1

    while buf[p] != 0x3B:
        if buf[p] == 0x21 and buf[p + 1] == 0xFF:
            assert buf[p + 2] == 11
            ident = buf[p + 3:p + 14]
            data, p = blocks(p + 14)
            items.append(("app", (ident, data)))
        elif buf[p] == 0x21 and buf[p + 1] == 0xF9:
            assert buf[p + 2] == 4 and buf[p + 7] == 0
            items.append(("gce", struct.unpack("<BHB", buf[p + 3:p + 7])))
            p += 8
        elif buf[p] == 0x2C:
            desc = struct.unpack("<HHHHB", buf[p + 1:p + 10])
            assert not desc[4] & 0x80, "no local colour table"
            mcs = buf[p + 10]
            data, p = blocks(p + 11)
            items.append(("image", (desc, mcs, data)))
        else:
            raise AssertionError(f"unknown block {buf[p]:#x} at {p}")
    assert p == len(buf) - 1, "the trailer ends the file"
    return (W, H, flags, bg, aspect), table, items


@pytest.mark.parametrize("fps,loop,delay", [(25, 0, 4), (8, 3, 12), (12.5, 0, 8)])
def test_write_gif_structure(tmp_path, fps, loop, delay):
    rng = np.random.default_rng(8)
    pal = distinct_palette(1)
    frames = rng.integers(0, 256, (3, 40, 56), dtype=np.uint8)
    frames[1] = 9                                                                                          # a very short frame
    blobs = [sub_blocks(lzw_encode(f)[0]) for f in frames]
    path = tmp_path / "c.gif"
    assert write_gif(str(path), pal, blobs, 56, 40, fps, loop=loop) == path.stat().st_size
    screen, table, items = _walk(path.read_bytes())
    assert screen == (56, 40, 0xF7, 0, 0) and table == pal.tobytes()
    assert [k for k, _ in items] == ["app"] + ["gce", "image"] * 3
    assert items[0][1] == (b"NETSCAPE2.0", b"\x01" + struct.pack("<H", loop))
    for k in range(3):
        assert items[1 + 2 * k][1] == (0, delay, 0)                                                       # no disposal, no transparency
        desc, mcs, data = items[2 + 2 * k][1]
        assert desc == (0, 0, 56, 40, 0) and mcs == 8
        assert np.array_equal(lzw_decode(data, 40 * 56).reshape(40, 56), frames[k])
    back, img = read_gif_indices(path, pal)
    assert img.n_frames == 3 and img.size == (56, 40) and img.info["duration"] == 10 * delay and img.info["loop"] == loop
    assert np.array_equal(back, frames)


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise(tmp_path):
    good = np.zeros((2, 8, 8, 3), np.uint8)
    for bad in (good.astype(np.float32), good[0], good[..., :2], good[:0], np.zeros((2, 0, 8, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8|empty"):
            video_out.encode_gif_frames(bad)
    for pal in (np.zeros((255, 3), np.uint8), np.zeros((256, 4), np.uint8), np.zeros((256, 3), np.int32)):
        with pytest.raises(ValueError, match="palette"):
            video_out.encode_gif_frames(good, palette=pal)
        with pytest.raises(ValueError, match="palette"):
            gif_lut(pal)
        with pytest.raises(ValueError, match="palette"):
            write_gif(str(tmp_path / "x.gif"), pal, [b"\0"], 8, 8, 25)
    with pytest.raises(ValueError, match="strip_rows"):
        video_out.encode_gif_frames(good, strip_rows=0)
    with pytest.raises(ValueError, match="gif_encoder"):
        video_out.save_videos_grid(good[None], str(tmp_path / "x.gif"), gif_encoder="ffmpeg")
    with pytest.raises(ValueError, match="no frames"):
        write_gif(str(tmp_path / "x.gif"), distinct_palette(), [], 8, 8, 25)
    with pytest.raises(ValueError, match="terminator"):
        write_gif(str(tmp_path / "x.gif"), distinct_palette(), [b"\x01\x02"], 8, 8, 25)
    with pytest.raises(ValueError, match="histogram"):
        gif_palette(np.zeros(32768, np.uint32))
    with pytest.raises(ValueError, match="histogram"):
        gif_palette(np.ones(4096, np.uint32))
    assert not (tmp_path / "x.gif").exists()
