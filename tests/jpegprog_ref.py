"""Test-side restatement of the entropy decode of a progressive JPEG file (ITU T.81 G.2 as libjpeg's jdphuff.c does it) in plain Python: the
scans of an SOF2 file -> the coefficient arrays tests/jpegdec_ref.py::coefficients returns, which then go through that module's inverse DCT,
up-sampling and colour conversion.  Test infrastructure: it imports nothing of the package, and the package never imports it.
tests/test_jpegprog.py holds it to PIL byte for byte.

Scope: SOF2, 8 bit, one or three components, luma 1x1 / 2x1 / 2x2 with chroma 1x1, Huffman coding, any legal scan script that brings every
coefficient to full precision, any restart interval per scan."""
import numpy as np

from tests import jpegdec_ref as R


def parse(data):
    """-> dict(H, W, comps=[(id, h, v, tq)], q={id: (64,) natural}, scans=[dict(comps, ss, se, ah, al, ri, td, ta, huff, segments=[bytes])])."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    pos, out, huff, ri = 2, dict(q={}, scans=[]), {}, 0
    while True:
        assert data[pos] == 0xFF, f"no marker at {pos}"
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0xD9:
            return out
        length = int.from_bytes(data[pos:pos + 2], "big")
        body = data[pos + 2:pos + length]
        pos += length
        if m == 0xDB:
            assert not out["scans"], "DQT between scans"
            while body:
                assert body[0] >> 4 == 0, "16-bit DQT"
                q = np.zeros(64, np.int64)
                q[R.ZIGZAG] = list(body[1:65])
                out["q"][body[0] & 15] = q
                body = body[65:]
        elif m == 0xC2:
            assert body[0] == 8
            out["H"], out["W"] = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            out["comps"] = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(body[5])]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise AssertionError(f"SOF{m - 0xC0} is out of scope")
        elif m == 0xC4:
            while body:
                n = sum(body[1:17])
                huff[(body[0] >> 4, body[0] & 15)] = (bytes(body[1:17]), bytes(body[17:17 + n]))
                body = body[17 + n:]
        elif m == 0xDD:
            ri = int.from_bytes(body, "big")
        elif m == 0xDA:
            ns = body[0]
            ids = [c[0] for c in out["comps"]]
            scan = dict(comps=[ids.index(body[1 + 2 * i]) for i in range(ns)], td=[body[2 + 2 * i] >> 4 for i in range(ns)],
                        ta=[body[2 + 2 * i] & 15 for i in range(ns)], ss=body[1 + 2 * ns], se=body[2 + 2 * ns], ah=body[3 + 2 * ns] >> 4,
                        al=body[3 + 2 * ns] & 15, ri=ri, huff=dict(huff), segments=[])
            start = i = pos                                             # cut at every marker (0xFF followed by neither 0x00 nor 0xFF)
            while True:
                i = data.index(b"\xff", i)
                nxt = data[i + 1]
                if nxt == 0 or nxt == 0xFF:
                    i += 1
                    continue
                scan["segments"].append(data[start:i])
                if not 0xD0 <= nxt <= 0xD7:
                    break
                assert nxt == 0xD0 + ((len(scan["segments"]) - 1) & 7), f"marker {nxt:#x} in a scan"
                i = start = i + 2
            out["scans"].append(scan)
            pos = i


def scan_units(p, scan):
    """(units, columns) of a scan: the frame's MCUs when it interleaves the components, else the one component's own blocks."""
    ncomp, hs, vs, rows, cols = R.geometry(p)
    if len(scan["comps"]) > 1:
        return rows * cols, cols
    w, h = (p["W"], p["H"]) if scan["comps"][0] == 0 else (-(-p["W"] // hs), -(-p["H"] // vs))
    return (-(-w // 8)) * (-(-h // 8)), -(-w // 8)


def levels(scans):
    """The definition, literally: 0 if no earlier scan shares a (component, coefficient) pair, else 1 + the largest level among those that do."""
    out = []
    for i, s in enumerate(scans):
        mine = {(c, k) for c in s[0] for k in range(s[1], s[2] + 1)}
        shared = [out[j] for j, t in enumerate(scans[:i]) if mine & {(c, k) for c in t[0] for k in range(t[1], t[2] + 1)}]
        out.append(1 + max(shared) if shared else 0)
    return out


def coefficients(p):
    """-> one int64 array (block_rows, block_cols, 64) in natural order per component, the shape jpegdec_ref.coefficients gives."""
    ncomp, hs, vs, rows, cols = R.geometry(p)
    samp = [(hs, vs)] + [(1, 1)] * (ncomp - 1)
    coef = [np.zeros((rows * v, cols * h, 64), np.int64) for h, v in samp]
    zz = R.ZIGZAG.tolist()
    for scan in p["scans"]:
        ss, se, ah, al, ns = scan["ss"], scan["se"], scan["ah"], scan["al"], len(scan["comps"])
        units, ucols = scan_units(p, scan)
        step = scan["ri"] or units
        assert len(scan["segments"]) == -(-units // step), "segment count"
        p1, m1 = 1 << al, -(1 << al)
        dc_look = [R._lookup(*scan["huff"][(0, t)]) for t in scan["td"]] if ss == 0 and ah == 0 else None
        ac_look = R._lookup(*scan["huff"][(1, scan["ta"][0])]) if ss > 0 else None
        for s, seg in enumerate(scan["segments"]):
            b = R._Bits(seg)
            pred, eobrun = [0] * ns, 0
            for u in range(s * step, min((s + 1) * step, units)):
                uy, ux = divmod(u, ucols)
                if ss == 0:
                    for i, c in enumerate(scan["comps"]):
                        h, v = samp[c] if ns > 1 else (1, 1)
                        for by in range(v):
                            for bx in range(h):
                                blk = coef[c][uy * v + by, ux * h + bx]
                                if ah == 0:
                                    ln, sym = dc_look[i]
                                    w = b.peek16()
                                    assert ln[w], "bad DC code"
                                    b.pos += ln[w]
                                    cat = sym[w]
                                    if cat:
                                        pred[i] += R._extend(b.take(cat), cat)
                                    blk[0] = pred[i] << al
                                elif b.take(1):
                                    blk[0] |= p1
                    continue
                c = scan["comps"][0]
                ln, sym = ac_look
                blk = coef[c][uy, ux]
                k = ss
                if eobrun == 0:
                    while k <= se:
                        w = b.peek16()
                        assert ln[w], "bad AC code"
                        b.pos += ln[w]
                        r, cat = sym[w] >> 4, sym[w] & 15
                        if cat == 0 and r != 15:
                            eobrun = (1 << r) + (b.take(r) if r else 0)
                            p.setdefault("eob_runs", []).append(eobrun)            # for the tests that want a long run among their fixtures
                            break
                        if ah == 0:
                            if cat == 0:
                                k += 16
                                continue
                            k += r
                            assert k <= se, "index past Se"
                            blk[zz[k]] = R._extend(b.take(cat), cat) << al
                            k += 1
                            continue
                        new = 0
                        if cat:
                            assert cat == 1, "refinement category"
                            new = p1 if b.take(1) else m1
                        while k <= se:
                            v = int(blk[zz[k]])
                            if v:
                                if b.take(1) and not v & p1:
                                    blk[zz[k]] = v + (p1 if v >= 0 else m1)
                            else:
                                r -= 1
                                if r < 0:
                                    break
                            k += 1
                        if new:
                            assert k <= se, "index past Se"
                            blk[zz[k]] = new
                        k += 1
                if eobrun > 0:
                    if ah:
                        while k <= se:
                            v = int(blk[zz[k]])
                            if v and b.take(1) and not v & p1:
                                blk[zz[k]] = v + (p1 if v >= 0 else m1)
                            k += 1
                    eobrun -= 1
            assert eobrun == 0, "EOB run past the segment"
            assert b.pos <= b.n, "segment exhausted"
    return coef


def decode(data):
    """One progressive JPEG file -> (H, W, 3) uint8 RGB; a one-component file gives Y in all three channels."""
    p = parse(data)
    ncomp, hs, vs, _, _ = R.geometry(p)
    H, W = p["H"], p["W"]
    planes = [R.idct_plane(c, p["q"][p["comps"][k][3]]) for k, c in enumerate(coefficients(p))]
    if ncomp == 1:
        return np.repeat(planes[0][:H, :W, None], 3, axis=2)
    cb, cr = (R.upsample(planes[k], hs, vs, H, W)[:H, :W] for k in (1, 2))
    return R.colour(planes[0][:H, :W], cb, cr)
