"""The yardstick of the lossy WebP decoder: a plain numpy / Python decoder of VP8 key frames as libwebp decodes them, written from the
format (RFC 6386) and held to PIL on every byte by tests/test_vp8dec.py; independent of csrc/vp8dec_core.h.  Whole frames in raster order: parse
everything, reconstruct, filter in place, convert (tests/vp8_ref.decoded_rgb).  It carries counters of what a stream used, so that the tests can
show that their inputs reach every part of the format.

decode_vp8(payload, counters=None) -> dict(W, H, header, mbs (mbh, mbw) of dicts, coeffs (mbh, mbw, 24, 16) raster, unfiltered (Y, U, V),
filtered (Y, U, V), rgb (H, W, 3)); Bad for what libwebp refuses."""
import numpy as np

from tests import vp8_ref as E

DC, TM, VE, HE, RD, VR, LD, VL, HD, HU = range(10)
BMODE_NAMES = ("DC", "TM", "VE", "HE", "RD", "VR", "LD", "VL", "HD", "HU")
BMODE_TREE = (-DC, 1, -TM, 2, -VE, 3, 4, 6, -HE, 5, -RD, -VR, -LD, 7, -VL, 8, -HD, -HU)
# sub-block mode probabilities [top][left][node], as located in the read-only data of the libwebp that Pillow ships
BMODE_PROBS = np.frombuffer(bytes.fromhex(
    "e7783059737178987098b3407eaa762e465faf458f505552489b67383a0aabdabd110d98721a11a32cc3150aad791850c31a3e2c405590470a26abd590221aaa2e371388a021ce47"
    "3f14087272d00c09e251280b60b6541d102486b7598962656aa59448bb64829d6f204b504266a7634a3e28ea80293509b2f18d1a086b4a2b1a9249a631179d412669a033341f7380"
    "684f0c1bd9ff5711075744472c72330fba172f290e6eb6b71511c2422d1966c5bd171216585893962a2e2dc4cd2b61b775552623b33d2735c8571a152be8ab3822336872661d5d4d"
    "271c55ab3aa55a6240221674ce17222ba6496b36201a3301512b1f44196a1640ab24e1722213156684bc104c7c3e124e5f5539323033c165239fd76f592e6f3c941facdbe415126f"
    "70714d55b3ff267872282a01c4f5d10a196d582b1d8ca6d5252b9a3d3f1e9b432d4401d16450082b9a01331a478e4e4e10ff8022c5ab29280566d3b70401dd333211a8d1c0171952"
    "8a1f24ab1ba6262ce543573aa952731a3bb33f3b5ab43ba65d499a282815748fd12227af2f0f10b722df312db72e1121b706620f20b7392e16188001361125412049731c801780cd"
    "2803097333c01206df572509733b4d40152f68372cda09363582e2405a46cd2829171a39363970b8052926a6d51e221a8598740a2086271335dd1a722049ff1f0941ea020f017649"
    "4b200c33c0ffa02b33581f2343665537ba553815176f3bcd2d25c03726467c49660122627d622a58685575af525f543559806471652d4b4f7b2f338051ab01391105476639352931"
    "26210d7939491a0155290a438a4d6e5a2f727315020a66ffa61706651d100a558065c41a39120a6666d522142b75140f24a38044011a663d472522351ff3c0453c472649771cde25"
    "442d8022012f0bf5ab3e1113469255373e46252b259a64a355a0013f095c881c4020c9554b0f090940ffb8771056061c0540ff19f8013808118489ff3774803a0f145287391a7928"
    "a4321f899a851923da33672c83837b1f069e5628408794e02db780161a1183f09a0e01d12d10155b40de0701c53815279b3c8a1766d5530c0d36c0ff442f1c551a555580802092ab"
    "120b073f90ab0404f6231b0a92aeab0c1a80be502363b4507e362d557e2f57b033291420654b808b769274805538290fb0ec5525093e471e117776ff11128a65263c8a37462b1a8e"
    "9224131eabff611b148a2d3d3edb0151bc4020291475978e1415a370130c3dc380300418"), np.uint8).reshape(10, 10, 9)
TOKEN_KINDS = ("eob", "zero", "one", "two", "three", "four", "cat1", "cat2", "cat3", "cat4", "cat5", "cat6")


class Bad(Exception):
    pass


def new_counters():
    return dict(segments=set(), map_update=0, no_map_update=0, absolute=0, delta=0, i4x4=0, i16=0, bmodes=set(), ymodes=set(), uvmodes=set(),
                prob_updates=0, skip_on=0, skip_off=0, tokens=set(), simple=0, normal=0, unfiltered=0, inner_skips=0, hev=0, no_hev=0,
                partitions=set(), profiles=set(), sharpness=set(), lf_delta=0, lf_delta_update=0, quant_deltas=0, levels=set())


class BoolReader:
    """RFC 6386 section 7.3, with libwebp's end-of-data flag: set once a symbol is read for which a byte past the end had to be loaded."""

    def __init__(self, data):
        self.data, self.size = data, len(data)
        self.value = (self._byte(0) << 8) | self._byte(1)
        self.pos, self.range, self.count, self.shifts, self.eof = 2, 255, 0, 0, len(data) == 0

    def _byte(self, k):
        return self.data[k] if k < self.size else 0

    def get(self, prob):
        if 1 + (self.shifts + 7) // 8 > self.size:
            self.eof = True
        split = 1 + (((self.range - 1) * prob) >> 8)
        big = split << 8
        if self.value >= big:
            bit = 1
            self.range -= split
            self.value -= big
        else:
            bit = 0
            self.range = split
        while self.range < 128:
            self.value <<= 1
            self.range <<= 1
            self.shifts += 1
            self.count += 1
            if self.count == 8:
                self.count = 0
                self.value |= self._byte(self.pos)
                self.pos += 1
        return bit

    def bits(self, n):
        v = 0
        for k in range(n - 1, -1, -1):
            v |= self.get(128) << k
        return v

    def signed(self, n):
        v = self.bits(n)
        return -v if self.get(128) else v

    def opt_signed(self, n):
        return self.signed(n) if self.get(128) else 0


def parse_header(br, c):
    h = dict(colour_space=br.get(128), clamp=br.get(128), use_segment=br.get(128), update_map=0, absolute=1, quantizer=[0] * 4, strength=[0] * 4,
             seg_probs=[255] * 3, ref_delta=[0] * 4, mode_delta=[0] * 4)
    if h["use_segment"]:
        h["update_map"] = br.get(128)
        if br.get(128):
            h["absolute"] = br.get(128)
            h["quantizer"] = [br.opt_signed(7) for _ in range(4)]
            h["strength"] = [br.opt_signed(6) for _ in range(4)]
            c["absolute" if h["absolute"] else "delta"] += 1
        if h["update_map"]:
            h["seg_probs"] = [br.bits(8) if br.get(128) else 255 for _ in range(3)]
        c["map_update" if h["update_map"] else "no_map_update"] += 1
    h["simple"], h["level"], h["sharpness"] = br.get(128), br.bits(6), br.bits(3)
    h["use_lf_delta"] = br.get(128)
    if h["use_lf_delta"]:
        c["lf_delta"] += 1
        if br.get(128):
            c["lf_delta_update"] += 1
            for arr in (h["ref_delta"], h["mode_delta"]):
                for i in range(4):
                    if br.get(128):
                        arr[i] = br.signed(6)
    h["parts"] = 1 << br.bits(2)
    h["base_q"] = br.bits(7)
    h["dq"] = [br.opt_signed(4) for _ in range(5)]                               # y1 dc, y2 dc, y2 ac, uv dc, uv ac
    c["quant_deltas"] += any(h["dq"])
    h["refresh"] = br.get(128)
    probs = E.COEF_PROBS.astype(np.int64).reshape(-1).copy()
    for i, up in enumerate(E.UPDATE_PROBS.reshape(-1)):
        if br.get(int(up)):
            probs[i] = br.bits(8)
            c["prob_updates"] += 1
    h["probs"] = probs.reshape(4, 8, 3, 11)
    h["use_skip"] = br.get(128)
    h["skip_p"] = br.bits(8) if h["use_skip"] else 0
    c["skip_on" if h["use_skip"] else "skip_off"] += 1
    c["partitions"].add(h["parts"]), c["sharpness"].add(h["sharpness"]), c["levels"].add(h["level"])
    clip = lambda v, hi: min(max(v, 0), hi)
    h["quant"], h["filter"] = [], []
    for s in range(4):
        q = h["base_q"]
        if h["use_segment"]:
            q = h["quantizer"][s] + (0 if h["absolute"] else h["base_q"])
        d = h["dq"]
        h["quant"].append((E.DC_Q[clip(q + d[0], 127)], E.AC_Q[clip(q, 127)], E.DC_Q[clip(q + d[1], 127)] * 2,
                           max(8, E.AC_Q[clip(q + d[2], 127)] * 155 // 100), E.DC_Q[clip(q + d[3], 117)], E.AC_Q[clip(q + d[4], 127)]))
        base = h["level"]
        if h["use_segment"]:
            base = h["strength"][s] + (0 if h["absolute"] else h["level"])
        pair = []
        for i4 in (0, 1):
            level = base
            if h["use_lf_delta"]:
                level += h["ref_delta"][0] + (h["mode_delta"][0] if i4 else 0)
            level = clip(level, 63)
            if level == 0:
                pair.append((0, 0, 0))
                continue
            il = level
            if h["sharpness"]:
                il >>= 2 if h["sharpness"] > 4 else 1
                il = min(il, 9 - h["sharpness"])
            il = max(il, 1)
            pair.append((2 * level + il, il, 2 if level >= 40 else 1 if level >= 15 else 0))
        h["filter"].append(pair)
    h["filter_type"] = 0 if h["level"] == 0 else 1 if h["simple"] else 2           # a header level of 0 switches the filter off for every segment
    return h


def read_modes(br, h, up, left, c):
    mb = dict(segment=0, skip=0)
    if h["update_map"]:
        mb["segment"] = br.get(h["seg_probs"][1]) if not br.get(h["seg_probs"][0]) else 2 + br.get(h["seg_probs"][2])
    if h["use_skip"]:
        mb["skip"] = br.get(h["skip_p"])
    mb["i4x4"] = not br.get(145)
    if not mb["i4x4"]:
        m = (TM if br.get(128) else HE) if br.get(156) else (VE if br.get(163) else DC)
        mb["modes"] = [m] * 16
        c["i16"] += 1
        c["ymodes"].add(m)
    else:
        modes = [0] * 16
        for y in range(4):
            for x in range(4):
                top = modes[4 * y - 4 + x] if y else up["modes"][12 + x] if up else DC
                lft = modes[4 * y + x - 1] if x else left["modes"][4 * y + 3] if left else DC
                p = BMODE_PROBS[top][lft]
                i = BMODE_TREE[br.get(int(p[0]))]
                while i > 0:
                    i = BMODE_TREE[2 * i + br.get(int(p[i]))]
                modes[4 * y + x] = -i
                c["bmodes"].add((-i, y, x))
        mb["modes"] = modes
        c["i4x4"] += 1
    mb["uvmode"] = DC if not br.get(142) else VE if not br.get(114) else TM if br.get(183) else HE
    c["uvmodes"].add(mb["uvmode"])
    c["segments"].add(mb["segment"])
    return mb


def read_block(br, probs, ctx, dq, first, out, c):
    """One block's tokens from position `first`; out: 16 raster coefficients.  Returns the position behind the last coded coefficient."""
    n = first
    p = probs[E.BANDS[n]][ctx]
    while n < 16:
        if not br.get(int(p[0])):
            c["tokens"].add("eob")
            return n
        while not br.get(int(p[1])):
            c["tokens"].add("zero")
            n += 1
            p = probs[E.BANDS[n]][0]
            if n == 16:
                return 16
        nxt = probs[E.BANDS[n + 1]]
        if not br.get(int(p[2])):
            v, kind, q = 1, "one", nxt[1]
        else:
            q = nxt[2]
            if not br.get(int(p[3])):
                if not br.get(int(p[4])):
                    v, kind = 2, "two"
                else:
                    v = 3 + br.get(int(p[5]))
                    kind = "three" if v == 3 else "four"
            elif not br.get(int(p[6])):
                if not br.get(int(p[7])):
                    v, kind = 5 + br.get(159), "cat1"
                else:
                    v = 7 + 2 * br.get(165)
                    v, kind = v + br.get(145), "cat2"
            else:
                b1 = br.get(int(p[8]))
                b0 = br.get(int(p[9 + b1]))
                cat = 2 * b1 + b0
                v = 0
                for pr in (E.CAT3, E.CAT4, E.CAT5, E.CAT6)[cat]:
                    v = 2 * v + br.get(pr)
                v += 3 + (8 << cat)
                kind = f"cat{3 + cat}"
        c["tokens"].add(kind)
        if br.get(128):
            v = -v
        out[E.ZIGZAG[n]] = int(np.int16(np.int64(v * dq[1 if n else 0]) & 0xFFFF))  # libwebp stores 16 bits
        p = q
        n += 1
    return 16


def read_residuals(br, h, mb, top, left, c):
    """top, left: dicts(nz: 8 flags [4 luma, 2 U, 2 V], dc) of the column's and the row's context, updated in place."""
    coef = np.zeros((24, 16), np.int64)
    q = h["quant"][mb["segment"]]
    if h["use_skip"] and mb["skip"]:
        top["nz"], left["nz"] = [0] * 8, [0] * 8
        if not mb["i4x4"]:
            top["dc"] = left["dc"] = 0
        return coef, False
    any_coded = False
    if not mb["i4x4"]:
        dc = np.zeros(16, np.int64)
        nz = read_block(br, h["probs"][1], top["dc"] + left["dc"], q[2:4], 0, dc, c)
        top["dc"] = left["dc"] = int(nz > 0)
        if nz > 1:
            coef[:16, 0] = E.iwht(dc)
        else:
            coef[:16, 0] = (dc[0] + 3) >> 3
        first, probs = 1, h["probs"][0]
    else:
        first, probs = 0, h["probs"][3]
    for y in range(4):
        for x in range(4):
            b = 4 * y + x
            nz = read_block(br, probs, top["nz"][x] + left["nz"][y], q[0:2], first, coef[b], c)
            top["nz"][x] = left["nz"][y] = int(nz > first)
            any_coded |= nz > 1 or coef[b, 0] != 0
    for ch in (0, 1):
        for y in range(2):
            for x in range(2):
                b = 16 + 4 * ch + 2 * y + x
                nz = read_block(br, h["probs"][2], top["nz"][4 + 2 * ch + x] + left["nz"][4 + 2 * ch + y], q[4:6], 0, coef[b], c)
                top["nz"][4 + 2 * ch + x] = left["nz"][4 + 2 * ch + y] = int(nz > 0)
                any_coded |= nz > 1 or coef[b, 0] != 0
    return coef, bool(any_coded)


# ---- prediction ---------------------------------------------------------------------------------------------------------------------------------------
def _avg2(a, b):
    return (a + b + 1) >> 1


def _avg3(a, b, c):
    return (a + 2 * b + c + 2) >> 2


# RFC 6386 section 12.3 on the edge E = L K J I X A B C D: (row, column) -> (taps, first edge index)
_VR = {(3, 0): (3, 1), (2, 0): (3, 2), (3, 1): (3, 3), (1, 0): (3, 3), (2, 1): (2, 4), (0, 0): (2, 4), (3, 2): (3, 4), (1, 1): (3, 4), (2, 2): (2, 5),
       (0, 1): (2, 5), (3, 3): (3, 5), (1, 2): (3, 5), (2, 3): (2, 6), (0, 2): (2, 6), (1, 3): (3, 6), (0, 3): (2, 7)}
_HD = {(3, 0): (2, 0), (3, 1): (3, 0), (2, 0): (2, 1), (3, 2): (2, 1), (2, 1): (3, 1), (3, 3): (3, 1), (2, 2): (2, 2), (1, 0): (2, 2), (2, 3): (3, 2),
       (1, 1): (3, 2), (1, 2): (2, 3), (0, 0): (2, 3), (1, 3): (3, 3), (0, 1): (3, 3), (0, 2): (3, 4), (0, 3): (3, 5)}


def _fill(p, e, table):
    for (y, x), (taps, k) in table.items():
        p[y, x] = _avg2(e[k], e[k + 1]) if taps == 2 else _avg3(e[k], e[k + 1], e[k + 2])


def predict4(mode, edge, left):
    """edge: the 9 pixels X A B C D E F G H above (corner first); left: I J K L.  -> (4, 4) [y][x]."""
    X, A, B, C, D, Ee, F, G, H = (int(v) for v in edge)
    I, J, K, L = (int(v) for v in left)
    p = np.zeros((4, 4), np.int64)
    if mode == DC:
        p[:] = (A + B + C + D + I + J + K + L + 4) >> 3
    elif mode == TM:
        p[:] = np.clip(np.array([I, J, K, L])[:, None] + np.array([A, B, C, D])[None] - X, 0, 255)
    elif mode == VE:
        p[:] = np.array([_avg3(X, A, B), _avg3(A, B, C), _avg3(B, C, D), _avg3(C, D, Ee)])[None]
    elif mode == HE:
        p[:] = np.array([_avg3(X, I, J), _avg3(I, J, K), _avg3(J, K, L), _avg3(K, L, L)])[:, None]
    elif mode == LD:
        t = [A, B, C, D, Ee, F, G, H, H]
        for y in range(4):
            for x in range(4):
                p[y, x] = _avg3(t[x + y], t[x + y + 1], t[x + y + 2])
    elif mode == RD:
        e = [L, K, J, I, X, A, B, C, D]                                          # the edge from bottom-left to top-right
        for y in range(4):
            for x in range(4):
                k = 3 - y + x
                p[y, x] = _avg3(e[k], e[k + 1], e[k + 2])
    elif mode == VR:
        _fill(p, [L, K, J, I, X, A, B, C, D], _VR)
    elif mode == VL:
        t = [A, B, C, D, Ee, F, G, H]
        for y in range(4):
            for x in range(4):
                k = x + (y >> 1)
                p[y, x] = _avg2(t[k], t[k + 1]) if y % 2 == 0 else _avg3(t[k], t[k + 1], t[k + 2])
        p[2, 3], p[3, 3] = _avg3(Ee, F, G), _avg3(F, G, H)                         # the format's two exceptions in the last column
    elif mode == HD:
        _fill(p, [L, K, J, I, X, A, B, C, D], _HD)
    elif mode == HU:
        e = [I, J, K, L, L, L, L, L]
        for y in range(4):
            for x in range(4):
                z = x + 2 * y
                if z > 5:
                    p[y, x] = L
                elif z % 2 == 0:
                    p[y, x] = _avg2(e[z >> 1], e[(z >> 1) + 1])
                else:
                    p[y, x] = _avg3(e[z >> 1], e[(z >> 1) + 1], e[(z >> 1) + 2])
    return p


_MODE16 = {DC: 0, VE: 1, HE: 2, TM: 3}                                             # -> tests/vp8_ref.predictions' order


def reconstruct(W, H, mbs, coeffs):
    mbh, mbw = len(mbs), len(mbs[0])
    Y, U, V = np.zeros((16 * mbh, 16 * mbw), np.uint8), np.zeros((8 * mbh, 8 * mbw), np.uint8), np.zeros((8 * mbh, 8 * mbw), np.uint8)
    for my in range(mbh):
        for mx in range(mbw):
            mb, cf = mbs[my][mx], coeffs[my, mx]
            if mb["i4x4"]:
                above = Y[16 * my - 1, :].astype(np.int64) if my else None
                right = (np.full(4, 127) if not my else np.full(4, above[16 * mx + 15]) if mx == mbw - 1 else above[16 * mx + 16:16 * mx + 20])
                for b in range(16):
                    by, bx = divmod(b, 4)
                    y0, x0 = 16 * my + 4 * by, 16 * mx + 4 * bx
                    edge = np.full(9, 127, np.int64)
                    if y0:
                        row = Y[y0 - 1].astype(np.int64)
                        edge[0] = row[x0 - 1] if x0 else 129
                        edge[1:5] = row[x0:x0 + 4]
                        edge[5:9] = row[x0 + 4:x0 + 8] if bx < 3 else right        # the right-hand column: the row above the macroblock
                    left = Y[y0:y0 + 4, x0 - 1].astype(np.int64) if x0 else np.full(4, 129, np.int64)
                    Y[y0:y0 + 4, x0:x0 + 4] = E.idct_add(cf[b], predict4(mb["modes"][b], edge, left))
            else:
                pred = E.predictions(Y, my, mx, 16)[_MODE16[mb["modes"][0]]]
                for b in range(16):
                    by, bx = divmod(b, 4)
                    Y[16 * my + 4 * by:16 * my + 4 * by + 4, 16 * mx + 4 * bx:16 * mx + 4 * bx + 4] = \
                        E.idct_add(cf[b], pred[4 * by:4 * by + 4, 4 * bx:4 * bx + 4])
            for k, P in enumerate((U, V)):
                pred = E.predictions(P, my, mx, 8)[_MODE16[mb["uvmode"]]]
                for b in range(4):
                    by, bx = divmod(b, 2)
                    P[8 * my + 4 * by:8 * my + 4 * by + 4, 8 * mx + 4 * bx:8 * mx + 4 * bx + 4] = \
                        E.idct_add(cf[16 + 4 * k + b], pred[4 * by:4 * by + 4, 4 * bx:4 * bx + 4])
    return Y, U, V


# ---- the loop filter: RFC 6386 section 15, on int arrays ------------------------------------------------------------------------------------------------
def _c(v):                                                                         # signed 8-bit clamp
    return -128 if v < -128 else 127 if v > 127 else v


def _common_adjust(use_outer, px):
    """px: list of pixel values across the edge (P3 .. Q3), as signed (value - 128); adjusts P0 (px[3]) and Q0 (px[4]); returns the filter value."""
    p1, p0, q0, q1 = px[2], px[3], px[4], px[5]
    a = _c((_c(p1 - q1) if use_outer else 0) + 3 * (q0 - p0))
    f1 = _c(a + 4) >> 3
    f2 = _c(a + 3) >> 3
    px[4], px[3] = _c(q0 - f1), _c(p0 + f2)
    return f1


def filter_position(px, kind, limit, interior, hevt, c):
    """px: the 8 unsigned pixels P3 P2 P1 P0 Q0 Q1 Q2 Q3 across an edge -> the filtered 8.  kind: 'simple', 'mb' or 'sub'."""
    p3, p2, p1, p0, q0, q1, q2, q3 = px
    if abs(p0 - q0) * 4 + abs(p1 - q1) > 2 * limit + 1:
        return px
    if kind == "simple":
        s = [v - 128 for v in px]
        _common_adjust(True, s)
        return [v + 128 for v in s]
    if max(abs(p3 - p2), abs(p2 - p1), abs(p1 - p0), abs(q3 - q2), abs(q2 - q1), abs(q1 - q0)) > interior:
        return px
    hev = abs(p1 - p0) > hevt or abs(q1 - q0) > hevt
    c["hev" if hev else "no_hev"] += 1
    s = [v - 128 for v in px]
    if hev:
        _common_adjust(True, s)
    elif kind == "sub":
        a = (_common_adjust(False, s) + 1) >> 1
        s[5], s[2] = _c(s[5] - a), _c(s[2] + a)
    else:
        w = _c(_c(s[2] - s[5]) + 3 * (s[4] - s[3]))
        for k, mul in enumerate((27, 18, 9)):
            a = _c((mul * w + 63) >> 7)
            s[4 + k], s[3 - k] = _c(s[4 + k] - a), _c(s[3 - k] + a)
    return [v + 128 for v in s]


def _filter_edge(P, y, x, vertical_edge, n, kind, limit, interior, hevt, c):
    """The edge whose first Q0 pixel is P[y, x]: a vertical edge runs down n rows (taps along x), a horizontal one along n columns."""
    for i in range(n):
        if vertical_edge:
            px = [int(v) for v in P[y + i, x - 4:x + 4]]
            P[y + i, x - 4:x + 4] = filter_position(px, kind, limit, interior, hevt, c)
        else:
            px = [int(v) for v in P[y - 4:y + 4, x + i]]
            P[y - 4:y + 4, x + i] = filter_position(px, kind, limit, interior, hevt, c)


def loop_filter(h, mbs, planes, inner, c):
    """In place, macroblocks in raster order; within one: left edge, inner vertical edges, top edge, inner horizontal edges."""
    Y, U, V = (p.copy() for p in planes)
    if h["filter_type"] == 0:
        c["unfiltered"] += 1
        return Y, U, V
    c["simple" if h["filter_type"] == 1 else "normal"] += 1
    simple = h["filter_type"] == 1
    # edges on the frame's border are never filtered, so every 8-pixel window lies inside the planes
    for my in range(len(mbs)):
        for mx in range(len(mbs[0])):
            mb = mbs[my][mx]
            limit, interior, hevt = h["filter"][mb["segment"]][int(mb["i4x4"])]
            if limit == 0:
                continue
            do_inner = inner[my][mx]
            if not do_inner:
                c["inner_skips"] += 1
            kinds = ("simple", "simple") if simple else ("mb", "sub")
            planes_here = [(Y, 16)] if simple else [(Y, 16), (U, 8), (V, 8)]
            for vertical in (True, False):
                for P, n in planes_here:
                    y0, x0 = n * my, n * mx
                    if (mx if vertical else my) > 0:
                        _filter_edge(P, y0, x0, vertical, n, kinds[0], limit + 4, interior, hevt, c)
                for P, n in planes_here:
                    y0, x0 = n * my, n * mx
                    if do_inner:
                        for k in range(4, n, 4):
                            _filter_edge(P, y0 + (0 if vertical else k), x0 + (k if vertical else 0), vertical, n, kinds[1], limit, interior, hevt, c)
    return Y, U, V


# ---- a frame ------------------------------------------------------------------------------------------------------------------------------------------
def decode_vp8(payload, counters=None):
    c = counters if counters is not None else new_counters()
    if len(payload) < 10:
        raise Bad("no room for the frame header")
    tag = int.from_bytes(payload[:3], "little")
    if tag & 1 or (tag >> 1 & 7) > 3 or not tag >> 4 & 1 or payload[3:6] != b"\x9d\x01\x2a":
        raise Bad("not a shown key frame of profile 0 .. 3")
    c["profiles"].add(tag >> 1 & 7)
    W, H = int.from_bytes(payload[6:8], "little") & 0x3FFF, int.from_bytes(payload[8:10], "little") & 0x3FFF
    first = tag >> 5
    if first > len(payload) - 10:
        raise Bad("the first partition runs past the payload")
    br = BoolReader(payload[10:10 + first])
    h = parse_header(br, c)
    if br.eof:
        raise Bad("the first partition ends inside the header")
    rest = payload[10 + first:]
    last = h["parts"] - 1
    if len(rest) < 3 * last:
        raise Bad("the partition table runs past the payload")
    at, readers = 3 * last, []
    for p in range(last):
        size = min(int.from_bytes(rest[3 * p:3 * p + 3], "little"), len(rest) - at)
        readers.append(BoolReader(rest[at:at + size]))
        at += size
    if at >= len(rest):
        raise Bad("the last partition is empty")
    readers.append(BoolReader(rest[at:]))
    mbw, mbh = (W + 15) // 16, (H + 15) // 16
    mbs, coeffs, inner = [], np.zeros((mbh, mbw, 24, 16), np.int64), []
    tops = [dict(nz=[0] * 8, dc=0) for _ in range(mbw)]
    for my in range(mbh):
        row = []
        for mx in range(mbw):
            row.append(read_modes(br, h, mbs[my - 1][mx] if my else None, row[mx - 1] if mx else None, c))
        if br.eof:
            raise Bad("the first partition ends inside the macroblock modes")
        mbs.append(row)
        left, tr, flags = dict(nz=[0] * 8, dc=0), readers[my & last], []
        for mx in range(mbw):
            coeffs[my, mx], coded = read_residuals(tr, h, row[mx], tops[mx], left, c)
            flags.append(bool(row[mx]["i4x4"]) or coded)                          # the parsed result decides, not the skip flag
            if tr.eof:
                raise Bad("a token partition ends inside its macroblocks")
        inner.append(flags)
    unfiltered = reconstruct(W, H, mbs, coeffs)
    filtered = loop_filter(h, mbs, unfiltered, inner, c)
    return dict(W=W, H=H, header=h, mbs=mbs, coeffs=coeffs, inner=inner, unfiltered=unfiltered, filtered=filtered, rgb=E.decoded_rgb(filtered, H, W))


def _chunks(data, pos, end):
    """(kind, body, body with its padding byte where the chunk's length is odd and the byte is there)."""
    while pos + 8 <= end:
        kind, ln = data[pos:pos + 4], int.from_bytes(data[pos + 4:pos + 8], "little")
        yield kind, data[pos + 8:pos + 8 + ln], data[pos + 8:min(pos + 8 + ln + (ln & 1), end)]
        pos += 8 + ln + (ln & 1)


def decode_file(data, counters=None):
    """A WebP file whose frames are `VP8 ` or VP8L chunks, still or animated -> list of (H, W, 3) uint8 RGB canvases, one per frame, composed as
    libwebp's WebPAnimDecoder composes them (tests/webpdec_ref.compose; a lossy frame without ALPH is opaque).  libwebp hands the VP8 decoder a
    chunk WITH its padding byte, so the last partition of an odd-length chunk is one byte longer than the chunk says."""
    from tests import webpdec_ref as L
    frames, canvas = [], None
    for kind, body, padded in _chunks(data, 12, min(len(data), 8 + int.from_bytes(data[4:8], "little"))):
        if kind == b"VP8X":
            canvas = (L._u24(body, 4) + 1, L._u24(body, 7) + 1)
        elif kind in (b"VP8 ", b"VP8L"):
            frames.append({"x": 0, "y": 0, "blend": False, "dispose": False, "kind": kind, "payload": padded if kind == b"VP8 " else body})
        elif kind == b"ALPH":
            raise Bad("ALPH")
        elif kind == b"ANMF":
            sub = list(_chunks(body, 16, len(body)))
            if any(k == b"ALPH" for k, _, _ in sub):
                raise Bad("ALPH")
            k, b, padded = next(c for c in sub if c[0] in (b"VP8 ", b"VP8L"))
            frames.append({"x": 2 * L._u24(body, 0), "y": 2 * L._u24(body, 3), "blend": not body[15] & 2, "dispose": bool(body[15] & 1), "kind": k,
                           "payload": padded if k == b"VP8 " else b})
    decoded = []
    for f in frames:
        if f["kind"] == b"VP8L":
            decoded.append(L.decode_vp8l(f["payload"]))
        else:
            d = decode_vp8(f["payload"], counters)
            r = d["rgb"].astype(np.uint32)
            decoded.append({"width": d["W"], "height": d["H"], "alpha_is_used": False, "argb": 0xFF000000 | r[..., 0] << 16 | r[..., 1] << 8 | r[..., 2]})
    if canvas is None:
        canvas = (decoded[0]["width"], decoded[0]["height"])
    return [c[..., :3] for c in L.compose(canvas[0], canvas[1], frames, decoded)]
