"""The JPEG encoder's samplings (4:2:0, 4:2:2, 4:4:4) and optimised Huffman tables as a numpy / Python statement, a parser of any
baseline three-component stream that also counts the symbols, and the case table of the sampling tests.

The statement is written from include/whenet_hip.h (JPEG ENCODER, SAMPLING AND OPTIMISED TABLES) and shares no code with
csrc/jpeg_host.h; the standard's data, the DCT, the quantiser and the block coder are those of tests/jpeg_cases.py.

    planes_of_packed(frame, bgr, sampling) -> (Y, Cb, Cr)
    optimal_table(freq) -> (bits [16], vals)                      # T.81 K.2, figures K.1 - K.4, libjpeg's ties
    encode(planes, h, w, quality, sampling, optimize) -> Encoded(data, coef, interval_bits, stuffed, hist, tables)
    parse(data) -> Parsed(h, w, hs, vs, ri, tables, coef, hist, header_bytes, qtables)
    CASES: name -> Case;  GEOMETRY: name -> Case
"""
from collections import namedtuple

import numpy as np

from tests import jpeg_cases as JC

SAMPLINGS = {"4:2:0": (2, 2), "4:2:2": (2, 1), "4:4:4": (1, 1)}      # luma sampling factors hs, vs
PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
TC_TH = (0x00, 0x10, 0x01, 0x11)                                     # DC0, AC0, DC1, AC1 as the DHT byte


# ---- the planes ----------------------------------------------------------------------------------------------------------------
def planes_of_packed(frame, bgr=True, sampling="4:2:0"):
    """uint8 [h,w,3] -> (Y [h,w], Cb, Cr [ceil(h/vs), ceil(w/hs)]): chroma from R, G, B sums WORTH FOUR PIXELS, the edge replicated"""
    hs, vs = SAMPLINGS[sampling]
    f = frame.astype(np.int64)
    r, g, b = (f[..., 2], f[..., 1], f[..., 0]) if bgr else (f[..., 0], f[..., 1], f[..., 2])
    k = JC.JFIF_ROW
    y = np.clip((k[0] * r + k[1] * g + k[2] * b + (1 << 19)) >> 20, 0, 255)
    h, w = y.shape
    ys, xs = np.minimum(np.arange(vs * -(-h // vs)), h - 1), np.minimum(np.arange(hs * -(-w // hs)), w - 1)

    def sums(p):
        p = p[ys][:, xs]
        return (4 // (hs * vs)) * sum(p[dy::vs, dx::hs] for dy in range(vs) for dx in range(hs))

    rs, gs, bs = sums(r), sums(g), sums(b)
    cb = np.clip(((k[3] * rs + k[4] * gs + k[5] * bs + (1 << 21)) >> 22) + 128, 0, 255)
    cr = np.clip(((k[6] * rs + k[7] * gs + k[8] * bs + (1 << 21)) >> 22) + 128, 0, 255)
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


# ---- the tables ----------------------------------------------------------------------------------------------------------------
def code_sizes(freq):
    """frequencies [256] -> the code size of the 257 symbols before the lengths are limited: figure K.1 with a reserved 257th symbol
    of frequency 1, the least frequency first and the LARGER symbol on a tie (libjpeg)"""
    f = [int(v) for v in freq] + [1]
    size, other = [0] * 257, [-1] * 257
    while True:
        live = [i for i in range(257) if f[i]]
        if len(live) < 2:
            break
        c1 = min(live, key=lambda i: (f[i], -i))
        c2 = min((i for i in live if i != c1), key=lambda i: (f[i], -i))
        f[c1] += f[c2]
        f[c2] = 0
        size[c1] += 1
        while other[c1] >= 0:
            c1 = other[c1]
            size[c1] += 1
        other[c1] = c2
        size[c2] += 1
        while other[c2] >= 0:
            c2 = other[c2]
            size[c2] += 1
    return size


def optimal_table(freq):
    """frequencies [256] -> (bits [16], vals): figure K.3 limits the lengths of code_sizes() to 16; figure K.4 sorts the symbols by
    code size (the one before the limiting, as libjpeg does), then by value"""
    size = code_sizes(freq)
    bits = [0] * (max(max(size), 16) + 1)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                     # the reserved code point leaves the longest length
    vals = sorted((s for s in range(256) if size[s]), key=lambda s: (size[s], s))
    return bits[1:17], vals


def code_lengths(bits, vals):
    return {sym: length for sym, (_, length) in JC.huffman_codes(bits, vals).items()}


def coded_bits(freq, bits, vals):
    """the bits the symbols of a histogram cost with a table (the extra bits are the same with every table)"""
    lengths = code_lengths(bits, vals)
    return sum(int(n) * lengths[s] for s, n in enumerate(freq) if n)


def header(h, w, quality, sampling="4:2:0", tables=JC.HUFF):
    hs, vs = SAMPLINGS[sampling]
    q = [JC.scaled_q(JC.Q_LUMA, quality), JC.scaled_q(JC.Q_CHROMA, quality)]
    out = b"\xff\xd8" + JC.segment(0xE0, b"JFIF\0" + bytes([1, 1, 0]) + JC.be16(1) + JC.be16(1) + bytes([0, 0]))
    for t in range(2):
        out += JC.segment(0xDB, bytes([t]) + bytes(q[t][JC.ZIGZAG[k]] for k in range(64)))
    out += JC.segment(0xC0, bytes([8]) + JC.be16(h) + JC.be16(w) + bytes([3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (bits, vals), tc_th in zip(tables, TC_TH):
        out += JC.segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += JC.segment(0xDD, JC.be16(-(-w // (8 * hs))))
    out += JC.segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def bound(h, w, sampling="4:2:0"):
    hs, vs = SAMPLINGS[sampling]
    blocks = (hs * vs + 2) * -(-w // (8 * hs))
    return 629 + -(-h // (8 * vs)) * (2 * ((1660 * blocks + 7) // 8) + 2)


def restart_overhead(h, rows):
    """bytes the restart intervals cost at most next to a stream without them: the DRI segment (6), and per marker its two bytes
    and up to one byte of padding in front of it.  There is a marker behind every interval but the last, and an interval is `rows`
    pixel rows: 16 at 4:2:0 (tests/test_jpeg_cpu.py's restart_overhead is this with rows = 16), 8 at 4:2:2 (H2V1) and 4:4:4,
    whose MCUs are 8 rows high.  Nothing else enters: the allowance follows from the interval count alone."""
    return 6 + 3 * (-(-h // rows) - 1)


# ---- the encoder ---------------------------------------------------------------------------------------------------------------
Encoded = namedtuple("Encoded", "data coef interval_bits stuffed hist tables")


def block_component(i, sampling):
    hs, vs = SAMPLINGS[sampling]
    c = i % (hs * vs + 2)
    return 0 if c < hs * vs else c - hs * vs + 1


def coefficients(planes, h, w, quality, sampling):
    """int64 [R, B, 64]: the quantised coefficients of every interval's blocks in coding order (zigzag, DC absolute)"""
    hs, vs = SAMPLINGS[sampling]
    y, cb, cr = planes
    assert y.shape == (h, w) and cb.shape == cr.shape == (-(-h // vs), -(-w // hs))
    R, M = -(-h // (8 * vs)), -(-w // (8 * hs))
    ql, qc = JC.scaled_q(JC.Q_LUMA, quality), JC.scaled_q(JC.Q_CHROMA, quality)
    ky = JC.quantised(JC.blocks_of(y, vs * R, hs * M), ql)
    coef = np.zeros((R, M, hs * vs + 2, 64), np.int64)
    for i in range(hs * vs):
        coef[:, :, i] = ky[i // hs::vs, i % hs::hs]
    coef[:, :, hs * vs] = JC.quantised(JC.blocks_of(cb, R, M), qc)
    coef[:, :, hs * vs + 1] = JC.quantised(JC.blocks_of(cr, R, M), qc)
    return coef.reshape(R, -1, 64)


def block_symbol_list(zz, pred):
    """[(class 0 DC / 1 AC, symbol)] of a block: the DC category, the (run, size) symbols, ZRL and EOB"""
    out = [(0, int(abs(int(zz[0]) - pred)).bit_length())]
    run = 0
    for k in range(1, 64):
        c = int(zz[k])
        if c == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0))
            run -= 16
        out.append((1, (run << 4) | int(abs(c)).bit_length()))
        run = 0
    if run:
        out.append((1, 0x00))
    return out


def histograms(coef, sampling):
    """uint32-valued [4][256]: DC0, AC0, DC1, AC1"""
    hist = np.zeros((4, 256), np.int64)
    for interval in coef:
        pred = [0, 0, 0]
        for i, zz in enumerate(interval):
            comp = block_component(i, sampling)
            for cls, sym in block_symbol_list(zz, pred[comp]):
                hist[(0 if comp == 0 else 2) + cls, sym] += 1
            pred[comp] = int(zz[0])
    return hist


def encode(planes, h, w, quality, sampling="4:2:0", optimize=False, coef=None):
    coef = coefficients(planes, h, w, quality, sampling) if coef is None else coef
    hist = histograms(coef, sampling)
    tables = [optimal_table(hist[t]) for t in range(4)] if optimize else list(JC.HUFF)
    codes = [JC.huffman_codes(*t) for t in tables]
    data, interval_bits, stuffed = bytearray(header(h, w, quality, sampling, tables)), [], 0
    R = coef.shape[0]
    for r in range(R):
        acc, nbits, pred = 0, 0, [0, 0, 0]
        for i, zz in enumerate(coef[r]):
            comp = block_component(i, sampling)
            for code, length in JC.block_symbols(zz, pred[comp], codes[0 if comp == 0 else 2], codes[1 if comp == 0 else 3]):
                acc, nbits = (acc << length) | code, nbits + length
            pred[comp] = int(zz[0])
        interval_bits.append(nbits)
        pad = -nbits % 8
        raw = ((acc << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big")
        stuffed += raw.count(b"\xff")
        data += raw.replace(b"\xff", b"\xff\x00") + bytes([0xFF, 0xD0 + (r & 7) if r + 1 < R else 0xD9])
    return Encoded(bytes(data), coef, interval_bits, stuffed, hist, tables)


# ---- the parser ----------------------------------------------------------------------------------------------------------------
Parsed = namedtuple("Parsed", "h w hs vs ri tables coef hist header_bytes qtables")


def parse(data):
    """Any baseline stream of three components with 1x1 chroma, one scan, tables 0 for Y and 1 for Cb / Cr, and restart intervals of
    whole MCU rows (this encoder's, Pillow's with restart_marker_rows=1): the size, the sampling, DRI, the DHT tables as
    {tc_th: (bits, vals)}, the coefficients int64 [R, B, 64] (zigzag, DC absolute), the histograms [4][256] of the symbols met,
    the header's length, the quantisers (zigzag)."""
    assert data[:2] == b"\xff\xd8"
    pos, qtables, tables, ri = 2, {}, {}, 0
    while True:
        assert data[pos] == 0xFF, f"no marker at {pos}"
        marker, n = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        s = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if marker == 0xDB:
            for i in range(0, len(s), 65):
                assert s[i] >> 4 == 0
                qtables[s[i] & 15] = list(s[i + 1:i + 65])
        elif marker == 0xC0:
            assert s[0] == 8 and s[5] == 3 and s[10] == s[13] == 0x11
            h, w, hs, vs = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[7] >> 4, s[7] & 15
        elif marker == 0xC4:
            i = 0
            while i < len(s):
                bits = list(s[i + 1:i + 17])
                tables[s[i]] = (bits, list(s[i + 17:i + 17 + sum(bits)]))
                i += 17 + sum(bits)
        elif marker == 0xDD:
            ri = (s[0] << 8) | s[1]
        elif marker == 0xDA:
            assert list(s) == [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]
            break
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, f"marker {marker:#x} in the header"
    header_bytes = pos
    R, M, bpm = -(-h // (8 * vs)), -(-w // (8 * hs)), hs * vs + 2
    assert ri == M, "one restart interval per MCU row"
    intervals, cur = [], bytearray()
    while True:
        b = data[pos]
        pos += 1
        if b != 0xFF:
            cur.append(b)
            continue
        m = data[pos]
        pos += 1
        if m == 0x00:
            cur.append(0xFF)
        else:
            assert m == (0xD0 + (len(intervals) & 7) if len(intervals) + 1 < R else 0xD9), f"marker {m:#x} behind interval {len(intervals)}"
            intervals.append(bytes(cur))
            cur = bytearray()
            if m == 0xD9:
                break
    assert pos == len(data) and len(intervals) == R
    decode = {t: {(length, code): sym for sym, (code, length) in JC.huffman_codes(*bv).items()} for t, bv in tables.items()}
    coef, hist = np.zeros((R, M * bpm, 64), np.int64), np.zeros((4, 256), np.int64)
    for r, raw in enumerate(intervals):
        bitstr, at, pred = "".join(f"{b:08b}" for b in raw), 0, [0, 0, 0]

        def symbol(t):
            nonlocal at
            for length in range(1, 17):
                sym = decode[TC_TH[t]].get((length, int(bitstr[at:at + length], 2)))
                if sym is not None:
                    at += length
                    hist[t, sym] += 1
                    return sym
            raise AssertionError("no Huffman code matches")

        def extra(s):
            nonlocal at
            if s == 0:
                return 0
            v = int(bitstr[at:at + s], 2)
            at += s
            return v if v >> (s - 1) else v - (1 << s) + 1

        for i in range(M * bpm):
            comp = 0 if i % bpm < hs * vs else i % bpm - hs * vs + 1
            t = 0 if comp == 0 else 2
            pred[comp] += extra(symbol(t))
            coef[r, i, 0] = pred[comp]
            k = 1
            while k < 64:
                sym = symbol(t + 1)
                if sym == 0x00:
                    break
                if sym == 0xF0:
                    k += 16
                    continue
                k += sym >> 4
                coef[r, i, k] = extra(sym & 15)
                k += 1
            assert k <= 64
        assert len(bitstr) - at < 8 and set(bitstr[at:]) <= {"1"}, "an interval ends with up to 7 one-bits"
    return Parsed(h, w, hs, vs, ri, tables, coef, hist, header_bytes, qtables)


def natural_dequantised(coef, qtables, sampling):
    """[R, B, 64] zigzag quantised -> int64 [R * B, 64] natural order, dequantised and clamped as the decoder does"""
    out = np.zeros((coef.shape[0] * coef.shape[1], 64), np.int64)
    flat = coef.reshape(-1, 64)
    for i in range(flat.shape[0]):
        q = qtables[0 if block_component(i % coef.shape[1], sampling) == 0 else 1]
        out[i, JC.ZIGZAG] = np.clip(flat[i] * np.array(q, np.int64), -2048, 2047)
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------------
def flat(h, w):
    return np.full((h, w, 3), (40, 200, 90), np.uint8)


def lines(h, w):
    """a grey frame with one-pixel lines in pure red, green and blue (B, G, R order), horizontal, vertical and diagonal: the pose
    axes and text strokes of the overlay.  All of their information is chroma."""
    f = np.full((h, w, 3), 96, np.uint8)
    colours = ((0, 0, 255), (0, 255, 0), (255, 0, 0))
    for i, c in enumerate(colours):
        f[(3 + 5 * i) % h::16, :] = c
        f[:, (2 + 5 * i) % w::16] = c
    for d in range(min(h, w)):
        f[d, (d + 7) % w] = colours[d // 8 % 3]
    return f


CONTENT = {"flat": flat, "gradient": JC.gradient, "noise": lambda h, w: JC.noise(h, w, 31 + h + w), "lines": lines}
SIZES = ((1, 1), (8, 8), (9, 7), (17, 17), (33, 18), (35, 50), (64, 48))      # (h, w)
QUALITIES = (30, 95, 100)


class Case:
    def __init__(self, name, pixels, quality, sampling, bgr=True):
        self.name, self.pixels, self.quality, self.sampling, self.bgr = name, pixels, quality, sampling, bgr

    def planes(self):
        return planes_of_packed(self.pixels, self.bgr, self.sampling)


def _table():
    """every size x sampling x quality x channel order (optimize off and on is the tests' own loop: the two share the DCT); the
    content rotates so that every size meets every content, and every content meets every sampling and quality"""
    out, names = [], list(CONTENT)
    for si, (h, w) in enumerate(SIZES):
        for qi, q in enumerate(QUALITIES):
            for oi, bgr in enumerate((True, False)):
                content = names[(si + qi + 2 * oi) % 4]
                for sampling in SAMPLINGS:
                    out.append(Case(f"{h}x{w}_{content}_q{q}_{'bgr' if bgr else 'rgb'}_{sampling}", CONTENT[content](h, w), q, sampling, bgr))
    return out


CASES = {c.name: c for c in _table()}
# 8 x 704 at 4:4:4: 264 blocks in the interval, 8 x 1040 at 4:2:2: 260 -- both more than the pack kernel's 256-lane step (its
# carry); 8 and 9 rows: one and two intervals at the new samplings
GEOMETRY = {c.name: c for c in (
    Case("8x704_444", JC.smooth(8, 704, 41), 95, "4:4:4"), Case("8x1040_422", JC.smooth(8, 1040, 42), 95, "4:2:2"),
    Case("8x24_444", lines(8, 24), 95, "4:4:4"), Case("9x24_444", lines(9, 24), 95, "4:4:4"),
    Case("8x24_422", lines(8, 24), 95, "4:2:2"), Case("9x24_422", lines(9, 24), 95, "4:2:2"))}
ALL = {**CASES, **GEOMETRY}


def by_sampling(cases=None):
    out = {s: [] for s in SAMPLINGS}
    for c in (ALL if cases is None else cases).values():
        out[c.sampling].append(c)
    return out


_STATEMENTS = {}


def statement(case, optimize):
    """the statement's Encoded of a case, computed once (the coefficients are shared by optimize off and on)"""
    key = (case.name, bool(optimize))
    if key not in _STATEMENTS:
        planes = case.planes()
        h, w = planes[0].shape
        other = _STATEMENTS.get((case.name, not optimize))
        _STATEMENTS[key] = encode(planes, h, w, case.quality, case.sampling, optimize, None if other is None else other.coef)
    return _STATEMENTS[key]


# ---- frequencies for whenet_jpeg_optimal_table directly ------------------------------------------------------------------------
def _fibonacci():
    f, a, b = np.zeros(256, np.int64), 1, 1
    for i in range(40):                                              # 40 symbols: the unlimited code is 40 bits deep
        f[3 * i + 1] = a
        a, b = b, a + b
    return f


def _large():
    """the sums an 8192 x 8192 frame can reach at 4:4:4: 2^21 chroma blocks of 63 coefficients each, most of them one symbol"""
    f = np.zeros(256, np.int64)
    f[0x01] = (1 << 21) * 63 - 1000
    f[0x00], f[0x11], f[0xF0] = 1 << 21, 700, 300
    return f


FREQUENCIES = {
    "single": np.eye(1, 256, 5, dtype=np.int64)[0] * 9,
    "two": np.eye(1, 256, 0, dtype=np.int64)[0] * 3 + np.eye(1, 256, 0xF0, dtype=np.int64)[0] * 3,
    "all_equal": np.full(256, 7, np.int64),
    "fibonacci": _fibonacci(),
    "large": _large(),
}
