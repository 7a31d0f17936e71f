"""The JPEG encoder's format as a numpy / Python statement, a minimal parser of its streams, and the case table of the JPEG tests.

The statement is written from include/whenet_hip.h (JPEG ENCODER) and shares no code with csrc/jpeg_host.h: the DCT matrix is
computed from its formula, the zigzag order is walked, the Huffman codes are derived from the standard's (bits, values) lists, and
the stream is assembled from Python integers.  The Annex K tables are the JPEG standard's (ITU-T T.81), written out as data.

    encode(planes, h, w, quality) -> Encoded(data, coef, interval_bits, stuffed)
    parse(data) -> Parsed(segments, h, w, layer, qtables, restart_interval, coef, rst)      # Huffman-decoded back to coefficients
    CASES / GPU_CASES: name -> Case;  case.source() -> ((Y, Cb, Cr) tight planes, the frame object whenet_hip.jpeg takes)
"""
import hashlib
import json
import os
from collections import namedtuple

import numpy as np

from whenet_hip.yuv import YUVFrame

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DIGESTS = os.path.join(ROOT, "tests", "golden", "jpeg_digests.json")
HEADER_BYTES = 629

# ---- the standard's data (T.81 Annex K) ----------------------------------------------------------------------------------------
Q_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
          103, 99]
Q_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + \
    [99] * 32
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
    0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
    0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
    0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
    0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
    0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA])
HUFF = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)      # the order of the stream's DHT segments
# the JFIF row of the header's BGR -> 4:2:0 rule: {RY, GY, BY, RU, GU, BU, RV, GV, BV} = rint(2^20 x) of its expressions
_KR, _KB = 0.299, 0.114
_KG = 1 - _KR - _KB
JFIF_ROW = [int(np.rint((1 << 20) * v)) for v in (_KR, _KG, _KB, -_KR / (2 * (1 - _KB)), -_KG / (2 * (1 - _KB)), 0.5,
                                                   0.5, -_KG / (2 * (1 - _KR)), -_KB / (2 * (1 - _KR)))]


def zigzag():
    """zigzag position -> natural index, walked along the anti-diagonals (T.81 figure A.6)"""
    order = []
    for s in range(15):
        cells = [(y, s - y) for y in range(8) if 0 <= s - y < 8]      # top right to bottom left
        order += [y * 8 + x for y, x in (cells if s % 2 else cells[::-1])]
    return order


ZIGZAG = zigzag()
DCT = np.array([[int(np.rint(4096 * (np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16))) for x in range(8)]
                for u in range(8)], np.int64)


def scaled_q(base, quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * scale + 50) // 100, 1), 255) for b in base]


def huffman_codes(bits, vals):
    """symbol -> (code, length): the canonical codes, counting up within a length and doubling between lengths"""
    table, code, n = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[n]] = (code, length)
            code, n = code + 1, n + 1
        code <<= 1
    return table


def be16(v):
    return bytes([v >> 8, v & 255])


def segment(marker, payload):
    return bytes([0xFF, marker]) + be16(len(payload) + 2) + payload


def header(h, w, quality):
    q = [scaled_q(Q_LUMA, quality), scaled_q(Q_CHROMA, quality)]
    out = b"\xff\xd8" + segment(0xE0, b"JFIF\0" + bytes([1, 1, 0]) + be16(1) + be16(1) + bytes([0, 0]))
    for t in range(2):
        out += segment(0xDB, bytes([t]) + bytes(q[t][ZIGZAG[k]] for k in range(64)))
    out += segment(0xC0, bytes([8]) + be16(h) + be16(w) + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (bits, vals), tc_th in zip(HUFF, (0x00, 0x10, 0x01, 0x11)):
        out += segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += segment(0xDD, be16((w + 15) // 16))
    out += segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


# ---- the planes ----------------------------------------------------------------------------------------------------------------
def planes_of_packed(frame, bgr=True):
    """uint8 [h,w,3] -> (Y, Cb, Cr) by the header's BGR -> 4:2:0 rule with the JFIF row"""
    f = frame.astype(np.int64)
    r, g, b = (f[..., 2], f[..., 1], f[..., 0]) if bgr else (f[..., 0], f[..., 1], f[..., 2])
    k = JFIF_ROW
    y = np.clip((k[0] * r + k[1] * g + k[2] * b + (1 << 19)) >> 20, 0, 255)
    h, w = y.shape
    ys, xs = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1), np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)

    def sums(p):
        p = p[ys][:, xs]
        return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]

    rs, gs, bs = sums(r), sums(g), sums(b)
    cb = np.clip(((k[3] * rs + k[4] * gs + k[5] * bs + (1 << 21)) >> 22) + 128, 0, 255)
    cr = np.clip(((k[6] * rs + k[7] * gs + k[8] * bs + (1 << 21)) >> 22) + 128, 0, 255)
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def blocks_of(plane, rows, cols):
    """plane -> int64 [rows, cols, 8, 8]: its 8 x 8 blocks, the last column and row replicated beyond the edge"""
    p = np.pad(plane.astype(np.int64), ((0, rows * 8 - plane.shape[0]), (0, cols * 8 - plane.shape[1])), mode="edge")
    return p.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)


def quantised(blocks, q):
    """int64 [..., 8, 8] samples -> int64 [..., 64] quantised coefficients in ZIGZAG order"""
    p = blocks - 128
    a = np.einsum("ux,...yx->...yu", DCT, p)
    r = (a + 256) >> 9
    b = np.einsum("vy,...yu->...vu", DCT, r)
    assert np.abs(b).max(initial=0) < 1 << 25
    qq = np.array(q, np.int64).reshape(8, 8)
    k = np.sign(b) * ((np.abs(b) + (qq << 14)) // (qq << 15))
    dc = k[..., 0, 0].copy()
    k = np.clip(k, -1023, 1023)
    k[..., 0, 0] = dc
    return k.reshape(k.shape[:-2] + (64,))[..., ZIGZAG]


Encoded = namedtuple("Encoded", "data coef interval_bits stuffed")


def block_symbols(zz, pred, dc, ac):
    """the (code, length) pairs of a block"""
    out = []

    def value(sym_table, sym, v):
        s = int(abs(v)).bit_length()
        code, length = sym_table[sym]
        out.append(((code << s) | ((v if v >= 0 else v - 1) & ((1 << s) - 1)), length + s))

    d = int(zz[0]) - pred
    value(dc, int(abs(d)).bit_length(), d)
    run = 0
    for k in range(1, 64):
        c = int(zz[k])
        if c == 0:
            run += 1
            continue
        while run > 15:
            out.append(ac[0xF0])
            run -= 16
        value(ac, (run << 4) | int(abs(c)).bit_length(), c)
        run = 0
    if run:
        out.append(ac[0x00])
    return out


def encode(planes, h, w, quality):
    """(Y [h,w], Cb, Cr [ceil(h/2), ceil(w/2)]) -> Encoded: the stream; coef int64 [R, B, 64] in coding order (zigzag, DC absolute);
    the bit length of every interval before padding; the number of stuffed zero bytes"""
    y, cb, cr = planes
    assert y.shape == (h, w) and cb.shape == cr.shape == ((h + 1) // 2, (w + 1) // 2)
    R, M = (h + 15) // 16, (w + 15) // 16
    ql, qc = scaled_q(Q_LUMA, quality), scaled_q(Q_CHROMA, quality)
    ky = quantised(blocks_of(y, 2 * R, 2 * M), ql)
    kcb, kcr = quantised(blocks_of(cb, R, M), qc), quantised(blocks_of(cr, R, M), qc)
    coef = np.zeros((R, M, 6, 64), np.int64)
    for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        coef[:, :, i] = ky[dy::2, dx::2]
    coef[:, :, 4], coef[:, :, 5] = kcb, kcr
    codes = [huffman_codes(*t) for t in HUFF]
    data, interval_bits, stuffed = bytearray(header(h, w, quality)), [], 0
    for r in range(R):
        acc, nbits, pred = 0, 0, [0, 0, 0]
        for m in range(M):
            for i in range(6):
                comp = 0 if i < 4 else i - 3
                for code, length in block_symbols(coef[r, m, i], pred[comp], codes[0 if comp == 0 else 2], codes[1 if comp == 0 else 3]):
                    acc, nbits = (acc << length) | code, nbits + length
                pred[comp] = int(coef[r, m, i, 0])
        interval_bits.append(nbits)
        pad = -nbits % 8
        raw = ((acc << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big")
        stuffed += raw.count(b"\xff")
        data += raw.replace(b"\xff", b"\xff\x00") + bytes([0xFF, 0xD0 + (r & 7) if r + 1 < R else 0xD9])
    return Encoded(bytes(data), coef.reshape(R, M * 6, 64), interval_bits, stuffed)


# ---- the parser ----------------------------------------------------------------------------------------------------------------
Parsed = namedtuple("Parsed", "segments h w layer qtables restart_interval coef rst")


def parse(data):
    """A stream of this encoder's layout -> its marker segments [(marker, payload)], the frame size, the components' (id, H, V, Tq),
    the quantisers (zigzag order), the restart interval, the Huffman-decoded coefficients int64 [R, B, 64] (zigzag, DC absolute) and
    the RSTm numbers met.  Decodes with the tables the STREAM carries."""
    assert data[:2] == b"\xff\xd8"
    pos, segments, qtables, huff = 2, [], {}, {}
    h = w = ri = None
    layer = []
    while True:
        assert data[pos] == 0xFF, f"no marker at {pos}"
        marker, n = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        payload = data[pos + 4:pos + 2 + n]
        segments.append((marker, payload))
        pos += 2 + n
        if marker == 0xDB:
            assert payload[0] >> 4 == 0 and len(payload) == 65
            qtables[payload[0] & 15] = list(payload[1:])
        elif marker == 0xC0:
            assert payload[0] == 8 and payload[5] == 3
            h, w = (payload[1] << 8) | payload[2], (payload[3] << 8) | payload[4]
            layer = [(payload[6 + 3 * i], payload[7 + 3 * i] >> 4, payload[7 + 3 * i] & 15, payload[8 + 3 * i]) for i in range(3)]
        elif marker == 0xC4:
            bits, vals = list(payload[1:17]), list(payload[17:])
            assert sum(bits) == len(vals)
            huff[payload[0]] = {(length, code): sym for sym, (code, length) in huffman_codes(bits, vals).items()}
        elif marker == 0xDD:
            ri = (payload[0] << 8) | payload[1]
        elif marker == 0xDA:
            assert list(payload) == [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]
            break
    R, M = (h + 15) // 16, (w + 15) // 16
    assert ri == M
    # the intervals: 0xFF 0x00 is a stuffed byte, 0xFF 0xD0..0xD7 a restart marker, 0xFF 0xD9 the end
    intervals, rst, cur = [], [], bytearray()
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
        elif 0xD0 <= m <= 0xD7 or m == 0xD9:
            intervals.append(bytes(cur))
            cur = bytearray()
            if m == 0xD9:
                break
            rst.append(m - 0xD0)
        else:
            raise AssertionError(f"marker {m:#x} inside the entropy-coded data")
    assert pos == len(data) and len(intervals) == R
    coef = np.zeros((R, M * 6, 64), np.int64)
    for r, raw in enumerate(intervals):
        bitstr, at, pred = "".join(f"{b:08b}" for b in raw), 0, [0, 0, 0]

        def symbol(table):
            nonlocal at
            for length in range(1, 17):
                sym = table.get((length, int(bitstr[at:at + length], 2)))
                if sym is not None:
                    at += length
                    return sym
            raise AssertionError("no Huffman code matches")

        def extra(s):
            nonlocal at
            if s == 0:
                return 0
            v = int(bitstr[at:at + s], 2)
            at += s
            return v if v >> (s - 1) else v - (1 << s) + 1

        for i in range(M * 6):
            comp = 0 if i % 6 < 4 else i % 6 - 3
            dc, ac = huff[0x00 if comp == 0 else 0x01], huff[0x10 if comp == 0 else 0x11]
            pred[comp] += extra(symbol(dc))
            coef[r, i, 0] = pred[comp]
            k = 1
            while k < 64:
                sym = symbol(ac)
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
    return Parsed(segments, h, w, layer, qtables, ri, coef, rst)


def reconstruct_luma(coef, qtable_zigzag, h, w):
    """float64 [h,w]: the inverse DCT (in float64, orthonormal basis) of the dequantised luma coefficients, + 128, unclipped"""
    R, B, _ = coef.shape
    M = B // 6
    nat = np.zeros((R, M, 4, 64))
    nat[..., ZIGZAG] = coef.reshape(R, M, 6, 64)[:, :, :4] * np.array(qtable_zigzag, np.float64)
    c = np.array([[(np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])
    pix = np.einsum("vy,...vu,ux->...yx", c, nat.reshape(R, M, 4, 8, 8), c) + 128
    # [R, M, dy, dx, y, x] -> [R, dy, y, M, dx, x]
    return pix.reshape(R, M, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(R * 16, M * 16)[:h, :w]


# ---- the case table ------------------------------------------------------------------------------------------------------------
def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


def gradient(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(2 * xx + yy) % 256, (xx + 3 * yy) // 2 % 256, (255 - xx - yy) % 256], -1).astype(np.uint8)


def smooth(h, w, seed):
    """low-pass noise: a picture whose blocks have a handful of coefficients, like a camera frame"""
    rs = np.random.RandomState(seed)
    small = rs.randint(0, 256, ((h + 7) // 8 + 1, (w + 7) // 8 + 1, 3)).astype(np.float64)
    big = np.kron(small, np.ones((8, 8, 1)))[:h, :w]
    return np.clip(big + rs.randint(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


def pitched(a, extra, fill=0xEE):
    """a copy of the 2-D uint8 array whose rows are `extra` bytes further apart"""
    buf = np.full((a.shape[0], a.shape[1] + extra), fill, np.uint8)
    buf[:, :a.shape[1]] = a
    return buf[:, :a.shape[1]]


class Case:
    """kind 'bgr' / 'rgb': `pixels` uint8 [h,w,3] is the frame; 'i420' / 'nv12': `pixels` gives the planes (by the packed rule, or
    directly as (Y, Cb, Cr)) and the frame is a YUVFrame over pitched copies of them."""

    def __init__(self, name, pixels, quality=95, kind="bgr", extra=0):
        self.name, self.quality, self.kind, self.extra = name, quality, kind, extra
        self._pixels = pixels

    def source(self):
        px = self._pixels() if callable(self._pixels) else self._pixels
        if isinstance(px, tuple):
            planes = tuple(np.ascontiguousarray(p, np.uint8) for p in px)
            assert self.kind in ("i420", "nv12")
        else:
            planes = planes_of_packed(px, bgr=self.kind != "rgb")
        h, w = planes[0].shape
        if self.kind in ("bgr", "rgb"):
            frame = pitched(px.reshape(h, 3 * w), self.extra).reshape(h, w, 3) if self.extra else px
        elif self.kind == "i420":
            frame = YUVFrame.i420(pitched(planes[0], self.extra), pitched(planes[1], self.extra + 3), pitched(planes[2], self.extra + 1), "jfif")
        else:
            uv = np.stack([planes[1], planes[2]], -1).reshape(planes[1].shape[0], -1)
            frame = YUVFrame.nv12(pitched(planes[0], self.extra), pitched(uv, self.extra + 2), "jfif")
        return planes, frame

    @property
    def bgr(self):
        return self.kind != "rgb"


def _flat():
    return np.full((32, 48), 128, np.uint8), np.full((16, 24), 128, np.uint8), np.full((16, 24), 128, np.uint8)


def _black_white():
    y = np.zeros((16, 32), np.uint8)
    y[:, 16:] = 255
    return y, np.full((8, 16), 128, np.uint8), np.full((8, 16), 128, np.uint8)


def _checkerboard(lo=0, hi=255):
    yy, xx = np.mgrid[0:16, 0:32]
    return np.where((yy + xx) & 1, hi, lo).astype(np.uint8), np.full((8, 16), 128, np.uint8), np.full((8, 16), 128, np.uint8)


STUFFED_SEED = 7          # 48 x 40 noise at quality 100: the statement reports stuffed 0xFF bytes (asserted)
UNPADDED_SEED = 3         # found by test-side search (find_unpadded_seed): an interval of 8 k bits, no padding (asserted)
QUALITIES = (1, 25, 49, 50, 51, 75, 95, 100)

_CASES = [
    Case("1x1", noise(1, 1, 11)), Case("8x8", noise(8, 8, 12)), Case("16x16", noise(16, 16, 13)), Case("17x17", noise(17, 17, 14)),
    Case("15x33", smooth(15, 33, 15)), Case("48x40", smooth(48, 40, 16)),
    Case("tall_160x16", smooth(160, 16, 17)),               # 16 wide, 160 tall: 10 intervals, RSTm wraps past 7
    Case("wide_16x272", smooth(16, 272, 18)),               # 272 wide: one interval of 17 MCUs
    Case("130x250_noise", noise(130, 250, 19)), Case("130x250_gradient", gradient(130, 250)),
    Case("flat", _flat, kind="i420"),                       # every block an EOB, every DC difference 0
    Case("black_white_q100", _black_white, 100, "i420"),    # a DC difference of category 11
    Case("checkerboard_q50", lambda: _checkerboard(112, 144), 50, "i420"),      # 128 +- 16: coefficient 63 alone behind 62 zeros, ZRL
    Case("checkerboard_q100", _checkerboard, 100, "nv12"),  # coefficient 63 non-zero: no EOB
    Case("noise_q100_stuffed", noise(40, 48, STUFFED_SEED), 100),
    Case("unpadded", smooth(48, 40, UNPADDED_SEED), 95),
    Case("i420_pitched", smooth(33, 47, 20), 75, "i420", extra=5), Case("nv12_pitched", smooth(33, 47, 21), 75, "nv12", extra=7),
    Case("bgr_pitched", smooth(33, 47, 22), 75, "bgr", extra=6), Case("rgb_pitched", smooth(33, 47, 23), 75, "rgb", extra=9),
] + [Case(f"q{q}", smooth(40, 48, 24), q) for q in QUALITIES]
CASES = {c.name: c for c in _CASES}
# the GPU suite's own: an interval whose scan spans several waves' blocks (65 MCUs = 390 blocks), 129 intervals, and the widest
# frame there is (512 MCUs = 3,072 blocks in one interval: twelve scan steps with a carry)
_GPU_EXTRA = [Case("wide_16x1040", smooth(16, 1040, 25)), Case("tall_2064x16", smooth(2064, 16, 26)), Case("wide_16x8192", smooth(16, 8192, 27))]
GPU_CASES = {**CASES, **{c.name: c for c in _GPU_EXTRA}}


def find_unpadded_seed(limit=64):
    """the first seed whose 'unpadded' picture has an interval of a multiple of 8 bits"""
    for seed in range(limit):
        px = smooth(48, 40, seed)
        if any(n % 8 == 0 for n in encode(planes_of_packed(px), 48, 40, 95).interval_bits):
            return seed
    return None


def statement(case):
    planes, _ = case.source()
    h, w = planes[0].shape
    return encode(planes, h, w, case.quality)


def digest(data):
    return hashlib.sha256(bytes(data)).hexdigest()


def load_digests():
    with open(DIGESTS) as f:
        return json.load(f)


if __name__ == "__main__":      # regenerate tests/golden/jpeg_digests.json from the statement
    table = {name: {"sha256": digest(statement(c).data), "bytes": len(statement(c).data)} for name, c in GPU_CASES.items()}
    with open(DIGESTS, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} digests, unpadded seed {find_unpadded_seed()}")
