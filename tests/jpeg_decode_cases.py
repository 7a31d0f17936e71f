"""The JPEG decoder's format as a numpy / Python statement, and the case table of the decoder tests.

The statement is written from include/whenet_hip.h (JPEG DECODER) and shares no code with csrc/jpeg_dec_host.h: the markers are
walked with Python integers, the Huffman codes are derived from each DHT's (counts, values) lists and matched bit by bit, the
inverse DCT matrix is computed from its formula, the conversion row from the JFIF constants.

    parse(data) -> Header                      # raises Refused(reason) for what the decoder does not accept
    decode(data) -> Decoded(header, coef, planes, status)      # coef: dequantised, clamped, natural order, [blocks][64]
    frame(decoded, bgr) -> uint8 [h,w,3];  i420(decoded) -> (Y, U, V)
    float_planes(decoded) -> the float64 inverse DCT of the same coefficients, unrounded, cropped like the planes
    CASES: name -> the stream's bytes (built on first use);  DAMAGED: name -> (bytes, the first bad interval)
"""
import functools
import io
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OK, EFORMAT = 0, -74


class Refused(ValueError):
    pass


def zigzag():
    """zigzag position -> natural index, walked along the anti-diagonals (T.81 figure A.6)"""
    order = []
    for s in range(15):
        cells = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        order += [y * 8 + x for y, x in (cells if s % 2 else cells[::-1])]
    return order


ZIGZAG = zigzag()
DCT = np.array([[int(np.rint(4096 * (np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16))) for x in range(8)]
                for u in range(8)], np.int64)
DCT_F = np.array([[(np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])
# yoff, CY, CVR, CUG, CVG, CUB of the JFIF row: rint(2^20 x {1, 1.402, 0.344136, 0.714136, 1.772})
JFIF = [0] + [int(np.rint((1 << 20) * v)) for v in (1, 1.402, 0.344136, 0.714136, 1.772)]

Header = namedtuple("Header", "h w comps hs vs qt dc ac ri intervals data_offset q huff mcu_cols mcu_rows bpm")
Decoded = namedtuple("Decoded", "header coef planes status")


# ---- parse -----------------------------------------------------------------------------------------------------------------------
def parse(data):
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    p, sof, q, huff, ri = 2, None, {}, {}, 0
    while True:
        if p + 2 > len(data):
            raise Refused("truncated header")
        if data[p] != 0xFF:
            raise Refused("no marker")
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        p += 2
        if m in (0xD8, 0xD9, 0x01) or 0xD0 <= m <= 0xD7:
            raise Refused(f"marker {m:#x} in the header")
        if p + 2 > len(data):
            raise Refused("truncated header")
        n = (data[p] << 8) | data[p + 1]
        if n < 2 or p + n > len(data):
            raise Refused("truncated segment")
        s = data[p + 2:p + n]
        if 0xC0 < m <= 0xCF and m != 0xC4:
            raise Refused(f"frame type / coding {m:#x}")
        if m == 0xC0:
            if sof is not None or len(s) < 6:
                raise Refused("SOF0")
            if s[0] != 8:
                raise Refused(f"{s[0]} bit")
            h, w, nc = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if nc not in (1, 3) or not (1 <= h <= 8192 and 1 <= w <= 8192) or len(s) != 6 + 3 * nc:
                raise Refused("components / size")
            comps = [(s[6 + 3 * c], s[7 + 3 * c], s[8 + 3 * c]) for c in range(nc)]
            if any(c[2] > 3 for c in comps):
                raise Refused("quantiser id")
            if nc == 3 and (comps[0][1] not in (0x22, 0x21, 0x11) or comps[1][1] != 0x11 or comps[2][1] != 0x11):
                raise Refused("sampling")
            sof = (h, w, comps)
        elif m == 0xDB:
            i = 0
            while i < len(s):
                if s[i] >> 4 or (s[i] & 15) > 3 or i + 65 > len(s) or 0 in s[i + 1:i + 65]:
                    raise Refused("DQT")
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = s[i + 1 + k]
                q[s[i] & 15] = t
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(s):
                tc, th = s[i] >> 4, s[i] & 15
                if tc > 1 or th > 1 or i + 17 > len(s):
                    raise Refused("DHT")
                counts = list(s[i + 1:i + 17])
                if i + 17 + sum(counts) > len(s):
                    raise Refused("DHT")
                vals = list(s[i + 17:i + 17 + sum(counts)])
                table, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[(length, code)] = vals[k]
                        code, k = code + 1, k + 1
                    if code > (1 << length):
                        raise Refused("DHT: no prefix code")
                    code <<= 1
                if tc == 0 and any(v > 11 for v in vals):
                    raise Refused("DHT: DC symbol")
                huff[(tc, th)] = table
                i += 17 + sum(counts)
        elif m == 0xDD:
            if len(s) != 2:
                raise Refused("DRI")
            ri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            if sof is None:
                raise Refused("SOS before SOF0")
            h, w, comps = sof
            nc = len(comps)
            if len(s) < 1 or s[0] != nc or len(s) != 4 + 2 * nc:
                raise Refused("several scans")
            dc, ac = [], []
            for c in range(nc):
                if s[1 + 2 * c] != comps[c][0] or (s[2 + 2 * c] >> 4) > 1 or (s[2 + 2 * c] & 15) > 1:
                    raise Refused("scan components")
                dc.append(s[2 + 2 * c] >> 4), ac.append(s[2 + 2 * c] & 15)
            if tuple(s[1 + 2 * nc:]) != (0, 63, 0):
                raise Refused("spectral selection")
            for c in range(nc):
                if comps[c][2] not in q or (0, dc[c]) not in huff or (1, ac[c]) not in huff:
                    raise Refused("missing table")
            hs, vs = (comps[0][1] >> 4, comps[0][1] & 15) if nc == 3 else (1, 1)
            mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
            mcus = mcu_cols * mcu_rows
            eff = ri if 0 < ri < mcus else mcus
            return Header(h, w, nc, hs, vs, [c[2] for c in comps], dc, ac, ri, -(-mcus // eff), p + n, q, huff, mcu_cols, mcu_rows,
                          hs * vs + 2 if nc == 3 else 1)
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise Refused(f"marker {m:#x} in the header")
        p += n


# ---- entropy decode --------------------------------------------------------------------------------------------------------------
class _Damage(Exception):
    pass


def _interval_bits(data, start):
    """the bits of an interval from `start` on: 0xFF 0x00 is one 0xFF byte, any other 0xFF pair or the end of the data ends them"""
    out, p = bytearray(), start
    while True:
        f = data.find(b"\xff", p)
        if f < 0:
            out += data[p:]
            break
        out += data[p:f]
        if f + 1 < len(data) and data[f + 1] == 0:
            out.append(0xFF)
            p = f + 2
        else:
            break
    return np.unpackbits(np.frombuffer(bytes(out), np.uint8)).tolist()


class _Bits:
    def __init__(self, bits):
        self.bits, self.at = bits, 0

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            if self.at >= len(self.bits):
                raise _Damage
            code = (code << 1) | self.bits[self.at]
            self.at += 1
            if (length, code) in table:
                return table[(length, code)]
        raise _Damage

    def value(self, s):
        if s == 0:
            return 0
        if self.at + s > len(self.bits):
            raise _Damage
        v = 0
        for b in self.bits[self.at:self.at + s]:
            v = (v << 1) | b
        self.at += s
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _decode_interval(hd, data, start, i, coef):
    br = _Bits(_interval_bits(data, start))
    mcus = hd.mcu_cols * hd.mcu_rows
    eff = hd.ri if 0 < hd.ri < mcus else mcus
    pred = [0, 0, 0]
    ny = hd.bpm - 2
    for m in range(i * eff, min((i + 1) * eff, mcus)):
        for b in range(hd.bpm):
            c = 0 if hd.comps == 1 or b < ny else b - ny + 1
            q, dct, act = hd.q[hd.qt[c]], hd.huff[(0, hd.dc[c])], hd.huff[(1, hd.ac[c])]
            out = coef[m * hd.bpm + b]
            pred[c] = clamp(pred[c] + br.value(br.symbol(dct)), -32768, 32767)
            out[0] = clamp(pred[c] * q[0], -2048, 2047)
            k = 1
            while k < 64:
                sym = br.symbol(act)
                r, s = sym >> 4, sym & 15
                if s == 0:
                    if r != 15:
                        break
                    k += 16
                    if k > 64:
                        raise _Damage
                    continue
                k += r
                if k > 63:
                    raise _Damage
                nat = ZIGZAG[k]
                out[nat] = clamp(br.value(s) * q[nat], -2048, 2047)
                k += 1


def restart_markers(data):
    """(position, number) of every 0xFF 0xD0..0xD7 pair of the entropy data, in order"""
    out, p = [], 0
    while True:
        f = data.find(b"\xff", p)
        if f < 0 or f + 1 >= len(data):
            return out
        if 0xD0 <= data[f + 1] <= 0xD7:
            out.append((f, data[f + 1] & 7))
        p = f + 1


def idct_int(coef):
    c = coef.reshape(-1, 8, 8).astype(np.int64)
    a = np.einsum("vy,nvu->nyu", DCT, c)
    r = (a + 128) >> 8
    b = np.einsum("ux,nyu->nyx", DCT, r)
    return np.clip(((b + 32768) >> 16) + 128, 0, 255).astype(np.uint8)


def _place(hd, blocks, dtype):
    """[blocks][8][8] samples -> the component planes, cropped at the plane edges"""
    ny = hd.bpm - 2
    shapes = [(hd.mcu_rows * 8 * hd.vs, hd.mcu_cols * 8 * hd.hs)] + [(hd.mcu_rows * 8, hd.mcu_cols * 8)] * (hd.comps - 1)
    planes = [np.zeros(s, dtype) for s in shapes]
    per = blocks.reshape(hd.mcu_rows, hd.mcu_cols, hd.bpm, 8, 8)
    for b in range(hd.bpm):
        if hd.comps == 1 or b < ny:
            by, bx = (0, 0) if hd.comps == 1 else divmod(b, hd.hs)
            view = planes[0].reshape(hd.mcu_rows, hd.vs, 8, hd.mcu_cols, hd.hs, 8)
            view[:, by, :, :, bx, :] = per[:, :, b].transpose(0, 2, 1, 3)
        else:
            view = planes[b - ny + 1].reshape(hd.mcu_rows, 8, hd.mcu_cols, 8)
            view[:] = per[:, :, b].transpose(0, 2, 1, 3)
    ch, cw = -(-hd.h // hd.vs), -(-hd.w // hd.hs)
    return [planes[0][:hd.h, :hd.w]] + [p[:ch, :cw] for p in planes[1:]]


def decode(data):
    data = bytes(data)
    hd = parse(data)
    ent = data[hd.data_offset:]
    marks = restart_markers(ent)
    N = hd.intervals
    bad = None
    for k, (_, number) in enumerate(marks):
        if k >= N - 1:
            bad = N - 1 if bad is None else min(bad, N - 1)
        elif number != k % 8:
            bad = k if bad is None else min(bad, k)
    if len(marks) < N - 1:
        bad = len(marks) if bad is None else min(bad, len(marks))
    scan_bad = bad
    coef = [[0] * 64 for _ in range(hd.mcu_cols * hd.mcu_rows * hd.bpm)]
    for i in range(N):
        if scan_bad is not None and i > scan_bad:
            break
        try:
            _decode_interval(hd, ent, 0 if i == 0 else marks[i - 1][0] + 2, i, coef)
        except _Damage:
            bad = i if bad is None else min(bad, i)
    coef = np.array(coef, np.int64)
    planes = _place(hd, idct_int(coef), np.uint8)
    status = np.array([OK, -1] if bad is None else [EFORMAT, bad], np.int32)
    return Decoded(hd, coef, planes, status)


def float_planes(dec):
    """the float64 inverse DCT of the statement's coefficients (+128, unrounded, unclipped), placed and cropped like the planes"""
    c = dec.coef.reshape(-1, 8, 8).astype(np.float64)
    s = np.einsum("vy,nvu,ux->nyx", DCT_F, c, DCT_F) + 128.0
    return _place(dec.header, s, np.float64)


def frame(dec, bgr=True):
    hd = dec.header
    y = dec.planes[0].astype(np.int64)
    if hd.comps == 1:
        return np.repeat(dec.planes[0][..., None], 3, axis=2)
    ys, xs = np.arange(hd.h) >> (hd.vs - 1), np.arange(hd.w) >> (hd.hs - 1)
    d = dec.planes[1].astype(np.int64)[ys][:, xs] - 128
    e = dec.planes[2].astype(np.int64)[ys][:, xs] - 128
    yoff, cy, cvr, cug, cvg, cub = JFIF
    base = cy * np.maximum(y - yoff, 0) + (1 << 19)
    r = np.clip((base + cvr * e) >> 20, 0, 255)
    g = np.clip((base - cug * d - cvg * e) >> 20, 0, 255)
    b = np.clip((base + cub * d) >> 20, 0, 255)
    return np.stack([b, g, r] if bgr else [r, g, b], -1).astype(np.uint8)


# ---- the case table --------------------------------------------------------------------------------------------------------------
def picture(h, w, seed=0):
    """A seeded RGB picture with smooth areas, edges and some texture"""
    rng = np.random.default_rng(1000 * seed + 7 * h + w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 9.0 + seed) * np.cos(y / 13.0), 60 + 0.9 * ((x + 2 * y) % 190), 255 * ((x // 11 + y // 7) % 2)], -1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def pillow_stream(h, w, mode="RGB", quality=90, seed=0, **kw):
    from PIL import Image
    im = Image.fromarray(picture(h, w, seed))
    if mode == "L":
        im = im.convert("L")
    out = io.BytesIO()
    im.save(out, "JPEG", quality=quality, **kw)
    return out.getvalue()


def own_stream(h, w, quality=95, seed=0):
    from whenet_hip import jpeg
    return jpeg.encode_host(np.ascontiguousarray(picture(h, w, seed)[..., ::-1]), quality)


def sample(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


SIZES = [(1, 1), (8, 8), (16, 16), (17, 17), (8, 33), (70, 50), (16, 8192)]      # (h, w): 1x1 ... 8192x16 as width x height


def _table():
    t = {}
    for h, w in SIZES:
        t[f"pil_420_{w}x{h}"] = functools.partial(pillow_stream, h, w, subsampling=2)
        t[f"own_{w}x{h}"] = functools.partial(own_stream, h, w)
    for sub, name in ((0, "444"), (1, "422")):
        for h, w in ((17, 17), (70, 50), (8, 33), (1, 1)):
            t[f"pil_{name}_{w}x{h}"] = functools.partial(pillow_stream, h, w, subsampling=sub)
    for h, w in ((1, 1), (17, 17), (70, 50)):
        t[f"pil_grey_{w}x{h}"] = functools.partial(pillow_stream, h, w, mode="L")
    for q in (10, 50, 95, 100):
        t[f"pil_420_q{q}"] = functools.partial(pillow_stream, 70, 50, quality=q, subsampling=2, seed=q)
        t[f"pil_444_q{q}"] = functools.partial(pillow_stream, 33, 40, quality=q, subsampling=0, seed=q)
    t["pil_420_optimize"] = functools.partial(pillow_stream, 70, 50, subsampling=2, optimize=True, seed=3)
    t["pil_444_optimize"] = functools.partial(pillow_stream, 33, 40, subsampling=0, optimize=True, seed=3)
    t["pil_grey_optimize"] = functools.partial(pillow_stream, 33, 40, mode="L", optimize=True, seed=3)
    t["pil_420_rst_rows"] = functools.partial(pillow_stream, 70, 50, subsampling=2, restart_marker_rows=1, seed=4)
    t["pil_422_rst_rows"] = functools.partial(pillow_stream, 70, 50, subsampling=1, restart_marker_rows=1, seed=4)
    t["pil_444_rst_blocks3"] = functools.partial(pillow_stream, 33, 40, subsampling=0, restart_marker_blocks=3, seed=4)
    t["pil_420_rst_blocks3"] = functools.partial(pillow_stream, 70, 50, subsampling=2, restart_marker_blocks=3, seed=4)
    t["pil_grey_rst_blocks3"] = functools.partial(pillow_stream, 33, 40, mode="L", restart_marker_blocks=3, seed=4)
    # 300 intervals: the marker number wraps 37 times and the marker scan crosses its 4,096-byte steps
    t["pil_420_16x4800_rst_rows"] = functools.partial(pillow_stream, 4800, 16, subsampling=2, restart_marker_rows=1, quality=95, seed=5)
    t["own_16x4800"] = functools.partial(own_stream, 4800, 16, seed=5)
    t["sample_001"] = functools.partial(sample, "sample_mov_001_007585.jpeg")
    t["sample_012"] = functools.partial(sample, "sample_mov_012_022606.jpeg")
    return t


_BUILDERS = _table()
CASE_NAMES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def statement(name):
    """the numpy statement's decode of a case or a damaged case: computed once, shared, never modified"""
    return decode(DAMAGED[name]()[0] if name in DAMAGED else case(name))


# ---- damaged streams: (bytes, the first bad interval) ----------------------------------------------------------------------------
def _split(data):
    """(header bytes, entropy bytes, positions of the restart markers in the entropy bytes)"""
    hd = parse(data)
    ent = data[hd.data_offset:]
    return data[:hd.data_offset], ent, [p for p, _ in restart_markers(ent)]


def _base():
    return case("pil_420_rst_rows")          # 70 rows: 5 intervals of one MCU row


def _truncated(interval, frac):
    head, ent, marks = _split(_base())
    bounds = [0] + [m + 2 for m in marks] + [len(ent)]
    cut = bounds[interval] + int((bounds[interval + 1] - 2 - bounds[interval]) * frac)
    return head + ent[:cut], interval


def _noncode():
    head, ent, marks = _split(own_stream(70, 50, 95, seed=6))       # the Annex K tables: sixteen 1-bits are no code word
    at = (marks[1] + 2 + marks[2]) // 2
    return head + ent[:at] + b"\xff\x00" * 4 + ent[at + 8:], 2


def _run_past_63():
    from tests import jpeg_cases as JC
    dc, ac = JC.huffman_codes(*JC.DC_LUMA), JC.huffman_codes(*JC.AC_LUMA)
    bits = "".join(format(c, f"0{n}b") for c, n in [dc[0]] + [ac[0xF0]] * 4)       # DC difference 0, then four ZRL: k = 1 + 64
    bits += "1" * (-len(bits) % 8)
    body = int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")
    return JC.header(16, 16, 95) + body + b"\xff\xd9", 0


def _wrong_rst():
    head, ent, marks = _split(_base())
    e = bytearray(ent)
    e[marks[1] + 1] = 0xD0 + 5                # marker 1 says RST5
    return head + bytes(e), 1


def _removed_rst():
    head, ent, marks = _split(_base())
    return head + ent[:marks[2]] + ent[marks[2] + 2:], 2


def _stray_marker():
    head, ent, marks = _split(_base())
    at = (marks[0] + 2 + marks[1]) // 2
    return head + ent[:at] + b"\xff\xc4" + ent[at:], 1


def _early_eoi():
    head, ent, marks = _split(_base())
    at = (marks[2] + 2 + marks[3]) // 2
    return head + ent[:at] + b"\xff\xd9" + ent[at:], 3


def _no_dri_truncated():
    data = case("pil_444_q50")
    hd = parse(data)
    return data[:hd.data_offset + (len(data) - hd.data_offset) // 2], 0


def _extra_rst():
    head, ent, marks = _split(_base())
    return head + ent[:-2] + b"\xff\xd4" + ent[-2:], 4      # a fifth marker behind the last interval


DAMAGED = {
    "truncated_first_byte": functools.partial(_truncated, 0, 0.0),
    "truncated_interval0": functools.partial(_truncated, 0, 0.5),
    "truncated_interval2": functools.partial(_truncated, 2, 0.4),
    "truncated_last_interval": functools.partial(_truncated, 4, 0.7),
    "truncated_no_dri": _no_dri_truncated,
    "noncode": _noncode,
    "run_past_63": _run_past_63,
    "wrong_rst": _wrong_rst,
    "removed_rst": _removed_rst,
    "stray_marker": _stray_marker,
    "early_eoi": _early_eoi,
    "extra_rst": _extra_rst,
}
DAMAGED_NAMES = list(DAMAGED)


# ---- refused streams: name -> bytes ----------------------------------------------------------------------------------------------
def _patch_sof(data, **kw):
    """the stream with fields of its SOF0 segment (or the marker itself) replaced"""
    d = bytearray(data)
    at = bytes(d).find(b"\xff\xc0")
    if "marker" in kw:
        d[at + 1] = kw["marker"]
    if "precision" in kw:
        d[at + 4] = kw["precision"]
    return bytes(d)


def _four_components():
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(picture(16, 16)).convert("CMYK").save(out, "JPEG")
    return out.getvalue()


def _progressive():
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(picture(32, 32)).save(out, "JPEG", progressive=True)
    return out.getvalue()


def _two_scans():
    """a baseline three-component frame whose first scan holds the luma only (non-interleaved)"""
    data = bytearray(case("pil_444_17x17"))
    at = bytes(data).find(b"\xff\xda")
    return bytes(data[:at]) + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + bytes(data[at + 14:])


def _missing_dht():
    data = case("pil_420_17x17")
    at = data.find(b"\xff\xc4")
    n = (data[at + 2] << 8) | data[at + 3]
    return data[:at] + data[at + 2 + n:]


def _dqt16():
    data = case("pil_420_17x17")
    at = data.find(b"\xff\xdb")
    n = (data[at + 2] << 8) | data[at + 3]
    body = data[at + 4:at + 2 + n]
    wide = b""
    for i in range(0, len(body), 65):
        wide += bytes([0x10 | body[i]]) + b"".join(bytes([0, v]) for v in body[i + 1:i + 65])
    return data[:at] + b"\xff\xdb" + (len(wide) + 2).to_bytes(2, "big") + wide + data[at + 2 + n:]


REFUSED = {
    "progressive": _progressive,
    "sof1": lambda: _patch_sof(case("pil_420_17x17"), marker=0xC1),
    "arithmetic": lambda: _patch_sof(case("pil_420_17x17"), marker=0xC9),
    "12bit": lambda: _patch_sof(case("pil_420_17x17"), precision=12),
    "4_components": _four_components,
    "two_scans": _two_scans,
    "missing_dht": _missing_dht,
    "dqt_16bit": _dqt16,
    "truncated_header": lambda: case("pil_420_17x17")[:200],
    "not_a_jpeg": lambda: b"RIFF" + bytes(100),
}
