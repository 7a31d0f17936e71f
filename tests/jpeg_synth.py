"""A writer of baseline JPEG streams whose decoded coefficients are known by construction, and the case table of the synthetic
decoder tests (tests/test_jpeg_decode_synth_cpu.py, tests/test_jpeg_decode_synth_gpu.py).

The decoder accepts far more than any encoder in the suite emits (include/whenet_hip.h, JPEG DECODER): DC predictors that run into
-32768 / 32767, Huffman codes of 10..16 bits, complete codes whose padding is a code word, value sizes up to 15, crossed table ids,
other (r, 0) symbols as EOB, a ZRL that lands on k = 64, fill bytes before markers, bytes behind an interval's last block.  `write`
takes a stream's description down to every block's DC DIFFERENCE and its 63 quantised AC values and returns the bytes together with
what a decoder must find in them -- computed here, in the writer's own loop, from the header's rules and from nothing else: no code
of csrc/ and no decoder of tests/jpeg_decode_cases.py is called.  The inverse DCT and the pixel rule stay the statement's
(`jpeg_decode_cases.idct_int`, `_place`, `frame`): `expected` applies them to the writer's coefficients.

    write(h, w, blocks, ...) -> Synth          # the stream, the expected coefficients, and the bookkeeping the tests assert on
    CASES: name -> builder;  case(name) -> Synth (built once);  expected(name) -> Expected(planes, frame, status)
"""
import functools
from collections import Counter, namedtuple

import numpy as np

from tests import jpeg_cases as JC
from tests import jpeg_decode_cases as DC

ZIGZAG = JC.ZIGZAG
ANNEX_K = {(0, 0): JC.DC_LUMA, (1, 0): JC.AC_LUMA, (0, 1): JC.DC_CHROMA, (1, 1): JC.AC_CHROMA}

# data: the stream.  data_offset: where its entropy data begins.  coef: int64 [blocks, 64], dequantised and clamped, natural order.
# dc_offset: per block the byte of the entropy data (stuffed bytes counted) in which its DC code word begins.  pad_bits: per interval.
# interval_start: per interval its first byte in the entropy data.  body_bytes: the entropy data without EOI and its fill bytes.
# pred / raw_pred: per block its component's predictor, clamped as the header says / the plain sum of the interval's differences.
# bound: per component the set of bounds ("lo", "hi") at which the clamp changed a predictor.  comp: per block its component.
# lengths: class -> Counter of the code-word lengths written.  sizes: class -> Counter of the value sizes written.
# closed: Counter of how blocks end: "eob", "full" (coefficient 63 is coded, no EOB), "zrl" (a ZRL lands on k = 64).
# zrls: per block the number of ZRL symbols.  rst: the numbers of the restart markers written.  header: a DC.Header for _place / frame.
Synth = namedtuple("Synth", "data data_offset coef dc_offset pad_bits interval_start body_bytes pred raw_pred bound comp lengths sizes "
                            "closed zrls rst header")
Expected = namedtuple("Expected", "header coef planes frame status")


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _value_bits(v, s):
    """the s extra bits of value v (T.81 F.1.2.1: a negative value is written as v - 1 in s bits)"""
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


def write(h, w, blocks, comps=1, sampling=(1, 1), q=None, huff=None, tables=None, comp_ids=(1, 2, 3), ri=0, pad_bit=1, eob=0x00,
          zrl_close=False, fill=0, tail=b"", merged=False):
    """blocks: in coding order (MCU by MCU; in an MCU hs x vs luma blocks in row order, then Cb, then Cr), each (the DC difference,
    63 quantised AC values in zigzag order).  q: id -> 64 quantisers in natural order.  huff: (class, id) -> (counts[16], values).
    tables: per component (quantiser id, DC id, AC id).  ri: the restart interval in MCUs (0: no DRI).
    pad_bit: the bit an interval's last byte is filled with.  eob: the symbol that ends a block, 0x00 or another (r, 0), r != 15.
    zrl_close: a block whose last coefficient is at 47 ends with a ZRL (k = 48 + 16 = 64) instead of an EOB.
    fill: 0xFF bytes in front of every marker of the entropy data (RSTn, EOI).  tail: bytes without 0xFF behind every interval's
    last block.  merged: all DQT tables in one segment and all DHT tables in one segment, instead of a segment each."""
    hs, vs = sampling if comps == 3 else (1, 1)
    q = {0: [1] * 64} if q is None else q
    huff = {k: v for k, v in ANNEX_K.items() if comps == 3 or k[1] == 0} if huff is None else huff
    tables = ([(0, 0, 0), (1, 1, 1), (1, 1, 1)] if len(q) > 1 else [(0, 0, 0), (0, 1, 1), (0, 1, 1)])[:comps] if tables is None else tables
    assert comps in (1, 3) and (hs, vs) in ((2, 2), (2, 1), (1, 1)) and len(tables) == comps and b"\xff" not in tail
    assert eob & 15 == 0 and eob >> 4 != 15 and pad_bit in (0, 1)
    mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
    mcus, bpm, ny = mcu_cols * mcu_rows, (hs * vs + 2 if comps == 3 else 1), hs * vs
    assert len(blocks) == mcus * bpm
    eff = ri if 0 < ri < mcus else mcus
    intervals = -(-mcus // eff)
    codes = {k: JC.huffman_codes(*v) for k, v in huff.items()}

    # ---- the header ----
    out = bytearray(b"\xff\xd8")
    dqt = [bytes([i]) + bytes(q[i][ZIGZAG[k]] for k in range(64)) for i in sorted(q)]
    for payload in ([b"".join(dqt)] if merged else dqt):
        out += JC.segment(0xDB, payload)
    sof = bytes([8]) + JC.be16(h) + JC.be16(w) + bytes([comps])
    for c in range(comps):
        sof += bytes([comp_ids[c], ((hs << 4) | vs) if c == 0 and comps == 3 else 0x11, tables[c][0]])
    out += JC.segment(0xC0, sof)
    dht = [bytes([(cls << 4) | i]) + bytes(huff[(cls, i)][0]) + bytes(huff[(cls, i)][1]) for cls, i in sorted(huff, key=lambda k: (k[1], k[0]))]
    for payload in ([b"".join(dht)] if merged else dht):
        out += JC.segment(0xC4, payload)
    if ri:
        out += JC.segment(0xDD, JC.be16(ri))
    out += JC.segment(0xDA, bytes([comps]) + b"".join(bytes([comp_ids[c], (tables[c][1] << 4) | tables[c][2]]) for c in range(comps)) +
                      bytes([0, 63, 0]))
    data_offset = len(out)

    # ---- the entropy data, and what a decoder must find in it ----
    coef = np.zeros((len(blocks), 64), np.int64)
    dc_offset, pad_bits, interval_start, pred_of, raw_of, comp_of, zrls, rst = [], [], [], [], [], [], [], []
    bound = [set() for _ in range(comps)]
    lengths, sizes, closed = {0: Counter(), 1: Counter()}, {0: Counter(), 1: Counter()}, Counter()
    ent = bytearray()
    for i in range(intervals):
        acc, nbits, pred, raw, starts = 0, 0, [0, 0, 0], [0, 0, 0], []

        def put(cls, table, sym, v=None):
            nonlocal acc, nbits
            code, length = table[sym]
            s = sym & 15
            lengths[cls][length] += 1
            acc, nbits = (acc << length) | code, nbits + length
            if v is not None:
                assert s > 0 and int(abs(v)).bit_length() == s
                sizes[cls][s] += 1
                acc, nbits = (acc << s) | _value_bits(v, s), nbits + s

        for m in range(i * eff, min((i + 1) * eff, mcus)):
            for b in range(bpm):
                c = 0 if comps == 1 or b < ny else b - ny + 1
                qt, dct, act = q[tables[c][0]], codes[(0, tables[c][1])], codes[(1, tables[c][2])]
                d, ac = int(blocks[m * bpm + b][0]), [int(v) for v in blocks[m * bpm + b][1]]
                assert len(ac) == 63 and abs(d) <= 2047
                starts.append(nbits)
                # the header's rules, once more: the predictor inside -32768..32767, every coefficient inside -2048..2047
                raw[c] += d
                if pred[c] + d < -32768:
                    bound[c].add("lo")
                if pred[c] + d > 32767:
                    bound[c].add("hi")
                pred[c] = clamp(pred[c] + d, -32768, 32767)
                pred_of.append(pred[c]), raw_of.append(raw[c]), comp_of.append(c)
                out_row = coef[m * bpm + b]
                out_row[0] = clamp(pred[c] * qt[0], -2048, 2047)
                s = abs(d).bit_length()
                put(0, dct, s, d if s else None)
                if s == 0:
                    sizes[0][0] += 1
                last = max((k for k in range(1, 64) if ac[k - 1] != 0), default=0)
                run = nz = 0
                for k in range(1, last + 1):
                    v = ac[k - 1]
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        put(1, act, 0xF0)
                        run, nz = run - 16, nz + 1
                    put(1, act, (run << 4) | abs(v).bit_length(), v)
                    out_row[ZIGZAG[k]] = clamp(v * qt[ZIGZAG[k]], -2048, 2047)
                    run = 0
                if last == 63:
                    closed["full"] += 1
                elif zrl_close and last == 47:
                    put(1, act, 0xF0)
                    nz += 1
                    closed["zrl"] += 1
                else:
                    put(1, act, eob)
                    closed["eob"] += 1
                zrls.append(nz)
        pad = -nbits % 8
        pad_bits.append(pad)
        raw_bytes = ((acc << pad) | (((1 << pad) - 1) if pad_bit else 0)).to_bytes((nbits + pad) // 8, "big")
        ff = np.frombuffer(raw_bytes, np.uint8) == 0xFF
        before = np.concatenate([[0], np.cumsum(ff)])          # stuffed zeros in front of raw byte j
        interval_start.append(len(ent))
        dc_offset += [len(ent) + at // 8 + int(before[at // 8]) for at in starts]
        ent += raw_bytes.replace(b"\xff", b"\xff\x00") + tail
        if i + 1 < intervals:
            ent += b"\xff" * fill + bytes([0xFF, 0xD0 + (i & 7)])
            rst.append(i & 7)
    body_bytes = len(ent)
    ent += b"\xff" * fill + b"\xff\xd9"
    header = DC.Header(h, w, comps, hs, vs, [t[0] for t in tables], [t[1] for t in tables], [t[2] for t in tables], ri, intervals,
                       data_offset, None, None, mcu_cols, mcu_rows, bpm)
    return Synth(bytes(out + ent), data_offset, coef, np.array(dc_offset), pad_bits, interval_start, body_bytes, np.array(pred_of),
                 np.array(raw_of), bound, np.array(comp_of), lengths, sizes, closed, zrls, rst, header)


# ---- Huffman tables that no encoder of the suite emits ---------------------------------------------------------------------------
def _counts(**at):
    """counts[16] with at['l9'] = 6 codes of 9 bits, ..."""
    c = [0] * 16
    for k, n in at.items():
        c[int(k[1:]) - 1] = n
    return c


AC_ALL = [(r << 4) | s for s in range(1, 16) for r in range(16)] + [0x00, 0xF0, 0x50]           # 243 symbols: value sizes up to 15
AC_129 = [0x00, 0xF0] + [(r << 4) | s for s in range(1, 8) for r in range(16)] + [(r << 4) | 8 for r in range(15)]      # sizes up to 8
LEN16 = {(0, 0): (_counts(l16=12), list(range(12))), (0, 1): (_counts(l16=12), list(range(11, -1, -1))),
         (1, 0): (_counts(l16=243), AC_ALL), (1, 1): (_counts(l16=243), AC_ALL[100:] + AC_ALL[:100])}
EDGE910 = {(0, 0): (_counts(l9=6, l10=6), list(range(12))), (1, 0): (_counts(l9=100, l10=29), AC_129)}
# complete codes (Kraft sum 1): DC 0, 10, 110, 111 with 111 = category 0; AC 127 codes of 7 bits and 1111111x
PHANTOM = {(0, 0): (_counts(l1=1, l2=1, l3=2), [1, 2, 3, 0]), (1, 0): (_counts(l7=127, l8=2), AC_129)}


def kraft(counts):
    return sum(n / (1 << (l + 1)) for l, n in enumerate(counts))


# ---- blocks ----------------------------------------------------------------------------------------------------------------------
def _ac(rng, n, sizes, last=63, symbols=None):
    """63 AC values of which n, at random places up to `last`, are non-zero with a bit size drawn from `sizes`; a value whose
    (run, size) is not among `symbols` is halved until it is"""
    ac = [0] * 63
    for k in rng.choice(np.arange(1, last + 1), size=min(n, last), replace=False).tolist():
        s = int(rng.choice(sizes))
        ac[k - 1] = int(rng.integers(1 << (s - 1), 1 << s)) * (1 if rng.integers(2) else -1)
    run = 0
    for k in range(63):
        if ac[k] == 0:
            run += 1
            continue
        while symbols is not None and (((run & 15) << 4) | abs(ac[k]).bit_length()) not in symbols:
            ac[k] = int(ac[k] / 2)
        run = 0
    return ac


def _random_blocks(rng, n, dc=2047, most=8, sizes=(1, 2, 3, 4, 5, 6), symbols=None):
    return [(int(rng.integers(-dc, dc + 1)), _ac(rng, int(rng.integers(0, most + 1)), sizes, symbols=symbols)) for _ in range(n)]


def _sat_grey():
    rng = np.random.default_rng(11)
    blocks = _random_blocks(rng, 256, most=14, sizes=(1,))                       # AC +-1: the blocks differ in length
    for b in range(256):
        if 20 <= b < 70:
            blocks[b] = (2047, blocks[b][1])
        elif 120 <= b < 220:
            blocks[b] = (-2047, blocks[b][1])
    return write(128, 128, blocks)


def _sat_420():
    # 80 x 64 and not 64 x 64: a DC difference is at most 2047 (category 11), so a chroma predictor needs 17 blocks to pass 32767 and
    # a 64 x 64 frame has 16 per chroma component; 80 x 64 (20 MCUs) is the smallest 4:2:0 frame of whole MCUs that has them
    rng = np.random.default_rng(12)
    blocks = _random_blocks(rng, 20 * 6, most=5, sizes=(1, 2, 3))
    luma = cb = 0
    for i, (d, ac) in enumerate(blocks):
        b = i % 6
        if b < 4:
            blocks[i] = (-2047 if luma < 30 else int(rng.integers(-300, 2048)), ac)
            luma += 1
        elif b == 4:
            blocks[i] = (2047 if cb < 18 else int(rng.integers(-2047, 300)), ac)
            cb += 1
        else:
            blocks[i] = (int(rng.integers(-500, 501)), ac)
    return write(64, 80, blocks, comps=3, sampling=(2, 2), q={0: [1] * 64, 1: [1] * 64})


def _len16_444():
    rng = np.random.default_rng(13)
    blocks = _random_blocks(rng, 15 * 3, most=7, sizes=tuple(range(1, 16)))
    q = {3: [16] * 64, 0: [1] * 64, 2: list(range(1, 65))}
    return write(24, 40, blocks, comps=3, sampling=(1, 1), q=q, huff=LEN16, tables=[(3, 1, 0), (0, 0, 1), (2, 1, 1)])


def _edge910_grey():
    rng = np.random.default_rng(14)
    return write(120, 120, _random_blocks(rng, 225, most=8, sizes=tuple(range(1, 9)), symbols=AC_129), q={0: JC.Q_LUMA}, huff=EDGE910, ri=4)


def _phantom(pad_bit, seed):
    rng = np.random.default_rng(seed)
    return write(120, 120, _random_blocks(rng, 225, dc=7, most=6, sizes=tuple(range(1, 9)), symbols=AC_129), q={0: JC.Q_LUMA}, huff=PHANTOM, ri=4,
                 pad_bit=pad_bit)


def _ri1_grey():
    rng = np.random.default_rng(16)
    huff = {(0, 0): LEN16[(0, 0)], (1, 0): LEN16[(1, 0)]}
    return write(16, 2400, _random_blocks(rng, 600, most=3, sizes=(1, 2, 3, 9, 12)), q={0: [3] * 64}, huff=huff, ri=1, eob=0x50)


def _q2():
    return {0: JC.scaled_q(JC.Q_LUMA, 90), 1: JC.scaled_q(JC.Q_CHROMA, 90)}


def _tail_bytes_420():
    rng = np.random.default_rng(17)
    return write(48, 48, _random_blocks(rng, 9 * 6, dc=300), comps=3, sampling=(2, 2), q=_q2(), ri=2, tail=bytes([0x12, 0x34, 0x00, 0x56]) * 9)


def _fill_420():
    rng = np.random.default_rng(18)
    return write(48, 48, _random_blocks(rng, 9 * 6, dc=300), comps=3, sampling=(2, 2), q=_q2(), ri=2, fill=3)


def idct_extreme_signs(b):
    """[v][u] signs that align every term of sample (y0, x0) = divmod(b, 8) of the inverse DCT, negated on even b"""
    y0, x0 = divmod(b, 8)
    s = np.sign(np.outer(DC.DCT[:, y0], DC.DCT[:, x0])).astype(np.int64)
    return -s if b % 2 == 0 else s


def _idct_extreme():
    blocks, pred = [], 0
    for b in range(64):
        zz = (1023 * idct_extreme_signs(b)).reshape(64)[ZIGZAG]
        blocks.append((int(zz[0]) - pred, [int(v) for v in zz[1:]]))
        pred = int(zz[0])
    return write(64, 64, blocks, q={0: [255] * 64})


def _zrl_close_422():
    rng = np.random.default_rng(20)
    blocks = []
    for i in range(15 * 4):
        d = int(rng.integers(-200, 201))
        if i % 4 == 0:                       # the last coefficient at 63: no EOB
            ac = _ac(rng, 5, (1, 2, 3), last=62)
            ac[62] = 3
        elif i % 4 == 1:                     # coefficient 63 alone: three ZRL and (14, s)
            ac = [0] * 62 + [-2]
        elif i % 4 == 2:                     # the last coefficient at 47, closed by a ZRL: k = 64
            ac = _ac(rng, 4, (1, 2, 3), last=46)
            ac[46] = -5
        else:
            ac = _ac(rng, 4, (1, 2, 3))
        blocks.append((d, ac))
    return write(40, 48, blocks, comps=3, sampling=(2, 1), q=_q2(), ri=5, zrl_close=True)


def _multi_table_segments():
    rng = np.random.default_rng(21)
    return write(32, 32, _random_blocks(rng, 4 * 6, dc=300), comps=3, sampling=(2, 2), q=_q2(), comp_ids=(82, 71, 66), merged=True)


CASES = {
    "sat_grey": _sat_grey, "sat_420": _sat_420, "len16_444": _len16_444, "edge910_grey": _edge910_grey,
    "phantom_grey": functools.partial(_phantom, 1, 15), "phantom_pad0": functools.partial(_phantom, 0, 22), "ri1_grey": _ri1_grey,
    "tail_bytes_420": _tail_bytes_420, "fill_420": _fill_420, "idct_extreme": _idct_extreme, "zrl_close_422": _zrl_close_422,
    "multi_table_segments": _multi_table_segments,
}
CASE_NAMES = list(CASES)
MAX_BYTES = 72 * 1024


@functools.lru_cache(maxsize=None)
def case(name):
    s = CASES[name]()
    assert len(s.data) <= MAX_BYTES
    return s


@functools.lru_cache(maxsize=None)
def expected(name):
    """what a decoder must return for a case, from the writer's coefficients: computed once, shared, never modified"""
    s = case(name)
    planes = DC._place(s.header, DC.idct_int(s.coef), np.uint8)
    status = np.array([DC.OK, -1], np.int32)
    frame = DC.frame(DC.Decoded(s.header, s.coef, planes, status))
    return Expected(s.header, s.coef, planes, frame, status)
