"""The progressive JPEG decoder's format as a numpy / Python statement, a scan writer, and the case table of its tests.

The statement is written from include/whenet_hip.h (JPEG DECODER, PROGRESSIVE) and shares no code with csrc/jpeg_prog_host.h: the
markers are walked with Python integers, the Huffman codes are matched bit by bit (tests/jpeg_decode_cases._Bits), the four scan
kinds are plain loops over lists.  Behind the finish it hands over to the statements of the baseline decoder (rule 0:
jpeg_decode_cases, rule 1: jpeg_exact_cases), which start from dequantised records.

    parse(data) -> (Header, [scan dicts])      # raises Refused(reason)
    decode(data) -> Prog(header, raw, coef, planes, status, counters)      # .header/.coef/.planes/.status as jpeg_decode_cases.Decoded
    write(planes_coef, h, w, script, ...) -> bytes      # the scan writer: quantised blocks -> a progressive stream under a script
    CASES / DAMAGED / REFUSED: name -> builder
"""
import functools
import io
from collections import namedtuple

import numpy as np

from tests import jpeg_decode_cases as DC

OK, EFORMAT = DC.OK, DC.EFORMAT
Refused = DC.Refused
ZIGZAG = DC.ZIGZAG
MAX_SCANS = 128
Prog = namedtuple("Prog", "header raw coef planes status counters scans")


# ---- parse -----------------------------------------------------------------------------------------------------------------------
def _codes(counts, values):
    """(length, code) -> symbol of a DHT"""
    table, code, n = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = values[n]
            code, n = code + 1, n + 1
        code <<= 1
    return table


def _scan_end(data, p):
    """(where the entropy data that begins at p ends, [(position, number)] of its restart markers)"""
    marks = []
    while True:
        f = data.find(b"\xff", p)
        if f < 0 or f + 1 >= len(data):
            return len(data), marks
        b = data[f + 1]
        if b == 0:
            p = f + 2
        elif b == 0xFF:
            p = f + 1
        elif 0xD0 <= b <= 0xD7:
            marks.append((f, b & 7))
            p = f + 2
        else:
            return f, marks


def parse(data):
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    p, frame, q, huff, dri, scans, ids = 2, None, {}, {}, 0, [], []
    al_of = {}
    while True:
        if p + 2 > len(data):
            if scans:
                break
            raise Refused("truncated header")
        if data[p] != 0xFF:
            raise Refused("no marker")
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        p += 2
        if m == 0xD9:
            if scans:
                break
            raise Refused("EOI before SOS")
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            raise Refused("unexpected marker")
        if p + 2 > len(data) or p + ((data[p] << 8) | data[p + 1]) > len(data) or ((data[p] << 8) | data[p + 1]) < 2:
            if scans:
                break
            raise Refused("truncated segment")
        n = ((data[p] << 8) | data[p + 1]) - 2
        s = data[p + 2:p + 2 + n]
        if m == 0xC2:
            if frame is not None or s[0] != 8:
                raise Refused("frame header")
            h, w, comps = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if comps not in (1, 3) or not 1 <= h <= 8192 or not 1 <= w <= 8192 or n != 6 + 3 * comps:
                raise Refused("frame")
            ids = [s[6 + 3 * c] for c in range(comps)]
            hv = [s[7 + 3 * c] for c in range(comps)]
            qt = [s[8 + 3 * c] for c in range(comps)]
            if comps == 3 and (hv[0] not in (0x22, 0x21, 0x11) or hv[1] != 0x11 or hv[2] != 0x11):
                raise Refused("sampling")
            hs, vs = (hv[0] >> 4, hv[0] & 15) if comps == 3 else (1, 1)
            frame = (h, w, comps, hs, vs, qt)
        elif 0xC0 <= m <= 0xCF and m != 0xC4:
            raise Refused("not a progressive Huffman frame")
        elif m == 0xDB:
            if scans:
                raise Refused("DQT behind the first SOS")
            i = 0
            while i < n:
                if s[i] >> 4 or (s[i] & 15) > 3 or i + 65 > n:
                    raise Refused("DQT")
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = s[i + 1 + k]
                q[s[i] & 15] = nat
                i += 65
        elif m == 0xC4:
            i = 0
            while i < n:
                tc, th = s[i] >> 4, s[i] & 15
                counts = list(s[i + 1:i + 17])
                if tc > 1 or th > 3 or i + 17 + sum(counts) > n:
                    raise Refused("DHT")
                huff[(tc, th)] = _codes(counts, list(s[i + 17:i + 17 + sum(counts)]))
                i += 17 + sum(counts)
        elif m == 0xDD:
            dri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            if frame is None:
                raise Refused("SOS before SOF")
            h, w, comps, hs, vs, qt = frame
            ns = s[0]
            if ns == 2 or ns not in (1, comps) or n != 4 + 2 * ns:
                raise Refused("Ns")
            if len(scans) >= MAX_SCANS:
                raise Refused("more than 128 scans")
            cs = [ids.index(s[1 + 2 * i]) if s[1 + 2 * i] in ids else -1 for i in range(ns)]
            if -1 in cs or (ns > 1 and cs != list(range(ns))):
                raise Refused("scan components")
            td, ta = [s[2 + 2 * i] >> 4 for i in range(ns)], [s[2 + 2 * i] & 15 for i in range(ns)]
            ss, se, ah, al = s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns] >> 4, s[3 + 2 * ns] & 15
            if ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and ns > 1) or ah > 13 or al > 13 or max(td + ta) > 3:
                raise Refused("script")
            for c in cs:
                if ss > 0 and (c, 0) not in al_of:
                    raise Refused("AC before DC")
                for k in range(ss, se + 1):
                    have = al_of.get((c, k))
                    if ah == 0 and have is not None:
                        raise Refused("second first scan")
                    if ah > 0 and (have is None or have != ah or al != ah - 1):
                        raise Refused("refinement")
            for c in cs:
                for k in range(ss, se + 1):
                    al_of[(c, k)] = al
            if any(t not in q for t in qt):
                raise Refused("missing DQT")
            if ss == 0 and ah == 0:
                tabs = [huff.get((0, t)) for t in td]
            elif ss > 0:
                tabs = [huff.get((1, ta[0]))]
            else:
                tabs = []
            if None in tabs:
                raise Refused("missing DHT")
            mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
            if ns > 1 or comps == 1:
                bw, bh = mcu_cols, mcu_rows
            else:
                cw, ch = (w, h) if cs[0] == 0 else (-(-w // hs), -(-h // vs))
                bw, bh = -(-cw // 8), -(-ch // 8)
            units = bw * bh
            ri = dri if 0 < dri < units else units
            level = 1
            for e in scans:
                if set(e["comps"]) & set(cs) and e["ss"] <= se and ss <= e["se"]:
                    level = max(level, e["level"] + 1)
            start = p + 2 + n
            end, marks = _scan_end(data, start)
            scans.append(dict(comps=cs, ss=ss, se=se, ah=ah, al=al, tabs=tabs, bw=bw, bh=bh, units=units, ri=ri,
                              intervals=-(-units // ri), level=level, start=start, end=end, marks=marks, dri=dri))
            p = end
            continue
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        else:
            raise Refused("marker")
        p += n + 2
    h, w, comps, hs, vs, qt = frame
    mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
    first = scans[0]
    mcus = mcu_cols * mcu_rows
    ri0 = first["dri"] if 0 < first["dri"] < mcus else mcus
    hd = DC.Header(h, w, comps, hs, vs, qt, [0] * 3, [0] * 3, first["dri"], -(-mcus // ri0), first["start"], q, huff, mcu_cols, mcu_rows,
                   hs * vs + 2 if comps == 3 else 1)
    complete = all(al_of.get((c, k)) == 0 for c in range(comps) for k in range(64))
    return hd, scans, complete


# ---- the scan decode -------------------------------------------------------------------------------------------------------------
def _record(hd, sc, u, b):
    if len(sc["comps"]) > 1:
        return u * hd.bpm + b
    if hd.comps == 1:
        return u
    by, bx = divmod(u, sc["bw"])
    if sc["comps"][0] == 0:
        return ((by // hd.vs) * hd.mcu_cols + bx // hd.hs) * hd.bpm + (by % hd.vs) * hd.hs + bx % hd.hs
    return (by * hd.mcu_cols + bx) * hd.bpm + hd.bpm - 2 + sc["comps"][0] - 1


def _raw_bits(br, k):
    if br.at + k > len(br.bits):
        raise DC._Damage
    v = 0
    for b in br.bits[br.at:br.at + k]:
        v = (v << 1) | b
    br.at += k
    return v


def _i16(v):
    return DC.clamp(v, -32768, 32767)


def _item(hd, sc, data, start, i, raw, cnt):
    br = DC._Bits(DC._interval_bits(data[:sc["end"]], start))
    first, last = i * sc["ri"], min((i + 1) * sc["ri"], sc["units"])
    ss, se, p1 = sc["ss"], sc["se"], 1 << sc["al"]
    interleaved = len(sc["comps"]) > 1
    nb, ny = (hd.bpm if interleaved else 1), hd.bpm - 2

    def correct(rec, k):
        bit = _raw_bits(br, 1)
        cnt["correction_bits"] += 1
        if bit and not rec[k] & p1:
            rec[k] = _i16(rec[k] + (p1 if rec[k] >= 0 else -p1))
            cnt["corrections"] += 1

    if ss == 0:
        pred = [0, 0, 0]
        for u in range(first, last):
            for b in range(nb):
                ci = b - ny + 1 if interleaved and b >= ny else 0
                rec = raw[_record(hd, sc, u, b)]
                if sc["ah"] == 0:
                    pred[ci] = DC.clamp(pred[ci] + br.value(br.symbol(sc["tabs"][ci]) & 15), -32768, 32767)
                    rec[0] = _i16(pred[ci] * p1)
                elif _raw_bits(br, 1):
                    rec[0] = rec[0] | p1
        return
    eobrun = 0
    for u in range(first, last):
        rec = raw[_record(hd, sc, u, 0)]
        k = ss
        if sc["ah"] == 0:
            if eobrun > 0:
                eobrun -= 1
                continue
            while k <= se:
                sym = br.symbol(sc["tabs"][0])
                r, s = sym >> 4, sym & 15
                if s:
                    k += r
                    if k > se:
                        raise DC._Damage
                    rec[k] = _i16(br.value(s) * p1)
                    k += 1
                elif r == 15:
                    k += 16
                    if k > se + 1:
                        raise DC._Damage
                else:
                    eobrun = (1 << r) + _raw_bits(br, r)
                    cnt["max_eobrun"] = max(cnt["max_eobrun"], eobrun)
                    if u + eobrun > last:
                        raise DC._Damage
                    eobrun -= 1
                    break
            continue
        if eobrun == 0:
            while k <= se:
                sym = br.symbol(sc["tabs"][0])
                r, s = sym >> 4, sym & 15
                new = 0
                if s:
                    if s != 1:
                        raise DC._Damage
                    new = p1 if _raw_bits(br, 1) else -p1
                elif r != 15:
                    eobrun = (1 << r) + _raw_bits(br, r)
                    cnt["max_eobrun"] = max(cnt["max_eobrun"], eobrun)
                    if u + eobrun > last:
                        raise DC._Damage
                    break
                else:
                    cnt["refine_zrl"] += 1
                while True:
                    if k > se:
                        raise DC._Damage      # the run passes Se
                    if rec[k]:
                        correct(rec, k)
                    else:
                        r -= 1
                        if r < 0:
                            break
                    k += 1
                if s:
                    rec[k] = new
                k += 1
        if eobrun > 0:
            while k <= se:
                if rec[k]:
                    correct(rec, k)
                k += 1
            eobrun -= 1


@functools.lru_cache(maxsize=256)
def decode(data):
    data = bytes(data)
    hd, scans, complete = parse(data)
    blocks = hd.mcu_cols * hd.mcu_rows * hd.bpm
    raw = [[0] * 64 for _ in range(blocks)]
    cnt = dict(scans=len(scans), items=0, levels=max(s["level"] for s in scans), max_eobrun=0, refine_zrl=0, correction_bits=0, corrections=0)
    bad = None
    for sc in scans:
        n, marks = sc["intervals"], sc["marks"]
        mbad = None
        for k, (_, number) in enumerate(marks):
            if k >= n - 1:
                mbad = n - 1 if mbad is None else min(mbad, n - 1)
            elif number != k % 8:
                mbad = k if mbad is None else min(mbad, k)
        if len(marks) < n - 1:
            mbad = len(marks) if mbad is None else min(mbad, len(marks))
        sbad = mbad
        for i in range(n):
            if mbad is not None and i > mbad:
                break
            try:
                _item(hd, sc, data, sc["start"] if i == 0 else marks[i - 1][0] + 2, i, raw, cnt)
            except DC._Damage:
                sbad = i if sbad is None else min(sbad, i)
        if sbad is not None and bad is None:
            bad = cnt["items"] + sbad
        cnt["items"] += n
    if bad is None and not complete:
        bad = cnt["items"]
    raw = np.array(raw, np.int64)
    coef = np.zeros_like(raw)
    ny = hd.bpm - 2
    for b in range(blocks):
        c = 0 if hd.comps == 1 or b % hd.bpm < ny else b % hd.bpm - ny + 1
        qn = hd.q[hd.qt[c]]
        for k in range(64):
            coef[b, ZIGZAG[k]] = DC.clamp(int(raw[b, k]) * qn[ZIGZAG[k]], -2048, 2047)
    planes = DC._place(hd, DC.idct_int(coef), np.uint8)
    status = np.array([OK, -1] if bad is None else [EFORMAT, bad], np.int32)
    for a in (raw, coef, status):
        a.setflags(write=False)
    return Prog(hd, raw, coef, planes, status, cnt, scans)


def off_the_clamp(dec):
    return -2048 < int(dec.coef.min()) and int(dec.coef.max()) < 2047


# ---- the scan writer -------------------------------------------------------------------------------------------------------------
class _Out:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def flush(self):
        """pad with 1 bits to a byte, stuff 0xFF"""
        self.bits += [1] * (-len(self.bits) % 8)
        out = bytearray()
        for b in np.packbits(np.array(self.bits, np.uint8)).tolist() if self.bits else []:
            out.append(b)
            if b == 0xFF:
                out.append(0)
        self.bits = []
        return bytes(out)


def fixed_table(dc):
    """a general-purpose table: (counts, values).  DC: the 12 categories at 4 bits.  AC: every symbol, 64 at 8 and 192 at 10 bits
    (the Kraft sum is 7/16: sixteen 1 bits are no code)"""
    counts = [0] * 16
    if dc:
        counts[3] = 12
        return counts, list(range(12))
    first = [0x00, 0x01, 0x11, 0x02, 0x21, 0x10, 0xF0, 0x31, 0x41, 0x03, 0x12, 0x20, 0x30, 0x40, 0x51, 0x61]
    vals = first + [v for v in range(256) if v not in first]
    counts[7], counts[9] = 64, 192
    return counts, vals


def ranked_table(freq):
    """a table of the scan's own symbols, the most frequent first: rank r gets 2 floor(log2(r + 1)) + 2 bits (Kraft sum 1/2)"""
    syms = sorted(freq, key=lambda s: (-freq[s], s))
    counts = [0] * 16
    for r in range(len(syms)):
        counts[min(2 * ((r + 1).bit_length() - 1) + 1, 15)] += 1
    return counts, syms


def _enc_table(counts, values):
    return {sym: (code, length) for (length, code), sym in _codes(counts, values).items()}


def _nbits(v):
    return int(v).bit_length()


def _scan_tokens(blocks, sc, ri):
    """the scan's intervals as token lists: ('s', table index, symbol) | ('b', value, nbits); blocks: per unit, per block in the unit,
    (scan component index, the block's 64 zigzag coefficients)"""
    ss, se, ah, al = sc["ss"], min(sc["se"], 63), sc.get("ah", 0), sc["al"]      # (a refused script may say Se = 64)
    out = []
    for first in range(0, len(blocks), ri):
        t, pred, eobrun, be = [], [0, 0, 0], 0, []

        def emit_eobrun():
            nonlocal eobrun, be
            if eobrun > 0:
                n = _nbits(eobrun) - 1
                t.append(("s", 0, n << 4))
                if n:
                    t.append(("b", eobrun & ((1 << n) - 1), n))
                eobrun = 0
            t.extend(be)
            be = []

        for unit in blocks[first:first + ri]:
            for ci, z in unit:
                if ss == 0 and ah == 0:
                    v = int(z[0]) >> al
                    d, pred[ci] = v - pred[ci], v
                    n = _nbits(abs(d))
                    t.append(("s", ci, n))
                    if n:
                        t.append(("b", d if d >= 0 else d + (1 << n) - 1, n))
                elif ss == 0:
                    t.append(("b", (int(z[0]) >> al) & 1, 1))
                elif ah == 0:
                    r = 0
                    for k in range(ss, se + 1):
                        a = abs(int(z[k])) >> al
                        if a == 0:
                            r += 1
                            continue
                        emit_eobrun()
                        while r > 15:
                            t.append(("s", 0, 0xF0))
                            r -= 16
                        n = _nbits(a)
                        t.append(("s", 0, (r << 4) | n))
                        t.append(("b", a if z[k] >= 0 else a ^ ((1 << n) - 1), n))
                        r = 0
                    if r > 0:
                        eobrun += 1
                        if eobrun == 0x7FFF:
                            emit_eobrun()
                else:
                    av = [abs(int(z[k])) >> al for k in range(64)]
                    eob = max([k for k in range(ss, se + 1) if av[k] == 1], default=0)
                    r, br = 0, []
                    for k in range(ss, se + 1):
                        a = av[k]
                        if a == 0:
                            r += 1
                            continue
                        while r > 15 and k <= eob:
                            emit_eobrun()
                            t.append(("s", 0, 0xF0))
                            r -= 16
                            t.extend(br)
                            br = []
                        if a > 1:
                            br.append(("b", a & 1, 1))
                            continue
                        emit_eobrun()
                        t.append(("s", 0, (r << 4) | 1))
                        t.append(("b", 0 if z[k] < 0 else 1, 1))
                        t.extend(br)
                        br, r = [], 0
                    if r > 0 or br:
                        eobrun += 1
                        be += br
                        if eobrun == 0x7FFF or len(be) > 937:
                            emit_eobrun()
        emit_eobrun()
        out.append(t)
    return out


def write(comp_blocks, h, w, script, hs=2, vs=2, quant=None, optimise=False, comments=True):
    """A progressive stream.  comp_blocks: per component an int array [rows][cols][64] of QUANTISED coefficients in zigzag order,
    rows x cols the component's blocks padded to whole MCUs.  script: a list of scans, each a dict: comps (indices), ss, se, ah, al
    and optionally dri (a DRI segment in front of it), dc / ac (table ids, default 0 for luma and 1 for chroma), tokens (a list of
    interval token lists that stands for the encoded blocks), dqt (a DQT segment in front of it)."""
    comps = len(comp_blocks)
    if comps == 1:
        hs = vs = 1
    quant = quant or [[1 + (k // 8) for k in range(64)]] * 2      # zigzag order
    mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))

    def seg(m, body):
        return bytes([0xFF, m, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)

    out = bytearray(b"\xff\xd8")
    if comments:
        out += seg(0xFE, b"whenet scan writer")
    for i in range(2 if comps == 3 else 1):
        out += seg(0xDB, [i] + list(quant[i]))
    sof = [8, h >> 8, h & 255, w >> 8, w & 255, comps]
    for c in range(comps):
        sof += [c + 1, ((hs << 4) | vs) if c == 0 else 0x11, 0 if c == 0 else 1]
    out += seg(0xC2, sof)
    ri_now = 0
    for sc in script:
        cs = sc["comps"]
        if "dqt" in sc:
            out += seg(0xDB, [0] + list(quant[0]))
        if "dri" in sc:
            ri_now = sc["dri"]
            out += seg(0xDD, [ri_now >> 8, ri_now & 255])
        # the scan's units
        units = []
        if len(cs) > 1:
            for my in range(mcu_rows):
                for mx in range(mcu_cols):
                    unit = [(0, comp_blocks[0][my * vs + by][mx * hs + bx]) for by in range(vs) for bx in range(hs)]
                    unit += [(c, comp_blocks[c][my][mx]) for c in (1, 2)]
                    units.append(unit)
        else:
            c = cs[0]
            cw, ch = (w, h) if c == 0 or comps == 1 else (-(-w // hs), -(-h // vs))
            for by in range(-(-ch // 8)):
                for bx in range(-(-cw // 8)):
                    units.append([(0, comp_blocks[c][by][bx])])
        ri = ri_now if 0 < ri_now < len(units) else len(units)
        tokens = sc.get("tokens") or _scan_tokens(units, sc, ri)
        dc_scan, first = sc["ss"] == 0, sc.get("ah", 0) == 0
        ids = sc.get("dc" if dc_scan else "ac", [0 if c == 0 else 1 for c in cs])
        tables = {}
        if not (dc_scan and not first):
            for i, tid in enumerate(ids):
                if optimise:
                    freq = {}
                    for t in tokens:
                        for tok in t:
                            if tok[0] == "s" and ids[tok[1]] == tid:
                                freq[tok[2]] = freq.get(tok[2], 0) + 1
                    counts, vals = ranked_table(freq or {0: 1})
                else:
                    counts, vals = fixed_table(dc_scan)
                tables[i] = _enc_table(counts, vals)
                if not sc.get("no_dht"):
                    out += seg(0xC4, [((0 if dc_scan else 1) << 4) | tid] + counts + vals)
        sos = [len(cs)]
        for i, c in enumerate(cs):
            tid = ids[i] if i < len(ids) else 0
            sos += [c + 1, (tid << 4) if dc_scan else tid]
        out += seg(0xDA, sos + [sc["ss"], sc["se"], (sc.get("ah", 0) << 4) | sc["al"]])
        for i, t in enumerate(tokens):
            o = _Out()
            for tok in t:
                if tok[0] == "s":
                    code, length = tables[tok[1]][tok[2]]
                    o.put(code, length)
                else:
                    o.put(tok[1], tok[2])
            out += o.flush()
            if i + 1 < len(tokens):
                out += bytes([0xFF, 0xD0 + (i & 7)])
    out += b"\xff\xd9"
    return bytes(out)


# ---- pictures and the case table -------------------------------------------------------------------------------------------------
def picture(h, w, seed=0, noise=10.0):
    """a seeded RGB picture of moderate contrast (its coefficients stay off the +-2048 clamp at every quality)"""
    rng = np.random.default_rng(1000 * seed + 7 * h + w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 60 * np.sin(x / 5.0 + seed) * np.cos(y / 7.0), 90 + 0.5 * ((3 * x + 5 * y) % 150), 70 + 110 * ((x // 5 + y // 3) % 2)], -1)
    return np.clip(base + rng.normal(0, noise, (h, w, 3)), 0, 255).astype(np.uint8)


def pillow_stream(h, w, sub, quality, progressive=True, picture_of=picture, **kw):
    """sub: 0 (4:4:4), 1 (4:2:2), 2 (4:2:0) or 'grey'"""
    from PIL import Image
    im = Image.fromarray(picture_of(h, w))
    args = dict(quality=quality, **kw)
    if sub == "grey":
        im = im.convert("L")
    else:
        args["subsampling"] = sub
    if progressive:
        args["progressive"] = True
    else:
        args["optimize"] = True
    out = io.BytesIO()
    im.save(out, "JPEG", **args)
    return out.getvalue()


SIZES = [(1, 1), (8, 8), (7, 9), (17, 17), (18, 33), (50, 35), (48, 64)]      # (h, w)
SUBS = {"444": 0, "422": 1, "420": 2, "grey": "grey"}
DRIS = {"nodri": {}, "blocks3": {"restart_marker_blocks": 3}, "rows1": {"restart_marker_rows": 1}}


def _pillow_table():
    """every size x sampling at quality 75 and every restart setting; every quality at 17 x 17 and 50 x 35 without DRI and with
    3-block intervals"""
    t = {}
    for h, w in SIZES:
        for sn, sub in SUBS.items():
            for dn, kw in DRIS.items():
                t[f"pil_{sn}_{w}x{h}_q75_{dn}"] = (h, w, sub, 75, kw)
            if (h, w) in ((17, 17), (50, 35)):
                for q in (30, 95, 100):
                    for dn in ("nodri", "blocks3"):
                        t[f"pil_{sn}_{w}x{h}_q{q}_{dn}"] = (h, w, sub, q, DRIS[dn])
    return t


PILLOW = _pillow_table()
PILLOW_NAMES = list(PILLOW)


@functools.lru_cache(maxsize=None)
def pillow_case(name):
    h, w, sub, q, kw = PILLOW[name]
    return pillow_stream(h, w, sub, q, **kw)


@functools.lru_cache(maxsize=None)
def pillow_twin(name):
    """the baseline stream of the same picture, quality, sampling and DRI: it holds the same quantised coefficients"""
    h, w, sub, q, kw = PILLOW[name]
    return pillow_stream(h, w, sub, q, progressive=False, **kw)


@functools.lru_cache(maxsize=None)
def flat_grey_1024():
    """1024 x 1024 of one level: 16,384 blocks whose AC scans are single long EOB runs"""
    return pillow_stream(1024, 1024, "grey", 75, picture_of=lambda h, w: np.full((h, w, 3), 97, np.uint8))


@functools.lru_cache(maxsize=None)
def noisy_q100(progressive=True):
    """quality 100 with noise of one level: many coefficients are 0 or +-1, so the last refinement meets runs of more than 15
    coefficients without a history in front of a new one (ZRL in a refinement scan); strong noise leaves no such run"""
    return pillow_stream(48, 64, 2, 100, progressive=progressive, picture_of=lambda h, w: picture(h, w, seed=3, noise=1.0))


def quantised(h, w, comps, hs=2, vs=2, seed=0, scale=1.0):
    """seeded quantised blocks for the scan writer: per component [rows][cols][64] zigzag, sparse, decaying with k, |DC| <= 200"""
    rng = np.random.default_rng(seed)
    if comps == 1:
        hs = vs = 1
    mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
    out = []
    for c in range(comps):
        rows, cols = mcu_rows * (vs if c == 0 else 1), mcu_cols * (hs if c == 0 else 1)
        mag = np.maximum(1, (40 * scale / (1 + np.arange(64) / 3.0))).astype(np.int64)
        z = rng.integers(-mag, mag + 1, (rows, cols, 64))
        z[rng.random((rows, cols, 64)) < 0.45] = 0
        z[..., 40:][rng.random((rows, cols, 24)) < 0.8] = 0
        z[..., 0] = rng.integers(-100, 101, (rows, cols))
        out.append(z)
    return out


def _script(comps, kind):
    cs = list(range(comps))
    each = [[c] for c in cs]
    if kind == "minimal":
        return [dict(comps=cs, ss=0, se=0, al=0)] + [dict(comps=c, ss=1, se=63, al=0) for c in each]
    if kind == "approx3":
        s = [dict(comps=cs, ss=0, se=0, al=3)] + [dict(comps=c, ss=1, se=63, al=3) for c in each]
        for a in (3, 2, 1):
            s += [dict(comps=cs, ss=0, se=0, ah=a, al=a - 1)] + [dict(comps=c, ss=1, se=63, ah=a, al=a - 1) for c in each]
        return s
    if kind == "bands":
        return [dict(comps=cs, ss=0, se=0, al=0)] + [dict(comps=c, ss=a, se=b, al=0) for c in each for a, b in ((1, 1), (2, 2), (3, 63))]
    if kind == "dc_split":
        return [dict(comps=c, ss=0, se=0, al=0) for c in each] + [dict(comps=c, ss=1, se=63, al=0) for c in each]
    if kind == "dri_changes":
        return [dict(comps=cs, ss=0, se=0, al=0, dri=2)] + [dict(comps=c, ss=1, se=63, al=1, dri=1 + i) for i, c in enumerate(each)] + \
               [dict(comps=c, ss=1, se=63, ah=1, al=0, dri=0 if i else 3) for i, c in enumerate(each)]
    if kind == "ids23":
        return [dict(comps=cs, ss=0, se=0, al=0, dc=[2, 3, 3][:comps])] + [dict(comps=c, ss=1, se=63, al=0, ac=[2 + (c[0] > 0)]) for c in each]
    if kind == "levels14":      # the deepest script there is: a chain of overlapping scans lowers Al at every step, 13 -> 0
        s = [dict(comps=cs, ss=0, se=0, al=2), dict(comps=[0], ss=1, se=63, al=13)]
        s += [dict(comps=[0], ss=1, se=63, ah=a, al=a - 1) for a in range(13, 0, -1)]
        s += [dict(comps=cs, ss=0, se=0, ah=2, al=1), dict(comps=cs, ss=0, se=0, ah=1, al=0)]
        return s + [dict(comps=c, ss=1, se=63, al=0) for c in each[1:]]
    raise KeyError(kind)


SCRIPTS = ("minimal", "approx3", "bands", "dc_split", "dri_changes", "ids23", "levels14")
SHAPES = {"420_17x17": (17, 17, 3), "grey_9x7": (7, 9, 1)}      # (h, w, components)
CONSTRUCTED_NAMES = [f"{k}_{s}_{t}" for k in SCRIPTS for s in SHAPES for t in ("fixed", "ranked")]


@functools.lru_cache(maxsize=None)
def constructed(name):
    kind, rest = next((k, name[len(k) + 1:]) for k in SCRIPTS if name.startswith(k + "_"))
    shape, tables = rest.rsplit("_", 1)
    h, w, comps = SHAPES[shape]
    scale = 35.0 if kind == "levels14" else 1.0      # (values of up to 11 bits: the scans above Al 10 are EOB runs)
    return write(quantised(h, w, comps, seed=len(name), scale=scale), h, w, _script(comps, kind), optimise=tables == "ranked")


# ---- refused streams: name -> bytes ----------------------------------------------------------------------------------------------
def _refused():
    z3, z1 = quantised(17, 17, 3), quantised(7, 9, 1)
    dc, ac = dict(comps=[0, 1, 2], ss=0, se=0, al=0), dict(comps=[0], ss=1, se=63, al=0)
    w3 = lambda script: write(z3, 17, 17, script)      # noqa: E731
    t = {
        "ss_above_se": w3([dc, dict(comps=[0], ss=5, se=4, al=0)]),
        "se_above_63": w3([dc, dict(comps=[0], ss=1, se=64, al=0)]),
        "dc_with_ac": w3([dict(comps=[0, 1, 2], ss=0, se=5, al=0)]),
        "interleaved_ac": w3([dc, dict(comps=[0, 1, 2], ss=1, se=63, al=0)]),
        "al_above_13": w3([dict(comps=[0, 1, 2], ss=0, se=0, al=14)]),
        "ah_above_13": w3([dict(comps=[0, 1, 2], ss=0, se=0, al=13), dict(comps=[0, 1, 2], ss=0, se=0, ah=14, al=13)]),
        "second_first_scan": w3([dc, ac, dict(comps=[0], ss=10, se=20, al=0)]),
        "refine_without_first": w3([dc, dict(comps=[0], ss=1, se=63, ah=1, al=0)]),
        "refine_wrong_ah": w3([dict(comps=[0, 1, 2], ss=0, se=0, al=2), dict(comps=[0, 1, 2], ss=0, se=0, ah=1, al=0)]),
        "refine_al_not_ah_minus_1": w3([dict(comps=[0, 1, 2], ss=0, se=0, al=2), dict(comps=[0, 1, 2], ss=0, se=0, ah=2, al=0)]),
        "ac_before_dc": w3([dict(comps=[1], ss=0, se=0, al=0), ac]),
        "missing_table": w3([dc, dict(comps=[0], ss=1, se=63, al=0, ac=[3], no_dht=True)]),
        "dqt_behind_sos": w3([dc, dict(comps=[0], ss=1, se=63, al=0, dqt=True)]),
        # 129 scans, each one the script allows: DC from Al 13 down (14), 63 single-coefficient AC bands at Al 1, 52 of them refined
        "scans_129": write(z1, 7, 9, [dict(comps=[0], ss=0, se=0, al=13)] + [dict(comps=[0], ss=0, se=0, ah=a, al=a - 1) for a in range(13, 0, -1)] +
                           [dict(comps=[0], ss=k, se=k, al=1) for k in range(1, 64)] + [dict(comps=[0], ss=k, se=k, ah=1, al=0) for k in range(1, 53)]),
    }
    two = bytearray(w3([dc, ac]))      # Ns = 2: the first SOS rewritten by hand
    p = two.find(b"\xff\xda")
    two[p:p + 14] = bytes([0xFF, 0xDA, 0, 10, 2, 1, 0x00, 2, 0x11, 0, 0, 0])
    t["ns_2"] = bytes(two)
    return t


REFUSED = _refused()


# ---- damaged streams: name -> bytes; the statement says what they decode to ------------------------------------------------------
def _base10():
    return pillow_stream(50, 35, 1, 75, restart_marker_blocks=3)      # 4:2:2, ten scans, 7 and 12 intervals


def _damaged():
    base = _base10()
    _, scans, _ = parse(base)
    assert len(scans) == 10
    t = {}
    for i, sc in enumerate(scans):
        t[f"truncated_in_scan_{i}"] = base[:(sc["start"] + sc["end"]) // 2]
    t["cut_before_last_two_scans"] = base[:scans[7]["end"]] + b"\xff\xd9"
    t["incomplete_no_eoi"] = base[:scans[7]["end"]]
    s3 = scans[3]
    m = s3["marks"]
    wrong = bytearray(base)
    wrong[m[1][0] + 1] = 0xD5
    t["wrong_rst_scan_3"] = bytes(wrong)
    t["missing_rst_scan_3"] = base[:m[2][0]] + base[m[2][0] + 2:]
    t["extra_rst_scan_3"] = base[:s3["end"]] + bytes([0xFF, 0xD0 + len(m) % 8]) + base[s3["end"]:]
    z = quantised(7, 9, 1, seed=5)
    dc = dict(comps=[0], ss=0, se=0, al=0)
    wz = lambda script: write(z, 7, 9, script)      # noqa: E731
    t["noncode"] = wz([dc, dict(comps=[0], ss=1, se=63, al=0, tokens=[[("b", 0xFFFF, 16)]])])
    t["run_past_se"] = wz([dc, dict(comps=[0], ss=1, se=5, al=0, tokens=[[("s", 0, 0x61), ("b", 1, 1)]]), dict(comps=[0], ss=6, se=63, al=0)])
    first = dict(comps=[0], ss=1, se=63, al=1)
    t["s2_in_refinement"] = wz([dc, first, dict(comps=[0], ss=1, se=63, ah=1, al=0, tokens=[[("s", 0, 0x02), ("b", 1, 1)]])])
    t["eobrun_past_interval"] = wz([dc, dict(comps=[0], ss=1, se=63, al=0, tokens=[[("s", 0, 0x20), ("b", 0, 2)]])])
    t["ends_in_correction_bits"] = wz([dc, first, dict(comps=[0], ss=1, se=63, ah=1, al=0, tokens=[[("s", 0, 0x00)]])])
    return t


DAMAGED = _damaged()
DAMAGED_NAMES = list(DAMAGED)
