"""The JPEG decoder's LAYOUTS section (include/whenet_hip.h, JPEG DECODER, LAYOUTS) as a numpy / Python statement, a writer of
sequential streams, and the case table of its tests.

The statement is written from the header and shares no code with csrc/: the markers are walked with Python integers, the Huffman
codes are matched bit by bit (tests/jpeg_decode_cases._Bits), the MCU walk is a plain loop over (component, block row, block column).
Pillow cannot write the samplings of this section (its subsampling="4:1:1" writes 2x2), so every stream here comes from the writer.

    write(blocks, h, w, hs, vs, groups=..., sof=0xC0, ...) -> bytes      # quantised blocks -> a sequential stream (SOF0 / SOF1)
    decode(data) -> Seq(header, coef, status, scans)      # any number of scans; coef [blocks][64] dequantised, clamped, natural order
    planes(dec, rule) -> [Y, Cb, Cr];  upsampled(dec, rule) -> [h,w] Cb, Cr;  frame(dec, rule, bgr) -> uint8 [h,w,3]
    blocks_of(h, w, hs, vs) -> the quantised blocks of a noisy picture (every coefficient off the +-2048 clamp)
    SINGLE / SOF1 / SOF2 / MULTI / REFUSED / DAMAGED: name -> bytes
"""
import functools
import io
from collections import namedtuple

import numpy as np

from tests import jpeg_decode_cases as DC
from tests import jpeg_exact_cases as EX
from tests import jpeg_prog_cases as PC

OK, EFORMAT = DC.OK, DC.EFORMAT
ZIGZAG = DC.ZIGZAG
Seq = namedtuple("Seq", "header coef status scans")

QUANT = [[2 + (k // 6) for k in range(64)], [3 + (k // 4) for k in range(64)]]      # zigzag order: luma, chroma


# ---- pictures -> quantised blocks ------------------------------------------------------------------------------------------------
def blocks_of(h, w, hs, vs, comps=3, seed=0, quant=QUANT, picture_of=PC.picture):
    """per component an int array [rows][cols][64] of quantised coefficients in zigzag order, rows x cols the component's blocks
    padded to whole MCUs: the float DCT of PC.picture (noise of 10 levels), chroma box-averaged over hs x vs.  |coefficient x Q| stays
    below 1100: every stream of these blocks is off the +-2048 clamp."""
    if comps == 1:
        hs = vs = 1
    rgb = np.asarray(picture_of(h, w, seed), np.float64)      # (R, G, B)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    full = [0.299 * r + 0.587 * g + 0.114 * b, 128 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128 + 0.5 * r - 0.418688 * g - 0.081312 * b][:comps]
    mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
    H, W = mcu_rows * 8 * vs, mcu_cols * 8 * hs
    out = []
    for c, p in enumerate(full):
        p = np.pad(p, ((0, H - h), (0, W - w)), mode="edge")
        if c > 0:
            p = p.reshape(H // vs, vs, W // hs, hs).mean(axis=(1, 3))
        rows, cols = p.shape[0] // 8, p.shape[1] // 8
        blk = p.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3) - 128.0
        f = np.einsum("vy,rcyx,ux->rcvu", DC.DCT_F, blk, DC.DCT_F).reshape(rows, cols, 64)      # natural order
        q = np.array(quant[min(c, 1)], np.float64)
        out.append(np.rint(f[..., ZIGZAG] / q).astype(np.int64))
    return out


# ---- the writer ------------------------------------------------------------------------------------------------------------------
def _block_tokens(z, pred, i):
    """the tokens of one sequential block (T.81 F.1.2): ('s', table slot 2 i + class, symbol) | ('b', value, nbits)"""
    t = []
    d = int(z[0]) - pred
    n = int(abs(d)).bit_length()
    t.append(("s", 2 * i, n))
    if n:
        t.append(("b", d if d >= 0 else d + (1 << n) - 1, n))
    r = 0
    for k in range(1, 64):
        v = int(z[k])
        if v == 0:
            r += 1
            continue
        while r > 15:
            t.append(("s", 2 * i + 1, 0xF0))
            r -= 16
        n = abs(v).bit_length()
        t.append(("s", 2 * i + 1, (r << 4) | n))
        t.append(("b", v if v >= 0 else v + (1 << n) - 1, n))
        r = 0
    if r:
        t.append(("s", 2 * i + 1, 0x00))
    return t


def scan_units(blocks, h, w, hs, vs, cs):
    """the MCUs of a sequential scan of the components cs: per unit a list of (index in the scan, component, block row, block column).
    Ns > 1 (and a grey frame): the FRAME's MCU grid, H_c x V_c blocks of each of the scan's components in scan order (T.81 A.2.3);
    one component of three: its own ceil(cw / 8) x ceil(ch / 8) blocks in raster order."""
    comps = len(blocks)
    mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
    units = []
    if len(cs) > 1 or comps == 1:
        for my in range(mcu_rows):
            for mx in range(mcu_cols):
                u = []
                for i, c in enumerate(cs):
                    if c == 0 and comps == 3:
                        u += [(i, 0, my * vs + by, mx * hs + bx) for by in range(vs) for bx in range(hs)]
                    else:
                        u.append((i, c, my, mx))
                units.append(u)
    else:
        c = cs[0]
        cw, ch = (w, h) if c == 0 else (-(-w // hs), -(-h // vs))
        units = [[(0, c, by, bx)] for by in range(-(-ch // 8)) for bx in range(-(-cw // 8))]
    return units


def write(blocks, h, w, hs=2, vs=2, groups=None, sof=0xC0, ids=None, dris=None, quant=QUANT, tokens=None, chroma_hv=(0x11, 0x11),
          sos_tail=(0, 63, 0), dqt16=False, dht=True, between=b"", annexk=False, luma_hv=None):
    """A sequential stream.  blocks: blocks_of()'s.  groups: the scans as lists of component indices (default: one interleaved scan).
    sof: 0xC0 or 0xC1.  ids: per component (DC id, AC id), default (0, 0) for luma and (1, 1) for chroma.  dris: per scan None or a
    restart interval (a DRI segment in front of that scan).  tokens: {scan index: [interval token lists]} in the place of the encoded
    blocks.  between: bytes put in front of every scan but the first (APPn / COM segments).  dht=False: no DHT segment at all.
    annexk=True: the codes are T.81 Annex K's (ids 0..1: what a player installs for a stream without DHT), not the writer's own."""
    comps = len(blocks)
    if comps == 1:
        hs = vs = 1
    groups = groups or [list(range(comps))]
    ids = ids or [(0, 0), (1, 1), (1, 1)][:comps]
    dris = dris or [None] * len(groups)

    def seg(m, body):
        return bytes([0xFF, m, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)

    out = bytearray(b"\xff\xd8") + seg(0xFE, b"whenet layout writer")
    for i in range(2 if comps == 3 else 1):
        if dqt16:
            out += seg(0xDB, [0x10 | i] + [b for v in quant[i] for b in (0, v)])
        else:
            out += seg(0xDB, [i] + list(quant[i]))
    body = [8, h >> 8, h & 255, w >> 8, w & 255, comps]
    for c in range(comps):
        body += [c + 1, (luma_hv or ((hs << 4) | vs)) if c == 0 else chroma_hv[c - 1], 0 if c == 0 else 1]      # (luma_hv: a refused header)
    out += seg(sof, body)
    def table(cls, tid):
        if not annexk:
            return PC.fixed_table(cls == 0)
        from tests import jpeg_default_tables_cases as DT
        t = DT.annex_k()[(cls, tid)]
        return list(t[1:17]), list(t[17:])

    for si, cs in enumerate(groups):
        if si and between:
            out += between
        if dris[si] is not None:
            out += seg(0xDD, [dris[si] >> 8, dris[si] & 255])
        if dht:
            for cls, tid in sorted({(0, ids[c][0]) for c in cs} | {(1, ids[c][1]) for c in cs}):
                counts, vals = table(cls, tid)
                out += seg(0xC4, [(cls << 4) | tid] + counts + vals)
        units = scan_units(blocks, h, w, hs, vs, cs)
        in_force = [d for d in dris[:si + 1] if d is not None]      # the DRI in force: this scan's, or an earlier scan's
        ri = in_force[-1] if in_force and 0 < in_force[-1] < len(units) else len(units)
        enc = {2 * i + cls: PC._enc_table(*table(cls, ids[c][cls])) for i, c in enumerate(cs) for cls in (0, 1)}
        sos = [len(cs)]
        for c in cs:
            sos += [c + 1, (ids[c][0] << 4) | ids[c][1]]
        out += seg(0xDA, sos + [sos_tail[0], sos_tail[1], sos_tail[2]])
        if tokens is not None and si in tokens:
            intervals = tokens[si]
        else:
            intervals = []
            for first in range(0, len(units), ri):
                t, pred = [], [0, 0, 0]
                for u in units[first:first + ri]:
                    for i, c, by, bx in u:
                        z = blocks[c][by][bx]
                        t += _block_tokens(z, pred[i], i)
                        pred[i] = int(z[0])
                intervals.append(t)
        for k, t in enumerate(intervals):
            o = PC._Out()
            for tok in t:
                if tok[0] == "s":
                    code, length = enc[tok[1]][tok[2]]
                    o.put(code, length)
                else:
                    o.put(tok[1], tok[2])
            out += o.flush()
            if k + 1 < len(intervals):
                out += bytes([0xFF, 0xD0 + (k & 7)])
    out += b"\xff\xd9"
    return bytes(out)


# ---- the statement: parse and entropy decode -------------------------------------------------------------------------------------
def parse(data):
    """(Header, scans): a sequential frame (SOF0 / SOF1) with any number of scans.  Raises DC.Refused for anything else."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise DC.Refused("no SOI")
    p, frame, q, huff, dri, scans, ids, seen = 2, None, {}, {}, 0, [], [], set()
    while p + 4 <= len(data):
        if data[p] != 0xFF:
            raise DC.Refused("no marker")
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0xD9:
            break
        n = ((data[p + 2] << 8) | data[p + 3]) - 2
        s = data[p + 4:p + 4 + n]
        p += 4 + n
        if p > len(data):
            break
        if m in (0xC0, 0xC1):
            if frame is not None or s[0] != 8:
                raise DC.Refused("frame header")
            h, w, comps = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            ids = [s[6 + 3 * c] for c in range(comps)]
            hv = [s[7 + 3 * c] for c in range(comps)]
            qt = [s[8 + 3 * c] for c in range(comps)]
            if comps == 3 and ((hv[0] >> 4) not in (1, 2, 4) or (hv[0] & 15) not in (1, 2) or hv[1] != 0x11 or hv[2] != 0x11):
                raise DC.Refused("sampling")
            hs, vs = (hv[0] >> 4, hv[0] & 15) if comps == 3 else (1, 1)
            frame = (h, w, comps, hs, vs, qt)
        elif 0xC0 <= m <= 0xCF and m != 0xC4:
            raise DC.Refused("not a sequential Huffman frame")
        elif m == 0xDB:
            i = 0
            while i < n:
                if s[i] >> 4:
                    raise DC.Refused("16-bit DQT")
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = s[i + 1 + k]
                q[s[i] & 15] = nat
                i += 65
        elif m == 0xC4:
            i = 0
            while i < n:
                counts = list(s[i + 1:i + 17])
                huff[(s[i] >> 4, s[i] & 15)] = PC._codes(counts, list(s[i + 17:i + 17 + sum(counts)]))
                i += 17 + sum(counts)
        elif m == 0xDD:
            dri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            h, w, comps, hs, vs, qt = frame
            ns = s[0]
            cs = [ids.index(s[1 + 2 * i]) for i in range(ns)]
            if tuple(s[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise DC.Refused("a sequential scan is Ss 0, Se 63, Ah = Al = 0")
            if seen & set(cs):
                raise DC.Refused("a component in two scans")
            seen |= set(cs)
            tabs = [(huff.get((0, s[2 + 2 * i] >> 4)), huff.get((1, s[2 + 2 * i] & 15))) for i in range(ns)]
            if any(a is None or b is None for a, b in tabs):
                raise DC.Refused("missing DHT")
            bpm = hs * vs + 2 if comps == 3 else 1
            mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
            units = []      # per unit: (index in the scan, the block's record)
            if ns > 1 or comps == 1:
                for mm in range(mcu_cols * mcu_rows):
                    u = []
                    for i, c in enumerate(cs):
                        if c == 0 and comps == 3:
                            u += [(i, mm * bpm + b) for b in range(hs * vs)]
                        else:
                            u.append((i, mm * bpm + (bpm - 2 + c - 1 if comps == 3 else 0)))
                    units.append(u)
            else:
                c = cs[0]
                cw, ch = (w, h) if c == 0 else (-(-w // hs), -(-h // vs))
                for by in range(-(-ch // 8)):
                    for bx in range(-(-cw // 8)):
                        if c == 0:
                            units.append([(0, ((by // vs) * mcu_cols + bx // hs) * bpm + (by % vs) * hs + bx % hs)])
                        else:
                            units.append([(0, (by * mcu_cols + bx) * bpm + bpm - 2 + c - 1)])
            ri = dri if 0 < dri < len(units) else len(units)
            end, marks = PC._scan_end(data, p)
            scans.append(dict(comps=cs, tabs=tabs, units=units, ri=ri, intervals=-(-len(units) // ri), start=p, end=end, marks=marks, dri=dri,
                              q=[q[qt[c]] for c in cs]))
            p = end
    h, w, comps, hs, vs, qt = frame
    mcu_cols, mcu_rows = -(-w // (8 * hs)), -(-h // (8 * vs))
    hd = DC.Header(h, w, comps, hs, vs, qt, [0] * 3, [0] * 3, scans[0]["dri"], scans[0]["intervals"], scans[0]["start"], q, huff, mcu_cols,
                   mcu_rows, hs * vs + 2 if comps == 3 else 1)
    return hd, scans, len(seen) == comps


def _block(br, dct, act, q, pred, out):
    pred = DC.clamp(pred + br.value(br.symbol(dct) & 15), -32768, 32767)
    out[0] = DC.clamp(pred * q[0], -2048, 2047)
    k = 1
    while k < 64:
        sym = br.symbol(act)
        r, s = sym >> 4, sym & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            if k > 64:
                raise DC._Damage
            continue
        k += r
        if k > 63:
            raise DC._Damage
        out[ZIGZAG[k]] = DC.clamp(br.value(s) * q[ZIGZAG[k]], -2048, 2047)
        k += 1
    return pred


@functools.lru_cache(maxsize=None)
def decode(data):
    """Items are numbered scan by scan, one per restart interval; status[1] = the smallest bad item, or the item count where a
    component has no scan at EOI (its planes come from zero coefficients).  One scan: the item is the restart interval."""
    data = bytes(data)
    hd, scans, complete = parse(data)
    coef = [[0] * 64 for _ in range(hd.mcu_cols * hd.mcu_rows * hd.bpm)]
    bad, items = None, 0
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
            br = DC._Bits(DC._interval_bits(data[:sc["end"]], sc["start"] if i == 0 else marks[i - 1][0] + 2))
            pred = [0, 0, 0]
            try:
                for u in sc["units"][i * sc["ri"]:(i + 1) * sc["ri"]]:
                    for ci, rec in u:
                        pred[ci] = _block(br, sc["tabs"][ci][0], sc["tabs"][ci][1], sc["q"][ci], pred[ci], coef[rec])
            except DC._Damage:
                sbad = i if sbad is None else min(sbad, i)
        if sbad is not None and bad is None:
            bad = items + sbad
        items += n
    if bad is None and not complete:
        bad = items
    coef = np.array(coef, np.int64)
    status = np.array([OK, -1] if bad is None else [EFORMAT, bad], np.int32)
    coef.setflags(write=False), status.setflags(write=False)
    return Seq(hd, coef, status, scans)


def off_the_clamp(dec):
    return -2048 < int(dec.coef.min()) and int(dec.coef.max()) < 2047


# ---- the statement: planes and frame under both rules ----------------------------------------------------------------------------
def planes(dec, rule):
    return DC._place(dec.header, EX.idct(dec.coef) if rule else DC.idct_int(dec.coef), np.uint8)


def _log2(f):
    return {1: 0, 2: 1, 4: 2}[f]


def upsample(p, hs, vs, h, w, rule):
    """a chroma plane [ch,cw] -> [h,w].  Rule 0: the sample (x >> log2 hs, y >> log2 vs).  Rule 1: jdsample.c -- hs = 4 replication
    in both directions; 4:4:0 the vertical triangle alone, at every width; hs = 2 what jpeg_exact_cases states."""
    p = p.astype(np.int64)
    ch, cw = p.shape
    if rule == 0 or hs == 4:
        return p[np.arange(h) >> _log2(vs)][:, np.arange(w) >> _log2(hs)]
    if hs == 1 and vs == 2:
        r = np.arange(ch)
        s = np.empty((2 * ch, cw), np.int64)
        s[0::2] = (3 * p + p[np.maximum(r - 1, 0)] + 1) >> 2
        s[1::2] = (3 * p + p[np.minimum(r + 1, ch - 1)] + 2) >> 2
        return s[:h, :w]
    return EX.upsample(p, hs, vs, h, w)


def upsampled(dec, rule):
    hd = dec.header
    pl = planes(dec, rule)
    return [upsample(pl[c], hd.hs, hd.vs, hd.h, hd.w, rule) for c in (1, 2)]


def frame(dec, rule, bgr=True):
    hd = dec.header
    pl = planes(dec, rule)
    if hd.comps == 1:
        return np.repeat(pl[0][..., None], 3, axis=2)
    y = pl[0].astype(np.int64)
    d, e = [u - 128 for u in upsampled(dec, rule)]
    if rule:
        F = EX.F
        r = np.clip(y + ((F(1.402) * e + 32768) >> 16), 0, 255)
        b = np.clip(y + ((F(1.772) * d + 32768) >> 16), 0, 255)
        g = np.clip(y + ((-F(0.34414) * d + 32768 - F(0.71414) * e) >> 16), 0, 255)
    else:
        yoff, cy, cvr, cug, cvg, cub = DC.JFIF
        base = cy * np.maximum(y - yoff, 0) + (1 << 19)
        r = np.clip((base + cvr * e) >> 20, 0, 255)
        g = np.clip((base - cug * d - cvg * e) >> 20, 0, 255)
        b = np.clip((base + cub * d) >> 20, 0, 255)
    return np.stack([b, g, r] if bgr else [r, g, b], -1).astype(np.uint8)


def pillow_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(data))).convert("RGB"))


def pillow_ycc(data, mode="YCbCr"):
    """the executed library's own planes, chroma upsampled, no colour conversion: uint8 [h,w,3] (mode "L", a grey stream: [h,w])"""
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(data)))
    im.draft(mode, im.size)
    im.load()
    assert im.mode == mode
    return np.asarray(im)


# ---- the case table --------------------------------------------------------------------------------------------------------------
SAMPLINGS = {"440": (1, 2), "411": (4, 1), "410": (4, 2)}      # the new luma (hs, vs)
SHAPES = [(1, 1), (1, 8), (3, 8), (17, 2), (15, 31), (17, 33), (16, 32), (33, 65)]      # (h, w); MCUs are 8 hs x 8 vs
GPU_SHAPES = [(15, 31), (17, 33), (33, 65)]


def _name(s, h, w):
    return f"{s}_{w}x{h}"


@functools.lru_cache(maxsize=None)
def _blocks(s, h, w):
    hs, vs = SAMPLINGS.get(s, {"420": (2, 2), "422": (2, 1), "444": (1, 1), "grey": (1, 1)}.get(s))
    return blocks_of(h, w, hs, vs, comps=1 if s == "grey" else 3, seed=h + w), hs, vs


def _dri_of(i, h, w):
    """DRI 1 and 3 on some streams and none on others"""
    return [None, 1, 3][i % 3]


# one interleaved scan, SOF0, ids <= 1: the baseline decoder's streams (both entropy forms)
SINGLE_NAMES = [_name(s, h, w) for s in SAMPLINGS for (h, w) in SHAPES]


@functools.lru_cache(maxsize=None)
def single(name):
    s, rest = name.split("_")
    w, h = map(int, rest.split("x"))
    b, hs, vs = _blocks(s, h, w)
    return write(b, h, w, hs, vs, dris=[_dri_of(SINGLE_NAMES.index(name), h, w)])


# SOF1 that qualifies for the baseline decoder (8 bit, one interleaved scan, ids 0..1)
SOF1_NAMES = [_name(s, 17, 33) + "_sof1" for s in SAMPLINGS] + ["420_33x17_sof1", "grey_33x17_sof1"]


@functools.lru_cache(maxsize=None)
def sof1(name):
    s, rest, _ = name.split("_")
    w, h = map(int, rest.split("x"))
    b, hs, vs = _blocks(s, h, w)
    return write(b, h, w, hs, vs, sof=0xC1, dris=[2 if s == "411" else None])


# SOF2 with the new samplings: the scan writer of jpeg_prog_cases on the same quantised blocks; `sof2_twin` is the sequential stream
# of those blocks, whose statement is the SOF2 stream's (the scripts reach Al = 0 for every coefficient: no value is lost)
SOF2_NAMES = [_name(s, h, w) + "_" + k for s in SAMPLINGS for (h, w) in ((17, 33), (15, 31)) for k in ("minimal", "dc_split", "dri_changes")]


@functools.lru_cache(maxsize=None)
def sof2(name):
    s, rest, kind = name.split("_", 2)
    w, h = map(int, rest.split("x"))
    b, hs, vs = _blocks(s, h, w)
    return PC.write(b, h, w, PC._script(3, kind), hs=hs, vs=vs, quant=QUANT)


@functools.lru_cache(maxsize=None)
def sof2_twin(name):
    s, rest, _ = name.split("_", 2)
    w, h = map(int, rest.split("x"))
    b, hs, vs = _blocks(s, h, w)
    return write(b, h, w, hs, vs)


# sequential frames that go through the scan plan: several scans, scans of two components, Huffman ids 2 / 3, SOF1
GROUPS = {"y_cb_cr": [[0], [1], [2]], "cb_cr_y": [[1], [2], [0]], "y_cbcr": [[0], [1, 2]], "ycb_cr": [[0, 1], [2]]}
IDS23 = [(2, 3), (3, 2), (3, 2)]


def plain(s, h, w):
    """one interleaved SOF0 scan of an old sampling ('420', '422', '444', 'grey'): what every call accepts"""
    b, hs, vs = _blocks(s, h, w)
    return write(b, h, w, hs, vs)


def _multi_table():
    t = {}
    for s in list(SAMPLINGS) + ["420", "422"]:
        for h, w in ((17, 33),) if s in ("420", "422") else SHAPES:
            for gi, (gn, groups) in enumerate(GROUPS.items()):      # every grouping at every shape of every new sampling
                dris = [[None, 1, 3][(gi + k + h) % 3] for k in range(len(groups))]      # DRI 1 and 3 on some scans, none on others
                t[f"{s}_{w}x{h}_{gn}"] = dict(s=s, h=h, w=w, groups=groups, dris=dris)
    for s in SAMPLINGS:
        t[f"{s}_33x17_y_cbcr_ids23"] = dict(s=s, h=17, w=33, groups=GROUPS["y_cbcr"], ids=IDS23, sof=0xC1, dris=[2, None])
        t[f"{s}_33x17_one_scan_ids23"] = dict(s=s, h=17, w=33, groups=[[0, 1, 2]], ids=IDS23, sof=0xC1)
    t["420_33x17_one_scan_sof0_ids23"] = dict(s="420", h=17, w=33, groups=[[0, 1, 2]], ids=IDS23)
    t["grey_33x17_ids2"] = dict(s="grey", h=17, w=33, groups=[[0]], ids=[(2, 2)], sof=0xC1, dris=[3])
    t["411_33x17_segments_between"] = dict(s="411", h=17, w=33, groups=GROUPS["y_cb_cr"], between=b"\xff\xfe\x00\x05abc\xff\xe5\x00\x04xy")
    return t


MULTI = _multi_table()
MULTI_NAMES = list(MULTI)


@functools.lru_cache(maxsize=None)
def multi(name):
    if name in MULTI_DAMAGED:
        return MULTI_DAMAGED[name]
    kw = dict(MULTI[name])
    b, hs, vs = _blocks(kw.pop("s"), kw["h"], kw["w"])
    return write(b, kw.pop("h"), kw.pop("w"), hs, vs, **kw)


def _multi_damaged():
    b, hs, vs = _blocks("440", 17, 33)
    three = write(b, 17, 33, hs, vs, groups=GROUPS["y_cb_cr"], dris=[2, None, None])
    scans = parse(three)[1]
    t = {"truncated_in_scan_2": three[:(scans[1]["start"] + scans[1]["end"]) // 2],
         "missing_last_scan": three[:scans[1]["end"]] + b"\xff\xd9",
         "noncode_in_scan_1": write(b, 17, 33, hs, vs, groups=GROUPS["y_cb_cr"], tokens={0: [[("b", 0xFFFF, 16)]]}),
         "run_past_63_in_scan_3": write(b, 17, 33, hs, vs, groups=GROUPS["y_cb_cr"],
                                        tokens={2: [[("s", 0, 0)] + [("s", 1, 0xF1), ("b", 1, 1)] * 4]})}
    wrong = bytearray(three)
    wrong[scans[0]["marks"][1][0] + 1] = 0xD6
    t["wrong_rst_in_scan_1"] = bytes(wrong)
    return t


MULTI_DAMAGED = _multi_damaged()
MULTI_DAMAGED_NAMES = list(MULTI_DAMAGED)


@functools.lru_cache(maxsize=None)
def annexk_411():
    """a 4:1:1 stream coded with T.81's Annex K tables: what a DV-derived camera's MJPG frame is once its DHT is put back"""
    b, hs, vs = _blocks("411", 33, 65)
    return write(b, 33, 65, hs, vs, annexk=True, dris=[2])


# a SOF2 frame whose DC scans hold two components (Ns = 2): the scan writer of jpeg_prog_cases with this module's tokens for them
@functools.lru_cache(maxsize=None)
def sof2_ns2(s="411", h=17, w=33, first=(0, 1)):
    b, hs, vs = _blocks(s, h, w)
    rest = [c for c in range(3) if c not in first]
    script = []
    for cs, al, ah in ((list(first), 1, 0), (rest, 1, 0), (list(first), 0, 1), (rest, 0, 1)):
        sc = dict(comps=cs, ss=0, se=0, al=al, ah=ah)
        units = [[(i, b[c][by][bx]) for i, c, by, bx in u] for u in scan_units(b, h, w, hs, vs, cs)]
        sc["tokens"] = PC._scan_tokens(units, sc, len(units))
        script.append(sc)
    script += [dict(comps=[c], ss=1, se=63, al=0) for c in range(3)]
    return PC.write(b, h, w, script, hs=hs, vs=vs, quant=QUANT)


def _refused():
    b, hs, vs = _blocks("411", 17, 33)
    return {
        "chroma_2x1": (write(b, 17, 33, hs, vs, chroma_hv=(0x21, 0x21)), "chroma sampling factors other than 1x1"),
        "cb_cr_differ": (write(b, 17, 33, hs, vs, chroma_hv=(0x11, 0x12)), "Cb and Cr sampling factors that differ"),
        "vs_4": (write(b, 17, 33, hs, vs, luma_hv=0x14), "vs = 4"),
        "luma_3x1": (write(b, 17, 33, hs, vs, luma_hv=0x31), "luma sampling factors other than"),
        "se_5": (write(b, 17, 33, hs, vs, sos_tail=(0, 5, 0)), "a spectral selection or successive approximation"),
        "al_1": (write(b, 17, 33, hs, vs, sos_tail=(0, 63, 1)), "a spectral selection or successive approximation"),
        "dqt_16bit": (write(b, 17, 33, hs, vs, dqt16=True), "a 16-bit quantiser table"),
        "component_twice": (write(b, 17, 33, hs, vs, groups=[[0], [1], [1], [2]]), "a component in two scans"),
        "scan_out_of_order": (write(b, 17, 33, hs, vs, groups=[[0], [2, 1]]), "not the frame's, in order"),
    }


REFUSED = _refused()


# damaged single-scan streams: name -> bytes; the statement says what they decode to
def _damaged():
    t = {}
    for s in SAMPLINGS:
        base = single(_name(s, 17, 33))
        hd, scans, _ = parse(base)
        sc = scans[0]
        t[f"{s}_truncated"] = base[:(sc["start"] + sc["end"]) // 2]
        b, hs, vs = _blocks(s, 17, 33)
        t[f"{s}_noncode"] = write(b, 17, 33, hs, vs, tokens={0: [[("b", 0xFFFF, 16)]]})
        t[f"{s}_run_past_63"] = write(b, 17, 33, hs, vs, tokens={0: [[("s", 0, 0), ("s", 1, 0xF1), ("b", 1, 1), ("s", 1, 0xF1), ("b", 1, 1), ("s", 1, 0xF1),
                                                                     ("b", 1, 1), ("s", 1, 0xF1), ("b", 1, 1)]]})
    b, hs, vs = _blocks("410", 33, 65)
    good = write(b, 33, 65, hs, vs, dris=[1])
    marks = parse(good)[1][0]["marks"]
    wrong = bytearray(good)
    wrong[marks[1][0] + 1] = 0xD5
    t["410_wrong_rst"] = bytes(wrong)
    t["410_missing_rst"] = good[:marks[2][0]] + good[marks[2][0] + 2:]
    return t


DAMAGED = _damaged()
DAMAGED_NAMES = list(DAMAGED)


def strip_dht(data):
    """the stream without its DHT segments (the MJPG frame of a UVC camera)"""
    data, out, p = bytes(data), bytearray(b"\xff\xd8"), 2
    while data[p + 1] != 0xDA:
        n = (data[p + 2] << 8) | data[p + 3]
        if data[p + 1] != 0xC4:
            out += data[p:p + 2 + n]
        p += 2 + n
    return bytes(out + data[p:])
