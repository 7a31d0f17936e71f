"""Rule 1 of the JPEG decoder (include/whenet_hip.h, JPEG DECODER, RULE 1: libjpeg's bytes) as a numpy statement, and the streams
of the rule-1 tests.

The statement is written from the header's paragraph and shares no code with csrc/jpeg_dec_host.h.  It starts from the dequantised,
clamped coefficients of tests/jpeg_decode_cases.decode (shared by both rules) and states the three things rule 1 changes: the
inverse DCT, the chroma upsampling and the colour row.

    frame(decoded, bgr) -> uint8 [h,w,3]       # decoded: jpeg_decode_cases.decode(data) or .statement(name)
    pillow(data) -> uint8 [h,w,3] RGB          # the executed pin: Pillow's bundled libjpeg-turbo with its defaults
    SWEEP: the 576 (sampling, h, w) of the size sweep; sweep_stream(s, h, w) -> bytes
"""
import functools
import io

import numpy as np

from tests import jpeg_decode_cases as DC


def _pass(i, shift):
    """one 8-point pass along the last axis (int64), descaled"""
    i = [i[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], -1)
    return (out + (1 << (shift - 1))) >> shift


def idct(coef):
    """[blocks][64] coefficients (natural order) -> [blocks][8][8] samples"""
    c = np.asarray(coef, np.int64).reshape(-1, 8, 8)
    cols = _pass(c.transpose(0, 2, 1), 11).transpose(0, 2, 1)      # pass 1 runs down the columns
    return np.clip(_pass(cols, 18) + 128, 0, 255).astype(np.uint8)


def planes(dec):
    """the component planes of rule 1's inverse DCT, cropped to ceil(h / vs) x ceil(w / hs)"""
    return DC._place(dec.header, idct(dec.coef), np.uint8)


def upsample(p, hs, vs, h, w):
    """a chroma plane [ch,cw] -> [h,w] by libjpeg's fancy upsampling (replication where cw <= 2)"""
    p = p.astype(np.int64)
    ch, cw = p.shape
    if hs == 1:
        return p[:h, :w]
    if cw <= 2:
        return p[np.arange(h) >> (vs - 1)][:, np.arange(w) >> 1]
    if vs == 2:
        r = np.arange(ch)
        s = np.empty((2 * ch, cw), np.int64)
        s[0::2] = 3 * p + p[np.maximum(r - 1, 0)]
        s[1::2] = 3 * p + p[np.minimum(r + 1, ch - 1)]
        bias, shift = (8, 7), 4
    else:
        s, bias, shift = p, (1, 2), 2
    i = np.arange(cw)
    out = np.empty((s.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (3 * s + s[:, np.maximum(i - 1, 0)] + bias[0]) >> shift
    out[:, 1::2] = (3 * s + s[:, np.minimum(i + 1, cw - 1)] + bias[1]) >> shift
    return out[:h, :w]


def F(x):
    return int(x * 65536 + 0.5)


def frame(dec, bgr=True):
    hd = dec.header
    pl = planes(dec)
    y = pl[0].astype(np.int64)
    if hd.comps == 1:
        return np.repeat(pl[0][..., None], 3, axis=2)
    d = upsample(pl[1], hd.hs, hd.vs, hd.h, hd.w) - 128
    e = upsample(pl[2], hd.hs, hd.vs, hd.h, hd.w) - 128
    r = np.clip(y + ((F(1.402) * e + 32768) >> 16), 0, 255)
    b = np.clip(y + ((F(1.772) * d + 32768) >> 16), 0, 255)
    g = np.clip(y + ((-F(0.34414) * d + 32768 - F(0.71414) * e) >> 16), 0, 255)
    return np.stack([b, g, r] if bgr else [r, g, b], -1).astype(np.uint8)


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(data))).convert("RGB"))


def off_the_clamp(dec):
    """the condition of rule 1's claim: no dequantised coefficient of the stream sits at the -2048..2047 clamp"""
    return -2048 < int(dec.coef.min()) and int(dec.coef.max()) < 2047


# the size sweep: every (sampling, h, w); cw <= 2 (replication), cw = 3 (the first filtered width), both vertical clamps, sizes
# around one and two MCUs
SWEEP_H = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18)
SWEEP_W = tuple(range(1, 10)) + (15, 16, 17, 18) + (31, 32, 33)
SWEEP = [(s, h, w) for s in (0, 1, 2) for h in SWEEP_H for w in SWEEP_W]
assert len(SWEEP) == 576


def sweep_stream(s, h, w):
    return DC.pillow_stream(h, w, subsampling=s, quality=92, seed=h * w)


@functools.lru_cache(maxsize=None)
def statement_frame(name, bgr=True):
    """the numpy statement's rule-1 frame of a case or a damaged case of jpeg_decode_cases: computed once, shared, never modified"""
    out = frame(DC.statement(name), bgr)
    out.setflags(write=False)
    return out
