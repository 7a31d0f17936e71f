"""The packed 4:2:2 (YUYV / UYVY) -> BGR conversion of include/whenet_hip.h stated in numpy -- written from the header text, sharing
no code with the library or with tests/yuv_cases.py: the statement csrc/yuv.hip (kernel and host function) is held to, bit for bit
-- and the table of frames the tests run.

One plane: h rows of 4 cw bytes, cw = (w + 1) >> 1, `pitch` bytes apart.  YUYV: bytes Y0 U Y1 V per pixel pair; UYVY: U Y0 V Y1.
Pixel (y, x) takes luma Y[x & 1] of pair x >> 1 of row y and that pair's U and V: every row has its own chroma.  The last pair of an
odd row is whole in memory, its second luma byte is not used.  int32 arithmetic, >> arithmetic:

    c = max(0, Y - yoff);  d = U - 128;  e = V - 128
    R = clip8((CY c         + CVR e + 2^19) >> 20);  G = clip8((CY c - CUG d - CVG e + 2^19) >> 20);  B = clip8((CY c + CUB d + 2^19) >> 20)
"""
import numpy as np

YUYV, UYVY = 3, 4
FORMATS = (("yuyv", YUYV), ("uyvy", UYVY))
MATRICES = (("bt601", 0), ("bt709", 1), ("jfif", 2))
# yoff, CY, CVR, CUG, CVG, CUB: the three rows of WHENET_YUV_COEFFS as the header prints them
COEFFS = {0: (16, 1220542, 1673527, 409993, 852492, 2116026),
          1: (16, 1220945, 1879825, 223578, 558767, 2215014),
          2: (0, 1048576, 1470104, 360853, 748826, 1858077)}
EXTREMES = (0, 16, 128, 235, 240, 255)
GAP = 0xA5              # what lies between a row's last byte and the next row of a pitched frame

# what a wrong implementation would do, and the case that sees each (tests/test_yuv_packed_cpu.py asserts it per mutation)
MUTATIONS = ("yuyv_as_uyvy", "chroma_of_next_pair", "second_luma_first", "chroma_row_shared", "pitch_as_row")
SEEN_BY = {"yuyv_as_uyvy": "random_2x2", "chroma_of_next_pair": "random_3x5", "second_luma_first": "random_1x7",
           "chroma_row_shared": "rowchroma_2x2", "pitch_as_row": "random_pitched_64x130"}


def bgr_of_triples(Y, U, V, matrix):
    """The per-pixel arithmetic on int arrays of one shape -> uint8 [..., 3] in B, G, R order."""
    yoff, CY, CVR, CUG, CVG, CUB = COEFFS[matrix]
    c = np.maximum(0, Y.astype(np.int32) - yoff)
    d, e = U.astype(np.int32) - 128, V.astype(np.int32) - 128
    base = CY * c + (1 << 19)
    R = np.clip((base + CVR * e) >> 20, 0, 255)
    G = np.clip((base - CUG * d - CVG * e) >> 20, 0, 255)
    B = np.clip((base + CUB * d) >> 20, 0, 255)
    return np.stack([B, G, R], axis=-1).astype(np.uint8)


def packed_to_bgr(buf, pitch, fmt, matrix, h, w, mutation=None):
    """buf: the flat uint8 buffer of the plane, pitch: its row pitch -> uint8 [h, w, 3] in B, G, R order."""
    assert mutation is None or mutation in MUTATIONS
    buf = np.asarray(buf, np.uint8).reshape(-1)
    cw = (w + 1) >> 1
    if mutation == "pitch_as_row":
        pitch = 4 * cw
    if mutation == "yuyv_as_uyvy":
        fmt = UYVY if fmt == YUYV else YUYV
    y_at, u_at, v_at = (0, 1, 3) if fmt == YUYV else (1, 0, 2)
    yy, xx = np.mgrid[0:h, 0:w]
    pair = xx >> 1
    which = 1 - (xx & 1) if mutation == "second_luma_first" else xx & 1
    cpair = np.minimum(pair + 1, cw - 1) if mutation == "chroma_of_next_pair" else pair
    crow = yy & ~1 if mutation == "chroma_row_shared" else yy          # (the 4:2:0 rule: both rows of a pair take the first one's)
    Y = buf[yy * pitch + 4 * pair + y_at + 2 * which]
    U = buf[crow * pitch + 4 * cpair + u_at]
    V = buf[crow * pitch + 4 * cpair + v_at]
    return bgr_of_triples(Y, U, V, matrix)


# ---- the case table ---------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (2, 2), (1, 7), (7, 1), (3, 5), (2, 16), (5, 17), (10, 18), (33, 7))
PITCHED = dict(h=64, w=130, pitch=544)
KINDS = ("random", "extremes", "rowchroma")


def _seed(name):
    return 7300 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100000


def content(name, kind, h, w):
    """(Y [h, 2 cw], U [h, cw], V [h, cw]) of a case: the same picture for both formats.  rowchroma: the two rows of every row pair
    carry DIFFERENT chroma (the odd row the complement of the even one) -- what tells 4:2:2 from 4:2:0."""
    cw = (w + 1) >> 1
    rng = np.random.default_rng(_seed(name))
    if kind == "extremes":
        return tuple(np.array(EXTREMES, np.uint8)[rng.integers(0, len(EXTREMES), s)] for s in ((h, 2 * cw), (h, cw), (h, cw)))
    Y, U, V = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, 2 * cw), (h, cw), (h, cw)))
    if kind == "rowchroma":
        U[1::2], V[1::2] = 255 - U[0:2 * (h // 2):2], 255 - V[0:2 * (h // 2):2]
    return Y, U, V


def interleave(Y, U, V, fmt):
    """Tight rows [h, 4 cw] of a format."""
    h, cw = U.shape
    out = np.empty((h, cw, 4), np.uint8)
    if fmt == YUYV:
        out[..., 0], out[..., 1], out[..., 2], out[..., 3] = Y[:, 0::2], U, Y[:, 1::2], V
    else:
        out[..., 0], out[..., 1], out[..., 2], out[..., 3] = U, Y[:, 0::2], V, Y[:, 1::2]
    return out.reshape(h, 4 * cw)


def case_list():
    """(name, kind, h, w, pitch or None)"""
    out = []
    for h, w in SHAPES:
        for kind in KINDS:
            out.append((f"{kind}_{h}x{w}", kind, h, w, None))
    for kind in KINDS:
        out.append((f"{kind}_pitched_{PITCHED['h']}x{PITCHED['w']}", kind, PITCHED["h"], PITCHED["w"], PITCHED["pitch"]))
    return out


CASES = case_list()
CASE_NAMES = [c[0] for c in CASES]


def place(rows2d, pitch=None, lead=0):
    """Tight rows -> (flat buffer with `lead` GAP bytes in front and GAP in the pitch's gaps, the 2-D view of the rows in it)."""
    rows2d = np.ascontiguousarray(rows2d, np.uint8)
    h, rb = rows2d.shape
    pitch = rb if pitch is None else pitch
    assert pitch >= rb
    flat = np.full(lead + pitch * (h - 1) + rb, GAP, np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[lead:], (h, rb), (pitch, 1))
    view[...] = rows2d
    return flat, view


def build(case, fmt):
    """A case in a format -> dict(name, h, w, fmt, flat, pitch, view): `flat` / `pitch` feed packed_to_bgr, `view` a YUVFrame."""
    name, kind, h, w, pitch = case
    rows = interleave(*content(name, kind, h, w), fmt)
    flat, view = place(rows, pitch)
    return dict(name=name, h=h, w=w, fmt=fmt, flat=flat, pitch=rows.shape[1] if pitch is None else pitch, view=view, rows=rows)


def built(name, fmt):
    return build(CASES[CASE_NAMES.index(name)], fmt)


def frame_of(b, matrix, view=None):
    """The whenet_hip.yuv.YUVFrame of a built case (its pitch comes from the view's strides)."""
    from whenet_hip.yuv import YUVFrame
    f = YUVFrame((b["view"] if view is None else view,), b["fmt"], matrix, b["h"], b["w"])
    assert (f.h, f.w) == (b["h"], b["w"]) and len(f.planes) == 1
    return f


def expected(b, matrix, mutation=None):
    return packed_to_bgr(b["flat"], b["pitch"], b["fmt"], matrix, b["h"], b["w"], mutation)


# ---- every (Y, U, V) triple in one 2048 x 8192 packed frame --------------------------------------------------------------------
TRIPLES_H, TRIPLES_W = 2048, 8192


def all_triples(fmt):
    """The tight rows [2048, 16384] of a frame of 2048 x 8192 pixels: pair b = row * 4096 + column holds the chroma (b >> 7) =
    U * 256 + V and the luma values 2 (b & 127) + {0, 1}: every one of the 2^24 triples exactly once."""
    b = np.arange(TRIPLES_H * (TRIPLES_W // 2), dtype=np.int64).reshape(TRIPLES_H, TRIPLES_W // 2)
    U, V = ((b >> 7) >> 8).astype(np.uint8), ((b >> 7) & 255).astype(np.uint8)
    Y = np.empty((TRIPLES_H, TRIPLES_W), np.uint8)
    Y[:, 0::2], Y[:, 1::2] = (b & 127) << 1, ((b & 127) << 1) + 1
    return interleave(Y, U, V, fmt)


def all_triples_expected(matrix, row0, rows):
    """What rows row0 .. row0 + rows of the all-triples frame convert to, from the triples themselves (no buffer is read)."""
    p = np.arange(row0 * TRIPLES_W, (row0 + rows) * TRIPLES_W, dtype=np.int64).reshape(rows, TRIPLES_W)
    b = p >> 1
    return bgr_of_triples(((b & 127) << 1) + (p & 1), (b >> 7) >> 8, (b >> 7) & 255, matrix)
