"""The YUV 4:2:0 -> BGR conversion of include/whenet_hip.h stated in numpy -- this statement is the specification that
csrc/yuv.hip (kernel and host function) is held to, bit for bit -- and the table of frames the tests run.

Frame of h x w luma samples; chroma planes of ch = (h + 1) >> 1 rows by cw = (w + 1) >> 1 samples; pixel (y, x) takes luma (y, x)
and the chroma sample (y >> 1, x >> 1).  Every plane is a flat byte buffer with its own pitch.  int32 arithmetic, >> arithmetic:

    c = max(0, Y - yoff);  d = U - 128;  e = V - 128
    R = clip8((CY c         + CVR e + 2^19) >> 20);  G = clip8((CY c - CUG d - CVG e + 2^19) >> 20);  B = clip8((CY c + CUB d + 2^19) >> 20)
"""
import numpy as np

NV12, I420 = 0, 1
BT601, BT709, JFIF = 0, 1, 2
FORMATS = (("nv12", NV12), ("i420", I420))
MATRICES = (("bt601", BT601), ("bt709", BT709), ("jfif", JFIF))
# yoff, CY, CVR, CUG, CVG, CUB
COEFFS = {
    BT601: (16, 1220542, 1673527, 409993, 852492, 2116026),      # OpenCV's cvtColor constants, truncated (a restatement: unpinned)
    BT709: (16, 1220945, 1879825, 223578, 558767, 2215014),      # rint of the expressions below (a restatement: unpinned)
    JFIF: (0, 1048576, 1470104, 360853, 748826, 1858077),        # within 1 level of executed Pillow (tests/test_yuv_cpu.py)
}
S = float(1 << 20)
COEFF_EXPRESSIONS = {
    BT601: (16, int(S * 1.164), int(S * 1.596), int(S * 0.391), int(S * 0.813), int(S * 2.018)),
    BT709: (16, int(np.rint(S * 255 / 219)), int(np.rint(S * 1.5748 * 255 / 224)), int(np.rint(S * 0.1873 * 255 / 224)),
            int(np.rint(S * 0.4681 * 255 / 224)), int(np.rint(S * 1.8556 * 255 / 224))),
    JFIF: (0, 1 << 20, int(np.rint(S * 1.402)), int(np.rint(S * 0.344136)), int(np.rint(S * 0.714136)), int(np.rint(S * 1.772))),
}
EXTREMES = (0, 16, 128, 235, 240, 255)

# what a wrong implementation would do: each is seen by the case table (tests/test_yuv_cpu.py)
MUTATIONS = ("swap_uv", "chroma_row_y", "pitch_as_width", "nv12_as_i420", "no_rounding", "no_max0")


def chroma_size(h, w):
    return (h + 1) >> 1, (w + 1) >> 1


def row_bytes(fmt, h, w):
    """Bytes of a row of each plane."""
    cw = (w + 1) >> 1
    return (w, 2 * cw) if fmt == NV12 else (w, cw, cw)


def plane_rows(fmt, h, w):
    ch = (h + 1) >> 1
    return (h, ch) if fmt == NV12 else (h, ch, ch)


def yuv_to_bgr(planes, pitches, fmt, matrix, h, w, mutation=None):
    """planes: flat uint8 buffers, pitches: their row pitches -> uint8 [h, w, 3] in B, G, R order."""
    assert mutation is None or mutation in MUTATIONS
    yoff, CY, CVR, CUG, CVG, CUB = COEFFS[matrix]
    ch, cw = chroma_size(h, w)
    planes = [np.asarray(p, np.uint8).reshape(-1) for p in planes]
    pitches = list(pitches)
    if mutation == "pitch_as_width":
        pitches = list(row_bytes(fmt, h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    cy = np.minimum(yy, ch - 1) if mutation == "chroma_row_y" else yy >> 1
    cx = xx >> 1
    Y = planes[0][yy * pitches[0] + xx].astype(np.int32)
    if fmt == NV12 and mutation == "nv12_as_i420":       # the interleaved block read as a U plane and a V plane behind it
        tight = np.concatenate([planes[1][r * pitches[1]: r * pitches[1] + 2 * cw] for r in range(ch)])
        U, V = tight[cy * cw + cx], tight[ch * cw + cy * cw + cx]
    elif fmt == NV12:
        U, V = planes[1][cy * pitches[1] + 2 * cx], planes[1][cy * pitches[1] + 2 * cx + 1]
    else:
        U, V = planes[1][cy * pitches[1] + cx], planes[2][cy * pitches[2] + cx]
    if mutation == "swap_uv":
        U, V = V, U
    c = Y - yoff if mutation == "no_max0" else np.maximum(0, Y - yoff)
    d, e = U.astype(np.int32) - 128, V.astype(np.int32) - 128
    half = 0 if mutation == "no_rounding" else 1 << 19
    base = (CY * c + half).astype(np.int32)
    R = np.clip((base + CVR * e) >> 20, 0, 255)
    G = np.clip((base - CUG * d - CVG * e) >> 20, 0, 255)
    B = np.clip((base + CUB * d) >> 20, 0, 255)
    return np.stack([B, G, R], axis=2).astype(np.uint8)


# ---- the case table ---------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (2, 2), (1, 7), (7, 1), (3, 5), (2, 16), (5, 17), (10, 18), (33, 7))
PITCHED = dict(h=64, w=130, y_pitch=192, chroma_pitch={NV12: 160, I420: 96})
GAP = 0xA5              # what lies between a row's last byte and the next row of a pitched plane


def _seed(name):
    return 4200 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100000


def _buffers(fmt, h, w, pitches, tight_planes):
    """Tight 2-D planes -> (flat buffers with the pitch's gap bytes, 2-D views of them whose strides are (pitch, 1))."""
    flats, views = [], []
    for p2, pitch, rb, rows in zip(tight_planes, pitches, row_bytes(fmt, h, w), plane_rows(fmt, h, w)):
        flat = np.full(pitch * (rows - 1) + rb, GAP, np.uint8)
        view = np.lib.stride_tricks.as_strided(flat, (rows, rb), (pitch, 1))
        view[...] = p2
        flats.append(flat)
        views.append(view)
    return flats, views


def sample_yuv(i):
    """(Y [h,w], U [ch,cw], V [ch,cw]) cut from committed sample frame i through a fixed integer RGB -> YUV (content, not a
    reference): the usual 8-bit studio-range form, chroma taken at the top-left pixel of each 2 x 2 block."""
    from tests import detector_cases as DC
    f = DC.sample_frame(i).astype(np.int32)
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    Y = ((66 * R + 129 * G + 25 * B + 128) >> 8) + 16
    U = ((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128
    V = ((112 * R - 94 * G - 18 * B + 128) >> 8) + 128
    return Y.astype(np.uint8), U[::2, ::2].astype(np.uint8), V[::2, ::2].astype(np.uint8)


def _content(name, kind, h, w):
    """Tight (Y, U, V) planes of a case."""
    ch, cw = chroma_size(h, w)
    rng = np.random.default_rng(_seed(name))
    if kind == "random":
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))
    if kind == "extremes":
        return tuple(np.array(EXTREMES, np.uint8)[rng.integers(0, len(EXTREMES), s)] for s in ((h, w), (ch, cw), (ch, cw)))
    i, y0, x0 = kind                    # a window of a sample frame, at even offsets (so that the chroma planes line up)
    Y, U, V = sample_yuv(i)
    return Y[y0:y0 + h, x0:x0 + w], U[y0 // 2:y0 // 2 + ch, x0 // 2:x0 // 2 + cw], V[y0 // 2:y0 // 2 + ch, x0 // 2:x0 // 2 + cw]


def case_list():
    """(name, kind, h, w, pitched)"""
    out = []
    for h, w in SHAPES:
        for kind in ("random", "extremes"):
            out.append((f"{kind}_{h}x{w}", kind, h, w, False))
    for kind in ("random", "extremes"):
        out.append((f"{kind}_pitched_{PITCHED['h']}x{PITCHED['w']}", kind, PITCHED["h"], PITCHED["w"], True))
    out.append(("sample0_224x528", (0, 0, 0), 224, 528, False))
    out.append(("sample1_225x547", (1, 0, 0), 225, 547, False))
    out.append(("sample1_window_97x131", (1, 60, 200), 97, 131, False))
    return out


CASES = case_list()
CASE_NAMES = [c[0] for c in CASES]


def build(case, fmt):
    """A case in a format -> dict(h, w, fmt, flats, pitches, views): `flats` / `pitches` feed yuv_to_bgr, `views` a YUVFrame."""
    name, kind, h, w, pitched = case
    Y, U, V = _content(name, kind, h, w)
    if fmt == NV12:
        tight = (Y, np.stack([U, V], axis=2).reshape(U.shape[0], -1))
    else:
        tight = (Y, U, V)
    if pitched:
        pitches = (PITCHED["y_pitch"],) + (PITCHED["chroma_pitch"][fmt],) * (len(tight) - 1)
    else:
        pitches = row_bytes(fmt, h, w)
    flats, views = _buffers(fmt, h, w, pitches, tight)
    return dict(name=name, h=h, w=w, fmt=fmt, flats=flats, pitches=tuple(pitches), views=views)


def frame_of(built, matrix):
    """The whenet_hip.yuv.YUVFrame of a built case (its pitches come from the views' strides)."""
    from whenet_hip.yuv import YUVFrame
    v = built["views"]
    f = YUVFrame.nv12(v[0], v[1], matrix=matrix) if built["fmt"] == NV12 else YUVFrame.i420(v[0], v[1], v[2], matrix=matrix)
    assert (f.h, f.w) == (built["h"], built["w"])
    return f


def expected(built, matrix, mutation=None):
    return yuv_to_bgr(built["flats"], built["pitches"], built["fmt"], matrix, built["h"], built["w"], mutation)


# ---- every (Y, U, V) triple in one 4096 x 4096 NV12 frame ---------------------------------------------------------------------
def all_triples():
    """(Y [4096,4096], UV [2048,4096]): 2 x 2 block b = by * 2048 + bx holds the chroma pair (b >> 6) = U * 256 + V and the luma
    values 4 (b & 63) + {0, 1, 2, 3}: every one of the 2^24 triples exactly once."""
    b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    pair = b >> 6
    UV = np.stack([pair >> 8, pair & 255], axis=2).astype(np.uint8).reshape(2048, 4096)
    Y = np.empty((4096, 4096), np.uint8)
    y4 = (b & 63) << 2
    Y[0::2, 0::2], Y[0::2, 1::2], Y[1::2, 0::2], Y[1::2, 1::2] = y4, y4 + 1, y4 + 2, y4 + 3
    return Y, UV


def triples_per_pixel(Y, UV):
    """[4096,4096,3] = (Y, U, V) of every pixel of the all-triples frame."""
    U = np.repeat(np.repeat(UV[:, 0::2], 2, axis=0), 2, axis=1)
    V = np.repeat(np.repeat(UV[:, 1::2], 2, axis=0), 2, axis=1)
    return np.stack([Y, U, V], axis=2)
