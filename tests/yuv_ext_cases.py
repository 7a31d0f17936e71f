"""The extended YUV -> BGR conversion of include/whenet_hip_yuv_ext.h stated in numpy, in int64 -- the specification that
csrc/yuvx.hip (kernels) and csrc/yuvx_host.h (host statement) are held to, bit for bit -- and the table of frames the tests run.
It shares no code with the package.

A frame is a layout (NV12-like, I420-like, planar 4:4:4) times a container: 8-bit samples, or 16-bit little-endian words with a
shift, the sample at 16 bits being s16 = (word << shift) & 0xFFFF.  4:2:0: pixel (y, x) takes the chroma sample (y >> 1, x >> 1);
4:4:4: the sample (y, x).  16-bit container, exact integers, >> arithmetic:

    c = max(0, Y16 - (yoff << 8));  d = U16 - 32768;  e = V16 - 32768;  base = CY c + 2^27
    B = clip8((base + CUB d) >> 28);  G = clip8((base - CUG d - CVG e) >> 28);  R = clip8((base + CVR e) >> 28)

8-bit container: the statement of include/whenet_hip.h (offsets 16 / 128, 2^19, >> 20).
"""
import functools

import numpy as np

NV12, I420, I444 = 0, 1, 16
BT601, BT709, JFIF, BT2020 = 0, 1, 2, 3
MATRICES = (("bt601", BT601), ("bt709", BT709), ("jfif", JFIF), ("bt2020", BT2020))
COEFFS = {
    BT601: (16, 1220542, 1673527, 409993, 852492, 2116026),
    BT709: (16, 1220945, 1879825, 223578, 558767, 2215014),
    JFIF: (0, 1048576, 1470104, 360853, 748826, 1858077),
    BT2020: (16, 1220945, 1760217, 196426, 682019, 2245811),
}
S = float(1 << 20)
KR, KB = 0.2627, 0.0593
KG = 1 - KR - KB
SC = 255 / 224
# the unrounded constants: {255/219 (or 1), CVR, CUG, CVG, CUB} / 2^20
REAL = {
    BT601: (16, 1.164, 1.596, 0.391, 0.813, 2.018),
    BT709: (16, 255 / 219, 1.5748 * SC, 0.1873 * SC, 0.4681 * SC, 1.8556 * SC),
    JFIF: (0, 1.0, 1.402, 0.344136, 0.714136, 1.772),
    BT2020: (16, 255 / 219, 2 * (1 - KR) * SC, 2 * KB * (1 - KB) / KG * SC, 2 * KR * (1 - KR) / KG * SC, 2 * (1 - KB) * SC),
}
BT2020_DERIVED = (16,) + tuple(int(np.rint(S * v)) for v in REAL[BT2020][1:])

# name (a name `YUVFrame.from_buffer` knows), layout, container bits, shift
FORMATS = (("p016", NV12, 16, 0), ("yuv420p10le", I420, 16, 6), ("yuv420p12le", I420, 16, 4), ("i444", I444, 8, 0), ("yuv444p16", I444, 16, 0))
FORMAT_NAMES = [f[0] for f in FORMATS]
WIDE_FORMATS = tuple(f for f in FORMATS if f[2] == 16)

# what a wrong implementation would do: each differs from the statement on at least one case (tests/test_yuv_ext_cpu.py)
MUTATIONS = ("wrap32", "drop_low8", "shift_plus_one", "swap_uv", "chroma_row_y", "yoff_unscaled", "round_19")


def plane_shapes(layout, h, w):
    """(rows, samples per row) of every plane."""
    ch, cw = (h + 1) >> 1, (w + 1) >> 1
    if layout == NV12:
        return ((h, w), (ch, 2 * cw))
    if layout == I420:
        return ((h, w), (ch, cw), (ch, cw))
    return ((h, w), (h, w), (h, w))


def _samples(buf, offsets, bits, shift, mutation):
    """The samples at sample-index `offsets` (int64 array of BYTE offsets) of a flat uint8 buffer, as int64."""
    if bits == 8:
        return buf[offsets].astype(np.int64)
    word = buf[offsets].astype(np.int64) | (buf[offsets + 1].astype(np.int64) << 8)
    s = (word << (shift + (1 if mutation == "shift_plus_one" else 0))) & 0xFFFF
    return s & 0xFF00 if mutation == "drop_low8" else s


def _wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def yuvx_to_bgr(planes, pitches, layout, bits, shift, matrix, h, w, mutation=None):
    """planes: flat uint8 buffers, pitches: their row pitches in bytes -> uint8 [h, w, 3] in B, G, R order."""
    assert mutation is None or mutation in MUTATIONS
    yoff, CY, CVR, CUG, CVG, CUB = COEFFS[matrix]
    planes = [np.asarray(p, np.uint8).reshape(-1) for p in planes]
    bs = bits // 8
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    if layout == I444:
        cy, cx = yy, xx
    else:
        cy = np.minimum(yy, ((h + 1) >> 1) - 1) if mutation == "chroma_row_y" else yy >> 1
        cx = xx >> 1
    Y = _samples(planes[0], yy * pitches[0] + xx * bs, bits, shift, mutation)
    if layout == NV12:
        U = _samples(planes[1], cy * pitches[1] + 2 * cx * bs, bits, shift, mutation)
        V = _samples(planes[1], cy * pitches[1] + (2 * cx + 1) * bs, bits, shift, mutation)
    else:
        U = _samples(planes[1], cy * pitches[1] + cx * bs, bits, shift, mutation)
        V = _samples(planes[2], cy * pitches[2] + cx * bs, bits, shift, mutation)
    if mutation == "swap_uv":
        U, V = V, U
    if bits == 8:
        sh, mid, off = 20, 128, yoff
    else:
        sh, mid, off = 28, 32768, yoff if mutation == "yoff_unscaled" else yoff << 8
    c, d, e = np.maximum(0, Y - off), U - mid, V - mid
    half = 1 << 19 if mutation == "round_19" else 1 << (sh - 1)
    fold = _wrap32 if mutation == "wrap32" else (lambda v: v)
    base = fold(CY * c + half)
    B = np.clip(fold(base + fold(CUB * d)) >> sh, 0, 255)
    G = np.clip(fold(base - fold(CUG * d) - fold(CVG * e)) >> sh, 0, 255)
    R = np.clip(fold(base + fold(CVR * e)) >> sh, 0, 255)
    return np.stack([B, G, R], axis=2).astype(np.uint8)


def float_reference(planes, pitches, layout, bits, shift, matrix, h, w):
    """float64 with the UNROUNDED constants, rounded half up and clipped: within 1 level of the statement."""
    yoff, cy_, cvr, cug, cvg, cub = REAL[matrix]
    planes = [np.asarray(p, np.uint8).reshape(-1) for p in planes]
    bs = bits // 8
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    cy, cx = (yy, xx) if layout == I444 else (yy >> 1, xx >> 1)
    Y = _samples(planes[0], yy * pitches[0] + xx * bs, bits, shift, None)
    if layout == NV12:
        U = _samples(planes[1], cy * pitches[1] + 2 * cx * bs, bits, shift, None)
        V = _samples(planes[1], cy * pitches[1] + (2 * cx + 1) * bs, bits, shift, None)
    else:
        U = _samples(planes[1], cy * pitches[1] + cx * bs, bits, shift, None)
        V = _samples(planes[2], cy * pitches[2] + cx * bs, bits, shift, None)
    scale = 1.0 if bits == 8 else 256.0
    c = np.maximum(0.0, Y / scale - yoff) * cy_
    d, e = U / scale - 128.0, V / scale - 128.0
    out = np.stack([c + cub * d, c - cug * d - cvg * e, c + cvr * e], axis=2)
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.int64)


# ---- the case table ---------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 2), (2, 1), (3, 4), (4, 3), (5, 17), (10, 18))
PITCHED = (64, 130)         # at a pitch wider than the row: row bytes + 13 samples (16-bit: 26 bytes, so rows lie at 0, 6, 4, 2 mod 8)
ODD = (97, 131)             # position 1 of a mixed clip: 97 * 131 * 3 is 1 mod 4
BIG = (225, 547)            # the pipeline test's frame
GAP = 0xA5


def case_list():
    """(name, kind, h, w, pitched)"""
    out = []
    for h, w in SHAPES:
        for kind in ("random", "extremes"):
            out.append((f"{kind}_{h}x{w}", kind, h, w, False))
    for kind in ("random", "extremes"):
        out.append((f"{kind}_pitched_{PITCHED[0]}x{PITCHED[1]}", kind, PITCHED[0], PITCHED[1], True))
    out.append((f"random_{ODD[0]}x{ODD[1]}", "random", ODD[0], ODD[1], False))
    return out


CASES = case_list()
CASE_NAMES = [c[0] for c in CASES]


def _seed(name):
    return 7100 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100000


def _content(name, kind, layout, bits, h, w):
    """Tight planes of stored values (uint8 samples or uint16 words).  random: every bit of a word is random, so the low bits
    are non-zero under every shift and a 10-bit word carries junk above bit 9.  extremes: 0 and the largest stored value in every
    (Y, U, V) combination: the two luma values alternate along x and y, the chroma samples walk through the four (U, V) pairs."""
    rng = np.random.default_rng(_seed(name) + layout + bits)
    top = (1 << bits) - 1
    dtype = np.uint8 if bits == 8 else np.dtype("<u2")
    shapes = plane_shapes(layout, h, w)
    if kind == "random":
        return [rng.integers(0, top + 1, s, dtype=np.int64).astype(dtype) for s in shapes]
    yy, xx = np.mgrid[0:h, 0:w]
    Y = (((yy + xx) & 1) * top).astype(dtype)
    crows, ccols = (h, w) if layout == I444 else ((h + 1) >> 1, (w + 1) >> 1)
    cyy, cxx = np.mgrid[0:crows, 0:ccols]
    step = 2 if layout == I444 else 1       # (4:4:4: a pair lasts two pixels, so that both luma values meet it)
    pair = (cxx // step + cyy // step) & 3
    U, V = ((pair & 1) * top).astype(dtype), ((pair >> 1) * top).astype(dtype)
    if layout == NV12:
        return [Y, np.stack([U, V], axis=2).reshape(crows, -1)]
    return [Y, U, V]


def build(case, fmt):
    """A case in a format (an entry of FORMATS) -> dict: `flats` (flat uint8 buffers) / `pitches` (bytes) feed yuvx_to_bgr,
    `views` (2-D byte views of the flats with strides (pitch, 1)) a YUVFrame."""
    name, kind, h, w, pitched = case
    fname, layout, bits, shift = fmt
    bs = bits // 8
    flats, views, pitches = [], [], []
    for p2 in _content(name, kind, layout, bits, h, w):
        rows, rb = p2.shape[0], p2.shape[1] * bs
        pitch = rb + 13 * bs if pitched else rb
        flat = np.full((pitch * (rows - 1) + rb + 1) // 2 * 2, GAP, np.uint8)      # (a fresh numpy allocation: 16-byte aligned)
        view = np.lib.stride_tricks.as_strided(flat, (rows, rb), (pitch, 1))
        view[...] = np.ascontiguousarray(p2).view(np.uint8).reshape(rows, rb)
        flats.append(flat), views.append(view), pitches.append(pitch)
    return dict(name=name, h=h, w=w, fmt=fmt, layout=layout, bits=bits, shift=shift, flats=flats, pitches=tuple(pitches), views=views)


def built(name, fname):
    return build(CASES[CASE_NAMES.index(name)], FORMATS[FORMAT_NAMES.index(fname)])


def frame_of(b, matrix):
    """The whenet_hip.yuv.YUVFrame of a built case (its pitches come from the views' strides)."""
    from whenet_hip.yuv import YUVFrame
    f = YUVFrame(b["views"], b["layout"], matrix, b["h"], b["w"], container=b["bits"], shift=b["shift"])
    assert (f.h, f.w) == (b["h"], b["w"])
    return f


def expected(b, matrix, mutation=None):
    return yuvx_to_bgr(b["flats"], b["pitches"], b["layout"], b["bits"], b["shift"], matrix, b["h"], b["w"], mutation)


@functools.lru_cache(maxsize=None)
def expected_bytes(name, fname, matrix):
    """The statement's bytes of a case, computed once and shared (the tests never change them)."""
    return expected(built(name, fname), matrix).tobytes()


def tight_buffer(b):
    """The planes of a built case tight in ONE flat uint8 buffer, as `YUVFrame.from_buffer(buf, h, w, name)` reads them."""
    return np.concatenate([np.ascontiguousarray(v).reshape(-1) for v in b["views"]])


def widen(planes8):
    """8-bit planes -> the 16-bit words whose samples are the 8-bit samples << 8."""
    return [(np.asarray(p).astype(np.uint16) << 8).astype("<u2") for p in planes8]
