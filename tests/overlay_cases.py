"""The pose overlay of include/whenet_hip.h (POSE OVERLAY) stated in numpy -- this statement is the specification that
`whenet_annotate_host` is held to byte for byte, and the kernels of csrc/overlay.hip through it -- and the table of cases the
tests run.

Segments of a head: window (y0, x0, y1, x1) and float32 angles -> utils.py:15-42 in Python floats (double) with tdx = (x0 + x1) / 2,
tdy = (y0 + y1) / 2, size = (x1 - x0) // 2, every endpoint int()-truncated.  Raster: pixel X is painted by P -> Q iff its distance
to the closed segment is <= 1, decided in int64 (d = Q - P, v = X - P, L2 = d.d: v.d <= 0 -> |v|^2 <= 1; v.d >= L2 -> |X - Q|^2 <= 1;
else (v x d)^2 <= L2).  Paint order: head by head, rectangle sides, X, Y, Z; the last primitive wins.  4:2:0: the integer rows of
WHENET_BGR2YUV_COEFFS, chroma from the 2 x 2 sums clamped at the last row / column.
"""
import math

import numpy as np

RGB, BGR = 0, 1
NV12, I420, PACKED = 0, 1, 2
BT601, BT709, JFIF = 0, 1, 2
FORMATS = (("packed", PACKED), ("nv12", NV12), ("i420", I420))
MATRICES = (("bt601", BT601), ("bt709", BT709), ("jfif", JFIF))
# RY GY BY | RU GU BU | RV GV BV | yoff: WHENET_BGR2YUV_COEFFS (tests/test_overlay_cpu.py holds the header, this table and the expressions together)
COEFFS = {
    BT601: (269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897, 16),
    BT709: (191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230, 16),
    JFIF: (313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262, 0),
}


def coeff_expressions(matrix):
    kr, kb = (.2126, .0722) if matrix == BT709 else (.299, .114)
    sy, sc, yoff = (1.0, 1.0, 0) if matrix == JFIF else (219 / 255, 224 / 255, 16)
    kg = 1 - kr - kb
    e = (kr * sy, kg * sy, kb * sy,
         -kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc,
         0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc)
    return tuple(int(np.rint(v * (1 << 20))) for v in e) + (yoff,)


# ---- segments ------------------------------------------------------------------------------------------------------------
def axis_arguments(rect, yaw, pitch, roll):
    """The arguments of draw_axis as section 1 builds them: Python floats of the float32 angles, tdx, tdy, size."""
    y0, x0, y1, x1 = (int(v) for v in rect)
    return dict(yaw=float(np.float32(yaw)), pitch=float(np.float32(pitch)), roll=float(np.float32(roll)),
                tdx=(x0 + x1) / 2, tdy=(y0 + y1) / 2, size=(x1 - x0) // 2)


def axis_coordinates(yaw, pitch, roll, tdx, tdy, size):
    """The six un-truncated end coordinates (X.x, X.y, Y.x, Y.y, Z.x, Z.y) of the three axes, in Python floats.  The ORDER of the
    operations is the reference's (utils.py:15-38) -- degrees times pi, then divided by 180; the yaw negated; every product
    associated left to right; the centre added last -- because every one of them rounds; the wording is this project's
    (csrc/overlay_host.h states the same arithmetic in C++)."""
    return axis_coordinates_of(axis_trig(yaw, pitch, roll), tdx, tdy, size)


def axis_trig(yaw, pitch, roll):
    """(cos y, sin y, cos p, sin p, cos r, sin r) of the radian arguments, from Python's math module: the host's libm."""
    to_rad = lambda deg: deg * math.pi / 180
    p, y, r = to_rad(pitch), -to_rad(yaw), to_rad(roll)
    return math.cos(y), math.sin(y), math.cos(p), math.sin(p), math.cos(r), math.sin(r)


def axis_coordinates_of(trig, tdx, tdy, size):
    """axis_coordinates from the six sines and cosines onward.  Python floats give six floats; float64 arrays of one shape give
    six arrays, every operation rounded on its own as in the scalar form (tests/overlay_lattice_cases.py moves one value of the
    six by one ulp and looks at what int() then returns)."""
    cos_y, sin_y, cos_p, sin_p, cos_r, sin_r = trig
    x_axis = (size * (cos_y * cos_r) + tdx, size * (cos_p * sin_r + cos_r * sin_p * sin_y) + tdy)
    y_axis = (size * (-cos_y * sin_r) + tdx, size * (cos_p * cos_r - sin_p * sin_y * sin_r) + tdy)
    z_axis = (size * sin_y + tdx, size * (-cos_y * sin_p) + tdy)
    return x_axis + y_axis + z_axis


def segments(rect, yaw, pitch, roll, valid=1):
    """-> (int list [16], flags)."""
    y0, x0, y1, x1 = (int(v) for v in rect)
    if not valid:
        return [0] * 16, 0
    a = axis_arguments(rect, yaw, pitch, roll)
    if not all(math.isfinite(a[k]) for k in ("yaw", "pitch", "roll")):
        return [x0, y0, x1, y1] + [0] * 12, 1
    c = axis_coordinates(**a)
    p = [int(a["tdx"]), int(a["tdy"])]
    return [x0, y0, x1, y1] + p + [int(c[0]), int(c[1])] + p + [int(c[2]), int(c[3])] + p + [int(c[4]), int(c[5])], 3


def head_primitives(seg, flags):
    """(px, py, qx, qy, colour index) of a head's segments in paint order; colour 0 black, 1 red, 2 green, 3 blue."""
    if not flags & 1:
        return []
    x0, y0, x1, y1 = seg[:4]
    out = [(x0, y0, x1, y0, 0), (x1, y0, x1, y1, 0), (x1, y1, x0, y1, 0), (x0, y1, x0, y0, 0)]
    if flags & 2:
        out += [tuple(seg[4 + 4 * i: 8 + 4 * i]) + (i + 1,) for i in range(3)]
    return out


# ---- raster --------------------------------------------------------------------------------------------------------------
def hit_mask(h, w, px, py, qx, qy):
    """bool [h, w]: the pixels within distance 1 of the closed segment, in int64."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    dx, dy = np.int64(qx - px), np.int64(qy - py)
    vx, vy = xx - px, yy - py
    L2 = dx * dx + dy * dy
    t = vx * dx + vy * dy
    near_p = vx * vx + vy * vy <= 1
    near_q = (xx - qx) ** 2 + (yy - qy) ** 2 <= 1
    cross = vx * dy - vy * dx
    return np.where(t <= 0, near_p, np.where(t >= L2, near_q, cross * cross <= L2))


def colour_bytes(colour, order):
    r, g, b = ((0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255))[colour]
    return (b, g, r) if order == BGR else (r, g, b)


def paint(frame, order, rects, valid, ypr):
    """The annotated frame, packed, in the frame's channel order."""
    out = np.array(frame, np.uint8, copy=True)
    h, w = out.shape[:2]
    for i, rect in enumerate(rects):
        seg, flags = segments(rect, *ypr[i], valid=1 if valid is None else int(valid[i]))
        for px, py, qx, qy, colour in head_primitives(seg, flags):
            out[hit_mask(h, w, px, py, qx, qy)] = colour_bytes(colour, order)
    return out


# ---- BGR -> 4:2:0 -----------------------------------------------------------------------------------------------------------
def clip8(v):
    return np.clip(v, 0, 255)


def to_yuv420(img, order, matrix):
    """packed [h, w, 3] -> (Y [h, w], U [ch, cw], V [ch, cw]) uint8."""
    RY, GY, BY, RU, GU, BU, RV, GV, BV, yoff = COEFFS[matrix]
    a = np.asarray(img).astype(np.int32)
    R, G, B = (a[..., 2], a[..., 1], a[..., 0]) if order == BGR else (a[..., 0], a[..., 1], a[..., 2])
    h, w = R.shape
    Y = clip8(((RY * R + GY * G + BY * B + (1 << 19)) >> 20) + yoff)
    ch, cw = (h + 1) >> 1, (w + 1) >> 1
    cy, cx = np.mgrid[0:ch, 0:cw]
    sums = []
    for P in (R, G, B):
        s = np.zeros((ch, cw), np.int32)
        for dy in (0, 1):
            for dx in (0, 1):
                s += P[np.minimum(2 * cy + dy, h - 1), np.minimum(2 * cx + dx, w - 1)]
        sums.append(s)
    Rs, Gs, Bs = sums
    U = clip8(((RU * Rs + GU * Gs + BU * Bs + (1 << 21)) >> 22) + 128)
    V = clip8(((RV * Rs + GV * Gs + BV * Bs + (1 << 21)) >> 22) + 128)
    return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)


def plane_shapes(fmt, h, w):
    """(rows, row bytes) of every plane of a surface."""
    ch, cw = (h + 1) >> 1, (w + 1) >> 1
    if fmt == PACKED:
        return [(h, 3 * w)]
    return [(h, w), (ch, 2 * cw)] if fmt == NV12 else [(h, w), (ch, cw), (ch, cw)]


def planes_of(img, order, fmt, matrix=BT601):
    """The planes of a destination that holds the packed frame `img`, tight: a list of uint8 [rows, row bytes]."""
    h, w = img.shape[:2]
    if fmt == PACKED:
        return [img.reshape(h, 3 * w)]
    Y, U, V = to_yuv420(img, order, matrix)
    if fmt == NV12:
        return [Y, np.stack([U, V], axis=2).reshape(U.shape[0], -1)]
    return [Y, U, V]


def annotate(frame, order, rects, valid, ypr, fmt, matrix=BT601):
    """The whole statement: the planes of the annotated frame."""
    return planes_of(paint(frame, order, rects, valid, ypr), order, fmt, matrix)


# ---- the case table --------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (5, 7), (33, 19), (64, 48), (96, 128))      # h x w


def frame_for(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def heads_cases(h, w):
    """name -> (rects int32 [k,4], valid or None, ypr float32 [k,3]) for an h x w frame.  Windows are (y0, x0, y1, x1) inside
    -4096..8192; the axes' directions come from the angles: yaw 0 / 90 / 180 turn the X axis horizontal / into the screen / back,
    roll 45 makes it diagonal, roll near 90 steep."""
    nan, inf = float("nan"), float("inf")
    full = (0, 0, h, w)
    mid = (h // 4, w // 4, max(h // 4, 3 * h // 4), max(w // 4, 3 * w // 4))
    big = (-h, -w, 2 * h, 2 * w)                   # endpoints outside every edge
    away = (h + 40, w + 40, h + 90, w + 120)       # wholly outside
    neg = (-90, -120, -40, -40)
    cases = {
        "none": ([], None, []),
        "full_zero": ([full], None, [(0, 0, 0)]),                        # horizontal X, vertical Y, Z a disc (P = Q)
        "mid_45": ([mid], None, [(0, 0, 45)]),
        "mid_steep": ([mid], None, [(0, 0, 80)]),
        "mid_pose": ([mid], None, [(30.5, -20.25, 10.125)]),
        "yaw_90": ([mid], None, [(90, 0, 0)]),
        "yaw_m90": ([mid], None, [(-90, 0, 0)]),
        "yaw_180": ([mid], None, [(180, 90, -90)]),
        "yaw_m180": ([mid], None, [(-180, -90, 90)]),
        "size0": ([(h // 2, w // 2, h // 2 + 1, w // 2)], None, [(10, 20, 30)]),      # x1 == x0: three discs
        "border": ([(0, 0, h, w), (0, 0, 1, 1), (h - 1, w - 1, h, w)], None, [(12, 3, 4), (0, 0, 0), (-170, 60, -45)]),
        "big": ([big], None, [(40, 30, 20)]),
        "away": ([away, neg], None, [(40, 30, 20), (-40, 30, 20)]),
        "two": ([mid, (mid[0] + 1, mid[1] + 2, mid[2] + 1, mid[3] + 2)], None, [(20, 10, 0), (-20, -10, 50)]),
        "invalid": ([mid, full, mid], [1, 0, 1], [(20, 10, 0), (0, 0, 0), (-60, 15, 33)]),
        "all_invalid": ([mid], [0], [(20, 10, 0)]),
        "nan": ([mid, full], None, [(nan, 10, 0), (10, 20, 30)]),
        "inf": ([full, mid], None, [(10, inf, 0), (0, -inf, nan)]),
        "nan_invalid": ([(9000, 9000, 9100, 9100), mid], [0, 1], [(nan, nan, nan), (5, 5, 5)]),      # an invalid head's window is never read
    }
    rng = np.random.default_rng(h * 1000 + w)
    rects, ypr = [], []
    for _ in range(64):                             # 64 overlapping heads: the order decides most pixels
        y0, x0 = int(rng.integers(-4, max(h - 1, 1))), int(rng.integers(-4, max(w - 1, 1)))
        rects.append((y0, x0, y0 + int(rng.integers(1, h + 6)), x0 + int(rng.integers(1, w + 6))))
        ypr.append((float(rng.uniform(-180, 180)), float(rng.uniform(-99, 99)), float(rng.uniform(-99, 99))))
    cases["sixty_four"] = (rects, None, ypr)
    return {k: (np.asarray(r, np.int32).reshape(-1, 4), None if v is None else np.asarray(v, np.int32),
                np.asarray(a, np.float32).reshape(-1, 3)) for k, (r, v, a) in cases.items()}


TILE_H, TILE_W = 16, 128      # the draw kernel's tile (csrc/overlay.hip)


def tiles_touched(h, w, heads):
    """The set of (tile row, tile column) whose pixels a head set can paint: every primitive's box grown by the raster's reach."""
    rects, valid, ypr = heads
    tiles = set()
    for i, rect in enumerate(rects):
        seg, flags = segments(rect, *ypr[i], valid=1 if valid is None else int(valid[i]))
        for px, py, qx, qy, _ in head_primitives(seg, flags):
            x0, x1 = max(min(px, qx) - 1, 0), min(max(px, qx) + 1, w - 1)
            y0, y1 = max(min(py, qy) - 1, 0), min(max(py, qy) + 1, h - 1)
            tiles |= {(ty, tx) for ty in range(y0 // TILE_H, y1 // TILE_H + 1) for tx in range(x0 // TILE_W, x1 // TILE_W + 1)}
    return tiles


def gpu_extra_cases():
    """(name, h, w, heads) beyond the table for the kernels: tiles of 128 x 16 pixels crossed by one long segment, a head inside
    one tile and one over four tiles, and 256 heads on 96 x 128."""
    f32 = np.float32
    out = []
    out.append(("long_diagonal", 70, 300, (np.asarray([(0, 0, 70, 300)], np.int32), None, np.asarray([(0, 0, 13)], f32))))
    out.append(("long_steep", 150, 140, (np.asarray([(-100, 0, 250, 140)], np.int32), None, np.asarray([(3, 2, 88)], f32))))
    out.append(("one_tile", 40, 300, (np.asarray([(20, 140, 28, 152)], np.int32), None, np.asarray([(25, -15, 5)], f32))))
    out.append(("four_tiles", 40, 300, (np.asarray([(8, 120, 24, 136)], np.int32), None, np.asarray([(25, -15, 5)], f32))))
    rng = np.random.default_rng(256)
    rects, ypr = [], []
    for _ in range(256):
        y0, x0 = int(rng.integers(-8, 90)), int(rng.integers(-8, 120))
        rects.append((y0, x0, y0 + int(rng.integers(1, 60)), x0 + int(rng.integers(1, 80))))
        ypr.append((float(rng.uniform(-180, 180)), float(rng.uniform(-99, 99)), float(rng.uniform(-99, 99))))
    valid = (rng.uniform(size=256) < 0.9).astype(np.int32)
    out.append(("heads_256", 96, 128, (np.asarray(rects, np.int32), valid, np.asarray(ypr, f32))))
    return out


# ---- the heads whose segments are compared with the EXECUTED reference (tests/golden/make_overlay_fixture.py) ----------------
REFERENCE_SEED, REFERENCE_HEADS = 20261019, 4096


def reference_heads():
    """(rects int32 [n,4], ypr float32 [n,3]): 4,096 seeded heads -- window origin x in [0,1800), y in [0,1000), sides 1..699, yaw
    +-180, pitch and roll +-99, rounded to float32 -- followed by the designed ones: all angles 0, +-90, +-180, size = 0."""
    rng = np.random.default_rng(REFERENCE_SEED)
    n = REFERENCE_HEADS
    # The draw order is part of the fixture: origins, then the sides as one [n,2] draw, then the angles as one [n,3] draw of
    # (-1, 1) scaled.  With it every coordinate that is computed with a rounding (size >= 1) lies 1.78e-6 or more from an integer
    # (integer_margin; test_overlay_cpu asserts >= 1e-6), so an implementation's last-bit differences in sin / cos cannot move an
    # int().  Other orders of the same seed gave 4.6e-8 .. 8.6e-7: such a set would test the libm, not the overlay.  (The heads that
    # do sit on an integer, on purpose, are the table of tests/overlay_lattice_cases.py.)
    x0, y0 = rng.integers(0, 1800, n), rng.integers(0, 1000, n)
    sides = rng.integers(1, 700, (n, 2))
    rects = np.stack([y0, x0, y0 + sides[:, 1], x0 + sides[:, 0]], axis=1).astype(np.int32)
    ypr = (rng.uniform(-1, 1, (n, 3)) * np.array([180, 99, 99])).astype(np.float32)
    designed_rects = [(100, 200, 300, 501), (0, 0, 1, 1), (40, 60, 640, 759)]
    designed_ypr = [(0, 0, 0), (90, 0, 0), (-90, 0, 0), (0, 90, 0), (0, -90, 0), (0, 0, 90), (0, 0, -90), (180, 0, 0), (-180, 0, 0),
                    (90, 90, 90), (-90, -90, -90), (180, 90, -90), (-180, -90, 90), (90, 0, 90), (90, 0, -90)]
    dr = [r for r in designed_rects for _ in designed_ypr]
    da = [a for _ in designed_rects for a in designed_ypr]
    dr += [(10, 50, 20, 50), (10, 50, 20, 51)]          # size = 0: x1 == x0, and a window one pixel wide
    da += [(33, 44, 55), (33, 44, 55)]
    return (np.concatenate([rects, np.asarray(dr, np.int32)]), np.concatenate([ypr, np.asarray(da, np.float32)]))


def integer_margin(rect, yaw, pitch, roll):
    """The smallest distance of a head's six un-truncated coordinates from an integer, or None for a head of size 0: there every
    coordinate is tdx or tdy exactly (0 * x + t), whatever the sines are."""
    a = axis_arguments(rect, yaw, pitch, roll)
    if a["size"] == 0:
        return None
    return min(abs(c - round(c)) for c in axis_coordinates(**a))
