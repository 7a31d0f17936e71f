"""The labels of the pose overlay (include/whenet_hip.h, LABELS) stated in numpy and Python integers -- the statement that
`whenet_annotate_host_ex(WHENET_DISPLAY_FULL)` is held to byte for byte, and the kernels through it -- with the table of cases.

Text: line i is "yaw: ", "pitch: " or "roll: " + Python's own `"{}".format(np.round(np.float32(a)))`, the expression of
demo_video.py:32-34.  A head has labels iff it paints its axes and every rounded angle is within +-9999.  Origins (x0, y0),
(x0, y0 - 15), (x0, y0 - 30).  Font: this file's OWN copy of the header's stroke table; a pixel is painted by a stroke iff its
distance to the closed segment is <= 1/2 (v.d <= 0: X = P; v.d >= L2: X = Q; else 4 (v x d)^2 <= L2), the advance is 7 pixels.
Colour (100, 255, 0) as B, G, R.  Paint order: head by head, rectangle sides, X, Y, Z, then the yaw, pitch and roll line.
"""
import numpy as np

from tests import overlay_cases as OC

GLYPHS = "0123456789achiloprtwy: -."
FONT = {
    '0': [(1, -8, 3, -8), (3, -8, 4, -7), (4, -7, 4, -1), (4, -1, 3, 0), (3, 0, 1, 0), (1, 0, 0, -1), (0, -1, 0, -7), (0, -7, 1, -8)],
    '1': [(1, -6, 2, -8), (2, -8, 2, 0), (1, 0, 3, 0)],
    '2': [(0, -8, 4, -8), (4, -8, 4, -4), (4, -4, 0, -4), (0, -4, 0, 0), (0, 0, 4, 0)],
    '3': [(0, -8, 4, -8), (4, -8, 4, 0), (4, 0, 0, 0), (1, -4, 4, -4)],
    '4': [(3, -8, 0, -3), (0, -3, 4, -3), (3, -8, 3, 0)],
    '5': [(4, -8, 0, -8), (0, -8, 0, -4), (0, -4, 4, -4), (4, -4, 4, 0), (4, 0, 0, 0)],
    '6': [(4, -8, 0, -8), (0, -8, 0, 0), (0, 0, 4, 0), (4, 0, 4, -4), (4, -4, 0, -4)],
    '7': [(0, -8, 4, -8), (4, -8, 1, 0)],
    '8': [(0, -8, 4, -8), (4, -8, 4, 0), (4, 0, 0, 0), (0, 0, 0, -8), (0, -4, 4, -4)],
    '9': [(4, -4, 0, -4), (0, -4, 0, -8), (0, -8, 4, -8), (4, -8, 4, 0), (4, 0, 0, 0)],
    'a': [(4, -5, 4, 0), (1, -5, 3, -5), (3, -5, 4, -4), (4, -1, 3, 0), (3, 0, 1, 0), (1, 0, 0, -1), (0, -1, 0, -4), (0, -4, 1, -5)],
    'c': [(1, -5, 3, -5), (3, -5, 4, -4), (4, -1, 3, 0), (3, 0, 1, 0), (1, 0, 0, -1), (0, -1, 0, -4), (0, -4, 1, -5)],
    'h': [(0, -8, 0, 0), (0, -4, 1, -5), (1, -5, 3, -5), (3, -5, 4, -4), (4, -4, 4, 0)],
    'i': [(1, -5, 2, -5), (2, -5, 2, 0), (1, 0, 3, 0), (2, -7, 2, -7)],
    'l': [(2, -8, 2, -1), (2, -1, 3, 0)],
    'o': [(1, -5, 3, -5), (3, -5, 4, -4), (4, -4, 4, -1), (4, -1, 3, 0), (3, 0, 1, 0), (1, 0, 0, -1), (0, -1, 0, -4), (0, -4, 1, -5)],
    'p': [(0, -5, 0, 3), (1, -5, 3, -5), (3, -5, 4, -4), (4, -4, 4, -1), (4, -1, 3, 0), (3, 0, 1, 0), (1, 0, 0, -1), (0, -4, 1, -5)],
    'r': [(0, -5, 0, 0), (0, -3, 2, -5), (2, -5, 4, -5)],
    't': [(2, -8, 2, -1), (2, -1, 3, 0), (3, 0, 4, 0), (0, -5, 4, -5)],
    'w': [(0, -5, 1, 0), (1, 0, 2, -3), (2, -3, 3, 0), (3, 0, 4, -5)],
    'y': [(0, -5, 2, 0), (4, -5, 1, 3), (1, 3, 0, 3)],
    ':': [(2, -5, 2, -4), (2, -1, 2, 0)],
    ' ': [],
    '-': [(0, -4, 4, -4)],
    '.': [(2, -1, 2, 0), (3, -1, 3, 0)],
}
BOX_X, BOX_Y = (0, 5), (-9, 3)             # a glyph's box, inclusive
ADVANCE, LINE_STEP, MAX_CHARS, MAX_ABS = 7, 15, 14, 9999
NAMES = ("yaw: ", "pitch: ", "roll: ")
COLOUR_BGR = (100, 255, 0)
SIMPLE, FULL = 0, 1


# ---- the raster rules in Python integers ------------------------------------------------------------------------------------
def hit(px, py, qx, qy, x, y, reach=1):
    """Is (x, y) within distance reach / 2 of the closed segment?  reach 1: the thin rule; reach 2: the rule of the axes."""
    dx, dy, vx, vy = qx - px, qy - py, x - px, y - py
    L2, t = dx * dx + dy * dy, vx * dx + vy * dy
    if t <= 0:
        return 4 * (vx * vx + vy * vy) <= reach * reach
    if t >= L2:
        return 4 * ((x - qx) ** 2 + (y - qy) ** 2) <= reach * reach
    c = vx * dy - vy * dx
    return 4 * c * c <= reach * reach * L2


_PIXELS = {}


def glyph_pixels(ch, segs=None, margin=3):
    """The set of (x, y) a glyph paints, searched `margin` pixels beyond its box on every side."""
    if segs is None:
        if (ch, margin) not in _PIXELS:
            _PIXELS[(ch, margin)] = frozenset(glyph_pixels(ch, FONT[ch], margin))
        return _PIXELS[(ch, margin)]
    return {(x, y) for x in range(BOX_X[0] - margin, BOX_X[1] + margin + 1) for y in range(BOX_Y[0] - margin, BOX_Y[1] + margin + 1)
            if any(hit(*s, x, y) for s in segs)}


# ---- text -------------------------------------------------------------------------------------------------------------------
def number(a):
    """What the reference prints for the float32 angle a (demo_video.py:32-34)."""
    return "{}".format(np.round(np.float32(a)))


def in_range(a):
    r = np.round(np.float32(a))
    return bool(np.isfinite(r)) and abs(float(r)) <= MAX_ABS


def labels(rect, yaw, pitch, roll, valid=1):
    """-> (texts [3], origins [3] of (x, y), flags) as whenet_overlay_labels returns them."""
    seg, flags = OC.segments(rect, yaw, pitch, roll, valid=valid)
    origins = [(seg[0], seg[1] - LINE_STEP * i) for i in range(3)]
    if flags & 2 and all(in_range(a) for a in (yaw, pitch, roll)):
        return [n + number(a) for n, a in zip(NAMES, (yaw, pitch, roll))], origins, flags | 4
    return ["", "", ""], origins, flags


def paint_text(out, order, text, ox, oy):
    h, w = out.shape[:2]
    colour = COLOUR_BGR if order == OC.BGR else COLOUR_BGR[::-1]
    assert len(text) <= MAX_CHARS, text
    for i, ch in enumerate(text):
        for gx, gy in glyph_pixels(ch, margin=0):
            x, y = ox + ADVANCE * i + gx, oy + gy
            if 0 <= x < w and 0 <= y < h:
                out[y, x] = colour


def paint(frame, order, rects, valid, ypr, display=FULL):
    """The annotated frame, packed, in the frame's channel order."""
    out = np.array(frame, np.uint8, copy=True)
    h, w = out.shape[:2]
    for i, rect in enumerate(rects):
        v = 1 if valid is None else int(valid[i])
        seg, flags = OC.segments(rect, *ypr[i], valid=v)
        for px, py, qx, qy, colour in OC.head_primitives(seg, flags):
            out[OC.hit_mask(h, w, px, py, qx, qy)] = OC.colour_bytes(colour, order)
        if display == FULL:
            texts, origins, lflags = labels(rect, *ypr[i], valid=v)
            if lflags & 4:
                for text, (ox, oy) in zip(texts, origins):
                    paint_text(out, order, text, ox, oy)
    return out


def annotate(frame, order, rects, valid, ypr, fmt, matrix=OC.BT601, display=FULL):
    return OC.planes_of(paint(frame, order, rects, valid, ypr, display), order, fmt, matrix)


# ---- the cases --------------------------------------------------------------------------------------------------------------
DESIGNED_ANGLES = (0.0, -0.0, 0.3, -0.3, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, 99.49999, -179.6, 177.0, 9999.4, 9999.5)
FIXTURE_SEED, FIXTURE_SPREAD = 20261101, 64


def fixture_angles():
    """float32 [n,3]: every designed angle three times in a head, every designed angle with its two successors, and a seeded
    spread over [-180, 180]."""
    d = list(DESIGNED_ANGLES)
    rows = [(a, a, a) for a in d] + [(d[i], d[(i + 1) % len(d)], d[(i + 2) % len(d)]) for i in range(len(d))]
    spread = np.random.default_rng(FIXTURE_SEED).uniform(-180, 180, (FIXTURE_SPREAD, 3))
    return np.concatenate([np.asarray(rows, np.float32), spread.astype(np.float32)])


def label_heads(h, w):
    """(rects int32 [8,4], valid int32 [8], ypr float32 [8,3]) on an h x w frame (w >= 101): a window with y0 < 30 (its lines are
    clipped off the top), one with x0 < 0, one whose x0 is 13 pixels from the right edge, one with an angle that is not finite
    (rectangle only), one with valid = 0, one with a rounded angle of 10000 (axes, no labels), and two that overlap: the second one's
    rectangle crosses the first one's text."""
    nan = float("nan")
    rects = [(12, 20, 60, 70), (50, -9, 90, 30), (45, w - 13, 80, w), (40, 40, 70, 70), (30, 30, 60, 60), (60, 60, 90, 100),
             (50, 40, 85, 90), (48, 50, 95, 100)]
    ypr = [(10.2, -5.5, 2.5), (-179.6, 99.49999, -0.3), (177.0, 3.5, -2.5), (nan, 1, 2), (5, 6, 7), (9999.5, 1, 2), (33, -44, 55),
           (-12, 7, 0.5)]
    valid = [1, 1, 1, 1, 0, 1, 1, 1]
    return np.asarray(rects, np.int32), np.asarray(valid, np.int32), np.asarray(ypr, np.float32)


def seam_heads():
    """On a 160 x 48 (w x h) frame: a head at x0 = 120, y0 = 40 whose lines cross the tile edge at x = 128 and the edges at y = 16
    and y = 32 (its line boxes are rows 31..43, 16..28 and 1..13: one line in each tile row), a head whose lines start at x = 127,
    and a head at y0 = 36 whose glyphs themselves straddle y = 32 and y = 16."""
    rects = [(40, 120, 47, 150), (44, 127, 47, 140), (36, 60, 47, 90)]
    ypr = [(-123.4, 56.7, -8.9), (100.0, -100.0, 0.0), (88.0, -17.5, 4.0)]
    return np.asarray(rects, np.int32), None, np.asarray(ypr, np.float32)


def capacity_heads(same):
    """256 labelled heads on a 128 x 48 frame: all with one window, or with windows one pixel apart."""
    rng = np.random.default_rng(256 + int(same))
    rects = [(40, 3, 46, 20) if same else (33 + i // 32, 1 + i % 32, 46, 40 + i % 32) for i in range(256)]
    ypr = rng.uniform(-180, 180, (256, 3)).astype(np.float32)
    return np.asarray(rects, np.int32), None, ypr
