"""The heads at which the host's libm and the device's math library could disagree about an overlay endpoint, as a table.

Every endpoint of an axis is int(size * (products of sines and cosines) + t).  A last-bit difference in one sine moves the int()
only where the un-truncated coordinate sits on or next to an integer, and with an integer `size` that happens where the products
are exact ratios: sines and cosines are rational only at multiples of 30 degrees (Niven), products such as cos 45 * cos 45 = 1/2
and sin 15 * cos 15 = 1/4 occur at multiples of 15.  There the double result lands on the integer or half-integer or one ulp
beside it (libm's sin of the double nearest pi/6 is 0.49999999999999994).  Such angles are outputs of a real forward: a head whose
softmax saturates decodes to its bin centre, and the bin centres are the multiples of 3 degrees.

The table, per window of WINDOWS:
  lattice      yaw -180..180 step 15, pitch and roll -90..90 step 15: 4,225 triples (yaw slowest, roll fastest)
  bin centres  yaw -180..177 step 3 with the eight (pitch, roll) of BIN_PITCH_ROLL: 960 triples
  controls     every 7th lattice triple with each angle moved to the next float32 above it, on the first three windows: one
               float32 step moves a coordinate by about 1e-6, which no last bit reaches

A head is SENSITIVE if moving any one of its six sin / cos values by one ulp up or down changes at least one of its six int()
results: `perturbed_segments` returns the twelve perturbed segment sets.  The sines and cosines themselves come from Python's
math module (the libm `whenet_overlay_segments` calls), never from numpy's own vector sin / cos; everything after them is float64
numpy, where every multiplication and addition rounds on its own exactly as the Python floats of tests/overlay_cases.py do.
"""
import functools

import numpy as np

from tests import overlay_cases as OC

WINDOWS = ((0, 0, 8, 8), (0, 0, 64, 64), (100, 200, 300, 500), (60, 10, 150, 211), (20, 0, 70, 25), (50, 7, 135, 107))   # y0, x0, y1, x1
LATTICE_YAW = tuple(range(-180, 181, 15))
LATTICE_PITCH_ROLL = tuple(range(-90, 91, 15))
BIN_YAW = tuple(range(-180, 180, 3))
BIN_PITCH_ROLL = ((0, 0), (30, 0), (0, 30), (45, 45), (60, -60), (-30, 90), (-99, 96), (3, -3))
CONTROL_STEP, CONTROL_WINDOWS = 7, 3
LATTICE, BIN, CONTROL = 0, 1, 2
FAMILY_NAME = ("lattice", "bin centre", "control")
REACH = 1                       # the raster paints to distance 1 of a segment
RECORD_STEP = 7                 # the executed reference records every sensitive head and every 7th other one


def lattice_angles():
    return np.asarray([(y, p, r) for y in LATTICE_YAW for p in LATTICE_PITCH_ROLL for r in LATTICE_PITCH_ROLL], np.float32)


def bin_centre_angles():
    return np.asarray([(y, p, r) for y in BIN_YAW for p, r in BIN_PITCH_ROLL], np.float32)


def control_angles():
    return np.nextafter(lattice_angles()[::CONTROL_STEP], np.float32(np.inf))


def trig_of(ypr):
    """float64 [n, 6]: OC.axis_trig of every row, one libm call per distinct angle."""
    out = np.empty((len(ypr), 6))
    memo = {}
    for i, (y, p, r) in enumerate(np.asarray(ypr, np.float32).tolist()):          # .tolist(): the float32 values as Python floats
        key = (y, p, r)
        if key not in memo:
            memo[key] = OC.axis_trig(y, p, r)
        out[i] = memo[key]
    return out


def ints_of(trig, tdx, tdy, size):
    """int64 [n, 6]: int() of the six coordinates (X.x, X.y, Y.x, Y.y, Z.x, Z.y) from trig float64 [n, 6]."""
    c = OC.axis_coordinates_of(tuple(trig[:, j] for j in range(6)), np.float64(tdx), np.float64(tdy), np.float64(size))
    return np.trunc(np.stack(c, axis=1)).astype(np.int64)


def perturbations(trig):
    """The twelve one-ulp moves of trig [n, 6] as [12, n, 6]: value j up (index 2 j) and down (2 j + 1)."""
    out = np.repeat(trig[None], 12, axis=0)
    for j in range(6):
        out[2 * j, :, j] = np.nextafter(trig[:, j], np.inf)
        out[2 * j + 1, :, j] = np.nextafter(trig[:, j], -np.inf)
    return out


def segments_of(rect, ints):
    """int64 [n, 16] in the layout of OC.segments from the six ints of every head of one window."""
    y0, x0, y1, x1 = (int(v) for v in rect)
    seg = np.empty((len(ints), 16), np.int64)
    seg[:, :4] = (x0, y0, x1, y1)
    for a in range(3):
        seg[:, 4 + 4 * a] = int((x0 + x1) / 2)
        seg[:, 5 + 4 * a] = int((y0 + y1) / 2)
        seg[:, 6 + 4 * a: 8 + 4 * a] = ints[:, 2 * a: 2 * a + 2]
    return seg


def perturbed_segments(rect, ypr):
    """(segments int64 [n, 16], perturbed int64 [12, n, 16]) of the heads `ypr` [n, 3] on one window: the numpy statement's
    segments, and what they become when one of the six sin / cos values moves by one ulp (perturbations() gives the order)."""
    a = OC.axis_arguments(rect, 0, 0, 0)
    trig = trig_of(ypr)
    base = segments_of(rect, ints_of(trig, a["tdx"], a["tdy"], a["size"]))
    moved = np.stack([segments_of(rect, ints_of(t, a["tdx"], a["tdy"], a["size"])) for t in perturbations(trig)])
    return base, moved


def sensitivity(rect, ypr):
    """bool [n]: the heads of which at least one perturbed segment set differs from the unperturbed one."""
    base, moved = perturbed_segments(rect, ypr)
    return (moved != base[None]).any(axis=(0, 2))


class WindowTable:
    """The table of one window: rect, ypr float32 [n, 3], family int [n], segments int64 [n, 16] (the numpy statement's),
    perturbed int64 [12, n, 16], sensitive bool [n], and the frame size that holds every endpoint grown by the raster's reach."""

    def __init__(self, index):
        self.index, self.rect = index, WINDOWS[index]
        parts = [(lattice_angles(), LATTICE), (bin_centre_angles(), BIN)]
        if index < CONTROL_WINDOWS:
            parts.append((control_angles(), CONTROL))
        self.ypr = np.concatenate([a for a, _ in parts]).astype(np.float32)
        self.family = np.concatenate([np.full(len(a), f) for a, f in parts])
        self.segments, self.perturbed = perturbed_segments(self.rect, self.ypr)
        self.sensitive = (self.perturbed != self.segments[None]).any(axis=(0, 2))
        ends = np.concatenate([self.segments[None], self.perturbed]).reshape(-1, 8, 2)
        assert ends.min() >= 0          # (windows that start at 0 have endpoints on row / column 0: the frame cannot grow that way)
        self.w, self.h = (int(v) + REACH + 1 for v in ends.max(axis=(0, 1)))
        self.rects = np.tile(np.asarray(self.rect, np.int32), (len(self.ypr), 1))

    def frame(self):
        return OC.frame_for(self.h, self.w, 7000 + self.index)

    def recorded(self):
        """The indices of the heads that the executed reference records: every sensitive one, every RECORD_STEP-th other one."""
        other = np.flatnonzero(~self.sensitive)[::RECORD_STEP]
        return np.sort(np.concatenate([np.flatnonzero(self.sensitive), other]))

    def describe(self, i):
        yaw, pitch, roll = self.ypr[i].tolist()
        return f"window {self.rect} {FAMILY_NAME[self.family[i]]} yaw {yaw!r} pitch {pitch!r} roll {roll!r} segments {self.segments[i, 4:].tolist()}"


@functools.lru_cache(maxsize=None)
def table(index):
    return WindowTable(index)


def tables():
    return [table(i) for i in range(len(WINDOWS))]


def hidden_by_a_later_axis(seg, moved):
    """True if the picture cannot tell `moved` from `seg`: every axis whose end differs lies, in both forms, on the closed
    segment of an axis painted after it (same start, collinear, not longer).  Then every pixel within the reach of the earlier
    axis is within the reach of the later one, which is painted over it in both pictures."""
    def on_segment(p, q, x):
        d, v = q - p, x - p
        return d[0] * v[1] - d[1] * v[0] == 0 and 0 <= d @ v <= d @ d and (d @ d > 0 or v @ v == 0)

    axes = [(np.asarray(seg[4 + 4 * a: 6 + 4 * a]), np.asarray(seg[6 + 4 * a: 8 + 4 * a]), np.asarray(moved[6 + 4 * a: 8 + 4 * a])) for a in range(3)]
    for a, (p, q, q_moved) in enumerate(axes):
        if np.array_equal(q, q_moved):
            continue
        if not any(np.array_equal(axes[b][1], axes[b][2]) and on_segment(p, axes[b][1], q) and on_segment(p, axes[b][1], q_moved)
                   for b in range(a + 1, 3)):
            return False
    return True


def paint_segments(frame, seg):
    """One head's 16 segment ints painted on a copy of `frame` (BGR) by the numpy raster statement.  OC.hit_mask is evaluated on
    every primitive's box grown by the reach, translated to the box's corner: the rule looks at differences of coordinates only
    and is false outside that box (tests/test_overlay_cpu.py holds this form to OC.paint's whole-frame one)."""
    out = np.array(frame, np.uint8, copy=True)
    h, w = out.shape[:2]
    for px, py, qx, qy, colour in OC.head_primitives([int(v) for v in seg], 3):
        x0, x1 = max(min(px, qx) - REACH, 0), min(max(px, qx) + REACH, w - 1)
        y0, y1 = max(min(py, qy) - REACH, 0), min(max(py, qy) + REACH, h - 1)
        if x0 > x1 or y0 > y1:
            continue
        box = out[y0:y1 + 1, x0:x1 + 1]
        box[OC.hit_mask(y1 - y0 + 1, x1 - x0 + 1, px - x0, py - y0, qx - x0, qy - y0)] = OC.colour_bytes(colour, OC.BGR)
    return out
