"""Records what the reference's own `draw_axis` (utils.py:13-43) hands to `cv2.line` -> tests/golden/reference_draw_axis.npz.

utils.py is EXECUTED as it stands under tests/refharness.py (its `cv2` is the recording stand-in) for every head of
tests/overlay_cases.reference_heads(): 4,096 seeded heads and the designed ones.  The call is the one INTEGRATION.md documents,
with Python-float arguments so that nothing depends on NumPy's scalar promotion:

    draw_axis(frame, yaw, pitch, roll, tdx=(x0 + x1) / 2, tdy=(y0 + y1) / 2, size=(x1 - x0) // 2)

Stored: rects int32 [n,4], ypr float32 [n,3], lines int32 [n,3,4] = (Px, Py, Qx, Qy) of the three calls in order, colours int32
[n,3,3] and thickness int32 [n,3] as passed.  tests/test_overlay_cpu.py compares `whenet_overlay_segments` with it and, wherever
the reference tree is present, reproduces it live.

The same call on the exact-ratio table of tests/overlay_lattice_cases.py -- every sensitive head and every 7th other head of every
window, in the table's order -- -> tests/golden/reference_draw_axis_lattice.npz: index int32 [n] = window * 65536 + the head's row
in its window's table, lines int16 [n,3,4].  The colours and the thickness are those of the first fixture (asserted, not stored).

    python tests/golden/make_overlay_fixture.py [seeded] [lattice]
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

from tests import overlay_cases as OC  # noqa: E402
from tests import overlay_lattice_cases as LC  # noqa: E402
from tests import refharness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_draw_axis.npz")
OUT_LATTICE = os.path.join(ROOT, "tests", "golden", "reference_draw_axis_lattice.npz")


def run_reference(rects, ypr):
    """utils.draw_axis executed for every head -> (lines [n,3,4], colours [n,3,3], thickness [n,3])."""
    n = len(rects)
    lines = np.zeros((n, 3, 4), np.int32)
    colours = np.zeros((n, 3, 3), np.int32)
    thick = np.zeros((n, 3), np.int32)
    frame = np.zeros((4, 4, 3), np.uint8)
    with refharness.reference() as R:
        utils = R.load("utils")
        for i in range(n):
            a = OC.axis_arguments(rects[i], *ypr[i])
            del R.cv2.calls[:]
            utils.draw_axis(frame, a["yaw"], a["pitch"], a["roll"], tdx=a["tdx"], tdy=a["tdy"], size=a["size"])
            calls = [c for c in R.cv2.calls if c[0] == "line"]
            assert len(calls) == 3, calls
            for j, (_, p, q, colour, thickness) in enumerate(calls):
                lines[i, j] = (p[0], p[1], q[0], q[1])
                colours[i, j] = colour
                thick[i, j] = thickness
    return lines, colours, thick


def lattice_heads():
    """(index int32 [n], rects int32 [n,4], ypr float32 [n,3]) of the recorded heads of the exact-ratio table."""
    index, rects, ypr = [], [], []
    for T in LC.tables():
        rows = T.recorded()
        index.append(T.index * 65536 + rows)
        rects.append(T.rects[rows])
        ypr.append(T.ypr[rows])
    return np.concatenate(index).astype(np.int32), np.concatenate(rects), np.concatenate(ypr)


def run_reference_lattice():
    """-> (index int32 [n], lines int16 [n,3,4]) of the executed reference on lattice_heads()."""
    index, rects, ypr = lattice_heads()
    lines, colours, thick = run_reference(rects, ypr)
    assert (colours == np.array([(0, 0, 255), (0, 255, 0), (255, 0, 0)])).all() and (thick == 2).all()
    assert np.abs(lines).max() < 1 << 15
    return index, lines.astype(np.int16)


def main(which):
    if "seeded" in which:
        rects, ypr = OC.reference_heads()
        lines, colours, thick = run_reference(rects, ypr)
        np.savez_compressed(OUT, rects=rects, ypr=ypr, lines=lines, colours=colours, thickness=thick)
        print(f"{OUT}: {len(rects)} heads, {os.path.getsize(OUT)} bytes")
    if "lattice" in which:
        index, lines = run_reference_lattice()
        np.savez_compressed(OUT_LATTICE, index=index, lines=lines)
        print(f"{OUT_LATTICE}: {len(index)} heads, {os.path.getsize(OUT_LATTICE)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:] or ["seeded", "lattice"])
