"""Would the device's sines, where they differ from libm, move an overlay endpoint?  A search on the CPU (docs/experiments.md, section 39).

tools/probes/overlay_trig_probe.hip found the device's double sin / cos one ulp from libm's at five of the bin-centre angles (the
table below: angle in degrees, which function, the sign of the device's move in magnitude).  This puts the device's value in place
of libm's in the numpy statement of tests/overlay_cases.py and counts the heads whose int() results change: yaw +-angle, pitch and
roll every multiple of 3 in -99..99, window origin 0 with every width 2..12289 (size 1..6144, tdx = size or size + 1/2).

    python tools/overlay_trig_search.py
"""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from tests import overlay_cases as OC  # noqa: E402

DEVICE_DIFFERS = {114: ("cos", +1), 117: ("cos", +1), 123: ("sin", +1), 138: ("cos", +1), 147: ("sin", -1)}      # measured on one MI355X


def main():
    sizes = np.arange(1, 6145, dtype=np.float64)
    steps = range(-99, 100, 3)
    heads, hits, t0 = 0, [], time.time()
    for angle, (which, ulp) in DEVICE_DIFFERS.items():
        for yaw in (float(angle), float(-angle)):
            for p in steps:
                for r in steps:
                    trig = list(OC.axis_trig(yaw, float(p), float(r)))
                    j = 0 if which == "cos" else 1
                    moved = list(trig)
                    moved[j] = math.nextafter(trig[j], math.copysign(math.inf, trig[j]) if ulp > 0 else 0.0)
                    for half in (0.0, 0.5):
                        t = sizes + half
                        a = OC.axis_coordinates_of(tuple(np.float64(v) for v in trig), t, t, sizes)
                        b = OC.axis_coordinates_of(tuple(np.float64(v) for v in moved), t, t, sizes)
                        heads += len(sizes)
                        for k in range(6):
                            for s in np.flatnonzero(np.trunc(a[k]) != np.trunc(b[k])):
                                hits.append((yaw, p, r, int(sizes[s]), half, k, float(a[k][s]), float(b[k][s])))
    print(f"{heads} heads, {len(hits)} with an endpoint that the device's value moves ({time.time() - t0:.1f} s)")
    for h in hits[:20]:
        print(h)


if __name__ == "__main__":
    main()
