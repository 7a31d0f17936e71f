"""Writes tests/golden/reference_detector.npz / .json: what the reference's own `yolo_body` and `tiny_yolo_body`
(yolo_v3/model.py:73-122) compute when EXECUTED (tests/detector_harness.py: the reference's wiring under float64 stand-ins for
its Keras layers) on seeded synthetic weights, and the CPU-side figures the GPU tests' tolerances are built from.

For both bodies (3 anchors per scale, 1 class; whenet_hip.detector_weights.synthetic, seeds in tests/detector_cases.py) and a
32 x 32 and a 64 x 96 letterbox of sample frame 0:
  npz   {kind}/{h}x{w}/map{l}   float64 output maps, coarsest first (float64, not float32: the table test compares to 1e-10)
        {kind}/{h}x{w}/emu{l}   the same maps from the binary16-storage emulation (tests/detector_ref.py mode "f16emu")
  json  rows      the recorded convolution / pool list in creation order
        stats     per row (rms, max |x|) of its output -- every rms must lie in [0.1, 10], every max below 1000
        routes    type and channels of darknet.layers[152] / [92]
        emu_err   per map max |emu - ref| / rms(ref): the whole-body GPU bound is 3 x this
        e32       per single-layer case (tests/detector_cases.py): max |float32 CPU - float64| on the random operands
        detect    score threshold at which the float64 oracle (oracle/yolo_oracle.py) selects 3..max_boxes boxes on the
                  64 x 96 maps of sample frame 0, and how many

Run from the repository root, where /root/reference is present:  python tests/golden/make_detector_fixture.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "headposeestimation-whenet_amd"))

from oracle import yolo_oracle as Y                       # noqa: E402
from tests import detector_cases as DC                    # noqa: E402
from tests import detector_harness as Hn                  # noqa: E402
from tests import detector_ref as R                       # noqa: E402
from whenet_hip import _lib, detector_weights as DW       # noqa: E402

MAX_BOXES, IOU = 20, 0.45


def main():
    assert Hn.available(), "the reference tree is needed to make this fixture"
    arrays, meta = {}, {"seeds": DC.SEEDS, "rows": {}, "stats": {}, "routes": {}, "emu_err": {}, "e32": {}, "detect": {}}
    for name, kind in DC.KINDS:
        w = DW.synthetic(kind, DC.SEEDS[name])
        rows = _lib.detector_spec(kind)
        for h, wd in DC.SIZES:
            tag = f"{name}/{h}x{wd}"
            img = DC.fixture_image(h, wd)
            run = Hn.run(kind, w, img)
            emu = R.forward(rows, w, img, "f16emu")
            meta["rows"][name] = [[r[k] for k in ("op", "k", "stride", "cin", "cout", "bn", "leaky")] for r in run["rows"]]
            meta["stats"][tag] = run["stats"]
            assert all(0.1 <= s[0] <= 10 and s[1] < 1000 for s in run["stats"]), (tag, min(run["stats"]), max(run["stats"]))
            if kind == 0:
                meta["routes"][name] = run["routes"]
            meta["emu_err"][tag] = []
            for l, (m, e) in enumerate(zip(run["maps"], emu)):
                arrays[f"{tag}/map{l}"] = m.astype(np.float64)
                arrays[f"{tag}/emu{l}"] = e.astype(np.float32)
                meta["emu_err"][tag].append(float(np.abs(e - m).max() / np.sqrt(np.mean(m ** 2))))
            print(tag, "emu_err", meta["emu_err"][tag], "rms", min(s[0] for s in run["stats"]), max(s[0] for s in run["stats"]))
            if (h, wd) == (64, 96):
                frame = DC.sample_frame(0)
                anchors = np.array(DC.ANCHORS[name], np.float32).reshape(-1, 2)
                maps = [m[0] for m in run["maps"]]
                chosen = None
                for thr in np.arange(0.90, 0.05, -0.01):
                    b, s, c = Y.yolo_eval(maps, anchors, 1, frame.shape[:2], max_boxes=MAX_BOXES, score_threshold=float(thr), iou_threshold=IOU)
                    if 5 <= len(b) <= MAX_BOXES:
                        chosen = (round(float(thr), 2), len(b))
                        break
                assert chosen, "no threshold selects 5..20 boxes"
                meta["detect"][name] = {"score": chosen[0], "iou": IOU, "max_boxes": MAX_BOXES, "oracle_count": chosen[1], "size": [h, wd]}
                print(tag, "detect", meta["detect"][name])
    for cname, c in DC.CONV_CASES:
        x, x2, kernel, bias, skip = DC.random_operands(c, DC.case_seed(cname))
        leaky = not c["f32_out"]
        ref = R.conv(x, kernel, bias, c["stride"], leaky, x2=x2, skip=skip, dtype=np.float64)
        f32 = R.conv(x, kernel, bias, c["stride"], leaky, x2=x2, skip=skip, dtype=np.float32)
        meta["e32"][cname] = float(np.abs(f32.astype(np.float64) - ref).max())
    here = os.path.dirname(os.path.abspath(__file__))
    np.savez_compressed(os.path.join(here, "reference_detector.npz"), **arrays)
    with open(os.path.join(here, "reference_detector.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("e32", meta["e32"])
    print("wrote", sum(a.nbytes for a in arrays.values()), "array bytes")


if __name__ == "__main__":
    main()
