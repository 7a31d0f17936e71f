"""Writes tests/golden/reference_detector_f32.json: the CPU-side figures that the float32 detector body's GPU tests
(tests/test_detector_f32_gpu.py) build their bounds from.  Everything is measured against the committed float64 fixture of the
EXECUTED reference bodies (reference_detector.npz, made by make_detector_fixture.py); nothing here needs the reference tree or a
GPU, only the built library for `whenet_detector_spec` and `whenet_frame_rects`.

  e32_body  {kind}/{h}x{w} -> per map max |R.forward(..., "f32") - float64 fixture map| / rms(fixture map): what float32
            arithmetic throughout costs on the CPU.  The whole-body GPU bound is 4 x this (another summation order).
  e32       per wide-operand single-layer case (tests/detector_f32_cases.py): max |float32 CPU - float64| on operands binary16
            cannot hold, as reference_detector.json["e32"] has it for the random operands.  The sums are exact integers below
            2^24; what remains is LeakyReLU's one float32 multiply and the float32 skip add.
  detect    per body, at the committed detect configuration (reference_detector.json["detect"], sample frame 0, 64 x 96):
            f32_count, f32_box_px and f32_score = the CPU-float32 maps' selection against the float64 oracle's (count, largest
            coordinate difference in pixels, largest score difference); oracle_boxes / oracle_scores / oracle_windows = the float64
            selection and demo_video.py's integer windows of its boxes (oracle/preprocess_oracle.py).

Run from the repository root:  python tests/golden/make_detector_f32_fixture.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "headposeestimation-whenet_amd"))

from tests import detector_cases as DC                    # noqa: E402
from tests import detector_f32_cases as FC                # noqa: E402
from tests import detector_ref as R                       # noqa: E402
from whenet_hip import _lib, detector_weights as DW       # noqa: E402


def measure():
    """The fixture's content, computed live (tests/test_detector_f32_cpu.py derives it again and compares)."""
    with open(os.path.join(FC.GOLDEN, "reference_detector.json")) as f:
        base = json.load(f)
    ref = FC.load_maps()
    meta = {"e32_body": {}, "e32": {}, "detect": {}}
    for name, kind in DC.KINDS:
        w = DW.synthetic(kind, DC.SEEDS[name])
        rows = _lib.detector_spec(kind)
        for h, wd in DC.SIZES:
            tag = f"{name}/{h}x{wd}"
            maps = R.forward(rows, w, DC.fixture_image(h, wd), "f32")
            want = [ref[f"{tag}/map{l}"] for l in range(len(maps))]
            meta["e32_body"][tag] = [FC.body_error(m, r) for m, r in zip(maps, want)]
            if [h, wd] != base["detect"][name]["size"]:
                continue
            d = base["detect"][name]
            ob, os_, oc, oi = FC.oracle_detect(name, d, want)
            fb, fs, fc, fi = FC.oracle_detect(name, d, maps)
            same = len(fb) == len(ob) and list(fi) == list(oi)
            meta["detect"][name] = {
                "f32_count": int(len(fb)),
                "f32_box_px": FC.box_distance(fb, ob) if same else None,
                "f32_score": float(np.abs(fs.astype(np.float64) - os_).max()) if same else None,
                "oracle_boxes": [[float(v) for v in b] for b in ob], "oracle_scores": [float(v) for v in os_],
                "oracle_windows": FC.oracle_windows(ob).tolist(),
                "f32_windows": _lib.frame_rects(*DC.sample_frame(0).shape[:2], fb).tolist(),
            }
    for cname in FC.WIDE_CASES:
        c = FC.CASES[cname]
        x, x2, kernel, bias, skip = FC.wide_operands(c)
        leaky = not c["f32_out"]
        f64 = R.conv(x, kernel, bias, c["stride"], leaky, x2=x2, skip=skip, dtype=np.float64)
        f32 = R.conv(x, kernel, bias, c["stride"], leaky, x2=x2, skip=skip, dtype=np.float32)
        meta["e32"][cname] = float(np.abs(f32.astype(np.float64) - f64).max())
    return meta


def main():
    meta = measure()
    with open(os.path.join(FC.GOLDEN, "reference_detector_f32.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps({k: meta[k] for k in ("e32_body", "e32")}, indent=1))
    for name, d in meta["detect"].items():
        print(name, {k: d[k] for k in ("f32_count", "f32_box_px", "f32_score")}, "windows equal:", d["f32_windows"] == d["oracle_windows"])


if __name__ == "__main__":
    main()
