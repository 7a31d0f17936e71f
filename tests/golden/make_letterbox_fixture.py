"""Record what the reference's own `letterbox_image` returns for the cases of tests/letterbox_cases.py.

Run where the reference checkout and Pillow are (the build container); the GPU box only reads the .npz.
  python tests/golden/make_letterbox_fixture.py

/root/reference/yolo_v3/utils.py is loaded BY PATH and its `letterbox_image` (lines 23-34) is EXECUTED
with the installed Pillow -- nothing of it is restated here.  `YOLO.detect` calls it as
`letterbox_image(image, tuple(reversed(self.model_image_size)))` (yolo_postprocess.py:186), i.e. with
(w, h).  Per case the file holds the geometry, the SHA-256 of the uint8 canvas, its [::8, ::8] subsample
and, for the small boxes and the two sample frames, the whole canvas; for a case the reference rejects,
the name of the exception it raised.
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests import letterbox_cases as LC   # noqa: E402

REF_UTILS = "/root/reference/yolo_v3/utils.py"


def load_reference_letterbox():
    spec = importlib.util.spec_from_file_location("reference_yolo_v3_utils", REF_UTILS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.letterbox_image


def run_case(letterbox_image, case):
    """-> (canvas uint8 [h, w, 3], geometry) or raises what the reference raises."""
    frame = LC.make_frame(case)
    image = Image.fromarray(frame, "RGB")
    boxed = letterbox_image(image, tuple(reversed(case.box_hw)))
    canvas = np.array(boxed)
    assert canvas.dtype == np.uint8 and canvas.shape == (*case.box_hw, 3)
    # the geometry lines of utils.py:25-33, evaluated by Python as the function evaluates them
    iw, ih = image.size
    w, h = tuple(reversed(case.box_hw))
    scale = min(w / iw, h / ih)
    nw, nh = int(iw * scale), int(ih * scale)
    return canvas, np.array([nw, nh, (w - nw) // 2, (h - nh) // 2], np.int32)


def main():
    letterbox_image = load_reference_letterbox()
    out = {"pillow_version": np.array(PIL.__version__)}
    for case in LC.CASES:
        if case.fails:
            try:
                run_case(letterbox_image, case)
            except Exception as e:          # noqa: BLE001  (recorded, whatever it is)
                out[case.name + "/error"] = np.array(type(e).__name__)
                print(f"{case.name}: reference raises {type(e).__name__}: {e}")
                continue
            raise SystemExit(f"{case.name}: the reference did not raise")
        canvas, geom = run_case(letterbox_image, case)
        out[case.name + "/geom"] = geom
        out[case.name + "/sha256"] = np.array(hashlib.sha256(canvas.tobytes()).hexdigest())
        out[case.name + "/sub"] = np.ascontiguousarray(canvas[::8, ::8])
        if case.full:
            out[case.name + "/full"] = canvas
        print(f"{case.name}: geom {geom.tolist()} sha256 {out[case.name + '/sha256']}")
    np.savez_compressed(LC.FIXTURE, **out)
    print(f"{LC.FIXTURE}: {os.path.getsize(LC.FIXTURE)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
