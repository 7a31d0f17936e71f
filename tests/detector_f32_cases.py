"""Operands and expected values of the float32 detector body's tests (tests/test_detector_f32_cpu.py, tests/test_detector_f32_gpu.py)
and of tests/golden/make_detector_f32_fixture.py: what tests/detector_cases.py does not have because binary16 storage could not
hold it.

  * `expected_f32`: the float32 kernel's arithmetic on exact operands -- `detector_cases.integer_expected` without its one
    rounding to binary16 (every layer stores float32 there, as the output convolutions always did).
  * `wide_operands`: sparse integers that binary16 cannot hold (odd values above 2,048, one above 65,504) against the small
    integer weights of `integer_operands`, so that every partial sum stays an exact float32 integer (< 2^24) in any order.
  * `detect_figures`: the boxes a set of maps selects at a committed detect configuration, against the float64 oracle's.
"""
from __future__ import annotations

import json
import os

import numpy as np

from tests import detector_cases as DC
from tests import detector_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDE_CASES = ("k3s1_5x7", "k1_1024to512", "k3_skip_deep", "cat_n2_6x10")
CASES = dict(DC.CONV_CASES)
BIG = 70001.0                                    # odd, above binary16's largest finite value 65,504


def expected_f32(c, x, x2, kernel, bias, skip, leaky):
    """(expected float32 output, magnitude bound sum |w||x| + |bias| + |skip|): exact accumulation, + bias exact, ONE float32
    multiply by float32(0.1) for negative values, float32 add of the skip, no other rounding."""
    return DC.integer_expected(dict(c, f32_out=True), x, x2, kernel, bias, skip, leaky)


def _widen(a, salt):
    """Every non-zero of a small-integer tensor times an odd factor in 2,049..3,999 (|1| -> an odd value above 2,048), and the
    first non-zero replaced by +-BIG."""
    idx = np.arange(a.size, dtype=np.int64).reshape(a.shape)
    out = a * (2049 + 2 * ((idx * 7 + salt) % 976)).astype(np.float64)
    first = np.flatnonzero(a.reshape(-1))[0]
    out.reshape(-1)[first] = np.sign(a.reshape(-1)[first]) * BIG
    return out


def wide_operands(c):
    """`integer_operands` with the activations (both sources and the skip) widened; weights and bias as they are."""
    x, x2, kernel, bias, skip = DC.integer_operands(c)
    return (_widen(x, 1), None if x2 is None else _widen(x2, 2), kernel, bias, None if skip is None else _widen(skip, 3))


def load_meta():
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        meta = json.load(f)
    with open(os.path.join(GOLDEN, "reference_detector_f32.json")) as f:
        meta32 = json.load(f)
    return meta, meta32


def load_maps():
    with np.load(os.path.join(GOLDEN, "reference_detector.npz")) as z:
        return {k: z[k] for k in z.files}


def body_error(m, ref):
    """max |x - ref| / rms(ref) of one output map."""
    return float(np.abs(np.asarray(m, np.float64) - ref).max() / np.sqrt(np.mean(ref ** 2)))


def oracle_detect(name, d, maps):
    """The selection of oracle/yolo_oracle.py on `maps` ([1,gh,gw,18] each) at the committed configuration d of body `name`, on
    sample frame 0: (boxes, scores, classes, index)."""
    from oracle import yolo_oracle as Y
    anchors = np.array(DC.ANCHORS[name], np.float32).reshape(-1, 2)
    return Y.yolo_eval([m[0] for m in maps], anchors, 1, DC.sample_frame(0).shape[:2], max_boxes=d["max_boxes"],
                       score_threshold=d["score"], iou_threshold=d["iou"], return_index=True)


def oracle_windows(boxes):
    """demo_video.py's integer windows of the boxes on sample frame 0, by the numpy restatement (oracle/preprocess_oracle.py)."""
    from oracle import preprocess_oracle as P
    fh, fw = DC.sample_frame(0).shape[:2]
    return np.array([P.crop_rect(fh, fw, b) for b in boxes], np.int32).reshape(-1, 4)


def box_distance(boxes, ref_boxes):
    """Largest coordinate difference in pixels, box i against box i."""
    return float(np.abs(np.asarray(boxes, np.float64) - np.asarray(ref_boxes, np.float64)).max())
