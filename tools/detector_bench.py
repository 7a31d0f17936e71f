"""Measurements of the detector body (csrc/dconv.hip, csrc/detector.cpp) on seeded synthetic weights.

  python tools/detector_bench.py [--size 416 416] [--reps 30] [--kinds full tiny] [--batch 1] [--dtype f16|f32]
      Per body: the FLOP count of one image from the layer table, the host-to-host wall time of whenet_detector_forward
      (image upload, captured forward, maps back) and of whenet_op_detect on a 720p frame (upload, letterbox, body, box
      selection), median and spread over --reps calls after warm-up.  --dtype is the detector's storage type (option
      "detector_dtype": f16 = binary16, the default; f32 = the parity-grade float32 body).  Put it behind
      `rocprofv3 --kernel-trace --stats -- python tools/detector_bench.py --reps 10 --kinds full` for per-kernel times.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "headposeestimation-whenet_amd"))

ANCHORS = {0: [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326],
           1: [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]}


def flops_per_image(rows, h, w):
    """2 x multiply-adds of every convolution of the table at input size (h, w)."""
    dims, total = [], 0
    for r in rows:
        full = r["src1"] if r["src1"] >= 0 else r["src0"]
        ih, iw = (h, w) if full < 0 else dims[full]
        if r["op"] == 1:
            oh, ow = ((ih + 1) // 2, (iw + 1) // 2) if r["stride"] == 2 else (ih, iw)
        else:
            oh, ow = ((ih - 2) // 2 + 1, (iw - 2) // 2 + 1) if r["stride"] == 2 else (ih, iw)
            total += 2 * oh * ow * r["k"] * r["k"] * r["cin"] * r["cout"]
        dims.append((oh, ow))
    return total


def timed(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(416, 416))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--kinds", nargs="+", default=["full", "tiny"])
    ap.add_argument("--dtype", choices=["f16", "f32"], default="f16")
    args = ap.parse_args()
    from whenet_hip import _lib, detector_weights as DW, synth
    h, w = args.size
    frame = synth.video_frame(720, 1280)
    rng = np.random.RandomState(0)
    image = rng.uniform(0, 1, (args.batch, h, w, 3)).astype(np.float32)
    for name in args.kinds:
        kind = 0 if name == "full" else 1
        rows = _lib.detector_spec(kind)
        gf = flops_per_image(rows, h, w) / 1e9
        handle = _lib.Handle.postproc(0)
        handle.detector_load(DW.pack(DW.synthetic(kind, 77 + kind)), dtype=args.dtype)
        med, lo, hi = timed(lambda: handle.detector_forward(image, kind, 18), args.reps)
        print(f"{name} {args.dtype} {h}x{w} batch {args.batch}: {gf:.2f} GFLOP per image; detector_forward {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) "
              f"= {gf * args.batch / med:.1f} TFLOP/s host to host")
        anchors = np.array(ANCHORS[kind], np.float32)
        med, lo, hi = timed(lambda: handle.op_detect(frame, anchors, 1, (h, w), 0.3, 0.45), args.reps)
        print(f"{name} {args.dtype} {h}x{w}: op_detect of a 720p frame {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
        handle.close()


if __name__ == "__main__":
    main()
