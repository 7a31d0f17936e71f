#!/usr/bin/env python3
"""A/B of the two per-frame forms of whenet_hip.frames.FramePipeline with a detector on the model's handle:

    two-step   begin; detect; heads; collect          (the host waits for the detector and builds the crop plans)
    fused      begin; detect_heads; collect           (one enqueue-only submission: csrc/headplan.hip)

on a seeded 1280 x 720 frame, the seeded tiny and full detectors at 416 x 416 and a seeded f16 pose model.

  python tools/frame_async_ab.py [--kinds tiny full] [--depths 1 2] [--max-boxes 4 20] [--frames 600] [--rounds 6] [--score 0.3]

Every (detector, max_boxes) is one child process under its own `timeout`; the first child that fails ends the run.  Inside a
child, per depth: both arms are warmed up, then run alternating, `--rounds` windows of `--frames` frames each (the order of
the two arms swaps from round to round).  `depth` frames are kept in flight: a frame is collected when the pipeline is full.
Per arm: frames/s of each window (median, min, max over the rounds), the median submit -> collect latency of a frame (from
the entry into `begin` to the return of its `collect`) and the median host time spent inside the enqueue calls of a frame
(`begin` + `detect` + `heads`, or `begin` + `detect_heads`).  One JSON line per (detector, max_boxes, depth).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "headposeestimation-whenet_amd"))

ANCHORS = {"full": [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326],
           "tiny": [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]}
SEEDS = {"full": 77, "tiny": 78}


def with_window(fh, fw, boxes):
    """The boxes `heads()` accepts: a non-empty window inside the frame (what the fused form decides on the device)."""
    from whenet_hip import _lib
    r = _lib.frame_rects(fh, fw, boxes)
    ok = (r[:, 0] >= 0) & (r[:, 1] >= 0) & (r[:, 2] <= fh) & (r[:, 3] <= fw) & (r[:, 0] < r[:, 2]) & (r[:, 1] < r[:, 3])
    return np.ascontiguousarray(boxes[ok])


def window(fp, frame, kw, fused: bool, frames: int, depth: int):
    """`frames` frames through the pipeline -> (frames/s, latencies [s], enqueue times [s], heads of the last frame)."""
    fh, fw = frame.shape[:2]
    started, lat, enq = [], [], []
    heads = 0
    t_begin = time.perf_counter()
    for _ in range(frames):
        if fp.in_flight == depth:
            heads = len(fp.collect()[0])
            lat.append(time.perf_counter() - started.pop(0))
        t0 = time.perf_counter()
        fp.begin(frame)
        if fused:
            fp.detect_heads(**kw)
        else:
            fp.heads(with_window(fh, fw, fp.detect(**kw)[0]))
        t1 = time.perf_counter()
        started.append(t0)
        enq.append(t1 - t0)
    while fp.in_flight:
        heads = len(fp.collect()[0])
        lat.append(time.perf_counter() - started.pop(0))
    return frames / (time.perf_counter() - t_begin), lat, enq, heads


def worker(args):
    import whenet
    from whenet_hip import detector_weights as DW, synth
    from whenet_hip.frames import FramePipeline
    name, max_boxes = args.kinds[0], args.max_boxes[0]
    frame = synth.video_frame(720, 1280)
    m = whenet.WHENet(dtype="f16")
    m._handle.detector_load(DW.pack(DW.synthetic(0 if name == "full" else 1, SEEDS[name])))
    kw = dict(size=tuple(args.size), score=args.score, iou=.45, max_boxes=max_boxes,
              anchors=np.array(ANCHORS[name], np.float32).reshape(-1, 2), num_classes=1)
    try:
        for depth in args.depths:
            with FramePipeline(m, depth=depth) as fp:
                for fused in (False, True):
                    window(fp, frame, kw, fused, max(20, 4 * depth), depth)           # warm-up: allocations, graph captures
                res = {False: [], True: []}
                for r in range(args.rounds):
                    for fused in ((False, True) if r % 2 == 0 else (True, False)):
                        res[fused].append(window(fp, frame, kw, fused, args.frames, depth))
                fp.begin(frame)
                detections = len(fp.detect(**kw)[0])
                fp.heads(np.zeros((0, 4), np.float32))
                fp.collect()
            out = {"detector": name, "size": list(args.size), "max_boxes": max_boxes, "depth": depth, "frames": args.frames,
                   "rounds": args.rounds, "detections": detections}
            for fused, key in ((False, "two_step"), (True, "fused")):
                fps = [w[0] for w in res[fused]]
                out[key] = {"fps_median": round(statistics.median(fps), 1), "fps_min": round(min(fps), 1), "fps_max": round(max(fps), 1),
                            "latency_ms_median": round(statistics.median([x for w in res[fused] for x in w[1]]) * 1e3, 3),
                            "enqueue_ms_median": round(statistics.median([x for w in res[fused] for x in w[2]]) * 1e3, 3),
                            "heads": res[fused][-1][3]}
            print(json.dumps(out), flush=True)
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", nargs="+", default=["tiny", "full"], choices=["tiny", "full"])
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--max-boxes", type=int, nargs="+", default=[4, 20])
    ap.add_argument("--size", type=int, nargs=2, default=(416, 416))
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--score", type=float, default=.3)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a child (one detector, one max_boxes) may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    for name in args.kinds:
        for mb in args.max_boxes:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--kinds", name,
                   "--max-boxes", str(mb), "--depths", *map(str, args.depths), "--size", *map(str, args.size), "--frames", str(args.frames),
                   "--rounds", str(args.rounds), "--score", str(args.score)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:                      # a fault, an abort or a time limit: nothing more is started on the GPU
                print(f"frame_async_ab: {name} max_boxes {mb} ended with status {rc}; stopping", file=sys.stderr)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
