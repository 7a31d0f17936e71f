#!/usr/bin/env python3
"""A/B of the pose overlay's cost in the video loop (whenet_hip.frames.FramePipeline with a detector on the model's handle):

    arm none     begin_yuv(device NV12); detect_heads; collect                                   today's loop, no picture
    arm nv12     begin_yuv(device NV12); detect_heads; annotate(device NV12 surface); collect    the annotated frame for an encoder
    arm host     begin_yuv(device NV12); detect_heads; annotate(host BGR array); collect         ... for a host consumer (D2H of 3 B/px)

on 16 seeded frames held as resident device planes (uploaded before the clock starts), seeded tiny detector at 416 x 416, seeded
f16 pose model, depth 2.  `--max-boxes` sets the head slots per frame (1 and 16: with the low score threshold used here the
seeded detector fills them; the heads painted in the last frame are reported).  `--display full` lets the annotate arms paint the
three text labels of every head as well (demo_video.py's `--display full`); every line says which display it ran.

  python tools/annotate_ab.py [--sizes 720x1280 1080x1920] [--max-boxes 1 16] [--frames 480] [--rounds 6] [--passes 2]
  python tools/annotate_ab.py --arms nv12 --display simple full       # the labels' cost: the two displays alternate like two arms
  WHENET_HIP_PKG=/another/checkout/headposeestimation-whenet_amd python tools/annotate_ab.py --arms none --label parent      # the same loop on another build

Every (size, heads, pass, arm) is one child process under its own `timeout`, the arms alternating; the first child that fails ends
the run.  A child warms up, then runs `--rounds` windows of `--frames` frames.  Per child one JSON line: frames/s of each window
(median, min, max), the median host time of the annotate call and of the whole enqueue, the median latency of a submission.  The
cost of annotate is the difference of the arms' microseconds per frame, to be read beside the `none` arm's own spread from pass to
pass.  The draw kernel's own time comes from a kernel trace of one child (`rocprofv3 --kernel-trace --stats -- python
tools/annotate_ab.py --worker --arms nv12 ...`); its algorithmic bytes are 3 B/px read + 1.5 B/px (NV12 / I420) or 3 B/px (packed)
written.  There is no gate here.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from yuv_ingest_ab import ANCHORS, DETECTOR_SEED, nv12_planes      # noqa: E402

# after the import above: yuv_ingest_ab puts this checkout's package in front of the path, and the other build has to come first
sys.path.insert(0, os.environ.get("WHENET_HIP_PKG") or os.path.join(ROOT, "headposeestimation-whenet_amd"))


def window(fp, begin, annotate, frames, kw, total: int, depth: int):
    """`total` frames, one per submission -> (frames/s, latencies [s], annotate times [s], enqueue times [s], heads of the last frame)."""
    started, lat, ann, enq = [], [], [], []
    heads = 0
    t_begin = time.perf_counter()
    for i in range(total):
        if fp.in_flight == depth:
            heads = len(fp.collect()[0])
            lat.append(time.perf_counter() - started.pop(0))
        t0 = time.perf_counter()
        begin(frames[i % len(frames)])
        fp.detect_heads(**kw)
        t1 = time.perf_counter()
        annotate(i)
        t2 = time.perf_counter()
        started.append(t0)
        ann.append(t2 - t1)
        enq.append(t2 - t0)
    while fp.in_flight:
        heads = len(fp.collect()[0])
        lat.append(time.perf_counter() - started.pop(0))
    return total / (time.perf_counter() - t_begin), lat, ann, enq, heads


def worker(args):
    import torch      # first: one HIP runtime in the process, torch's
    import whenet
    from whenet_hip import detector_weights as DW, synth
    from whenet_hip.frames import FramePipeline
    from whenet_hip.yuv import YUVFrame
    from whenet_hip import _lib
    arm, depth, max_boxes = args.arms[0], args.depth, args.max_boxes[0]
    h, w = (int(v) for v in args.sizes[0].split("x"))
    ch, cw = (h + 1) // 2, (w + 1) // 2
    m = whenet.WHENet(dtype="f16")
    m._handle.detector_load(DW.pack(DW.synthetic(1, DETECTOR_SEED)))
    kw = dict(size=tuple(args.size), score=args.score, iou=.45, max_boxes=max_boxes, anchors=np.array(ANCHORS, np.float32).reshape(-1, 2),
              num_classes=1)
    planes = [nv12_planes(synth.video_frame(h, w, seed=7 + i)) for i in range(16)]
    stream = torch.cuda.current_stream().cuda_stream
    try:
        with FramePipeline(m, depth=depth) as fp:
            frames = [YUVFrame.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), matrix=args.matrix) for y, uv in planes]
            begin = lambda f: fp.begin_yuv(f, stream=stream)
            # one destination per submission in flight: a surface is the caller's until its frame is collected
            surfaces = [YUVFrame.nv12(torch.empty((h, w), dtype=torch.uint8, device="cuda"), torch.empty((ch, 2 * cw), dtype=torch.uint8, device="cuda"),
                                      matrix=args.matrix) for _ in range(depth)]
            arrays = [np.empty((h, w, 3), np.uint8) for _ in range(depth)]
            if not hasattr(fp, "annotate"):
                assert arm == "none", "this build has no annotate"
            display = args.display[0]
            more = {"display": "full"} if display == "full" else {}      # (a build without the keyword still runs `simple`)
            annotate = {"none": lambda i: None, "nv12": lambda i: fp.annotate(surfaces[i % depth], stream=stream, **more),
                        "host": lambda i: fp.annotate(arrays[i % depth], **more)}[arm]
            torch.cuda.synchronize()
            window(fp, begin, annotate, frames, kw, max(20, 4 * depth), depth)              # warm-up: allocations, graph captures
            res = [window(fp, begin, annotate, frames, kw, args.frames, depth) for _ in range(args.rounds)]
        fps = [r[0] for r in res]
        med = lambda i: round(statistics.median([x for r in res for x in r[i]]) * 1e3, 4)
        print(json.dumps({"arm": arm, "display": display if arm != "none" else None, "frame": [h, w], "max_boxes": max_boxes, "depth": depth, "frames": args.frames, "rounds": args.rounds,
                          "fps_median": round(statistics.median(fps), 1), "fps_min": round(min(fps), 1), "fps_max": round(max(fps), 1),
                          "us_per_frame_median": round(1e6 / statistics.median(fps), 1), "annotate_call_ms_median": med(2),
                          "enqueue_ms_median": med(3), "latency_ms_median": med(1), "heads_last_frame": res[-1][4],
                          "build": args.label, "library": os.path.relpath(os.path.realpath(_lib.LIB_PATH), ROOT)}), flush=True)
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", nargs="+", default=["none", "nv12", "host"], choices=["none", "nv12", "host"])
    ap.add_argument("--sizes", nargs="+", default=["720x1280", "1080x1920"], help="frame sizes, HxW")
    ap.add_argument("--display", nargs="+", default=["simple"], choices=["simple", "full"], help="what the annotate arms paint")
    ap.add_argument("--matrix", default="bt601", choices=["bt601", "bt709", "jfif"])
    ap.add_argument("--max-boxes", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(416, 416))
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--passes", type=int, default=2, help="times every arm runs, each in a process of its own")
    ap.add_argument("--score", type=float, default=.01)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a child (one size, one head count, one arm) may take")
    ap.add_argument("--label", default="this", help="what a line's `build` key says (the run of another checkout: --label parent)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    for size in args.sizes:
        for boxes in args.max_boxes:
            for _ in range(args.passes):
                for arm, display in [(a, d) for a in args.arms for d in (args.display if a != "none" else args.display[:1])]:
                    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--arms", arm,
                           "--display", display, "--sizes", size, "--matrix", args.matrix, "--max-boxes", str(boxes), "--depth", str(args.depth), "--size",
                           *map(str, args.size), "--frames", str(args.frames), "--rounds", str(args.rounds), "--score", str(args.score), "--label", args.label]
                    rc = subprocess.run(cmd).returncode
                    if rc != 0:                  # a fault, an abort or a time limit: nothing more is started on the GPU
                        print(f"annotate_ab: {size} max_boxes {boxes} arm {arm} display {display} ended with status {rc}; stopping", file=sys.stderr)
                        return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
