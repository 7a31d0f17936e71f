#!/usr/bin/env python3
"""A/B of one frame per submission against MIXED clips, on a source whose frame size ALTERNATES (whenet_hip.frames.FramePipeline
with a detector on the model's handle):

    arm A   begin; detect_heads; collect                            per frame (one submission per frame)
    arm B   begin_clip_mixed; detect_heads_clip; collect_clip       per F frames, F = 2, 4, 8, with max_heads = F x K and = 32

on seeded frames of two sizes, 1280 x 720 and 960 x 540, alternating (16 of them, different content), the seeded tiny and full
detectors at 416 x 416, a seeded f16 pose model, max_boxes 20, depth 2.

  python tools/mixed_clip_ab.py [--kinds tiny full] [--clip 2 4 8] [--max-heads 0 32] [--frames 480] [--rounds 6] [--depth 2]
  python tools/mixed_clip_ab.py --arm-a-only      # arm A alone: it uses only entry points that exist without mixed clips, so the
                                                  # same file prices the per-frame path on a tree that has no geometry cache

Every (detector, F, max_heads) is one child process under its own `timeout`; the first child that fails ends the run.  Inside a
child both arms are warmed up, then run alternating, `--rounds` windows of `--frames` frames each (the order of the two arms
swaps from round to round), `depth` submissions in flight.  Per arm: frames/s of each window (median, min, max over the
rounds), the median latency of a submission (from the entry into `begin` / `begin_clip` to the return of its `collect` /
`collect_clip`), the median host time inside the enqueue calls of a submission; for arm B also `rows_used` and `overflow` of a
clip, and the letterbox cache's counters where the handle has them.  `gain` = arm B's median over arm A's; `beyond_spread` says
whether arm B's slowest window beats arm A's fastest.  One JSON line per child.  (`--max-heads 0` stands for F x K.)
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
SIZES = ((720, 1280), (540, 960))


def window_frames(fp, frames, kw, total: int, depth: int):
    """`total` frames, one per submission -> (frames/s, latencies [s], enqueue times [s], heads of the last frame)."""
    started, lat, enq = [], [], []
    heads = 0
    t_begin = time.perf_counter()
    for i in range(total):
        if fp.in_flight == depth:
            heads = len(fp.collect()[0])
            lat.append(time.perf_counter() - started.pop(0))
        t0 = time.perf_counter()
        fp.begin(frames[i % len(frames)])
        fp.detect_heads(**kw)
        started.append(t0)
        enq.append(time.perf_counter() - t0)
    while fp.in_flight:
        heads = len(fp.collect()[0])
        lat.append(time.perf_counter() - started.pop(0))
    return total / (time.perf_counter() - t_begin), lat, enq, heads


def window_clips(fp, clip, kw, max_heads, total: int, depth: int):
    """`total` frames, len(clip) per submission -> (frames/s, latencies [s], enqueue times [s], (rows_used, overflow))."""
    F = len(clip)
    started, lat, enq = [], [], []
    used = (0, 0)
    t_begin = time.perf_counter()
    for _ in range(total // F):
        if fp.in_flight == depth:
            used = fp.collect_clip()[1]
            lat.append(time.perf_counter() - started.pop(0))
        t0 = time.perf_counter()
        fp.begin_clip_mixed(clip)
        fp.detect_heads_clip(max_heads=max_heads, **kw)
        started.append(t0)
        enq.append(time.perf_counter() - t0)
    while fp.in_flight:
        used = fp.collect_clip()[1]
        lat.append(time.perf_counter() - started.pop(0))
    return (total // F) * F / (time.perf_counter() - t_begin), lat, enq, used


def worker(args):
    import whenet
    from whenet_hip import detector_weights as DW, synth
    from whenet_hip.frames import FramePipeline
    name, F, depth = args.kinds[0], args.clip[0], args.depth
    frames = [synth.video_frame(*SIZES[i % 2], seed=7 + i) for i in range(16)]
    clip = frames[:F]
    m = whenet.WHENet(dtype="f16")
    m._handle.detector_load(DW.pack(DW.synthetic(0 if name == "full" else 1, SEEDS[name])))
    kw = dict(size=tuple(args.size), score=args.score, iou=.45, max_boxes=args.max_boxes,
              anchors=np.array(ANCHORS[name], np.float32).reshape(-1, 2), num_classes=1)
    max_heads = args.max_heads[0] or min(F * args.max_boxes, 256)
    total = max(args.frames // F, 2 * depth) * F
    try:
        with FramePipeline(m, depth=depth) as fp:
            window_frames(fp, frames[:F], kw, max(20, 4 * depth), depth)               # warm-up: allocations, graph captures
            if not args.arm_a_only:
                window_clips(fp, clip, kw, max_heads, 4 * depth * F, depth)
            a, b = [], []
            for r in range(args.rounds):
                for arm in ("a" if args.arm_a_only else "ab" if r % 2 == 0 else "ba"):
                    if arm == "a":
                        a.append(window_frames(fp, frames[:F], kw, total, depth))
                    else:
                        b.append(window_clips(fp, clip, kw, max_heads, total, depth))
        out = {"detector": name, "size": list(args.size), "max_boxes": args.max_boxes, "depth": depth, "frames_per_clip": F, "max_heads": max_heads,
               "frames": total, "rounds": args.rounds}
        out["frame_sizes"] = [list(s) for s in SIZES]
        if hasattr(m._handle, "letterbox_cache_stats"):
            out["letterbox_cache"] = m._handle.letterbox_cache_stats()
        for key, res in (("frame", a),) if args.arm_a_only else (("frame", a), ("clip", b)):
            fps = [w[0] for w in res]
            out[key] = {"fps_median": round(statistics.median(fps), 1), "fps_min": round(min(fps), 1), "fps_max": round(max(fps), 1),
                        "latency_ms_median": round(statistics.median([x for w in res for x in w[1]]) * 1e3, 3),
                        "enqueue_ms_median": round(statistics.median([x for w in res for x in w[2]]) * 1e3, 3)}
        out["frame"]["heads_last_frame"] = a[-1][3]
        if not args.arm_a_only:
            out["clip"]["rows_used"], out["clip"]["overflow"] = b[-1][3]
            out["gain"] = round(out["clip"]["fps_median"] / out["frame"]["fps_median"], 3)
            out["beyond_spread"] = out["clip"]["fps_min"] > out["frame"]["fps_max"]
        print(json.dumps(out), flush=True)
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", nargs="+", default=["tiny", "full"], choices=["tiny", "full"])
    ap.add_argument("--clip", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--max-heads", type=int, nargs="+", default=[0, 32], help="rows of a clip's forward; 0 = F x K (at most 256)")
    ap.add_argument("--max-boxes", type=int, default=20)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(416, 416))
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--score", type=float, default=.3)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a child (one detector, one F, one max_heads) may take")
    ap.add_argument("--arm-a-only", action="store_true", help="the per-frame arm alone (runs on a tree without mixed clips)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    for name in args.kinds:
        for F in (args.clip[:1] if args.arm_a_only else args.clip):
            for mh in (args.max_heads[:1] if args.arm_a_only else args.max_heads):
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--kinds", name,
                       "--clip", str(F), "--max-heads", str(mh), "--max-boxes", str(args.max_boxes), "--depth", str(args.depth), "--size",
                       *map(str, args.size), "--frames", str(args.frames), "--rounds", str(args.rounds), "--score", str(args.score)] + (["--arm-a-only"] if args.arm_a_only else [])
                rc = subprocess.run(cmd).returncode
                if rc != 0:                  # a fault, an abort or a time limit: nothing more is started on the GPU
                    print(f"mixed_clip_ab: {name} F {F} max_heads {mh} ended with status {rc}; stopping", file=sys.stderr)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
