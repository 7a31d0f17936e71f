#!/usr/bin/env python3
"""A/B of the two ways a video frame enters the pipeline (whenet_hip.frames.FramePipeline with a detector on the model's handle):

    arm bgr   begin(frame_bgr);  detect_heads; collect      the packed BGR frame crosses PCIe, 3 bytes per pixel
    arm yuv   begin_yuv(planes); detect_heads; collect      the decoder's NV12 planes cross, 1.5 bytes per pixel, and csrc/yuv.hip
                                                            builds the BGR frame on the device

on the same pictures: seeded frames (16 of them, different content) turned into NV12 planes by a fixed integer RGB -> YUV; the bgr
arm is fed `planes.to_bgr()`, converted before the clock starts, so both arms detect on the same bytes.  Seeded tiny detector at
416 x 416, seeded f16 pose model, max_boxes 20, depth 2.

  python tools/yuv_ingest_ab.py [--sizes 720x1280 1080x1920] [--frames 480] [--rounds 6] [--passes 2] [--depth 2] [--matrix bt601]
  python tools/yuv_ingest_ab.py --arms bgr        # one arm alone

Every (size, pass, arm) is one child process under its own `timeout`; the first child that fails ends the run.  A child warms up,
then runs `--rounds` windows of `--frames` frames, `depth` submissions in flight.  Per child, one JSON line: frames/s of each window
(median, min, max over the rounds), the median host time inside `begin` / `begin_yuv`, the median host time of the whole enqueue
(`begin*` + `detect_heads`), the median latency of a submission, and the bytes a frame sends host to device.  The bgr arm runs once
per pass: its figures from pass to pass are the spread the yuv arm has to be read against.  There is no gate here.
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

ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
DETECTOR_SEED = 78


def nv12_planes(bgr: np.ndarray):
    """A BGR frame -> (Y [h,w], UV [ch, 2 cw]) by the usual 8-bit studio-range integer form, chroma from the top-left pixel of
    each 2 x 2 block: content for the measurement, not a reference."""
    f = bgr.astype(np.int32)
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    Y = ((66 * R + 129 * G + 25 * B + 128) >> 8) + 16
    U = ((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128
    V = ((112 * R - 94 * G - 18 * B + 128) >> 8) + 128
    UV = np.stack([U[::2, ::2], V[::2, ::2]], axis=2).astype(np.uint8)
    return np.ascontiguousarray(Y.astype(np.uint8)), np.ascontiguousarray(UV.reshape(UV.shape[0], -1))


def window(fp, begin, frames, kw, total: int, depth: int):
    """`total` frames, one per submission -> (frames/s, latencies [s], begin times [s], enqueue times [s], heads of the last frame)."""
    started, lat, beg, enq = [], [], [], []
    heads = 0
    t_begin = time.perf_counter()
    for i in range(total):
        if fp.in_flight == depth:
            heads = len(fp.collect()[0])
            lat.append(time.perf_counter() - started.pop(0))
        t0 = time.perf_counter()
        begin(frames[i % len(frames)])
        t1 = time.perf_counter()
        fp.detect_heads(**kw)
        started.append(t0)
        beg.append(t1 - t0)
        enq.append(time.perf_counter() - t0)
    while fp.in_flight:
        heads = len(fp.collect()[0])
        lat.append(time.perf_counter() - started.pop(0))
    return total / (time.perf_counter() - t_begin), lat, beg, enq, heads


def worker(args):
    import whenet
    from whenet_hip import detector_weights as DW, synth
    from whenet_hip.frames import FramePipeline
    arm, depth = args.arms[0], args.depth
    h, w = (int(v) for v in args.sizes[0].split("x"))
    m = whenet.WHENet(dtype="f16")
    m._handle.detector_load(DW.pack(DW.synthetic(1, DETECTOR_SEED)))
    kw = dict(size=tuple(args.size), score=args.score, iou=.45, max_boxes=args.max_boxes,
              anchors=np.array(ANCHORS, np.float32).reshape(-1, 2), num_classes=1)
    try:
        with FramePipeline(m, depth=depth) as fp:
            if arm == "yuv":
                from whenet_hip.yuv import YUVFrame
                frames = [YUVFrame.nv12(*nv12_planes(synth.video_frame(h, w, seed=7 + i)), matrix=args.matrix) for i in range(16)]
                begin, h2d = fp.begin_yuv, h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)
            else:
                frames = [bgr_of_planes(*nv12_planes(synth.video_frame(h, w, seed=7 + i)), args.matrix) for i in range(16)]
                begin, h2d = fp.begin, h * w * 3
            window(fp, begin, frames, kw, max(20, 4 * depth), depth)              # warm-up: allocations, graph captures
            res = [window(fp, begin, frames, kw, args.frames, depth) for _ in range(args.rounds)]
        fps = [r[0] for r in res]
        med = lambda i: round(statistics.median([x for r in res for x in r[i]]) * 1e3, 4)
        print(json.dumps({"arm": arm, "frame": [h, w], "matrix": args.matrix, "depth": depth, "frames": args.frames, "rounds": args.rounds,
                          "fps_median": round(statistics.median(fps), 1), "fps_min": round(min(fps), 1), "fps_max": round(max(fps), 1),
                          "begin_ms_median": med(2), "enqueue_ms_median": med(3), "latency_ms_median": med(1),
                          "h2d_bytes_per_frame": h2d, "heads_last_frame": res[-1][4]}), flush=True)
    finally:
        m.close()


def bgr_of_planes(y, uv, matrix):
    """The BGR frame of the planes by the library's own host conversion, so that both arms detect on the same bytes."""
    from whenet_hip.yuv import YUVFrame
    return YUVFrame.nv12(y, uv, matrix=matrix).to_bgr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", nargs="+", default=["bgr", "yuv"], choices=["bgr", "yuv"])
    ap.add_argument("--sizes", nargs="+", default=["720x1280", "1080x1920"], help="frame sizes, HxW")
    ap.add_argument("--matrix", default="bt601", choices=["bt601", "bt709", "jfif"])
    ap.add_argument("--max-boxes", type=int, default=20)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(416, 416))
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--passes", type=int, default=2, help="times every arm runs, each in a process of its own")
    ap.add_argument("--score", type=float, default=.3)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a child (one size, one arm) may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    for size in args.sizes:
        for _ in range(args.passes):
            for arm in args.arms:
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--arms", arm,
                       "--sizes", size, "--matrix", args.matrix, "--max-boxes", str(args.max_boxes), "--depth", str(args.depth), "--size",
                       *map(str, args.size), "--frames", str(args.frames), "--rounds", str(args.rounds), "--score", str(args.score)]
                rc = subprocess.run(cmd).returncode
                if rc != 0:                  # a fault, an abort or a time limit: nothing more is started on the GPU
                    print(f"yuv_ingest_ab: {size} arm {arm} ended with status {rc}; stopping", file=sys.stderr)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
