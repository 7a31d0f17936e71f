#!/usr/bin/env python3
"""A/B of where a video frame is when the pipeline begins it (whenet_hip.frames.FramePipeline with a detector on the model's handle):

    arm host     begin(numpy frame) / begin_yuv(numpy planes)     pinned staging copy on the host, then PCIe
    arm device   begin(torch tensor) / begin_yuv(device planes)   the frame is resident in HBM: one kernel (csrc/ingest.hip,
                                                                  csrc/yuv.hip) reads it where it is, ordered on torch's stream

for two sources, `bgr` (packed 3-byte pixels) and `nv12` (a decoder's planes), on the same pictures: 16 seeded frames of different
content; the device arm holds them as 16 resident uint8 tensors, uploaded before the clock starts -- what a caller that sits on a
hardware decoder or a torch data pipeline has.  What the device arm does NOT pay is exactly what such a caller does not have to
pay today's way round: the device-to-host copy that would feed the host arm is not in either arm.  Seeded tiny detector at
416 x 416, seeded f16 pose model, max_boxes 20, depth 2.

  python tools/device_ingest_ab.py [--sizes 720x1280 1080x1920] [--sources bgr nv12] [--frames 480] [--rounds 6] [--passes 2]
  python tools/device_ingest_ab.py --arms host        # one arm alone

Every (size, source, pass, arm) is one child process under its own `timeout`, the arms alternating; the first child that fails
ends the run.  A child warms up, then runs `--rounds` windows of `--frames` frames, `depth` submissions in flight.  Per child, one
JSON line: frames/s of each window (median, min, max over the rounds), the median host time inside `begin*`, the median host time
of the whole enqueue (`begin*` + `detect_heads`) and the median latency of a submission.  The host arm's figures from pass to
pass are the spread the device arm has to be read against.  There is no gate here.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "headposeestimation-whenet_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from yuv_ingest_ab import ANCHORS, DETECTOR_SEED, bgr_of_planes, nv12_planes, window      # noqa: E402


def worker(args):
    import torch      # first: one HIP runtime in the process, torch's
    import whenet
    from whenet_hip import detector_weights as DW, synth
    from whenet_hip.frames import FramePipeline
    from whenet_hip.yuv import YUVFrame
    arm, source, depth = args.arms[0], args.sources[0], args.depth
    h, w = (int(v) for v in args.sizes[0].split("x"))
    m = whenet.WHENet(dtype="f16")
    m._handle.detector_load(DW.pack(DW.synthetic(1, DETECTOR_SEED)))
    kw = dict(size=tuple(args.size), score=args.score, iou=.45, max_boxes=args.max_boxes,
              anchors=np.array(ANCHORS, np.float32).reshape(-1, 2), num_classes=1)
    planes = [nv12_planes(synth.video_frame(h, w, seed=7 + i)) for i in range(16)]
    stream = torch.cuda.current_stream().cuda_stream if arm == "device" else None
    try:
        with FramePipeline(m, depth=depth) as fp:
            if source == "nv12":
                if arm == "device":
                    frames = [YUVFrame.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), matrix=args.matrix) for y, uv in planes]
                else:
                    frames = [YUVFrame.nv12(y, uv, matrix=args.matrix) for y, uv in planes]
                begin = lambda f: fp.begin_yuv(f, stream=stream)
            else:
                frames = [bgr_of_planes(y, uv, args.matrix) for y, uv in planes]      # (both sources detect on the same bytes)
                if arm == "device":
                    frames = [torch.from_numpy(f).cuda() for f in frames]
                begin = lambda f: fp.begin(f, stream=stream)
            torch.cuda.synchronize()
            window(fp, begin, frames, kw, max(20, 4 * depth), depth)              # warm-up: allocations, graph captures
            res = [window(fp, begin, frames, kw, args.frames, depth) for _ in range(args.rounds)]
        fps = [r[0] for r in res]
        med = lambda i: round(statistics.median([x for r in res for x in r[i]]) * 1e3, 4)
        print(json.dumps({"arm": arm, "source": source, "frame": [h, w], "depth": depth, "frames": args.frames, "rounds": args.rounds,
                          "fps_median": round(statistics.median(fps), 1), "fps_min": round(min(fps), 1), "fps_max": round(max(fps), 1),
                          "begin_ms_median": med(2), "enqueue_ms_median": med(3), "latency_ms_median": med(1),
                          "heads_last_frame": res[-1][4]}), flush=True)
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", nargs="+", default=["host", "device"], choices=["host", "device"])
    ap.add_argument("--sources", nargs="+", default=["bgr", "nv12"], choices=["bgr", "nv12"])
    ap.add_argument("--sizes", nargs="+", default=["720x1280", "1080x1920"], help="frame sizes, HxW")
    ap.add_argument("--matrix", default="bt601", choices=["bt601", "bt709", "jfif"])
    ap.add_argument("--max-boxes", type=int, default=20)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(416, 416))
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--passes", type=int, default=2, help="times every arm runs, each in a process of its own")
    ap.add_argument("--score", type=float, default=.3)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds a child (one size, one source, one arm) may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    for size in args.sizes:
        for source in args.sources:
            for _ in range(args.passes):
                for arm in args.arms:
                    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--arms", arm,
                           "--sources", source, "--sizes", size, "--matrix", args.matrix, "--max-boxes", str(args.max_boxes), "--depth",
                           str(args.depth), "--size", *map(str, args.size), "--frames", str(args.frames), "--rounds", str(args.rounds),
                           "--score", str(args.score)]
                    rc = subprocess.run(cmd).returncode
                    if rc != 0:                  # a fault, an abort or a time limit: nothing more is started on the GPU
                        print(f"device_ingest_ab: {size} {source} arm {arm} ended with status {rc}; stopping", file=sys.stderr)
                        return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
