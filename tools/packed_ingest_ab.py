#!/usr/bin/env python3
"""What a camera's packed 4:2:2 frame costs on its way into the pipeline (whenet_hip.frames.FramePipeline, depth 1, no heads):
per frame, `begin*`; `heads(no boxes)`; `collect()` -- the upload, the conversion kernel where there is one, and the wait.

    arm yuyv       begin_yuv(YUYV frame)                    2 bytes per pixel cross the link, csrc/yuv.hip builds the BGR frame
    arm nv12       begin_yuv(NV12 planes)                   1.5 bytes per pixel: the 4:2:0 path, for the comparison with the parent commit
    arm bgr        begin(BGR frame)                         3 bytes per pixel, no kernel: the frame converted before the clock starts
    arm host_bgr   numpy conversion, then begin(BGR)        what a caller without the packed path does: the numpy statement of
                                                            tests/yuv_packed_cases.py on the host (not a tuned converter) and arm bgr
    arm yuyv_dev   begin_yuv(YUYV frame in device memory)   the kernel alone behind an event pair: no upload (for rocprofv3, below)

  python tools/packed_ingest_ab.py [--sizes 1080x1920 480x640] [--frames 200] [--regions 5] [--passes 2] [--arms yuyv nv12 bgr host_bgr]

Every (size, pass, arm) is one child process under its own `timeout`; the first child that fails ends the run.  A child warms up
(one region, not counted), then times `--regions` regions of `--frames` frames, each frame on the host clock from before `begin*` to
after `collect()` (which waits for the device), with a device synchronisation in front of every region.  Per child, one JSON line:
the median and the 10th / 90th percentile of the per-frame times [ms], the bytes a frame sends host to device and the GB/s that
5 bytes per pixel (2 read, 3 written) would mean at the median -- an end-to-end figure of the call, not the kernel's.  The kernel's
device time comes from a trace, in a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/packed_ingest_ab.py --worker --arms yuyv_dev --sizes 1080x1920

There is no gate here.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "headposeestimation-whenet_amd"))
sys.path.insert(0, ROOT)

ARMS = ["yuyv", "nv12", "bgr", "host_bgr", "yuyv_dev"]


def yuv444(bgr: np.ndarray):
    """(Y, U, V) [h,w] of a BGR frame by the usual 8-bit studio-range integer form: content for the measurement, not a reference."""
    f = bgr.astype(np.int32)
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    Y = ((66 * R + 129 * G + 25 * B + 128) >> 8) + 16
    U = ((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128
    V = ((112 * R - 94 * G - 18 * B + 128) >> 8) + 128
    return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)


def yuyv_rows(bgr: np.ndarray) -> np.ndarray:
    """uint8 [h, 2 w] (Y0 U Y1 V; even w): every row its own chroma, taken at the even pixel of each pair."""
    Y, U, V = yuv444(bgr)
    h, w = Y.shape
    out = np.empty((h, w // 2, 4), np.uint8)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = Y[:, 0::2], U[:, 0::2], Y[:, 1::2], V[:, 0::2]
    return out.reshape(h, 2 * w)


def nv12_planes(bgr: np.ndarray):
    Y, U, V = yuv444(bgr)
    UV = np.stack([U[::2, ::2], V[::2, ::2]], axis=2)
    return np.ascontiguousarray(Y), np.ascontiguousarray(UV.reshape(UV.shape[0], -1))


def percentiles(ms):
    a = np.sort(np.asarray(ms))
    return [round(float(np.percentile(a, q)), 4) for q in (50, 10, 90)]


def worker(args):
    import torch                      # (first, so that there is one HIP runtime in the process)
    import whenet
    from whenet_hip import synth
    from whenet_hip.frames import FramePipeline
    from whenet_hip.yuv import YUVFrame
    arm = args.arms[0]
    h, w = (int(v) for v in args.sizes[0].split("x"))
    assert w % 2 == 0, "even widths here"
    pictures = [synth.video_frame(h, w, seed=7 + i) for i in range(8)]
    rows = [yuyv_rows(p) for p in pictures]
    none = np.zeros((0, 4), np.float32)
    frames_per_region, keep = args.frames, []
    m = whenet.WHENet(dtype="f16")
    try:
        with FramePipeline(m, depth=1) as fp:
            if arm == "yuyv":
                src = [YUVFrame.yuyv(r, matrix=args.matrix) for r in rows]
                begin, h2d = fp.begin_yuv, 2 * h * w
            elif arm == "yuyv_dev":
                keep = [torch.from_numpy(r).to("cuda:0") for r in rows]
                src = [YUVFrame.yuyv(t, matrix=args.matrix) for t in keep]
                begin, h2d = fp.begin_yuv, 0
            elif arm == "nv12":
                src = [YUVFrame.nv12(*nv12_planes(p), matrix=args.matrix) for p in pictures]
                begin, h2d = fp.begin_yuv, h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)
            elif arm == "bgr":
                src = [YUVFrame.yuyv(r, matrix=args.matrix).to_bgr() for r in rows]
                begin, h2d = fp.begin, 3 * h * w
            else:                     # host_bgr: the conversion is inside the clock
                from tests import yuv_packed_cases as PC
                code = {"bt601": 0, "bt709": 1, "jfif": 2}[args.matrix]
                src = rows
                begin, h2d = (lambda r: fp.begin(PC.packed_to_bgr(r, r.shape[1], PC.YUYV, code, h, w))), 3 * h * w
                frames_per_region = max(2, min(frames_per_region, args.host_frames))

            def region(n):
                torch.cuda.synchronize()
                ms = []
                for i in range(n):
                    t0 = time.perf_counter()
                    begin(src[i % len(src)])
                    fp.heads(none)
                    fp.collect()
                    ms.append((time.perf_counter() - t0) * 1e3)
                return ms

            region(max(2, min(frames_per_region, 50)))                       # warm-up: allocations, first launches
            ms = [t for _ in range(args.regions) for t in region(frames_per_region)]
        med, p10, p90 = percentiles(ms)
        print(json.dumps({"arm": arm, "frame": [h, w], "matrix": args.matrix, "frames": len(ms), "regions": args.regions,
                          "ms_median": med, "ms_p10": p10, "ms_p90": p90, "h2d_bytes_per_frame": h2d,
                          "call_GBps_at_5_bytes_per_pixel": round(5 * h * w / (med * 1e-3) / 1e9, 2)}), flush=True)
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", nargs="+", default=["yuyv", "nv12", "bgr", "host_bgr"], choices=ARMS)
    ap.add_argument("--sizes", nargs="+", default=["1080x1920", "480x640"], help="frame sizes, HxW")
    ap.add_argument("--matrix", default="bt601", choices=["bt601", "bt709", "jfif"])
    ap.add_argument("--frames", type=int, default=200, help="frames of a region")
    ap.add_argument("--host-frames", type=int, default=4, help="frames of a region of arm host_bgr (numpy is slow)")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--passes", type=int, default=2, help="times every arm runs, each in a process of its own")
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
                       "--sizes", size, "--matrix", args.matrix, "--frames", str(args.frames), "--host-frames", str(args.host_frames),
                       "--regions", str(args.regions)]
                rc = subprocess.run(cmd).returncode
                if rc != 0:                  # a fault, an abort or a time limit: nothing more is started on the GPU
                    print(f"packed_ingest_ab: {size} arm {arm} ended with status {rc}; stopping", file=sys.stderr)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
