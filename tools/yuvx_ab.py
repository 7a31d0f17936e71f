#!/usr/bin/env python3
"""What a 10-bit or a 4:4:4 decoder surface costs on its way into the pipeline (whenet_hip.frames.FramePipeline, depth 1, no
heads): per frame, `begin*`; `heads(no boxes)`; `collect()` -- the upload, the conversion kernel where there is one, and the wait.

    arm p010       begin_yuv(P010 frame, BT.2020)           3 bytes per pixel cross the link, csrc/yuvx.hip builds the BGR frame
    arm p010_dev   the same frame in device memory          the kernel alone behind an event pair: no upload
    arm i444       begin_yuv(8-bit I444 frame)              3 bytes per pixel, csrc/yuvx.hip
    arm nv12       begin_yuv(NV12 planes)                   1.5 bytes per pixel, csrc/yuv.hip: the existing path, for the parent comparison
    arm yuyv       begin_yuv(YUYV frame)                    2 bytes per pixel, csrc/yuv.hip
    arm bgr        begin(BGR frame)                         3 bytes per pixel, no kernel

  python tools/yuvx_ab.py [--sizes 1080x1920 480x640] [--frames 50] [--regions 20] [--warmup 3] [--passes 1] [--arms ...]

Every (size, pass, arm) is one child process under its own `timeout`; the first child that fails ends the run.  A child first
checks every frame it will send against the host statement (`op_yuvx_to_bgr` / `op_yuv_to_bgr` == `to_bgr()`), warms up
(`--warmup` regions, not counted), then times `--regions` regions of `--frames` frames on the host clock, from before the first
`begin*` of a region to after its last `collect()`, with a device synchronisation in front of every region.  Per child, one JSON
line: the median and the 10th / 90th percentile of the regions' per-frame times [ms] and the bytes a frame sends host to device.
The old arms run the code of the parent commit; to compare with it, run them again with WHENET_HIP_PKG pointing at the package
directory (`headposeestimation-whenet_amd`) of a built checkout of the parent.  The kernel's device time comes from a trace, in a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/yuvx_ab.py --worker --arms p010_dev --sizes 1080x1920

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
sys.path.insert(0, os.environ.get("WHENET_HIP_PKG") or os.path.join(ROOT, "headposeestimation-whenet_amd"))
sys.path.insert(0, ROOT)

ARMS = ["p010", "p010_dev", "i444", "nv12", "yuyv", "bgr"]


def yuv444(bgr: np.ndarray):
    """(Y, U, V) [h,w] of a BGR frame by the usual 8-bit studio-range integer form: content for the measurement, not a reference."""
    f = bgr.astype(np.int32)
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    Y = ((66 * R + 129 * G + 25 * B + 128) >> 8) + 16
    U = ((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128
    V = ((112 * R - 94 * G - 18 * B + 128) >> 8) + 128
    return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)


def worker(args):
    import torch                      # (first, so that there is one HIP runtime in the process)
    import whenet
    from whenet_hip import synth
    from whenet_hip.frames import FramePipeline
    from whenet_hip.yuv import YUVFrame
    arm = args.arms[0]
    h, w = (int(v) for v in args.sizes[0].split("x"))
    assert w % 2 == 0 and h % 2 == 0, "even sizes here"
    pictures = [synth.video_frame(h, w, seed=7 + i) for i in range(4)]
    none = np.zeros((0, 4), np.float32)
    keep, src = [], []
    for p in pictures:
        Y, U, V = yuv444(p)
        UV = np.ascontiguousarray(np.stack([U[::2, ::2], V[::2, ::2]], axis=2).reshape(h // 2, w))
        if arm in ("p010", "p010_dev"):       # 10 significant bits in the high bits of a word
            y16 = ((Y.astype(np.uint16) << 8) | 0x40).astype("<u2")
            uv16 = ((UV.astype(np.uint16) << 8) | 0x80).astype("<u2")
            src.append(YUVFrame.p010(y16, uv16, matrix="bt2020"))
        elif arm == "i444":
            src.append(YUVFrame.i444(Y, U, V, matrix="bt709"))
        elif arm == "nv12":
            src.append(YUVFrame.nv12(np.ascontiguousarray(Y), UV, matrix="bt709"))
        elif arm == "yuyv":
            rows = np.empty((h, w // 2, 4), np.uint8)
            rows[..., 0], rows[..., 1], rows[..., 2], rows[..., 3] = Y[:, 0::2], U[:, 0::2], Y[:, 1::2], V[:, 0::2]
            src.append(YUVFrame.yuyv(rows.reshape(h, 2 * w), matrix="bt709"))
        else:
            src.append(p)
    m = whenet.WHENet(dtype="f16")
    try:
        hd = m._handle
        for f in src:                 # every frame against the host statement first
            if isinstance(f, YUVFrame):
                got, = hd.op_yuvx_to_bgr([f]) if getattr(f, "needs_ext", False) else hd.op_yuv_to_bgr([f])
                assert got.tobytes() == f.to_bgr().tobytes(), "the kernel differs from the host statement"
        h2d = {"p010": 3, "p010_dev": 0, "i444": 3, "nv12": 1.5, "yuyv": 2, "bgr": 3}[arm] * h * w
        if arm == "p010_dev":
            keep = [[torch.from_numpy(np.ascontiguousarray(pl)).to("cuda:0") for pl in f.planes] for f in src]
            src = [YUVFrame(k, f.format, f.matrix, h, w, container=16, shift=0) for k, f in zip(keep, src)]
        with FramePipeline(m, depth=1) as fp:
            begin = fp.begin if arm == "bgr" else fp.begin_yuv

            def region(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(n):
                    begin(src[i % len(src)])
                    fp.heads(none)
                    fp.collect()
                return (time.perf_counter() - t0) * 1e3 / n

            for _ in range(args.warmup):
                region(args.frames)
            ms = np.sort([region(args.frames) for _ in range(args.regions)])
        med, p10, p90 = (round(float(np.percentile(ms, q)), 4) for q in (50, 10, 90))
        print(json.dumps({"arm": arm, "frame": [h, w], "regions": args.regions, "frames_per_region": args.frames, "ms_median": med,
                          "ms_p10": p10, "ms_p90": p90, "ms_min": round(float(ms[0]), 4), "ms_max": round(float(ms[-1]), 4),
                          "h2d_bytes_per_frame": int(h2d), "pkg": os.environ.get("WHENET_HIP_PKG", "")}), flush=True)
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", nargs="+", default=ARMS, choices=ARMS)
    ap.add_argument("--sizes", nargs="+", default=["1080x1920", "480x640"], help="frame sizes, HxW")
    ap.add_argument("--frames", type=int, default=50, help="frames of a region")
    ap.add_argument("--regions", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3, help="regions run before the clock counts")
    ap.add_argument("--passes", type=int, default=1, help="times every arm runs, each in a process of its own")
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
                       "--sizes", size, "--frames", str(args.frames), "--regions", str(args.regions), "--warmup", str(args.warmup)]
                rc = subprocess.run(cmd).returncode
                if rc != 0:                  # a fault, an abort or a time limit: nothing more is started on the GPU
                    print(f"yuvx_ab: {size} arm {arm} ended with status {rc}; stopping", file=sys.stderr)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
