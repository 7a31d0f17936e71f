"""Measurements of the GPU letterbox (csrc/letterbox.hip) and of the resident-frame pipeline.

  python tools/letterbox_bench.py --mode kernels [--reps 20]
      Runs whenet_op_letterbox at 720p, 1080p and 2160p -> 416 x 416 and nothing else: the program to put behind
      `rocprofv3 --kernel-trace --stats -- python tools/letterbox_bench.py --mode kernels`.  One size per process
      with --only 1080 so that the two kernels' per-size averages can be read straight from the stats.
  python tools/letterbox_bench.py --mode stats --trace-dir DIR
      Reads the kernel-trace CSVs rocprofv3 left under DIR/<size>/ and prints, per size and kernel, the mean time and
      its share of the time the algorithmic bytes take at 8 TB/s (the bound: both kernels move bytes, they have no
      arithmetic to speak of).
  python tools/letterbox_bench.py --mode wall [--rounds 30]
      Host-to-host wall: FramePipeline.begin + detector_input + heads(k = 0) + collect against Pillow's letterbox_image
      + /255 on the same machine's CPU (when Pillow is importable), and begin + heads + collect against submit + collect
      for k = 1, 4, 16 on the same frame and boxes, rounds alternated, with each arm's own run-to-run spread.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "headposeestimation-whenet_amd"))

SIZES = {"720": (720, 1280), "1080": (1080, 1920), "2160": (2160, 3840)}
BOX = (416, 416)
HBM_BYTES_PER_S = 8e12


def algorithmic_bytes(fh, fw, box=BOX):
    """(horizontal kernel, vertical kernel): the frame once + the intermediate written | the intermediate read + both outputs."""
    from whenet_hip import _lib
    (nw, nh, _, _), _ = _lib.letterbox_plan(fh, fw, *box)
    mid = fh * nw * 3
    return fh * fw * 3 + mid, mid + box[0] * box[1] * 3 * (1 + 4)


def mode_kernels(args):
    import torch  # noqa: F401  (one HIP runtime in the process)
    from whenet_hip import _lib, synth
    h = _lib.Handle.postproc(0)
    for name, (fh, fw) in SIZES.items():
        if args.only and name != args.only:
            continue
        frame = synth.video_frame(fh, fw)
        for _ in range(args.reps):
            h.op_letterbox(frame, BOX, bgr=True)
        print(f"{name}: {args.reps} letterboxes of {fh}x{fw} -> {BOX[0]}x{BOX[1]}")
    h.close()


def mode_stats(args):
    for name, (fh, fw) in SIZES.items():
        rows = []
        for path in glob.glob(os.path.join(args.trace_dir, name, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += list(csv.DictReader(f))
        if not rows:
            print(f"{name}: no kernel trace under {os.path.join(args.trace_dir, name)}")
            continue
        bh, bv = algorithmic_bytes(fh, fw)
        for kern, nbytes in (("whenet_letterbox_h_kernel", bh), ("whenet_letterbox_v_kernel", bv)):
            d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kern in r["Kernel_Name"]]
            d = d[len(d) // 4:]                                   # the first launches load the code object
            if not d:
                print(f"{name} {kern}: not in the trace")
                continue
            mean, floor = statistics.mean(d), nbytes / HBM_BYTES_PER_S * 1e6
            print(f"{name:>5} {kern}: {len(d)} launches, mean {mean:8.2f} us, min {min(d):8.2f} us; algorithmic bytes {nbytes:>10} "
                  f"= {floor:6.2f} us at 8 TB/s (bandwidth bound) -> {100 * floor / mean:5.1f} % of that bound")


def timed(fn, rounds):
    out = []
    for _ in range(rounds):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e6)
    return out


def summary(us):
    s = sorted(us)
    return f"median {statistics.median(s):8.1f} us  (p10 {s[len(s) // 10]:8.1f}, p90 {s[(9 * len(s)) // 10]:8.1f})"


def mode_wall(args):
    import torch  # noqa: F401
    import whenet
    from whenet_hip import synth
    from whenet_hip.frames import FramePipeline
    try:
        from PIL import Image
    except ImportError:
        Image = None
    m = whenet.WHENet(dtype=args.dtype)
    none = np.zeros((0, 4), np.float32)
    print(f"# detector_input wall, host array to host array ({args.dtype} handle, {args.rounds} rounds each)")
    with FramePipeline(m, depth=1) as fp:
        for name, (fh, fw) in SIZES.items():
            frame = synth.video_frame(fh, fw)

            def gpu():
                fp.begin(frame)
                x = fp.detector_input(BOX)
                fp.heads(none)
                fp.collect()
                return x

            x = gpu()
            timed(gpu, 5)
            print(f"{name:>5} GPU begin + detector_input + release: {summary(timed(gpu, args.rounds))}")
            if Image is None:
                print(f"{name:>5} Pillow is not importable on this machine: no CPU arm")
                continue

            def cpu():
                image = Image.fromarray(frame[:, :, ::-1])             # (the reference converts its BGR frame to RGB first)
                iw, ih = image.size
                w, h = BOX[1], BOX[0]
                scale = min(w / iw, h / ih)
                nw, nh = int(iw * scale), int(ih * scale)
                boxed = Image.new("RGB", (w, h), (128, 128, 128))
                boxed.paste(image.resize((nw, nh), Image.BICUBIC), ((w - nw) // 2, (h - nh) // 2))
                data = np.array(boxed, dtype="float32")
                data /= 255.
                return np.expand_dims(data, 0)

            assert cpu().tobytes() == x.tobytes(), "GPU and Pillow canvases differ"
            timed(cpu, 3)
            print(f"{name:>5} CPU Pillow BICUBIC letterbox + /255:  {summary(timed(cpu, args.rounds))}   (same bits as the GPU arm)")

        print(f"# resident sequence against submit_frame, 720p frame, rounds alternated ({args.rounds} rounds each)")
        frame = synth.video_frame(720, 1280)
        for k in (1, 4, 16):
            boxes = synth.head_boxes(k, 720, 1280, seed=k)

            def parent():
                fp.submit(frame, boxes)
                return fp.collect()

            def resident():
                fp.begin(frame)
                fp.heads(boxes)
                return fp.collect()

            a, b = parent(), resident()
            assert all(np.array_equal(p, q) for p, q in zip(a, b))
            for _ in range(5):
                parent(), resident()
            tp, tr = [[], []], []
            for r in range(args.rounds):                               # parent arm twice per round: its own spread
                tp[0] += timed(parent, 1)
                tr += timed(resident, 1)
                tp[1] += timed(parent, 1)
            m0, m1, mr = statistics.median(tp[0]), statistics.median(tp[1]), statistics.median(tr)
            print(f"k = {k:>2} submit + collect (1st)     : {summary(tp[0])}")
            print(f"k = {k:>2} submit + collect (2nd)     : {summary(tp[1])}")
            print(f"k = {k:>2} begin + heads + collect    : {summary(tr)}")
            print(f"k = {k:>2} parent arm against itself {100 * (m1 - m0) / m0:+.1f} %, resident against the parent's mean "
                  f"{100 * (mr - (m0 + m1) / 2) / ((m0 + m1) / 2):+.1f} %")
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "stats", "wall"], required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=sorted(SIZES), default=None)
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--dtype", default="f32s")
    args = ap.parse_args()
    {"kernels": mode_kernels, "stats": mode_stats, "wall": mode_wall}[args.mode](args)


if __name__ == "__main__":
    main()
