#!/usr/bin/env python3
"""What the device JPEG encoder costs and what it replaces, for 1920 x 1080 and 640 x 480 frames at quality 95 (recorded, not gated):

    (i)   encoder_us            device time of the encoder alone on a resident I420 JFIF surface (whenet_jpeg_encode_device):
                                events around back-to-back calls; encoder_call_host_us = the host's time inside one call, which
                                bounds the first figure from below (the kernels' own times come from a kernel trace of this tool)
    (ii)  annotate_us, annotate_jpeg_us, added_us
                                one frame with 4 heads, submit -> annotate -> collect, into a device I420 surface against
                                annotate_jpeg: the added time per frame
    (iii) d2h_us, pillow_encode_us
                                what it replaces: D2H of the I420 surface, and Pillow's encode of the same planes on one core
    (iv)  bytes_surface, bytes_jpeg
                                bytes over PCIe per frame, both ways
    (v)   frame_pipeline_k4     the loop of bench.py's `frame_pipeline` leg (1280 x 720, k = 4: sync median, pipelined frames/s) as
                                it is -- the code path of the parent commit -- next to the same loop with annotate_jpeg

  python tools/jpeg_bench.py [--sizes 1080x1920 480x640] [--quality 95] [--rounds 7] [--iters 50] [--sampling 4:2:0] [--optimize]

--sampling 4:2:2 / 4:4:4: the encoder is timed on a resident PACKED surface (what annotate_jpeg paints for these samplings) and
Pillow encodes with the same `subsampling`; --optimize: Huffman tables of the frame's own symbols, on both sides.

Every figure is the median of `--rounds` regions bracketed by a device synchronisation on both sides; device times come from
events on the stream the work is enqueued on.  One JSON line per size, one for (v).
"""
from __future__ import annotations

import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("WHENET_HIP_PKG") or os.path.join(ROOT, "headposeestimation-whenet_amd"))


def median_us(fn, rounds, sync):
    out = []
    for _ in range(rounds):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e6)
    return statistics.median(out)


def size_leg(m, h, w, args):
    import torch
    from PIL import Image
    from whenet_hip import jpeg, overlay, synth
    from whenet_hip.frames import FramePipeline
    from whenet_hip.yuv import YUVFrame
    hnd = m._handle
    frame, boxes = synth.video_frame(h, w), synth.head_boxes(4, h, w)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    sync = torch.cuda.synchronize

    packed = args.sampling != "4:2:0"
    pillow_kw = dict(quality=args.quality, subsampling={"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}[args.sampling], optimize=args.optimize)
    keywords = dict(sampling=args.sampling, optimize=args.optimize)

    def device_surface():
        if packed:
            return torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        return YUVFrame.i420(torch.empty((h, w), dtype=torch.uint8, device="cuda"), torch.empty((ch, cw), dtype=torch.uint8, device="cuda"),
                             torch.empty((ch, cw), dtype=torch.uint8, device="cuda"), matrix="jfif")

    res = {"frame": [h, w], "quality": args.quality, "heads": 4, "sampling": args.sampling, "optimize": bool(args.optimize)}
    with FramePipeline(m, depth=1) as fp:
        # the annotated surface the encoder is timed on
        surf = device_surface()
        fp.submit(frame, boxes)
        fp.annotate(surf)
        fp.collect()
        sync()
        s, _ = overlay.surface_of(surf, h, w)
        cap = jpeg.bound(h, w, args.sampling)
        dst = torch.empty(cap, dtype=torch.uint8, device="cuda")
        dsize = torch.zeros(1, dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream or None
        encode = lambda: hnd.jpeg_encode_device(s, h, w, True, args.quality, dst.data_ptr(), cap, dsize.data_ptr(), stream=stream, **keywords)
        for _ in range(5):
            encode()
        sync()
        times, calls = [], []
        for _ in range(args.rounds):                      # (i): events around `iters` encodes on the caller's stream
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            a.record()
            t = time.perf_counter()
            for _ in range(args.iters):
                encode()
            calls.append((time.perf_counter() - t) * 1e6 / args.iters)
            b.record()
            sync()
            times.append(a.elapsed_time(b) * 1e3 / args.iters)
        res["encoder_us"] = round(statistics.median(times), 1)
        res["encoder_call_host_us"] = round(statistics.median(calls), 1)      # the host's time in the enqueue-only call
        nbytes = int(dsize.item())
        res["bytes_jpeg"], res["bytes_surface"] = nbytes, 3 * h * w if packed else h * w + 2 * ch * cw
        stream_bytes = dst[:nbytes].cpu().numpy().tobytes()
        # (ii): one frame, submit -> annotate -> collect, both ways
        def one(annotate):
            fp.submit(frame, boxes)
            annotate()
            fp.collect()
        for annotate in (lambda: fp.annotate(surf), lambda: fp.annotate_jpeg(quality=args.quality, **keywords)):
            for _ in range(5):
                one(annotate)
        res["annotate_us"] = round(median_us(lambda: [one(lambda: fp.annotate(surf)) for _ in range(args.iters)], args.rounds, sync) / args.iters, 1)
        res["annotate_jpeg_us"] = round(
            median_us(lambda: [one(lambda: fp.annotate_jpeg(quality=args.quality, **keywords)) for _ in range(args.iters)], args.rounds, sync) / args.iters, 1)
        res["added_us"] = round(res["annotate_jpeg_us"] - res["annotate_us"], 1)
        # the stream annotate_jpeg returns is the encoder's
        fp.submit(frame, boxes)
        jf = fp.annotate_jpeg(quality=args.quality, **keywords)
        fp.collect()
        res["annotate_jpeg_equals_encoder"] = jf.tobytes() == stream_bytes
    # (iii): what it replaces
    planes_dev = [torch.empty((h, w), dtype=torch.uint8, device="cuda"), torch.empty((ch, cw), dtype=torch.uint8, device="cuda"),
                  torch.empty((ch, cw), dtype=torch.uint8, device="cuda")]
    if packed:
        planes_dev = [torch.empty((h, 3 * w), dtype=torch.uint8, device="cuda")]
    pinned = [torch.empty(p.shape, dtype=torch.uint8).pin_memory() for p in planes_dev]

    def d2h():
        for dpl, hpl in zip(planes_dev, pinned):
            hpl.copy_(dpl, non_blocking=True)
    res["d2h_us"] = round(median_us(d2h, args.rounds, sync), 1)
    im = Image.open(io.BytesIO(stream_bytes))
    im.draft("YCbCr", im.size)
    ycc = im.copy()                                       # the same picture as full-resolution YCbCr for Pillow's encoder
    torch.set_num_threads(1)
    from PIL import ImageFile
    if args.optimize:
        ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 3 * h * w)      # Pillow's optimize=True needs the whole stream in one buffer

    def pillow():
        ycc.save(io.BytesIO(), format="JPEG", **pillow_kw)
    res["pillow_encode_us"] = round(median_us(pillow, args.rounds, lambda: None), 1)
    buf = io.BytesIO()
    ycc.save(buf, format="JPEG", **pillow_kw)
    res["bytes_pillow"] = len(buf.getvalue())
    return res


def pipeline_leg(m, args):
    """bench.py's frame_leg at k = 4, as it is and with annotate_jpeg behind every submit"""
    from whenet_hip import synth
    from whenet_hip.frames import FramePipeline
    frame, boxes = synth.video_frame(), synth.head_boxes(4)
    out = {"frame": list(frame.shape[:2]), "heads": 4, "quality": args.quality, "sampling": args.sampling, "optimize": bool(args.optimize)}
    keywords = dict(sampling=args.sampling, optimize=args.optimize)
    for arm in ("none", "annotate_jpeg"):
        with FramePipeline(m, depth=2) as fp:
            extra = (lambda: fp.annotate_jpeg(quality=args.quality, **keywords)) if arm == "annotate_jpeg" else (lambda: None)
            lat = []
            for _ in range(260):
                a = time.perf_counter()
                fp.submit(frame, boxes)
                extra()
                fp.collect()
                lat.append(time.perf_counter() - a)
            a, n = time.perf_counter(), 0
            for _ in range(200):
                if fp.in_flight == 2:
                    fp.collect()
                    n += 1
                fp.submit(frame, boxes)
                extra()
            while fp.in_flight:
                fp.collect()
                n += 1
            el = time.perf_counter() - a
        out[arm] = {"sync_median_us": round(float(np.median(np.array(lat[60:]) * 1e6)), 1), "pipelined_frames_per_s": round(n / el, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1080x1920", "480x640"], help="frame sizes, HxW")
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sampling", choices=["4:2:0", "4:2:2", "4:4:4"], default="4:2:0")
    ap.add_argument("--optimize", action="store_true", help="Huffman tables of the frame's own symbols")
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime in the process, torch's)
    import whenet
    m = whenet.WHENet(dtype="f16")
    try:
        for size in args.sizes:
            h, w = (int(v) for v in size.split("x"))
            print(json.dumps(size_leg(m, h, w, args)), flush=True)
        print(json.dumps({"frame_pipeline_k4": pipeline_leg(m, args)}), flush=True)
    finally:
        m.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
