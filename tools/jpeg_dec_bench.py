#!/usr/bin/env python3
"""What the device JPEG decoder costs and what it replaces, for 1920 x 1080 and 640 x 480 frames (recorded, not gated):

    (i)   decode_us             device time of the decoder alone on entropy bytes that are resident in device memory
                                (whenet_jpeg_decode_device into a tight BGR frame): events around back-to-back calls, for three
                                streams of the same picture:
                                    own        the library's encoder at quality 95: one restart interval per MCU row (68 / 30)
                                    pillow_rst Pillow at quality 95, 4:2:0, restart_marker_rows=1
                                    pillow     the same without DRI: ONE interval, the entropy decode is one lane
                                decode_call_host_us = the host's time inside one call (the kernels' own times come from a kernel
                                trace of this tool)
                                The entropy stage's two forms side by side: decode_us is a map {"interval": .., "seg64": ..,
                                "seg128": .., ...}, one entry per value of --entropy (0: an interval per lane, 1: segmented, 2: the
                                handle's auto choice) and, for the segmented form, per value of --seg-bytes; "forms" says which form
                                each entry ran in (whenet_jpeg_decode_counters).  --lanes: decoding lanes per wave of the segmented
                                kernels (option jpeg_seg_lanes; 0: the default).  --only-decode skips (ii) and (iii).
                                --rule 0 | 1: the decode rule of every decode of the run (option jpeg_rule: 0 the project's own,
                                1 libjpeg's bytes), checked against the host statement of the same rule; "rule" in the output.
                                Under rule 1 the colour stage of the tight BGR frame is the rule's frame kernel, under rule 0 the
                                plane kernel of the YUV ingest: a kernel trace of two runs gives the per-kernel times side by side.
                                --rgb decodes into R, G, B order, which takes the frame kernel under rule 0 as well.
    (ii)  begin_us, begin_jpeg_us
                                one frame with 4 heads, begin -> heads -> collect, from the BGR frame (the parent commit's path)
                                and from the stream (begin_jpeg), depth 1, the median of single frames
    (iii) pillow_decode_us, h2d_us
                                what it replaces: Pillow's decode of the stream on one core, and the H2D of 3 bytes per pixel
    (iv)  bytes_frame, bytes_jpeg
                                bytes over PCIe per frame, both ways

    (v)   --clip F [F ...]      clips of JPEG streams (recorded, not gated), INSTEAD of (i)-(iv): for the `own` stream (one restart
                                interval per MCU row) and the `pillow` stream (no DRI) of each size, F frames as ONE
                                whenet_clip_begin_jpeg against the same F frames as F whenet_frame_begin_jpeg submissions, in the
                                same process; each submission is released without heads and collected (the collect waits for the
                                decode and hands the status words over).  ms per frame: the median of --clip-samples (>= 20)
                                single regions after a warm-up, and their 10th..90th percentile spread; "enqueues" / "h2d" per clip
                                are whenet_jpeg_clip_counters' differences.  The handle's options stay at their defaults (auto).

    (vi)  --progressive         progressive streams (recorded, not gated), INSTEAD of (i)-(v): Pillow's progressive stream of the
                                picture (quality 95, 4:2:0; without DRI and with one interval per MCU row) through
                                whenet_frame_begin_jpeg_progressive, ms per frame for begin -> release -> collect, with option
                                jpeg_prog_levels 1 (a launch per level) and 0 (a launch per scan); "cumulative_level_ms": the same
                                for the stream cut behind level 1, 2, ... (differences: the time per level); next to it the baseline
                                twin (the same picture with optimize=True) through whenet_frame_begin_jpeg with the entropy stage
                                in form 0 and in the auto form, and Pillow's decode of the progressive stream on one core.  Medians
                                of --clip-samples (>= 20) regions and their 10th..90th percentiles.

    (vii) --clip F [F ...] --progressive
                                clips of progressive streams (recorded, not gated), INSTEAD of (i)-(vi): F copies of Pillow's
                                progressive stream (quality 95, 4:2:0; without DRI and with one interval per MCU row) as ONE
                                whenet_clip_begin_jpeg_progressive against F whenet_frame_begin_jpeg_progressive submissions, as row
                                (v) measures baseline clips: ms per frame, the median of --clip-samples (>= 20) regions after 3
                                warm-up regions, with the 10th..90th percentiles; where ONE region takes more than --slow-seconds (a
                                1080p stream without DRI: seconds per frame), --slow-samples regions after one warm-up region, and
                                "..._regions" says how many were taken.  "enqueues", "h2d", "scan_launches" per clip: the counters.

    (viii) --orient N [N ...]   the oriented decode (recorded, not gated), INSTEAD of (i)-(vii): Pillow's stream of the picture (quality
                                95, 4:2:0, one interval per MCU row) with an Exif APP1 of each value N spliced in, through
                                whenet_frame_begin_jpeg_oriented in the same process: ms per frame for begin -> release without heads ->
                                collect, the median of --clip-samples (>= 20) regions after 3 warm-up ones and their 10th..90th
                                percentiles (the method of row (vi)); every frame is checked against the host statement first.  Value 1
                                runs the upright launches, 2..4 the oriented frame kernel's row form, 5..8 its LDS tile form: the
                                kernels' own times come from a kernel trace of this row (--rgb or --rule 1 puts the upright frame
                                through the frame kernel too, so that the three can be read side by side).

    (ix)  --layouts old | new   the LAYOUTS section (recorded, not gated), INSTEAD of (i)-(viii); ms per frame for begin -> release without
                                heads -> collect through whenet_frame_begin_jpeg[_accept], every frame checked against the host
                                statement first.  Each figure is the median of --repeats (>= 5) REPEATS, a repeat being the median of
                                --clip-samples regions after 3 warm-up ones; "spread" is the repeats' own minimum and maximum.
                                  old   what existed before the section, through calls that existed before it (so that the row runs
                                        unchanged on the parent commit's library: WHENET_HIP_PKG): Pillow's 4:2:0, 4:2:2 and 4:4:4 streams
                                        of the picture (quality 95, one interval per MCU row) with the entropy stage in form 0 and
                                        form 1.  A commit does not regress where its medians lie inside the parent's spreads.
                                  new   what the section adds: the 4:4:0, 4:1:1 and 4:1:0 twins of the picture (the layout writer of
                                        tests/jpeg_layout_cases.py on the picture's own DCT blocks, one interval per MCU row) next to
                                        its 4:2:2 twin from the same writer (Annex K Huffman tables); and a three-scan 4:2:0 twin against the interleaved one,
                                        with one interval per MCU row and without DRI (a multi-scan stream without DRI is ONE lane
                                        per scan: the known limit of the scan-plan path).
                                The kernels' own times come from a kernel trace of this row.

  python tools/jpeg_dec_bench.py [--progressive] [--layouts old] [--orient 1 3 6] [--sizes 1080x1920 480x640] [--rounds 7] [--iters 30] [--entropy 0 1] [--seg-bytes 64 128 256 512]
                                 [--lanes 0] [--rule 0] [--rgb] [--only-decode] [--clip 1 4 16] [--clip-samples 20]
                                 [--slow-seconds 5] [--slow-samples 20]

Every figure is the median of `--rounds` regions bracketed by a device synchronisation on both sides; device times come from
events on the stream the work is enqueued on.  The frames the streams decode to are checked against the host statement first.
One JSON line per size.
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


RULES = ("own", "libjpeg")      # --rule 0, 1


def median_us(fn, rounds, sync):
    out = []
    for _ in range(rounds):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e6)
    return statistics.median(out)


def streams_of(frame_bgr, quality=95):
    from PIL import Image
    from whenet_hip import jpeg
    im = Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1]))
    out = {"own": jpeg.encode_host(frame_bgr, quality)}
    for name, kw in (("pillow_rst", {"restart_marker_rows": 1}), ("pillow", {})):
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=quality, subsampling=2, **kw)
        out[name] = buf.getvalue()
    return out


def size_leg(m, h, w, args):
    import torch
    from PIL import Image
    from whenet_hip import _lib, jpeg, synth
    from whenet_hip.frames import FramePipeline
    hnd = m._handle
    frame, boxes = synth.video_frame(h, w), synth.head_boxes(4, h, w)
    sync = torch.cuda.synchronize
    stream = torch.cuda.current_stream().cuda_stream or None
    res = {"frame": [h, w], "heads": 4, "bytes_frame": 3 * h * w, "rule": args.rule}
    dst = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = dst.data_ptr(), 3 * w, _lib.SURF_PACKED, 1
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.set_num_threads(1)
    for name, data in streams_of(frame).items():
        info = _lib.jpeg_parse(data)
        ent = torch.from_numpy(np.frombuffer(data, np.uint8)[info.data_offset:].copy()).cuda()
        decode = lambda: hnd.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s, not args.rgb, status.data_ptr(), stream=stream)
        want = jpeg.decode_host(data, bgr=not args.rgb, rule=RULES[args.rule])
        r = {"intervals": info.intervals, "bytes_jpeg": len(data), "equals_host": True, "decode_us": {}, "decode_call_host_us": {}, "forms": {}}
        configs = []
        for e in args.entropy:
            configs += [(e, sb) for sb in args.seg_bytes] if e != 0 else [(0, args.seg_bytes[0])]
        for entropy, seg_bytes in configs:
            key = "interval" if entropy == 0 else ("seg" if entropy == 1 else "auto") + str(seg_bytes)
            hnd.set_option("jpeg_entropy", entropy)
            hnd.set_option("jpeg_seg_bytes", seg_bytes)
            before = hnd.jpeg_decode_counters()
            dst.zero_()
            for _ in range(2):
                decode()
            sync()
            after = hnd.jpeg_decode_counters()
            r["forms"][key] = "segmented" if after["segmented"] > before["segmented"] else "interval"
            serial = info.intervals == 1 and r["forms"][key] == "interval"      # one lane walks the whole picture: fewer repeats
            iters = max(1, args.iters // 10) if serial else args.iters
            r["equals_host"] = r["equals_host"] and bool(np.array_equal(dst.cpu().numpy(), want)) and status.cpu().tolist() == [0, -1]
            times, calls = [], []
            for _ in range(args.rounds):                  # (i): events around `iters` decodes on the caller's stream
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                sync()
                a.record()
                t = time.perf_counter()
                for _ in range(iters):
                    decode()
                calls.append((time.perf_counter() - t) * 1e6 / iters)
                b.record()
                sync()
                times.append(a.elapsed_time(b) * 1e3 / iters)
            r["decode_us"][key] = round(statistics.median(times), 1)
            r["decode_call_host_us"][key] = round(statistics.median(calls), 1)
        hnd.set_option("jpeg_entropy", 2)
        hnd.set_option("jpeg_seg_bytes", 128)
        if args.only_decode:
            res[name] = r
            continue

        def pillow():                                     # (iii): the decode it replaces, one core
            im = Image.open(io.BytesIO(data))
            im.load()
        r["pillow_decode_us"] = round(median_us(pillow, args.rounds, lambda: None), 1)
        with FramePipeline(m, depth=1) as fp:             # (ii): one frame from the stream
            def one_jpeg():
                fp.begin_jpeg(data)
                fp.heads(boxes)
                fp.collect()
            for _ in range(3):
                one_jpeg()
            n = max(1, iters // 2)
            r["begin_jpeg_us"] = round(median_us(lambda: [one_jpeg() for _ in range(n)], args.rounds, sync) / n, 1)
        res[name] = r
    if args.only_decode:
        return res
    with FramePipeline(m, depth=1) as fp:                 # (ii): the same frame as BGR pixels, the parent commit's path
        def one():
            fp.begin(frame)
            fp.heads(boxes)
            fp.collect()
        for _ in range(5):
            one()
        res["begin_us"] = round(median_us(lambda: [one() for _ in range(args.iters)], args.rounds, sync) / args.iters, 1)
    pinned = torch.from_numpy(frame).pin_memory()
    res["h2d_us"] = round(median_us(lambda: dst.copy_(pinned, non_blocking=True), args.rounds, sync), 1)
    return res


def clip_leg(m, h, w, args):
    import torch
    from whenet_hip import jpeg, synth
    hnd = m._handle
    sync = torch.cuda.synchronize
    no_heads = np.zeros((0, 4), np.int32)
    res = {"frame": [h, w], "rule": args.rule, "clip": {}}
    streams = streams_of(synth.video_frame(h, w))
    for name in ("own", "pillow"):
        data = streams[name]
        want = jpeg.decode_host(data, rule=RULES[args.rule])
        got, _ = jpeg.decode_clip([data] * 3, handle=hnd, rule=RULES[args.rule])      # the clip kernels on this stream against the host statement first
        r = {"bytes_jpeg": len(data), "equals_host": all(np.array_equal(g, want) for g in got)}
        for F in args.clip:
            datas, status, single = [data] * F, np.zeros((F, 2), np.int32), np.zeros(2, np.int32)

            def clip():
                t = hnd.clip_begin_jpeg(datas, status)
                hnd.frame_heads(t, no_heads)
                hnd.collect(t, 0)

            def singles():
                for d in datas:
                    t = hnd.frame_begin_jpeg(d, single)
                    hnd.frame_heads(t, no_heads)
                    hnd.collect(t, 0)

            before = hnd.jpeg_clip_counters()
            clip()
            after = hnd.jpeg_clip_counters()
            assert status.tolist() == [[0, -1]] * F and after["h2d"] - before["h2d"] == 1
            out = {"enqueues": after["enqueues"] - before["enqueues"], "h2d": 1}
            for key, fn in (("clip", clip), ("singles", singles)):
                for _ in range(3):
                    fn()
                ms = []
                for _ in range(max(20, args.clip_samples)):
                    sync()
                    t = time.perf_counter()
                    fn()
                    ms.append((time.perf_counter() - t) * 1e3 / F)
                q = np.percentile(ms, [10, 50, 90])
                out[key + "_ms_per_frame"] = round(float(q[1]), 3)
                out[key + "_p10_p90"] = [round(float(q[0]), 3), round(float(q[2]), 3)]
            r[str(F)] = out
        res["clip"][name] = r
    return res


def prog_leg(m, h, w, args):
    """row (vi): progressive streams (SOF2), one frame per submission: whenet_frame_begin_jpeg_progressive -> release without heads
    -> collect, the wall time of the whole region (plan, one H2D, the launches, the wait), next to the baseline twin of the same
    picture through whenet_frame_begin_jpeg with the entropy stage in form 0 (an interval per lane: what the parent commit had for
    such a picture) and in the handle's auto form, and Pillow's decode of the progressive stream on one core."""
    import torch
    from PIL import Image
    from whenet_hip import _lib, jpeg, synth
    hnd = m._handle
    sync = torch.cuda.synchronize
    no_heads = np.zeros((0, 4), np.int32)
    torch.set_num_threads(1)
    im = Image.fromarray(np.ascontiguousarray(synth.video_frame(h, w)[..., ::-1]))
    res = {"frame": [h, w], "rule": args.rule, "progressive": {}}

    def stream(**kw):
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=95, subsampling=2, **kw)
        return buf.getvalue()

    def region(fn):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(max(20, args.clip_samples)):
            sync()
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        q = np.percentile(ms, [10, 50, 90])
        return {"ms": round(float(q[1]), 3), "p10_p90": [round(float(q[0]), 3), round(float(q[2]), 3)]}

    status = np.zeros(2, np.int32)

    def begin(data, progressive):
        t = hnd.frame_begin_jpeg(data, status, progressive=progressive)
        hnd.frame_heads(t, no_heads)
        hnd.collect(t, 0)

    for name, kw in (("no_dri", {}), ("row_intervals", {"restart_marker_rows": 1})):
        data, twin = stream(progressive=True, **kw), stream(optimize=True, **kw)
        info, scans = _lib.jpeg_parse_scans(data)
        want = jpeg.decode_host(data, rule=RULES[args.rule], progressive=True)
        r = {"bytes_jpeg": len(data), "bytes_twin": len(twin), "scans": len(scans), "levels": max(s.level for s in scans),
             "items": sum(s.intervals for s in scans),
             "equals_host": bool(np.array_equal(jpeg.decode(data, handle=hnd, rule=RULES[args.rule], progressive=True), want)),
             "equals_twin": bool(np.array_equal(want, jpeg.decode_host(twin, rule=RULES[args.rule])))}
        for levels in (1, 0):
            hnd.set_option("jpeg_prog_levels", levels)
            r["per_level_launches" if levels else "per_scan_launches"] = region(lambda: begin(data, True))
        hnd.set_option("jpeg_prog_levels", 1)
        # time per level: the stream cut behind the last scan of levels 1..L is an incomplete progression of L levels
        r["cumulative_level_ms"] = []
        for level in range(1, r["levels"] + 1):
            last = max(i for i, s in enumerate(scans) if s.level <= level)
            if any(s.level > level for s in scans[:last]):
                break      # (the script's scans are not in level order: no prefix holds exactly these levels)
            cut = data[:scans[last].data_offset + scans[last].data_bytes] + b"\xff\xd9"
            r["cumulative_level_ms"].append(region(lambda: begin(cut, True))["ms"])
        for key, entropy in (("twin_form0", 0), ("twin_auto", 2)):
            hnd.set_option("jpeg_entropy", entropy)
            r[key] = region(lambda: begin(twin, False))
        hnd.set_option("jpeg_entropy", 2)

        def pillow():
            Image.open(io.BytesIO(data)).convert("RGB").load()

        r["pillow_one_core"] = region(pillow)
        res["progressive"][name] = r
    return res


def prog_clip_leg(m, h, w, args):
    """row (vii): clips of progressive streams: F copies of Pillow's progressive stream of the picture as ONE
    whenet_clip_begin_jpeg_progressive against the same F streams as F whenet_frame_begin_jpeg_progressive submissions (the
    capability without clips), in the same process; each submission is released without heads and collected."""
    import torch
    from PIL import Image
    from whenet_hip import _lib, jpeg, synth
    hnd = m._handle
    sync = torch.cuda.synchronize
    no_heads = np.zeros((0, 4), np.int32)
    im = Image.fromarray(np.ascontiguousarray(synth.video_frame(h, w)[..., ::-1]))
    res = {"frame": [h, w], "rule": args.rule, "progressive_clip": {}}
    for name, kw in (("no_dri", {}), ("row_intervals", {"restart_marker_rows": 1})):
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=95, subsampling=2, progressive=True, **kw)
        data = buf.getvalue()
        scans = _lib.jpeg_parse_scans(data)[1]
        want = jpeg.decode_host(data, rule=RULES[args.rule], progressive=True)
        got, _ = jpeg.decode_clip([data] * 3, handle=hnd, rule=RULES[args.rule], progressive=True)      # against the host statement first
        r = {"bytes_jpeg": len(data), "scans": len(scans), "levels": max(s.level for s in scans), "items": sum(s.intervals for s in scans),
             "equals_host": all(np.array_equal(g, want) for g in got)}
        for F in args.clip:
            datas, status, single = [data] * F, np.zeros((F, 2), np.int32), np.zeros(2, np.int32)

            def clip():
                t = hnd.clip_begin_jpeg(datas, status, progressive=True)
                hnd.frame_heads(t, no_heads)
                hnd.collect(t, 0)

            def singles():
                for d in datas:
                    t = hnd.frame_begin_jpeg(d, single, progressive=True)
                    hnd.frame_heads(t, no_heads)
                    hnd.collect(t, 0)

            before, pbefore = hnd.jpeg_clip_counters(), hnd.jpeg_progressive_counters()
            clip()
            after, pafter = hnd.jpeg_clip_counters(), hnd.jpeg_progressive_counters()
            assert status.tolist() == [[0, -1]] * F and after["h2d"] - before["h2d"] == 1
            out = {"enqueues": after["enqueues"] - before["enqueues"], "h2d": 1, "scan_launches": pafter["launches"] - pbefore["launches"]}
            for key, fn in (("clip", clip), ("singles", singles)):
                sync()
                t = time.perf_counter()
                fn()                                      # a warm-up region, timed: a region of many seconds gets --slow-samples regions
                slow = time.perf_counter() - t > args.slow_seconds
                for _ in range(0 if slow else 2):
                    fn()
                ms = []
                for _ in range(args.slow_samples if slow else max(20, args.clip_samples)):
                    sync()
                    t = time.perf_counter()
                    fn()
                    ms.append((time.perf_counter() - t) * 1e3 / F)
                q = np.percentile(ms, [10, 50, 90])
                out[key + "_ms_per_frame"] = round(float(q[1]), 3)
                out[key + "_p10_p90"] = [round(float(q[0]), 3), round(float(q[2]), 3)]
                out[key + "_regions"] = len(ms)
                print(f"{h}x{w} {name} F={F} {key}: {out[key + '_ms_per_frame']} ms per frame", file=sys.stderr, flush=True)
            r[str(F)] = out
        res["progressive_clip"][name] = r
    return res


def exif_app1(value):
    """a big-endian Exif APP1 whose IFD0 holds the orientation tag alone"""
    import struct
    tiff = b"MM" + struct.pack(">HI", 42, 8) + struct.pack(">H", 1) + struct.pack(">HHIHH", 0x0112, 3, 1, value, 0) + struct.pack(">I", 0)
    payload = b"Exif\0\0" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def orient_leg(m, h, w, args):
    """row (viii): one stream per orientation value through whenet_frame_begin_jpeg_oriented, begin -> release -> collect"""
    import torch
    from PIL import Image
    from whenet_hip import jpeg, synth
    hnd = m._handle
    sync = torch.cuda.synchronize
    no_heads = np.zeros((0, 4), np.int32)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(synth.video_frame(h, w)[..., ::-1])).save(buf, "JPEG", quality=95, subsampling=2, restart_marker_rows=1)
    plain = buf.getvalue()
    app0_end = 4 + ((plain[4] << 8) | plain[5])
    res = {"frame": [h, w], "rule": args.rule, "rgb": bool(args.rgb), "bytes_jpeg": len(plain), "orient": {}}
    status = np.zeros(2, np.int32)
    for value in args.orient:
        data = plain[:app0_end] + exif_app1(value) + plain[app0_end:]
        want = jpeg.decode_host(data, bgr=not args.rgb, rule=RULES[args.rule], orient=True)
        got = jpeg.decode(data, handle=hnd, bgr=not args.rgb, rule=RULES[args.rule], orient=True)

        def begin():
            t, _ = hnd.frame_begin_jpeg_oriented(data, status, bgr=not args.rgb)
            hnd.frame_heads(t, no_heads)
            hnd.collect(t, 0)

        for _ in range(3):
            begin()
        ms = []
        for _ in range(max(20, args.clip_samples)):
            sync()
            t = time.perf_counter()
            begin()
            ms.append((time.perf_counter() - t) * 1e3)
        q = np.percentile(ms, [10, 50, 90])
        res["orient"][str(value)] = {"applied": jpeg.orientation(data), "shape": list(want.shape[:2]), "equals_host": bool(np.array_equal(got, want)),
                                     "ms": round(float(q[1]), 3), "p10_p90": [round(float(q[0]), 3), round(float(q[2]), 3)]}
    return res


def layouts_leg(m, h, w, args):
    """row (ix): begin -> release without heads -> collect, per stream and entropy form; see the module's text"""
    from PIL import Image
    from whenet_hip import jpeg, synth
    if m is not None:
        import torch
        hnd = m._handle
        sync = torch.cuda.synchronize
    no_heads = np.zeros((0, 4), np.int32)
    status = np.zeros(2, np.int32)
    frame = synth.video_frame(h, w)
    res = {"frame": [h, w], "rule": args.rule, "layouts": args.layouts, "repeats": max(5, args.repeats), "streams": {}}

    def timed(begin):
        for _ in range(3):
            begin()
        reps = []
        for _ in range(max(5, args.repeats)):
            ms = []
            for _ in range(max(5, args.clip_samples)):
                sync()
                t = time.perf_counter()
                begin()
                ms.append((time.perf_counter() - t) * 1e3)
            reps.append(statistics.median(ms))
        return {"ms": round(statistics.median(reps), 3), "spread": [round(min(reps), 3), round(max(reps), 3)]}

    def collect(t):
        hnd.frame_heads(t, no_heads)
        hnd.collect(t, 0)

    if args.layouts == "old":
        im = Image.fromarray(np.ascontiguousarray(frame[..., ::-1]))
        for name, sub in (("420", 2), ("422", 1), ("444", 0)):
            buf = io.BytesIO()
            im.save(buf, "JPEG", quality=95, subsampling=sub, restart_marker_rows=1)
            data = buf.getvalue()
            want = jpeg.decode_host(data, rule=RULES[args.rule])
            r = {"bytes_jpeg": len(data), "equals_host": True}
            for key, entropy in (("interval", 0), ("segmented", 1)):
                hnd.set_option("jpeg_entropy", entropy)
                r["equals_host"] = r["equals_host"] and bool(np.array_equal(jpeg.decode(data, handle=hnd, rule=RULES[args.rule], entropy=key), want))
                r[key] = timed(lambda: collect(hnd.frame_begin_jpeg(data, status)))
                print(f"{h}x{w} {name} {key}: {r[key]}", file=sys.stderr, flush=True)
            hnd.set_option("jpeg_entropy", 2)
            res["streams"][name] = r
        return res
    sys.path.insert(0, ROOT)
    from tests import jpeg_layout_cases as LC
    from whenet_hip import _lib
    accept = _lib.JPEG_ACCEPT_LAYOUTS
    table = [(n, hs, vs, [[0, 1, 2]], True) for n, (hs, vs) in (("422", (2, 1)), ("440", (1, 2)), ("411", (4, 1)), ("410", (4, 2)))]
    table += [("420_interleaved_rows", 2, 2, [[0, 1, 2]], True), ("420_three_scans_rows", 2, 2, [[0], [1], [2]], True),
              ("420_interleaved_nodri", 2, 2, [[0, 1, 2]], False), ("420_three_scans_nodri", 2, 2, [[0], [1], [2]], False)]
    for name, hs, vs, groups, rows in table:
        cached = os.path.join(args.stream_cache, f"layouts_{h}x{w}_{name}.jpg") if args.stream_cache else None
        if cached and os.path.exists(cached):
            with open(cached, "rb") as f:
                data = f.read()
        else:      # (the writer is plain Python: a 1080p stream takes it a minute)
            blocks = LC.blocks_of(h, w, hs, vs, picture_of=lambda hh, ww, seed: frame[..., ::-1])
            mcu_cols = -(-w // (8 * hs))
            # one interval per MCU row of the SCAN: a one-component scan's rows are its own block rows
            dris = [(mcu_cols if len(g) > 1 else -(-(w if g == [0] else -(-w // hs)) // 8)) if rows else None for g in groups]
            data = LC.write(blocks, h, w, hs, vs, groups=groups, dris=dris, annexk=True)      # (T.81 Annex K codes: what cameras write)
            if cached:
                os.makedirs(args.stream_cache, exist_ok=True)
                with open(cached, "wb") as f:
                    f.write(data)
        if args.write_only:
            res["streams"][name] = {"bytes_jpeg": len(data)}
            continue
        want = jpeg.decode_host(data, rule=RULES[args.rule], layouts=True)
        r = {"bytes_jpeg": len(data), "scans": len(groups), "equals_host": True}
        forms = (("interval", 0), ("segmented", 1)) if len(groups) == 1 else (("scan_plan", -1),)
        for key, entropy in forms:
            ent = "auto" if entropy < 0 else key
            r["equals_host"] = r["equals_host"] and bool(np.array_equal(jpeg.decode(data, handle=hnd, rule=RULES[args.rule], entropy=ent, layouts=True), want))
            if entropy >= 0:
                hnd.set_option("jpeg_entropy", entropy)
            r[key] = timed(lambda: collect(hnd.frame_begin_jpeg_accept(data, status, accept=accept)[0]))
            print(f"{h}x{w} {name} {key}: {r[key]}", file=sys.stderr, flush=True)
        hnd.set_option("jpeg_entropy", 2)
        res["streams"][name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1080x1920", "480x640"], help="frame sizes, HxW")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--entropy", type=int, nargs="+", default=[0, 1], choices=[0, 1, 2], help="forms of the entropy stage to time")
    ap.add_argument("--seg-bytes", type=int, nargs="+", default=[128], help="segment sizes of the segmented form")
    ap.add_argument("--lanes", type=int, default=0, choices=[0, 16, 32, 64], help="decoding lanes per wave of the segmented kernels")
    ap.add_argument("--rule", type=int, default=0, choices=[0, 1], help="the decode rule: 0 the project's own, 1 libjpeg's bytes")
    ap.add_argument("--rgb", action="store_true", help="row (i) decodes into R, G, B order (rule 0 then takes its frame kernel too)")
    ap.add_argument("--only-decode", action="store_true", help="rows (i) only")
    ap.add_argument("--clip", type=int, nargs="+", default=None, help="row (v) only: frames per clip of JPEG streams, 1..16 each")
    ap.add_argument("--clip-samples", type=int, default=20, help="regions per figure of row (v), at least 20")
    ap.add_argument("--progressive", action="store_true", help="row (vi) only: progressive streams against their baseline twins; with --clip: row (vii)")
    ap.add_argument("--orient", type=int, nargs="+", default=None, choices=range(1, 9), help="row (viii) only: EXIF orientation values to time")
    ap.add_argument("--layouts", choices=["old", "new"], default=None, help="row (ix) only: the streams that existed before the LAYOUTS section, or its new ones")
    ap.add_argument("--stream-cache", default=None, help="row (ix) new: a folder that keeps the written streams from run to run")
    ap.add_argument("--write-only", action="store_true", help="row (ix) new: write the streams into --stream-cache and stop (needs no GPU)")
    ap.add_argument("--repeats", type=int, default=5, help="row (ix): repeats per figure, at least 5")
    ap.add_argument("--slow-seconds", type=float, default=5.0, help="row (vii): a region longer than this counts as slow")
    ap.add_argument("--slow-samples", type=int, default=20, help="row (vii): regions per figure where one region is slow (after ONE warm-up region)")
    args = ap.parse_args()
    if args.layouts == "new" and args.write_only:
        for size in args.sizes:
            h, w = (int(v) for v in size.split("x"))
            print(json.dumps(layouts_leg(None, h, w, args)), flush=True)
        return 0
    import torch  # noqa: F401  (first: one HIP runtime in the process, torch's)
    import whenet
    m = whenet.WHENet(dtype="f16")
    m._handle.set_option("jpeg_seg_lanes", args.lanes)
    m._handle.set_option("jpeg_rule", args.rule)
    try:
        for size in args.sizes:
            h, w = (int(v) for v in size.split("x"))
            leg = (prog_clip_leg if args.clip else prog_leg) if args.progressive else (clip_leg if args.clip else size_leg)
            if args.orient:
                leg = orient_leg
            if args.layouts:
                leg = layouts_leg
            print(json.dumps(leg(m, h, w, args)), flush=True)
    finally:
        m.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
