"""The segmented form of the JPEG decoder's entropy stage on the GPU (csrc/jpeg_dec_seg.hip, routed by launch_jpeg_decode): no
tolerance anywhere.  Forced through whenet_op_jpeg_decode_ex it returns the bytes and the status of `whenet_jpeg_decode_host`, its
statistics are those of the host emulation (`whenet_jpeg_decode_segmented_host`, tests/test_jpeg_decode_seg_cpu.py), and the handle's
options route the three entry points to it.  Every stream is at most 72 KB."""
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_decode_cases as DC
from whenet_hip import _lib, jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 0xC3


def flat_stream(mode):
    im = Image.new(mode, (256, 256), (90, 140, 200) if mode == "RGB" else 117)
    out = io.BytesIO()
    im.save(out, "JPEG", quality=90, **({"subsampling": 2} if mode == "RGB" else {}))
    return out.getvalue()


STREAMS = {n: (lambda n=n: DC.case(n)) for n in
           ("pil_420_50x70", "pil_422_50x70", "pil_444_q100", "pil_grey_50x70", "pil_420_1x1", "pil_420_rst_rows", "pil_444_rst_blocks3",
            "pil_420_16x4800_rst_rows", "pil_420_8192x16", "sample_001", "sample_012")}
STREAMS["flat_420"] = lambda: flat_stream("RGB")
STREAMS["flat_grey"] = lambda: flat_stream("L")
for _n in DC.DAMAGED_NAMES:
    STREAMS[_n] = (lambda n=_n: DC.DAMAGED[n]()[0])
SEG_BYTES = (4, 8, 128)
STITCHED = "sample_001"      # at seg_bytes 8 the host emulation walks 91 segments in the stitch (checked on the CPU as well)


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def reference():
    """name -> (stream, frame, status, planes) of the host statement: computed once, shared, never modified"""
    out = {}
    for name, make in STREAMS.items():
        data = make()
        assert len(data) <= 72 * 1024
        i = _lib.jpeg_parse(data)
        frame = np.empty((i.h, i.w, 3), np.uint8)
        status = _lib.jpeg_decode_host(data, jpeg.packed_surface(frame), True)
        out[name] = (data, frame, status, jpeg.decode_planes_host(data)[0])
    return out


def guarded_rows(rows, row_bytes, extra, shift):
    pitch = row_bytes + extra
    block = np.full(shift + rows * pitch + 16, GAP, np.uint8)
    view = np.lib.stride_tricks.as_strided(block[shift:], (rows, row_bytes), (pitch, 1))
    return block, view, pitch


def untouched(block, view):
    mask = np.ones(block.size, bool)
    start = view.ctypes.data - block.ctypes.data
    for r in range(view.shape[0]):
        mask[start + r * view.strides[0]:start + r * view.strides[0] + view.shape[1]] = False
    return bool((block[mask] == GAP).all())


# ---- 1. the forced segmented form is the host statement, and its statistics are the host emulation's ---------------------------------
@pytest.mark.parametrize("seg_bytes", SEG_BYTES)
@pytest.mark.parametrize("name", list(STREAMS))
def test_forced_segmented_form_equals_decode_host(post, reference, name, seg_bytes):
    data, want, want_status, planes = reference[name]
    i = _lib.jpeg_parse(data)
    block, view, pitch = guarded_rows(i.h, 3 * i.w, 7, 3)                      # an odd pitch between guard bytes
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
    status, stats = post.op_jpeg_decode_ex(data, s, True, 1, seg_bytes)
    assert status.tolist() == want_status.tolist()
    assert np.array_equal(view.reshape(i.h, i.w, 3), want)
    assert untouched(block, view)
    _, host_status, host_stats = jpeg.decode_segmented_host(data, seg_bytes, _lib.JPEG_SEG_WINDOW, stats=True)
    assert host_status.tolist() == want_status.tolist()
    assert stats[:5].tolist() == host_stats[:5].tolist()                        # intervals, segments, windows, sync rounds, stitch walks
    assert stats[6] == seg_bytes and stats[7] == 1
    if (i.components, i.hs, i.vs) == (3, 2, 2):
        h, w, ch, cw = i.h, i.w, (i.h + 1) // 2, (i.w + 1) // 2
        blocks = [guarded_rows(*g) for g in [(h, w, 3, 1), (ch, cw, 5, 2), (ch, cw, 2, 3)]]
        s = _lib.SurfaceC()
        for p, (_, v, pt) in enumerate(blocks):
            s.plane[p], s.pitch[p] = v.ctypes.data, pt
        s.format, s.matrix, s.on_device = _lib.YUV_I420, _lib.YUV_JFIF, 0
        status, _ = post.op_jpeg_decode_ex(data, s, True, 1, seg_bytes)
        assert status.tolist() == want_status.tolist()
        for (blk, v, _), ref in zip(blocks, planes):
            assert np.array_equal(v, ref) and untouched(blk, v)


def test_the_stitch_ran_on_the_device(post, reference):
    data, want, _, _ = reference[STITCHED]
    got, stats = jpeg.decode(data, handle=post, entropy="segmented", seg_bytes=8, stats=True)
    assert np.array_equal(got, want)
    assert stats[1] == 21376 // 8 and stats[2] >= 10 and stats[4] >= 1 and stats[7] == 1


@pytest.mark.parametrize("name", ["pil_420_rst_rows", "sample_012", "stray_marker", "truncated_no_dri"])
def test_entropy_0_through_ex_equals_op_jpeg_decode(post, reference, name):
    data, want, want_status, _ = reference[name]
    a, b = np.zeros_like(want), np.zeros_like(want)
    st_a = post.op_jpeg_decode(data, jpeg.packed_surface(a), True)
    st_b, stats = post.op_jpeg_decode_ex(data, jpeg.packed_surface(b), True, 0)
    assert st_a.tolist() == st_b.tolist() == want_status.tolist()
    assert a.tobytes() == b.tobytes() == want.tobytes()
    assert stats[7] == 0 and stats[0] == jpeg.decode_segmented_host(data, 64, stats=True)[2][0] and not stats[1:7].any()


def test_bad_arguments_of_ex_are_refused(post, reference):
    data, want, _, _ = reference["pil_420_50x70"]
    frame = np.full_like(want, GAP)
    for entropy, seg_bytes in ((2, 128), (-1, 128), (1, 0), (1, 100), (1, 8192)):
        with pytest.raises(ValueError):
            post.op_jpeg_decode_ex(data, jpeg.packed_surface(frame), True, entropy, seg_bytes)
    for key, bad in (("jpeg_entropy", 3), ("jpeg_entropy", -1), ("jpeg_seg_bytes", 96), ("jpeg_seg_bytes", 2), ("jpeg_seg_bytes", 8192)):
        with pytest.raises(ValueError):
            post.set_option(key, bad)
    assert (frame == GAP).all()


# ---- 2. the handle's options route the entry points -----------------------------------------------------------------------------------
def device_packed(h, w, extra, shift):
    buf = torch.full((shift + h * (3 * w + extra) + 16,), GAP, dtype=torch.uint8, device=DEV)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = buf.data_ptr() + shift, 3 * w + extra, _lib.SURF_PACKED, 1
    return buf, s


def read_packed(buf, h, w, extra, shift):
    host = buf.cpu().numpy()
    pitch = 3 * w + extra
    view = np.lib.stride_tricks.as_strided(host[shift:], (h, 3 * w), (pitch, 1))
    return view.reshape(h, w, 3).copy(), untouched(host, view)


@pytest.fixture(scope="module")
def model():
    from tests.test_yuv_gpu import seeded_model
    m = seeded_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def kw():
    from tests.test_clip_gpu import kwargs
    with open(os.path.join(DC.ROOT, "tests", "golden", "reference_detector.json")) as f:
        return kwargs(json.load(f)["detect"], "tiny", score=0.02)


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


def test_begin_jpeg_follows_the_handles_option(model, kw, reference):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    data, frame, _, _ = reference["sample_001"]
    h = model._handle
    results = {}
    try:
        for option in (0, 1):
            h.set_option("jpeg_entropy", option)
            before = h.jpeg_decode_counters()
            with FramePipeline(model, depth=1) as fp:
                st = fp.begin_jpeg(data)
                fp.detect_heads(**kw)
                out = np.zeros_like(frame)
                fp.annotate(out, display="full")
                results[option] = (fp.collect(detections=True), out)
            assert st.ok and st.interval == -1
            assert delta(h.jpeg_decode_counters(), before) == {"interval": 1 - option, "segmented": option}
    finally:
        h.set_option("jpeg_entropy", 2)
    assert_same(results[1][0], results[0][0])
    assert np.array_equal(results[1][1], results[0][1]) and results[0][1].any()


def test_jpeg_decode_device_follows_the_option_on_the_librarys_own_stream(model, reference):
    from whenet_hip.frames import FramePipeline
    _, frame, _, _ = reference["sample_001"]
    boxes = np.asarray([(8, 8, 30, 30), (12, 14, 36, 40)], np.float32)
    with FramePipeline(model, depth=1) as fp:
        fp.begin(frame)
        fp.heads(boxes)
        stream = fp.annotate_jpeg(quality=90)
        fp.collect()
    data = stream.tobytes()
    assert len(data) <= 72 * 1024
    info = _lib.jpeg_parse(data)
    ent = torch.from_numpy(np.frombuffer(data, np.uint8)[info.data_offset:].copy()).to(DEV)
    want, want_status = np.empty((info.h, info.w, 3), np.uint8), None
    want_status = _lib.jpeg_decode_host(data, jpeg.packed_surface(want), True)
    h = _lib.Handle.postproc(0)
    try:
        got = {}
        for option in (0, 1):
            h.set_option("jpeg_entropy", option)
            before = h.jpeg_decode_counters()
            status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
            buf, s_dst = device_packed(info.h, info.w, 5, 3)
            h.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s_dst, True, status.data_ptr())
            torch.cuda.synchronize()
            got[option], clean = read_packed(buf, info.h, info.w, 5, 3)
            assert clean and status.cpu().tolist() == want_status.tolist() == [_lib.OK, -1]
            assert delta(h.jpeg_decode_counters(), before) == {"interval": 1 - option, "segmented": option}
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[1], want)
    finally:
        h.close()


def test_auto_takes_the_form_the_threshold_predicts(reference):
    """option jpeg_entropy = 2 (the default): segmented from JPEG_SEG_AUTO_BYTES = 4096 bytes of entropy data per interval on"""
    h = _lib.Handle.postproc(0)
    try:
        for name, form in (("sample_001", "segmented"), ("pil_420_rst_rows", "interval")):
            data, want, want_status, _ = reference[name]
            i = _lib.jpeg_parse(data)
            per_interval = (len(data) - i.data_offset) // i.intervals
            assert (per_interval >= _lib.JPEG_SEG_AUTO_BYTES) == (form == "segmented")
            before = h.jpeg_decode_counters()
            got = np.zeros_like(want)
            status = h.op_jpeg_decode(data, jpeg.packed_surface(got), True)
            assert np.array_equal(got, want) and status.tolist() == want_status.tolist()
            d = delta(h.jpeg_decode_counters(), before)
            assert d[form] == 1 and sum(d.values()) == 1, (name, d)
    finally:
        h.close()


# ---- 3. ordering ----------------------------------------------------------------------------------------------------------------------
def test_a_segmented_decode_is_ordered_on_the_callers_stream(reference):
    data, want, _, _ = reference["sample_012"]
    info = _lib.jpeg_parse(data)
    host_ent = torch.from_numpy(np.frombuffer(data, np.uint8)[info.data_offset:].copy()).pin_memory()
    ent = torch.zeros(host_ent.numel(), dtype=torch.uint8, device=DEV)
    status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    buf, s_dst = device_packed(info.h, info.w, 0, 0)
    h = _lib.Handle.postproc(0)
    try:
        h.set_option("jpeg_entropy", 1)
        h.set_option("jpeg_seg_bytes", 64)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            ent.copy_(host_ent, non_blocking=True)                                          # written before ...
            h.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s_dst, True, status.data_ptr(), stream=side.cuda_stream)
            seen, st = buf.clone(), status.clone()                                          # ... and read after
        side.synchronize()
        assert h.jpeg_decode_counters() == {"interval": 0, "segmented": 1}
    finally:
        h.close()
    assert st.cpu().tolist() == [_lib.OK, -1]
    assert np.array_equal(read_packed(seen, info.h, info.w, 0, 0)[0], want)
