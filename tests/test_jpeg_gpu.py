"""The JPEG encoder on the GPU (csrc/jpeg.hip; Engine::op_jpeg_encode / jpeg_encode_device of csrc/engine_post.cpp).  There is no
tolerance anywhere: the kernels return the bytes of `whenet_jpeg_encode_host`, which tests/test_jpeg_cpu.py holds to the numpy
statement, and those of the statement's committed digests; a device destination keeps every byte behind the stream."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_cases as JC
from whenet_hip import _lib, jpeg, overlay
from whenet_hip.yuv import YUVFrame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 0xC3                 # what device memory holds where nothing may be written


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def digests():
    return JC.load_digests()


# ---- 1. the kernels alone are the host statement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(JC.GPU_CASES))
def test_op_jpeg_encode_equals_the_host_function_and_the_digests(post, digests, name):
    case = JC.GPU_CASES[name]
    planes, frame = case.source()
    h, w = planes[0].shape
    got = jpeg.encode(frame, case.quality, handle=post, bgr=case.bgr)
    assert got == jpeg.encode_host(frame, case.quality, bgr=case.bgr)
    assert JC.digest(got) == digests[name]["sha256"] and len(got) == digests[name]["bytes"]
    im = Image.open(io.BytesIO(got))                    # (the host's bytes; asserted anyway, so that a GPU-only run stands alone)
    im.load()
    assert im.size == (w, h) and im.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]


def test_op_jpeg_encode_overflow_and_refusals(post):
    case = JC.CASES["noise_q100_stuffed"]
    _, frame = case.source()
    full = jpeg.encode_host(frame, case.quality)
    surface, h, w, _keep = jpeg.source_of(frame)
    for cap in (len(full), len(full) - 1, JC.HEADER_BYTES, 0):
        out = np.full(len(full) + 64, 0xC5, np.uint8)
        rc, size = post.op_jpeg_encode(surface, h, w, True, case.quality, out[:cap])
        assert rc == (_lib.OK if cap == len(full) else _lib.EOVERFLOW) and size == len(full)
        assert out[:cap].tobytes() == full[:cap] and (out[cap:] == 0xC5).all()
    with pytest.raises(jpeg.CapacityError) as err:
        jpeg.encode(frame, case.quality, handle=post, capacity=100)
    assert err.value.needed == len(full)
    y, c = np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError, match="JFIF"):
        jpeg.encode(YUVFrame.i420(y, c, c, "bt601"), handle=post)
    for q in (0, 101):
        with pytest.raises(ValueError):
            jpeg.encode(frame, q, handle=post)
    t = torch.zeros((16, 16, 3), dtype=torch.uint8, device=DEV)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = t.data_ptr(), 48, _lib.SURF_PACKED, 0       # device memory marked as host
    with pytest.raises(ValueError):
        post.op_jpeg_encode(s, 16, 16, True, 95, np.zeros(4096, np.uint8))
    assert jpeg.encode(frame, case.quality, handle=post) == full                                # the handle stays usable


# ---- 2. source and destination in device memory -----------------------------------------------------------------------------------
def device_plane(a, extra):
    """A tight uint8 [rows, rb] plane as a device view whose rows are rb + extra bytes apart, the padding filled with GAP."""
    buf = torch.full((a.shape[0], a.shape[1] + extra), GAP, dtype=torch.uint8, device=DEV)
    buf[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return buf, buf[:, :a.shape[1]]


def device_source(case):
    """(SurfaceC with on_device = 1, h, w, the tensors that hold the memory, [(tensor, tight plane)] for the padding check)"""
    planes, frame = case.source()
    h, w = planes[0].shape
    if case.kind in ("bgr", "rgb"):
        tight = np.ascontiguousarray(frame).reshape(h, 3 * w)
        buf, view = device_plane(tight, case.extra)
        s = _lib.SurfaceC()
        s.plane[0], s.pitch[0], s.format, s.on_device = buf.data_ptr(), 3 * w + case.extra, _lib.SURF_PACKED, 1
        return s, h, w, [buf], [(buf, tight)]
    if case.kind == "i420":
        tights = list(planes)
    else:
        tights = [planes[0], np.stack([planes[1], planes[2]], -1).reshape(planes[1].shape[0], -1)]
    pairs = [device_plane(t, case.extra + i) for i, t in enumerate(tights)]
    make = YUVFrame.i420 if case.kind == "i420" else YUVFrame.nv12
    dev = make(*[v for _, v in pairs], matrix="jfif")
    s, keep = overlay.surface_of(dev, h, w)
    assert s.on_device == 1
    return s, h, w, [keep] + [b for b, _ in pairs], [(b, t) for (b, _), t in zip(pairs, tights)]


DEVICE_CASES = ["17x17", "130x250_gradient", "i420_pitched", "nv12_pitched", "bgr_pitched", "rgb_pitched", "noise_q100_stuffed", "wide_16x1040"]


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_jpeg_encode_device(post, name):
    case = JC.GPU_CASES[name]
    _, frame = case.source()
    full = jpeg.encode_host(frame, case.quality, bgr=case.bgr)
    s, h, w, _keep, padded = device_source(case)
    for cap in (len(full) + 40, len(full), len(full) - 1):
        dst = torch.full((len(full) + 128,), GAP, dtype=torch.uint8, device=DEV)
        dsize = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        post.jpeg_encode_device(s, h, w, case.bgr, case.quality, dst.data_ptr(), cap, dsize.data_ptr())
        torch.cuda.synchronize()
        assert int(dsize.item()) == len(full)                  # the full length, also when it does not fit
        got = dst.cpu().numpy()
        n = min(cap, len(full))
        assert got[:n].tobytes() == full[:n] and (got[n:] == GAP).all(), (name, cap)
    for buf, tight in padded:                                  # the source is read only: rows and pitch padding as they were
        host = buf.cpu().numpy()
        assert host[:, :tight.shape[1]].tobytes() == tight.tobytes() and (host[:, tight.shape[1]:] == GAP).all()


def test_jpeg_encode_device_is_ordered_on_the_callers_stream(post):
    case = JC.CASES["130x250_noise"]
    _, frame = case.source()
    s, h, w, keep, _ = device_source(case)
    side = torch.cuda.Stream()
    dst = torch.empty(jpeg.bound(h, w), dtype=torch.uint8, device=DEV)
    dsize = torch.zeros(1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        keep[0].copy_(torch.from_numpy(np.ascontiguousarray(frame).reshape(h, -1)).to(DEV), non_blocking=True)    # written before ...
        post.jpeg_encode_device(s, h, w, True, case.quality, dst.data_ptr(), dst.numel(), dsize.data_ptr(), stream=side.cuda_stream)
        n = dsize.clone()                                                                                        # ... and read after
        head = dst[:JC.HEADER_BYTES].clone()
    side.synchronize()
    full = jpeg.encode_host(frame, case.quality)
    assert int(n.item()) == len(full) and head.cpu().numpy().tobytes() == full[:JC.HEADER_BYTES]
    assert dst[:len(full)].cpu().numpy().tobytes() == full


def test_jpeg_encode_device_refuses_host_pointers_before_anything_is_enqueued(post):
    case = JC.CASES["17x17"]
    _, frame = case.source()
    full = jpeg.encode_host(frame, case.quality)
    s, h, w, _keep, _ = device_source(case)
    dst = torch.full((len(full) + 64,), GAP, dtype=torch.uint8, device=DEV)
    dsize = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    host_dst, host_size = np.zeros(len(full) + 64, np.uint8), np.zeros(1, np.int64)
    hs, _, _, _keep2 = jpeg.source_of(frame)
    hs.on_device = 1                                                               # host planes marked as device memory
    with pytest.raises(ValueError):
        post.jpeg_encode_device(hs, h, w, True, case.quality, dst.data_ptr(), dst.numel(), dsize.data_ptr())
    with pytest.raises(ValueError):
        post.jpeg_encode_device(s, h, w, True, case.quality, host_dst.ctypes.data, host_dst.size, dsize.data_ptr())
    with pytest.raises(ValueError):
        post.jpeg_encode_device(s, h, w, True, case.quality, dst.data_ptr(), dst.numel(), host_size.ctypes.data)
    with pytest.raises(ValueError):                                                # a capacity beyond the allocation
        post.jpeg_encode_device(s, h, w, True, case.quality, dst.data_ptr(), (dst.numel() + 1) << 20, dsize.data_ptr())
    s.on_device = 0
    with pytest.raises(ValueError):
        post.jpeg_encode_device(s, h, w, True, case.quality, dst.data_ptr(), dst.numel(), dsize.data_ptr())
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == GAP).all() and int(dsize.item()) == -1 and not host_dst.any() and not host_size.any()
    s.on_device = 1
    post.jpeg_encode_device(s, h, w, True, case.quality, dst.data_ptr(), dst.numel(), dsize.data_ptr())
    torch.cuda.synchronize()
    assert dst[:len(full)].cpu().numpy().tobytes() == full and int(dsize.item()) == len(full)


# ---- 3. the pipeline: annotate_jpeg ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from tests.test_yuv_gpu import seeded_model
    m = seeded_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def kw():
    import json
    import os
    from tests.test_clip_gpu import kwargs
    with open(os.path.join(JC.ROOT, "tests", "golden", "reference_detector.json")) as f:
        return kwargs(json.load(f)["detect"], "tiny", score=0.02)       # a low threshold: the seeded detector then fires on small frames


@pytest.fixture(scope="module")
def frames():
    """Small BGR pictures cut from the committed sample frames: 97 x 131, 128 x 160 and 75 x 101."""
    from tests import detector_cases as DC
    f0, f1 = DC.sample_frame(0), DC.sample_frame(1)
    return [np.ascontiguousarray(f1[60:157, 200:331]), np.ascontiguousarray(f0[40:168, 180:340]), np.ascontiguousarray(f1[100:175, 300:401])]


HEAD_BOXES = [(10, 12, 50, 60), (30, 40, 90, 100), (5, 70, 60, 125)]


@pytest.mark.parametrize("display", ["simple", "full"])
@pytest.mark.parametrize("heads", [0, 1, 3])
def test_annotate_jpeg_is_the_stream_of_the_annotated_surface(model, frames, display, heads):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    frame = frames[0]
    h, w = frame.shape[:2]
    boxes = np.asarray(HEAD_BOXES[:heads], np.float32).reshape(-1, 4)
    quality = 90 if display == "simple" else 95
    with FramePipeline(model, depth=1) as fp:
        fp.begin(frame)
        fp.heads(boxes)
        plain = fp.collect()
        surface = overlay.new_output(h, w, "i420", "jfif")              # the surface annotate() writes for the same submission
        fp.begin(frame)
        fp.heads(boxes)
        fp.annotate(surface, display=display)
        assert_same(fp.collect(), plain)
        fp.begin(frame)
        fp.heads(boxes)
        jf = fp.annotate_jpeg(quality=quality, display=display)
        with pytest.raises(ValueError, match="not collected"):
            jf.tobytes()
        assert_same(fp.collect(), plain)                                 # collect returns what it returns without it
    assert len(plain[0]) == heads
    got = jf.tobytes()
    assert got == jpeg.encode_host(surface, quality)
    im = Image.open(io.BytesIO(got))
    im.load()
    assert im.size == (w, h) == (jf.width, jf.height)


def test_annotate_clip_jpeg_of_a_mixed_clip_equals_the_frames_alone(model, kw, frames):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    with FramePipeline(model, depth=2) as fp:
        fp.begin_clip_mixed(frames)
        fp.detect_heads_clip(**kw)
        plain = fp.collect_clip()
        fp.begin_clip_mixed(frames)
        fp.detect_heads_clip(**kw)
        clip = fp.annotate_clip_jpeg(quality=80, display="full")
        got = fp.collect_clip()
        assert got[1] == plain[1] and len(clip) == 3
        for g, p in zip(got[0], plain[0]):
            assert_same(g, p)
        alone, painted = [], 0
        for frame in frames:                                             # two frames in flight: the second is enqueued before the first ends
            fp.begin(frame)
            fp.detect_heads(**kw)
            alone.append(fp.annotate_jpeg(quality=80, display="full"))
            if len(alone) >= 2:
                painted += len(fp.collect()[0])
        painted += len(fp.collect()[0])
    assert painted >= 2
    for frame, c, a in zip(frames, clip, alone):
        data = c.tobytes()
        assert data == a.tobytes() and (c.width, c.height) == (frame.shape[1], frame.shape[0])
        assert data[:JC.HEADER_BYTES] == jpeg.header(frame.shape[0], frame.shape[1], 80)


def test_annotate_jpeg_call_order_and_overflow(model, frames):
    from whenet_hip.frames import FramePipeline
    frame = frames[2]
    boxes = np.asarray([(10, 10, 50, 60), (20, 40, 70, 90)], np.float32)
    with FramePipeline(model, depth=1) as fp:
        with pytest.raises(ValueError):
            fp.annotate_jpeg()                                           # nothing in flight
        fp.begin(frame)
        with pytest.raises(ValueError):
            fp.annotate_jpeg()                                           # before the heads
        hnd, ticket = fp._h, fp._begun[0]
        out, result = np.zeros(4096, np.uint8), np.zeros(2, np.int64)
        with pytest.raises(ValueError, match="not enqueued"):
            hnd.frame_annotate_jpeg(ticket, 0, _lib.DISPLAY_SIMPLE, 95, out, result)      # the library's own refusal
        fp.heads(boxes)
        for bad_quality in (0, 101):
            with pytest.raises(ValueError, match="quality"):
                hnd.frame_annotate_jpeg(ticket, 0, _lib.DISPLAY_SIMPLE, bad_quality, out, result)
        with pytest.raises(ValueError, match="frame index"):
            hnd.frame_annotate_jpeg(ticket, 1, _lib.DISPLAY_SIMPLE, 95, out, result)
        full = fp.annotate_jpeg()
        with pytest.raises(ValueError, match="annotated already"):
            fp.annotate_jpeg()                                           # a second call
        with pytest.raises(ValueError, match="annotated already"):
            hnd.frame_annotate_jpeg(ticket, 0, _lib.DISPLAY_SIMPLE, 95, out, result)
        with pytest.raises(ValueError, match="annotated already"):
            fp.annotate(np.zeros_like(frame))                            # it is the frame's one annotate call
        res = fp.collect()
        assert len(res[0]) == 2 and not out.any() and not result.any()
        data = full.tobytes()
        for capacity in (len(data) - 1, JC.HEADER_BYTES, 0):
            fp.begin(frame)
            fp.heads(boxes)
            small = fp.annotate_jpeg(capacity=capacity)
            fp.collect()
            with pytest.raises(jpeg.CapacityError, match=str(len(data))) as err:
                small.tobytes()
            assert err.value.needed == len(data)
            assert small._out.tobytes() == data[:capacity]
        fp.begin(frame)
        fp.heads(boxes)
        exact = fp.annotate_jpeg(capacity=len(data))
        fp.collect()
        assert exact.tobytes() == data
