"""The JPEG encoder's samplings and optimised Huffman tables on the GPU (csrc/jpeg.hip: the per-sampling dct / pack kernels, the
histogram and the table kernel).  There is no tolerance anywhere: the kernels return the bytes, the histograms, the tables and the
header of `whenet_jpeg_encode_host_ex`, which tests/test_jpeg_sampling_cpu.py holds to the numpy statement."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import jpeg_sampling_cases as SC
from whenet_hip import _lib, jpeg, overlay

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 0xC3
SAMPLINGS = list(SC.SAMPLINGS)


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


def _host(case, optimize, **kw):
    return jpeg.encode_host(case.pixels, case.quality, bgr=case.bgr, sampling=case.sampling, optimize=optimize, **kw)


def _device(case, optimize, post, **kw):
    return jpeg.encode(case.pixels, case.quality, handle=post, bgr=case.bgr, sampling=case.sampling, optimize=optimize, **kw)


def _tables_of(data):
    """the header of a stream and the DHT tables it carries"""
    n = data.index(b"\xff\xda") + 14
    return data[:n], SC.parse(data).tables


# ---- 1. the kernels alone are the host statement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_op_jpeg_encode_equals_the_host_function(post, sampling, optimize):
    for case in SC.by_sampling()[sampling]:
        want_hist, got_hist = np.zeros((4, 256), np.uint32), np.full((4, 256), 0xABCD, np.uint32)
        want = _host(case, optimize, hist=want_hist)
        got = _device(case, optimize, post, hist=got_hist)
        assert got == want, case.name
        if optimize:
            assert np.array_equal(got_hist, want_hist), case.name                      # the device histograms
            assert got[:got.index(b"\xff\xda") + 14] == want[:want.index(b"\xff\xda") + 14]      # the device-built tables and header
        else:
            assert (got_hist == 0xABCD).all()


def test_the_device_built_tables_are_the_statements(post):
    for name in ("35x50_lines_q100_bgr_4:4:4", "8x704_444", "9x24_422"):
        case = SC.ALL[name]
        want = SC.statement(case, True)
        head, tables = _tables_of(_device(case, True, post))
        assert [tables[t] for t in SC.TC_TH] == [([int(b) for b in bits], list(vals)) for bits, vals in want.tables]
        assert head == SC.header(*case.pixels.shape[:2], case.quality, case.sampling, want.tables) and len(head) < 629


def test_the_default_keywords_give_the_bytes_of_the_existing_calls(post):
    for name in ("17x17", "i420_pitched", "nv12_pitched", "rgb_pitched", "130x250_gradient"):
        case = JC.CASES[name]
        _, frame = case.source()
        old = jpeg.encode(frame, case.quality, handle=post, bgr=case.bgr)
        assert old == jpeg.encode(frame, case.quality, handle=post, bgr=case.bgr, sampling="4:2:0", optimize=False) == JC.statement(case).data
        s, h, w, _keep = jpeg.source_of(frame)
        out, size = np.zeros(jpeg.bound(h, w), np.uint8), C.c_int64(0)
        rc = _lib.load().whenet_op_jpeg_encode(post._h, C.byref(s), h, w, _lib.BGR if case.bgr else _lib.RGB, case.quality, out.ctypes.data,
                                               out.size, C.byref(size))        # the entry point without _ex
        assert rc == _lib.OK and out[:size.value].tobytes() == old


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_both_orders_of_two_frames_through_one_handle(sampling):
    """the per-encode tables and the zeroed histograms do not leak between calls"""
    a, b = (c for n, c in SC.CASES.items() if n.startswith("35x50_") and n.endswith(f"_q95_bgr_{sampling}") or
            n.startswith("64x48_") and n.endswith(f"_q30_rgb_{sampling}"))
    want = {c.name: _host(c, True) for c in (a, b)}
    for order in ((a, b, a), (b, a, b)):
        h = _lib.Handle.postproc(0)
        try:
            for c in order:
                hist = np.zeros((4, 256), np.uint32)
                assert _device(c, True, h, hist=hist) == want[c.name], (c.name, [o.name for o in order])
                assert np.array_equal(hist, SC.statement(c, True).hist)
                assert _device(c, False, h) == _host(c, False)           # and the standard tables in between keep theirs
        finally:
            h.close()


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("sampling", ["4:2:2", "4:4:4"])
def test_op_jpeg_encode_overflow_and_refusals(post, sampling, optimize):
    case, = (c for n, c in SC.CASES.items() if n.startswith("35x50_") and n.endswith(f"_q100_bgr_{sampling}"))
    full = _host(case, optimize)
    head = full.index(b"\xff\xda") + 14
    surface, h, w, _keep = jpeg.source_of(case.pixels)
    for cap in (len(full), len(full) - 1, 629, head, head - 1, 0):
        out = np.full(len(full) + 64, 0xC5, np.uint8)
        rc, size = post.op_jpeg_encode(surface, h, w, True, case.quality, out[:cap], sampling, optimize)
        assert rc == (_lib.OK if cap == len(full) else _lib.EOVERFLOW) and size == len(full)
        assert out[:cap].tobytes() == full[:cap] and (out[cap:] == 0xC5).all()
    with pytest.raises(jpeg.CapacityError) as err:
        _device(case, optimize, post, capacity=100)
    assert err.value.needed == len(full)
    with pytest.raises(ValueError, match="sampling"):
        jpeg.encode(case.pixels, handle=post, sampling="4:1:1")
    from whenet_hip.yuv import YUVFrame
    y, c = np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError, match="4:2:0 chroma"):
        jpeg.encode(YUVFrame.i420(y, c, c, "jfif"), handle=post, sampling=sampling, optimize=optimize)
    assert _device(case, optimize, post) == full                         # the handle stays usable


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("sampling", ["4:2:2", "4:4:4"])
def test_jpeg_encode_device(post, sampling, optimize):
    case, = (c for n, c in SC.CASES.items() if n.startswith("33x18_") and n.endswith(f"_q95_rgb_{sampling}"))
    full = _host(case, optimize)
    h, w = case.pixels.shape[:2]
    extra = 5
    buf = torch.full((h, 3 * w + extra), GAP, dtype=torch.uint8, device=DEV)
    buf[:, :3 * w] = torch.from_numpy(case.pixels.reshape(h, 3 * w)).to(DEV)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = buf.data_ptr(), 3 * w + extra, _lib.SURF_PACKED, 1
    for cap in (len(full) + 40, len(full), len(full) - 1):
        dst = torch.full((len(full) + 128,), GAP, dtype=torch.uint8, device=DEV)
        dsize = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        post.jpeg_encode_device(s, h, w, case.bgr, case.quality, dst.data_ptr(), cap, dsize.data_ptr(), sampling=sampling, optimize=optimize)
        torch.cuda.synchronize()
        assert int(dsize.item()) == len(full)                  # the full length, also when it does not fit
        got = dst.cpu().numpy()
        n = min(cap, len(full))
        assert got[:n].tobytes() == full[:n] and (got[n:] == GAP).all(), cap
    host = buf.cpu().numpy()                                   # the source is read only
    assert host[:, :3 * w].tobytes() == case.pixels.tobytes() and (host[:, 3 * w:] == GAP).all()


# ---- 2. the pipeline: annotate_jpeg / annotate_clip_jpeg -------------------------------------------------------------------------
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
    """Small BGR pictures cut from the committed sample frames: 97 x 131 and 128 x 160."""
    from tests import detector_cases as DC
    f0, f1 = DC.sample_frame(0), DC.sample_frame(1)
    return [np.ascontiguousarray(f1[60:157, 200:331]), np.ascontiguousarray(f0[40:168, 180:340])]


HEAD_BOXES = np.asarray([(10, 12, 50, 60), (30, 40, 90, 100), (5, 70, 60, 125)], np.float32)
KEYWORDS = [("4:2:2", False), ("4:4:4", True), ("4:2:0", True)]


@pytest.mark.parametrize("display", ["simple", "full"])
@pytest.mark.parametrize("sampling,optimize", KEYWORDS)
def test_annotate_jpeg_is_the_stream_of_the_annotated_frame(model, frames, display, sampling, optimize):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    frame = frames[0]
    h, w = frame.shape[:2]
    with FramePipeline(model, depth=1) as fp:
        fp.begin(frame)
        fp.heads(HEAD_BOXES)
        plain = fp.collect()
        fp.begin(frame)
        fp.heads(HEAD_BOXES)
        jf = fp.annotate_jpeg(quality=90, display=display, sampling=sampling, optimize=optimize)
        assert_same(fp.collect(), plain)                                 # collect returns what it returns without it
        fp.begin(frame)
        fp.heads(HEAD_BOXES)
        default = fp.annotate_jpeg(quality=90, display=display)
        fp.collect()
    rects, yaw, pitch, roll = plain
    assert len(rects) == 3
    fmt = "i420" if sampling == "4:2:0" else "bgr"                       # 4:2:0 keeps its I420 JFIF surface, the others a packed one
    painted = overlay.annotate_host(frame, rects, yaw, pitch, roll, format=fmt, matrix="jfif", display=display)
    assert jf.tobytes() == jpeg.encode_host(painted, 90, sampling=sampling, optimize=optimize)
    assert (jf.width, jf.height) == (w, h)
    surface = overlay.annotate_host(frame, rects, yaw, pitch, roll, format="i420", matrix="jfif", display=display)
    assert default.tobytes() == jpeg.encode_host(surface, 90)            # the default keywords: the bytes of the existing call


@pytest.mark.parametrize("sampling,optimize", KEYWORDS[:2])
def test_annotate_jpeg_in_the_pipelines_channel_order(model, frames, sampling, optimize):
    from whenet_hip.frames import FramePipeline
    frame = np.ascontiguousarray(frames[0][..., ::-1])                   # an RGB pipeline
    with FramePipeline(model, depth=1, bgr=False) as fp:
        fp.begin(frame)
        fp.heads(HEAD_BOXES)
        jf = fp.annotate_jpeg(quality=85, display="full", sampling=sampling, optimize=optimize)
        rects, yaw, pitch, roll = fp.collect()
    painted = overlay.annotate_host(frame, rects, yaw, pitch, roll, format="rgb", display="full", bgr=False)
    assert jf.tobytes() == jpeg.encode_host(painted, 85, bgr=False, sampling=sampling, optimize=optimize)


@pytest.mark.parametrize("display", ["simple", "full"])
@pytest.mark.parametrize("sampling,optimize", KEYWORDS)
def test_annotate_clip_jpeg_of_a_clip_of_two_sizes(model, kw, frames, display, sampling, optimize):
    from whenet_hip.frames import FramePipeline
    with FramePipeline(model, depth=2) as fp:
        fmt = "i420" if sampling == "4:2:0" else "bgr"
        outs = [overlay.new_output(f.shape[0], f.shape[1], fmt, "jfif") for f in frames]
        fp.begin_clip_mixed(frames)
        fp.detect_heads_clip(**kw)
        fp.annotate_clip(outs, display=display)                          # what tests/test_overlay_gpu.py holds to annotate_host
        plain = fp.collect_clip()
        fp.begin_clip_mixed(frames)
        fp.detect_heads_clip(**kw)
        clip = fp.annotate_clip_jpeg(quality=80, display=display, sampling=sampling, optimize=optimize)
        got = fp.collect_clip()
        assert got[1] == plain[1] and len(clip) == 2
    assert sum(len(f[0]) for f in plain[0]) >= 1
    for frame, out, (rects, yaw, pitch, roll), c in zip(frames, outs, plain[0], clip):
        assert c.tobytes() == jpeg.encode_host(out, 80, sampling=sampling, optimize=optimize)
        assert (c.width, c.height) == (frame.shape[1], frame.shape[0])


def test_annotate_jpeg_overflow_and_refusals(model, frames):
    from whenet_hip.frames import FramePipeline
    frame = frames[1]
    with FramePipeline(model, depth=1) as fp:
        fp.begin(frame)
        fp.heads(HEAD_BOXES[:2])
        with pytest.raises(ValueError, match="sampling"):
            fp.annotate_jpeg(sampling="4:1:1")
        out, result = np.zeros(4096, np.uint8), np.zeros(2, np.int64)
        lib = _lib.load()
        assert lib.whenet_frame_annotate_jpeg_ex(fp._h._h, fp._pending[-1][0], 0, _lib.DISPLAY_SIMPLE, 95, 3, 0, out.ctypes.data, out.size,
                                                 result.ctypes.data, result[1:].ctypes.data) == _lib.EINVAL
        full = fp.annotate_jpeg(sampling="4:4:4", optimize=True)
        fp.collect()
        data = full.tobytes()
        head = data.index(b"\xff\xda") + 14
        assert head < 629 and not out.any() and not result.any()
        for capacity in (len(data) - 1, head, 0):
            fp.begin(frame)
            fp.heads(HEAD_BOXES[:2])
            small = fp.annotate_jpeg(capacity=capacity, sampling="4:4:4", optimize=True)
            fp.collect()
            with pytest.raises(jpeg.CapacityError, match=str(len(data))) as err:
                small.tobytes()
            assert err.value.needed == len(data) and small._out.tobytes() == data[:capacity]


# ---- 3. the library's own stream back in ------------------------------------------------------------------------------------------
def test_begin_jpeg_of_the_librarys_444_optimised_stream(model, post, frames):
    from whenet_hip.frames import FramePipeline
    frame = frames[0]
    data = jpeg.encode(frame, 95, handle=post, sampling="4:4:4", optimize=True)
    assert data == jpeg.encode_host(frame, 95, sampling="4:4:4", optimize=True)
    decoded = jpeg.decode_host(data)
    assert decoded.shape == frame.shape and np.array_equal(jpeg.decode(data, handle=post), decoded)
    with FramePipeline(model, depth=1) as fp:
        fp.begin(decoded)
        fp.heads(HEAD_BOXES)
        want = fp.collect()
        status = fp.begin_jpeg(data)
        fp.heads(HEAD_BOXES)
        out = overlay.new_output(frame.shape[0], frame.shape[1], "bgr")
        fp.annotate(out)
        got = fp.collect()
        fp.begin(decoded)
        fp.heads(HEAD_BOXES)
        ref = overlay.new_output(frame.shape[0], frame.shape[1], "bgr")
        fp.annotate(ref)
        fp.collect()
    assert status.ok
    from tests.test_clip_gpu import assert_same
    assert_same(got, want)
    assert np.array_equal(out, ref)                                      # the resident frame is the frame decode_host gives
