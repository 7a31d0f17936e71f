"""The JPEG decoder on the GPU (csrc/jpeg_dec.hip; Engine::op_jpeg_decode / jpeg_decode_device / frame_begin_jpeg of
csrc/engine_post.cpp).  There is no tolerance anywhere: the kernels return the bytes and the status of `whenet_jpeg_decode_host`,
which tests/test_jpeg_decode_cpu.py holds to the numpy statement; pitched destinations keep every byte outside their rows."""
import json
import os

import numpy as np
import pytest
import torch

from tests import jpeg_decode_cases as DC
from whenet_hip import _lib, jpeg, overlay
from whenet_hip.yuv import YUVFrame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 0xC3                 # what memory holds where nothing may be written

ALL = DC.CASE_NAMES + DC.DAMAGED_NAMES


def stream_of(name):
    return DC.DAMAGED[name]()[0] if name in DC.DAMAGED else DC.case(name)


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


def host_reference(data, bgr):
    i = _lib.jpeg_parse(data)
    frame = np.empty((i.h, i.w, 3), np.uint8)
    status = _lib.jpeg_decode_host(data, jpeg.packed_surface(frame), bgr)
    return frame, status


def guarded_rows(rows, row_bytes, extra, shift):
    """A host block filled with GAP, and in it `rows` rows of `row_bytes` bytes, row_bytes + extra apart, starting `shift` bytes in
    (so that the rows start at any address modulo 4): (the block, the view of the rows, the pitch)"""
    pitch = row_bytes + extra
    block = np.full(shift + rows * pitch + 16, GAP, np.uint8)
    view = np.lib.stride_tricks.as_strided(block[shift:], (rows, row_bytes), (pitch, 1))
    return block, view, pitch


def untouched(block, view):
    """every byte of the block outside the view's rows is still GAP"""
    mask = np.ones(block.size, bool)
    start = view.ctypes.data - block.ctypes.data
    for r in range(view.shape[0]):
        mask[start + r * view.strides[0]:start + r * view.strides[0] + view.shape[1]] = False
    return bool((block[mask] == GAP).all())


# ---- 1. the kernels alone are the host statement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_op_jpeg_decode_equals_the_host_function(post, name):
    data = stream_of(name)
    i = _lib.jpeg_parse(data)
    for k, bgr in enumerate((True, False)):
        want, want_status = host_reference(data, bgr)
        block, view, pitch = guarded_rows(i.h, 3 * i.w, 7 + k, 1 + 2 * k)
        s = _lib.SurfaceC()
        s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
        status = post.op_jpeg_decode(data, s, bgr)
        assert status.tolist() == want_status.tolist(), name
        assert np.array_equal(view.reshape(i.h, i.w, 3), want), name
        assert untouched(block, view), name
    # the tight frame (for 4:2:0 BGR: the plane kernel of the YUV ingest) through the public function
    assert np.array_equal(jpeg.decode(data, handle=post, strict=False), host_reference(data, True)[0])
    if name in DC.DAMAGED:
        with pytest.raises(jpeg.DecodeError) as err:
            jpeg.decode(data, handle=post)
        assert err.value.interval == DC.DAMAGED[name]()[1]


FOUR_TWO_ZERO = [n for n in ALL if n.startswith(("pil_420", "own_", "sample_")) or n in DC.DAMAGED and n not in ("truncated_no_dri",)]


@pytest.mark.parametrize("name", FOUR_TWO_ZERO)
def test_op_jpeg_decode_into_i420_and_nv12_surfaces(post, name):
    data = stream_of(name)
    i = _lib.jpeg_parse(data)
    assert (i.hs, i.vs) == (2, 2)
    h, w, ch, cw = i.h, i.w, (i.h + 1) // 2, (i.w + 1) // 2
    planes, want_status = jpeg.decode_planes_host(data)
    for fmt in ("i420", "nv12"):
        geo = [(h, w, 3, 1), (ch, cw, 5, 2), (ch, cw, 2, 3)] if fmt == "i420" else [(h, w, 5, 3), (ch, 2 * cw, 3, 1)]
        blocks = [guarded_rows(*g) for g in geo]
        s = _lib.SurfaceC()
        for p, (_, view, pitch) in enumerate(blocks):
            s.plane[p], s.pitch[p] = view.ctypes.data, pitch
        s.format, s.matrix, s.on_device = (_lib.YUV_I420 if fmt == "i420" else _lib.YUV_NV12), _lib.YUV_JFIF, 0
        status = post.op_jpeg_decode(data, s, True)
        assert status.tolist() == want_status.tolist()
        assert np.array_equal(blocks[0][1], planes[0])
        if fmt == "i420":
            assert np.array_equal(blocks[1][1], planes[1]) and np.array_equal(blocks[2][1], planes[2])
        else:
            assert np.array_equal(blocks[1][1][:, 0::2], planes[1]) and np.array_equal(blocks[1][1][:, 1::2], planes[2])
        for block, view, _ in blocks:
            assert untouched(block, view), (name, fmt)


def test_op_jpeg_decode_refusals_leave_the_handle_usable(post):
    frame = np.full((64, 64, 3), GAP, np.uint8)
    for name, make in DC.REFUSED.items():
        with pytest.raises(ValueError):
            post.op_jpeg_decode(make(), jpeg.packed_surface(frame), True)
    data = DC.case("pil_444_17x17")
    small = np.zeros((17, 17, 3), np.uint8)
    s = jpeg.packed_surface(small)
    s.pitch[0] = 50
    with pytest.raises(ValueError, match="pitch"):
        post.op_jpeg_decode(data, s, True)
    y, c = np.zeros((17, 17), np.uint8), np.zeros((9, 9), np.uint8)
    with pytest.raises(ValueError, match="4:2:0"):
        post.op_jpeg_decode(data, overlay.surface_of(YUVFrame.i420(y, c, c, "jfif"), 17, 17)[0], True)
    t = torch.zeros((17, 17, 3), dtype=torch.uint8, device=DEV)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = t.data_ptr(), 51, _lib.SURF_PACKED, 0       # device memory marked as host
    with pytest.raises(ValueError):
        post.op_jpeg_decode(data, s, True)
    assert (frame == GAP).all() and not small.any()
    assert np.array_equal(jpeg.decode(data, handle=post), host_reference(data, True)[0])


# ---- 2. entropy data and destination in device memory ----------------------------------------------------------------------------
def device_packed(h, w, extra, shift):
    buf = torch.full((shift + h * (3 * w + extra) + 16,), GAP, dtype=torch.uint8, device=DEV)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = buf.data_ptr() + shift, 3 * w + extra, _lib.SURF_PACKED, 1
    return buf, s


def read_packed(buf, h, w, extra, shift):
    """(the frame, whether every byte outside its rows is still GAP)"""
    host = buf.cpu().numpy()
    pitch = 3 * w + extra
    view = np.lib.stride_tricks.as_strided(host[shift:], (h, 3 * w), (pitch, 1))
    return view.reshape(h, w, 3).copy(), untouched(host, view)


@pytest.mark.parametrize("size", [(17, 17), (48, 64), (70, 50), (16, 1040)])
def test_the_encoders_stream_round_trips_in_device_memory(post, size):
    """whenet_jpeg_encode_device leaves the stream in HBM; its header is whenet_jpeg_header's, parsed on the host; the entropy bytes
    are decoded where they lie.  Nothing of the stream is read by the host between the two calls (the buffer is zero-filled: what
    lies behind EOI holds no marker)."""
    h, w = size
    frame = np.ascontiguousarray(DC.picture(h, w, seed=9)[..., ::-1])
    full = jpeg.encode_host(frame, 90)
    want, _ = host_reference(full, True)
    src = torch.from_numpy(frame).to(DEV)
    s_src = _lib.SurfaceC()
    s_src.plane[0], s_src.pitch[0], s_src.format, s_src.on_device = src.data_ptr(), 3 * w, _lib.SURF_PACKED, 1
    cap = jpeg.bound(h, w)
    stream = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    dsize = torch.zeros(1, dtype=torch.int64, device=DEV)
    info = _lib.jpeg_parse(jpeg.header(h, w, 90))
    assert info.data_offset == jpeg.HEADER_BYTES and info.intervals == (h + 15) // 16
    status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    buf, s_dst = device_packed(h, w, 5, 3)
    post.jpeg_encode_device(s_src, h, w, True, 90, stream.data_ptr(), cap, dsize.data_ptr())
    post.jpeg_decode_device(info, stream.data_ptr() + jpeg.HEADER_BYTES, cap - jpeg.HEADER_BYTES, s_dst, True, status.data_ptr())
    torch.cuda.synchronize()
    assert stream[:len(full)].cpu().numpy().tobytes() == full and int(dsize.item()) == len(full)
    got, clean = read_packed(buf, h, w, 5, 3)
    assert status.cpu().tolist() == [_lib.OK, -1] and np.array_equal(got, want) and clean
    # ... and with the exact length, RGB, into an I420 surface
    buf, s_dst = device_packed(h, w, 0, 0)
    post.jpeg_decode_device(info, stream.data_ptr() + jpeg.HEADER_BYTES, len(full) - jpeg.HEADER_BYTES, s_dst, False, status.data_ptr())
    planes = [torch.full((r, c + 3), GAP, dtype=torch.uint8, device=DEV) for r, c in ((h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 1) // 2, (w + 1) // 2))]
    s_yuv = _lib.SurfaceC()
    for p, t in enumerate(planes):
        s_yuv.plane[p], s_yuv.pitch[p] = t.data_ptr(), t.shape[1]
    s_yuv.format, s_yuv.matrix, s_yuv.on_device = _lib.YUV_I420, _lib.YUV_JFIF, 1
    post.jpeg_decode_device(info, stream.data_ptr() + jpeg.HEADER_BYTES, len(full) - jpeg.HEADER_BYTES, s_yuv, True, status.data_ptr())
    torch.cuda.synchronize()
    got, clean = read_packed(buf, h, w, 0, 0)
    assert np.array_equal(got, host_reference(full, False)[0]) and clean
    for t, ref in zip(planes, jpeg.decode_planes_host(full)[0]):
        host = t.cpu().numpy()
        assert np.array_equal(host[:, :-3], ref) and (host[:, -3:] == GAP).all()


@pytest.mark.parametrize("name", ["pil_422_rst_rows", "pil_444_rst_blocks3", "pil_grey_50x70", "pil_420_16x4800_rst_rows", "noncode", "removed_rst"])
def test_jpeg_decode_device_on_other_streams(post, name):
    data = stream_of(name)
    info = _lib.jpeg_parse(data)
    ent = torch.from_numpy(np.frombuffer(data, np.uint8)[info.data_offset:].copy()).to(DEV)
    status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    buf, s_dst = device_packed(info.h, info.w, 2, 1)
    post.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s_dst, True, status.data_ptr())
    torch.cuda.synchronize()
    want, want_status = host_reference(data, True)
    got, clean = read_packed(buf, info.h, info.w, 2, 1)
    assert status.cpu().tolist() == want_status.tolist() and np.array_equal(got, want) and clean


def test_jpeg_decode_device_is_ordered_on_the_callers_stream(post):
    data = DC.case("pil_420_rst_rows")
    info = _lib.jpeg_parse(data)
    host_ent = torch.from_numpy(np.frombuffer(data, np.uint8)[info.data_offset:].copy()).pin_memory()
    ent = torch.zeros(host_ent.numel(), dtype=torch.uint8, device=DEV)
    status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    buf, s_dst = device_packed(info.h, info.w, 0, 0)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ent.copy_(host_ent, non_blocking=True)                                          # written before ...
        post.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s_dst, True, status.data_ptr(), stream=side.cuda_stream)
        seen, st = buf.clone(), status.clone()                                          # ... and read after
    side.synchronize()
    want, _ = host_reference(data, True)
    assert st.cpu().tolist() == [_lib.OK, -1]
    assert np.array_equal(read_packed(seen, info.h, info.w, 0, 0)[0], want)


def test_jpeg_decode_device_refuses_host_pointers_before_anything_is_enqueued(post):
    data = DC.case("pil_420_17x17")
    info = _lib.jpeg_parse(data)
    host_ent = np.frombuffer(data, np.uint8)[info.data_offset:].copy()
    ent = torch.from_numpy(host_ent).to(DEV)
    status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    host_status = np.full(2, 77, np.int32)
    buf, s_dst = device_packed(17, 17, 0, 0)
    host_frame = np.full((17, 17, 3), GAP, np.uint8)
    s_host = jpeg.packed_surface(host_frame)
    s_host.on_device = 1                                                               # host memory marked as device memory
    with pytest.raises(ValueError):
        post.jpeg_decode_device(info, host_ent.ctypes.data, host_ent.size, s_dst, True, status.data_ptr())
    with pytest.raises(ValueError):
        post.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s_host, True, status.data_ptr())
    with pytest.raises(ValueError):
        post.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s_dst, True, host_status.ctypes.data)
    with pytest.raises(ValueError):                                                    # more bytes than the allocation holds
        post.jpeg_decode_device(info, ent.data_ptr(), (ent.numel() + 1) << 20, s_dst, True, status.data_ptr())
    with pytest.raises(ValueError):
        post.jpeg_decode_device(info, ent.data_ptr(), 0, s_dst, True, status.data_ptr())
    bad = _lib.JpegInfoC.from_buffer_copy(info)
    bad.hs = 3
    with pytest.raises(ValueError, match="sampling"):
        post.jpeg_decode_device(bad, ent.data_ptr(), ent.numel(), s_dst, True, status.data_ptr())
    bad = _lib.JpegInfoC.from_buffer_copy(info)
    bad.intervals = 2
    with pytest.raises(ValueError, match="interval"):
        post.jpeg_decode_device(bad, ent.data_ptr(), ent.numel(), s_dst, True, status.data_ptr())
    s_dst.on_device = 0
    with pytest.raises(ValueError):
        post.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s_dst, True, status.data_ptr())
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GAP).all() and status.cpu().tolist() == [77, 77] and (host_frame == GAP).all() and (host_status == 77).all()
    s_dst.on_device = 1
    post.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s_dst, True, status.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(read_packed(buf, 17, 17, 0, 0)[0], host_reference(data, True)[0]) and status.cpu().tolist() == [_lib.OK, -1]


# ---- 3. the pipeline: begin_jpeg -------------------------------------------------------------------------------------------------
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
        return kwargs(json.load(f)["detect"], "tiny", score=0.02)       # a low threshold: the seeded detector then fires on small frames


def seeded_stream():
    return DC.own_stream(48, 64, 95, seed=11)                          # a seeded 64 x 48 frame: three restart intervals


PIPELINE_STREAMS = {"sample_001": lambda: DC.case("sample_001"), "sample_012": lambda: DC.case("sample_012"), "seeded_64x48": seeded_stream,
                    "pil_444_q50": lambda: DC.case("pil_444_q50"), "pil_grey_50x70": lambda: DC.case("pil_grey_50x70")}


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("name", list(PIPELINE_STREAMS))
def test_begin_jpeg_is_begin_of_the_decoded_frame(model, kw, name, bgr):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    data = PIPELINE_STREAMS[name]()
    frame = jpeg.decode_host(data, bgr=bgr)
    with FramePipeline(model, depth=1, bgr=bgr) as fp:
        fp.begin(frame)
        want_input = fp.detector_input(kw["size"], as_uint8=True)
        fp.detect_heads(**kw)
        want = fp.collect(detections=True)
        st = fp.begin_jpeg(data)
        with pytest.raises(ValueError, match="not collected"):
            st.ok
        got_input = fp.detector_input(kw["size"], as_uint8=True)          # the letterbox reads the decoded frame
        fp.detect_heads(**kw)
        got = fp.collect(detections=True)
    assert np.array_equal(got_input, want_input)
    assert_same(got, want)
    assert st.ok and st.interval == -1


def test_begin_jpeg_reuses_slots_both_ways_and_annotates_like_begin(model, kw):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    streams = [DC.case("sample_001"), seeded_stream(), DC.case("pil_422_rst_rows")]
    frames = [jpeg.decode_host(d) for d in streams]
    boxes = np.asarray([(8, 8, 30, 30), (12, 14, 36, 40)], np.float32)      # inside the smallest frame (70 x 50)
    with FramePipeline(model, depth=1) as fp:            # depth 1: ONE slot, taken by a JPEG, a BGR frame, a JPEG, ... in turn
        want = []
        for f in frames:
            fp.begin(f)
            fp.heads(boxes)
            out = np.zeros_like(f)
            fp.annotate(out, display="full")
            want.append((fp.collect(), out))
        for rounds in range(2):
            for d, f, (res, painted) in zip(streams, frames, want):
                st = fp.begin_jpeg(d)
                fp.heads(boxes)
                out = np.zeros_like(f)
                fp.annotate(out, display="full")
                assert_same(fp.collect(), res)
                assert np.array_equal(out, painted) and st.ok
                fp.begin(f[::-1].copy())                  # a BGR frame of the same size through the same slot
                fp.heads(boxes)
                fp.collect()
        # the annotated frame as a JPEG stream, after begin_jpeg as after begin
        fp.begin(frames[1])
        fp.heads(boxes)
        a = fp.annotate_jpeg(quality=90)
        fp.collect()
        fp.begin_jpeg(streams[1])
        fp.heads(boxes)
        b = fp.annotate_jpeg(quality=90)
        fp.collect()
        assert a.tobytes() == b.tobytes()
    with FramePipeline(model, depth=2) as fp:            # two in flight: a JPEG and a BGR frame side by side
        fp.begin_jpeg(streams[0])
        fp.detect_heads(**kw)
        fp.begin(frames[1])
        fp.detect_heads(**kw)
        first, second = fp.collect(), fp.collect()
        fp.begin(frames[0])
        fp.detect_heads(**kw)
        fp.begin_jpeg(streams[1])
        fp.detect_heads(**kw)
        assert_same(fp.collect(), first)
        assert_same(fp.collect(), second)


def test_begin_jpeg_with_a_damaged_or_refused_stream(model, kw):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    data, interval = DC.DAMAGED["stray_marker"]()
    frame = jpeg.decode_host(data, strict=False)
    with FramePipeline(model, depth=1) as fp:
        for name, make in DC.REFUSED.items():
            with pytest.raises(ValueError):
                fp.begin_jpeg(make())                     # refused before a slot is taken: nothing is in flight
        assert fp.in_flight == 0 and fp._begun is None
        fp.begin(frame)
        fp.detect_heads(**kw)
        want = fp.collect(detections=True)
        st = fp.begin_jpeg(data)
        fp.detect_heads(**kw)
        assert_same(fp.collect(detections=True), want)   # the defined frame of the damaged stream
        assert not st.ok and st.interval == interval
        good = DC.case("pil_420_rst_rows")               # the handle stays usable
        st = fp.begin_jpeg(good)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()                                      # a ticket collected without a forward: the status is there all the same
        assert st.ok and st.interval == -1
