"""Packed 4:2:2 ingest (YUYV / UYVY) on the GPU: csrc/yuv.hip's yuv_item_packed through the four kernels, the engine's host- and
device-pointer calls and FramePipeline.begin_yuv / begin_clip_yuv.  Everything is bitwise against the host function (which
tests/test_yuv_packed_cpu.py holds to the numpy statement): every load path (8-byte, dword, bytes) and every store alignment is
reached by placing the frame at every byte offset, frames packed back to back do not touch each other, and a submission begun from
a packed frame returns what the same submission begun from the converted BGR frame returns."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests import yuv_cases as YC
from tests import yuv_packed_cases as PC
from tests.test_clip_gpu import assert_same, hargs, kwargs
from tests.test_device_ingest_gpu import DEV, surface
from tests.test_yuv_gpu import seeded_model
from whenet_hip import _lib
from whenet_hip.frames import FramePipeline
from whenet_hip.yuv import YUVFrame

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "tiny"


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def model():
    m = seeded_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def kw():
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        return kwargs(json.load(f)["detect"], NAME)


def picture_rows(i, fmt, h, w):
    """The top-left h x w window of committed sample frame i as tight packed rows [h, 4 cw]: its 4:2:0 chroma repeated to every row,
    the odd rows' moved by a few levels so that the two rows of a pair differ (a 4:2:2 picture, not a 4:2:0 one in disguise)."""
    Y, U, V = YC.sample_yuv(i)
    assert Y.shape[0] >= h and Y.shape[1] >= w
    cw = (w + 1) >> 1
    Y = np.pad(Y[:h, :w], ((0, 0), (0, 2 * cw - w)), mode="edge")
    U, V = (np.repeat(p, 2, axis=0)[:h, :cw].astype(np.int32) for p in (U, V))
    U[1::2], V[1::2] = np.clip(U[1::2] + 9, 0, 255), np.clip(V[1::2] - 7, 0, 255)
    return PC.interleave(Y, U.astype(np.uint8), V.astype(np.uint8), fmt)


@pytest.fixture(scope="module")
def pictures():
    """name -> YUVFrame with content (the rows are kept alive beside it)."""
    keep, out = [], {}
    for key, (i, fmt, matrix, h, w) in dict(A=(0, PC.YUYV, "bt601", 224, 528), B=(1, PC.UYVY, "bt709", 225, 547),
                                            A2=(0, PC.UYVY, "jfif", 224, 528)).items():
        rows = picture_rows(i, fmt, h, w)
        keep.append(rows)
        out[key] = YUVFrame((rows,), fmt, matrix, h, w)
    return out, keep


@pytest.fixture(scope="module")
def single(model, kw):
    """begin(bgr); detect_heads; collect(detections=True) at depth 1 of a BGR frame, computed once per frame and shared."""
    memo = {}

    def get(bgr):
        key = (bgr.shape, bgr.tobytes())
        if key not in memo:
            with FramePipeline(model, depth=1) as fp:
                fp.begin(bgr)
                fp.detect_heads(**kw)
                memo[key] = fp.collect(detections=True)
        return memo[key]

    return get


# ---- 1. the kernel is the host function ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,matrix", PC.MATRICES)
@pytest.mark.parametrize("fname,fmt", PC.FORMATS)
def test_kernel_equals_host_function_on_every_case(post, fname, fmt, mname, matrix):
    for case in PC.CASES:
        b = PC.build(case, fmt)
        frame = PC.frame_of(b, mname)
        got, = post.op_yuv_to_bgr([frame])
        want = frame.to_bgr()
        assert got.dtype == np.uint8 and got.shape == want.shape == (b["h"], b["w"], 3)
        assert got.tobytes() == want.tobytes(), (case[0], fname, mname)


@pytest.mark.parametrize("fname,fmt", PC.FORMATS)
def test_kernel_equals_host_function_on_all_triples(post, fname, fmt):
    """BT.601 only: the per-pixel function is the one the 4:2:0 kernels run, whose sweep (tests/test_yuv_gpu.py) covers every row."""
    rows = PC.all_triples(fmt)
    frame = YUVFrame((rows,), fmt, "bt601", PC.TRIPLES_H, PC.TRIPLES_W)
    got, = post.op_yuv_to_bgr([frame])
    assert got.tobytes() == frame.to_bgr().tobytes()


# ---- 2. every source and destination alignment --------------------------------------------------------------------------------
def fronts():
    """Small frames to put in front of the frame under test in a mixed call: (frame, bytes it stages, bytes it writes)."""
    out = []
    for w in (1, 2, 3):
        b = YC.build((f"front_nv12_1x{w}", "random", 1, w, False), YC.NV12)
        out.append((YC.frame_of(b, "bt601"), w + 2 * ((w + 1) >> 1), 3 * w, b))
        p = PC.build((f"front_yuyv_1x{w}", "random", 1, w, None), PC.YUYV)
        out.append((PC.frame_of(p, "bt709"), 4 * ((w + 1) >> 1), 3 * w, p))
    return out


@pytest.mark.parametrize("fname,fmt", PC.FORMATS)
def test_every_source_offset_and_destination_offset_in_a_mixed_call(post, fname, fmt):
    """A staged source starts where the frames in front of it end: 1-, 2- and 3-pixel-wide frames in front put the frame under test
    at every source offset 0..7 (8-byte loads at 0, dwords at 4, bytes elsewhere) with every destination offset 0..3: 32 calls."""
    cat = fronts()
    b = PC.built("random_5x17", fmt)                    # 36-byte rows: the rows alternate between the two halves of 8 bytes
    frame = PC.frame_of(b, "jfif")
    want = frame.to_bgr().tobytes()
    seen = set()
    for n in range(0, 7):                               # (up to six frames in front: fewer do not reach all 32 pairs)
        for combo in itertools.combinations_with_replacement(range(len(cat)), n):
            s, d = sum(cat[i][1] for i in combo) % 8, sum(cat[i][2] for i in combo) % 4
            if (s, d) in seen:
                continue
            seen.add((s, d))
            clip = [cat[i][0] for i in combo] + [frame]
            got = post.op_yuv_to_bgr(clip)
            assert got[-1].tobytes() == want, (s, d, combo)
            for g, i in zip(got, combo):                # the frames in front keep their own bytes
                assert g.tobytes() == cat[i][0].to_bgr().tobytes(), (s, d, combo)
    assert seen == {(s, d) for s in range(8) for d in range(4)}


@pytest.mark.parametrize("fname,fmt", PC.FORMATS)
def test_every_leading_byte_count_on_the_device_path(post, fname, fmt):
    for name in ("random_5x17", "rowchroma_10x18", "random_33x7", "random_7x1"):
        b = PC.built(name, fmt)
        want = PC.frame_of(b, "bt709").to_bgr().tobytes()
        for lead in range(8):
            view, host = surface(b["rows"], b["rows"].shape[1] + (lead % 3), lead)      # (pitches 4 cw, + 1, + 2)
            frame = YUVFrame((view,), fmt, "bt709", b["h"], b["w"])
            assert frame.on_device and frame.planes[0].ptr % 8 == lead
            got, = post.op_yuv_to_bgr_device([frame])
            assert got.tobytes() == want, (name, lead)


# ---- 3. clips of the kernel alone ---------------------------------------------------------------------------------------------------
def test_sixteen_frames_of_four_formats_equal_their_single_calls(post):
    shapes = ((3, 5), (2, 2), (5, 17), (1, 1), (10, 18), (33, 7), (7, 1), (1, 7))
    keep, frames = [], []
    for i in range(16):
        h, w = shapes[i % len(shapes)]
        kind = i % 4
        if kind < 2:
            b = YC.build((f"clip{i}_{h}x{w}", "random", h, w, False), (YC.NV12, YC.I420)[kind])
            frames.append(YC.frame_of(b, YC.MATRICES[i % 3][0]))
        else:
            b = PC.build((f"clip{i}_{h}x{w}", "random", h, w, None), (PC.YUYV, PC.UYVY)[kind - 2])
            frames.append(PC.frame_of(b, PC.MATRICES[i % 3][0]))
        keep.append(b)
    assert {f.format for f in frames} == {0, 1, 3, 4}
    alone = [post.op_yuv_to_bgr([f])[0] for f in frames]
    for f, a in zip(frames, alone):
        assert a.tobytes() == f.to_bgr().tobytes()
    for order in (list(range(16)), list(range(16))[::-1]):
        got = post.op_yuv_to_bgr([frames[i] for i in order])
        for g, i in zip(got, order):
            assert g.tobytes() == alone[i].tobytes(), (order, i)


def test_uniform_batch_of_four_yuyv_frames(post):
    bs = [PC.built(n, PC.YUYV) for n in ("random_10x18", "extremes_10x18", "rowchroma_10x18", "random_10x18")]
    frames = [PC.frame_of(b, "bt601") for b in bs]
    for g, f in zip(post.op_yuv_to_bgr(frames), frames):
        assert g.tobytes() == f.to_bgr().tobytes()


def test_device_tensor_with_a_pitch_is_read_in_place_and_left_as_it_was(post):
    """(The call's landing buffer lies between two 0xA5 guard zones and the call fails if one byte of them changed.)"""
    for _, fmt in PC.FORMATS:
        b = PC.built("random_pitched_64x130", fmt)
        t = torch.from_numpy(b["flat"].copy()).to(DEV)
        frame = YUVFrame.from_buffer(t, 64, 130, fmt, pitch=544, matrix="jfif")
        assert frame.on_device and frame.pitches == (544,)
        got, = post.op_yuv_to_bgr_device([frame])
        assert got.tobytes() == PC.expected(b, 2).tobytes()
        assert t.cpu().numpy().tobytes() == b["flat"].tobytes()


# ---- 4. submissions -----------------------------------------------------------------------------------------------------------------
def test_submission_from_a_packed_frame_equals_the_bgr_path(model, kw, pictures, single):
    frames = pictures[0]
    bgr = {k: f.to_bgr() for k, f in frames.items()}
    ref = {k: single(bgr[k]) for k in frames}
    assert sum(len(ref[k][4]) for k in frames) >= 1                        # (the seeded detector does fire on these pictures)
    with FramePipeline(model, depth=1) as fp:
        for k in ("A", "B", "A2", "A"):
            fp.begin_yuv(frames[k])
            fp.detect_heads(**kw)
            got = fp.collect(detections=True)
            assert len(got) == 8
            assert_same(got, ref[k])
        # a clip of one size (two formats and matrices), and one of two sizes
        for clip in ([frames["A"], frames["A2"]], [frames["B"], frames["A"]]):
            fp.begin_clip_yuv(clip)
            fp.detect_heads_clip(**kw)
            got, (rows_used, overflow) = fp.collect_clip(detections=True)
            assert overflow == 0
            for g, f in zip(got, clip):
                assert_same(g, single(f.to_bgr()))
        # the same frame from device memory, ordered on a caller's stream
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = torch.from_numpy(np.ascontiguousarray(frames["B"].planes[0])).to(DEV, non_blocking=False)
            dev = YUVFrame.from_buffer(t, 225, 547, "uyvy", matrix="bt709")
            fp.begin_yuv(dev, stream=s.cuda_stream)
            fp.detect_heads(**kw)
            assert_same(fp.collect(detections=True), ref["B"])
            fp.begin_clip_yuv([dev, dev], stream=s.cuda_stream)
            fp.detect_heads_clip(**kw)
            got, _ = fp.collect_clip(detections=True)
            assert_same(got[1], ref["B"])
        s.synchronize()


def test_slots_reused_across_formats_give_what_fresh_slots_give(model, kw, pictures, single):
    frames = pictures[0]
    nv = YC.build(YC.CASES[YC.CASE_NAMES.index("sample0_224x528")], YC.NV12)
    nv12 = YC.frame_of(nv, "bt601")
    bgr = frames["B"].to_bgr()
    order = [("nv12", nv12), ("yuyv", frames["A"]), ("bgr", bgr), ("uyvy", frames["A2"])]
    want = {k: single(f if k == "bgr" else f.to_bgr()) for k, f in order}
    with FramePipeline(model, depth=1) as fp:
        for _ in range(_lib.MAX_INFLIGHT + 1):                             # every slot is reused every way
            for k, f in order:
                fp.begin(f) if k == "bgr" else fp.begin_yuv(f)
                fp.detect_heads(**kw)
                assert_same(fp.collect(detections=True), want[k])


def test_a_frame_one_pixel_wide_stages_more_bytes_than_it_converts_to(model):
    """4 cw = 4 source bytes per row and 3 output bytes: the one shape whose planes are larger than its BGR frame."""
    b = PC.built("random_7x1", PC.UYVY)
    frame = PC.frame_of(b, "bt601")
    with FramePipeline(model, depth=1) as fp:
        fp.begin_yuv(frame)
        got = fp.detector_input((32, 32), as_uint8=True)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
        fp.begin(frame.to_bgr())
        want = fp.detector_input((32, 32), as_uint8=True)
    assert got.tobytes() == want.tobytes()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_wrong_descriptors_are_refused_with_the_index_before_a_slot_is_taken(model, kw, pictures, single):
    frames = pictures[0]
    h = model._handle
    lib, t = _lib.load(), C.c_int(-1)
    good = frames["A"]
    b = PC.built("random_5x17", PC.YUYV)
    landing = np.empty((600, 600, 3), np.uint8)
    view, _ = surface(b["rows"], 36, 0)
    dev_good = YUVFrame((view,), PC.YUYV, "bt601", 5, 17)
    p = h.device_alloc(1000)
    try:
        for _ in range(_lib.MAX_INFLIGHT + 1):                             # (a refusal that took a slot would use them up)
            for fn, text in ((lambda d: d.pitch.__setitem__(0, 35), "pitch 35 of plane 0 is below its row of 36 bytes"),
                             (lambda d: d.plane.__setitem__(0, None), "plane 0 is NULL")):
                d = PC.frame_of(b, "bt601").descriptor()
                fn(d)
                assert lib.whenet_frame_begin_yuv(h._h, d, C.byref(t)) == _lib.EINVAL
                msg = lib.whenet_last_error(h._h).decode()
                assert "frame 0" in msg and text in msg, msg
                arr = (_lib.YuvFrameC * 2)(good.descriptor(), d)
                assert lib.whenet_clip_begin_yuv(h._h, arr, 2, C.byref(t)) == _lib.EINVAL
                msg = lib.whenet_last_error(h._h).decode()
                assert "frame 1" in msg and text in msg, msg
                out = (C.c_void_p * 2)(*[landing.ctypes.data] * 2)
                assert lib.whenet_op_yuv_to_bgr(h._h, arr, 2, out) == _lib.EINVAL
                assert "frame 1" in lib.whenet_last_error(h._h).decode()
                dd = dev_good.descriptor()
                fn(dd)
                for call in (lambda: h.frame_begin_yuv_device(dd), lambda: h.clip_begin_yuv_device([dev_good, dd]),
                             lambda: h.op_yuv_to_bgr_device([dev_good, dd])):
                    with pytest.raises(ValueError, match="frame [01].*" + text[:12]):
                        call()
            # a host pointer on the device calls
            hd = PC.frame_of(b, "bt601").descriptor()
            for call in (lambda: h.frame_begin_yuv_device(hd), lambda: h.clip_begin_yuv_device([dev_good, hd]),
                         lambda: h.op_yuv_to_bgr_device([dev_good, hd])):
                with pytest.raises(ValueError, match="frame [01]: plane 0 is not device memory"):
                    call()
            # 11 rows of 100 bytes (w = 50) = 1,100 bytes of a 1,000-byte allocation: the overrun would stay inside its page
            y = _lib.YuvFrameC()
            y.plane[0], y.pitch[0] = p, 100
            y.format, y.matrix, y.h, y.w = _lib.YUV_UYVY, _lib.YUV_BT601, 11, 50
            for call in (lambda: h.frame_begin_yuv_device(y), lambda: h.clip_begin_yuv_device([y]), lambda: h.op_yuv_to_bgr_device([y])):
                with pytest.raises(ValueError, match="frame 0: plane 0 needs 1100 bytes .* its allocation has 1000"):
                    call()
        # what fits is taken: 10 rows are the whole allocation
        host = (np.arange(1000) * 7 & 255).astype(np.uint8)
        h.h2d(p, host)
        y.h = 10
        got, = h.op_yuv_to_bgr_device([y])
        assert got.tobytes() == YUVFrame((host.reshape(10, 100),), "uyvy", "bt601", 10, 50).to_bgr().tobytes()
    finally:
        h.device_free(p)
    with FramePipeline(model, depth=1) as fp:                              # no slot leaked: every one is taken in turn
        for _ in range(_lib.MAX_INFLIGHT + 1):
            fp.begin_yuv(frames["B"])
            fp.detect_heads(**kw)
            assert_same(fp.collect(detections=True), single(frames["B"].to_bgr()))
