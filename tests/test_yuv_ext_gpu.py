"""The extended YUV ingest on the GPU (csrc/yuvx.hip; Engine::op_yuvx_to_bgr / begin_yuvx of csrc/engine_post.cpp;
FramePipeline.begin_yuv / begin_clip_yuv with 16-bit, 4:4:4 and BT.2020 frames).  Everything is bitwise: the kernels return the
bytes of the numpy statement (tests/yuv_ext_cases.py) and of the host function, from staged planes and from device planes at every
alignment the load ladder distinguishes; frames packed back to back do not touch each other (the landing buffer of the kernel-alone
calls lies between guard bytes that the library checks); a submission begun from such a frame returns what the same submission
begun from the converted BGR frame returns."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import yuv_cases as YC
from tests import yuv_ext_cases as XC
from tests import yuv_packed_cases as PC
from tests.test_clip_gpu import assert_same, kwargs
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


def device_frame(b, matrix, base=0):
    """The built case `b` with its planes uploaded WITH their pitches and gap bytes, every plane `base` bytes into its allocation."""
    views = [surface(v, p, base)[0] for v, p in zip(b["views"], b["pitches"])]
    f = YUVFrame(views, b["layout"], matrix, b["h"], b["w"], container=b["bits"], shift=b["shift"])
    assert f.on_device and all(pl.ptr % 16 == base for pl in f.planes)
    return f


# ---- 1. the kernels are the host function and the numpy statement -----------------------------------------------------------------
@pytest.mark.parametrize("fmt", XC.FORMATS, ids=XC.FORMAT_NAMES)
def test_kernel_equals_host_function_and_numpy_on_every_case(post, fmt):
    for case in XC.CASES:
        b = XC.build(case, fmt)
        for mname, matrix in XC.MATRICES:
            frame = XC.frame_of(b, mname)
            got, = post.op_yuvx_to_bgr([frame])
            assert got.dtype == np.uint8 and got.shape == (b["h"], b["w"], 3)
            assert got.tobytes() == XC.expected_bytes(case[0], fmt[0], matrix) == frame.to_bgr().tobytes(), (case[0], fmt[0], mname)


@pytest.mark.parametrize("fmt", XC.FORMATS, ids=XC.FORMAT_NAMES)
def test_device_planes_tight_and_pitched_equal_numpy(post, fmt):
    for i, case in enumerate(XC.CASES):
        b = XC.build(case, fmt)
        mname, matrix = XC.MATRICES[i % 4]
        got, = post.op_yuvx_to_bgr_device([device_frame(b, mname)])
        assert got.tobytes() == XC.expected_bytes(case[0], fmt[0], matrix), (case[0], fmt[0], mname)
    # one allocation as a decoder hands it out, tight and at a pitch
    b = XC.built("random_10x18", fmt[0])
    tight = torch.from_numpy(XC.tight_buffer(b)).to(DEV)
    frame = YUVFrame.from_buffer(tight, 10, 18, fmt[0], matrix="bt2020")
    assert frame.on_device and post.op_yuvx_to_bgr_device([frame])[0].tobytes() == XC.expected_bytes("random_10x18", fmt[0], XC.BT2020)


@pytest.mark.parametrize("fmt", XC.FORMATS, ids=XC.FORMAT_NAMES)
def test_every_plane_offset_the_load_ladder_distinguishes(post, fmt):
    """16-bit planes at every even byte offset 0..14 of an allocation (8-byte loads, dwords, words); 8-bit 4:4:4 planes at every
    offset 0..7 (dwords, bytes).  The pitched case moves the rows through the residues as well."""
    offsets = range(0, 16, 2) if fmt[2] == 16 else range(8)
    for name in ("random_5x17", "random_10x18", "extremes_pitched_64x130", "random_4x3"):
        b = XC.built(name, fmt[0])
        want = XC.expected_bytes(name, fmt[0], XC.BT709)
        for base in offsets:
            got, = post.op_yuvx_to_bgr_device([device_frame(b, "bt709", base)])
            assert got.tobytes() == want, (name, fmt[0], base)


# ---- 2. / 3. frames back to back ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", XC.FORMATS, ids=XC.FORMAT_NAMES)
def test_frames_behind_the_odd_frame_of_a_mixed_clip(post, fmt):
    """The 97 x 131 frame (8-bit 4:4:4: 38121 staged bytes, 38121 output bytes, both odd) in front, then every small case of the
    format: each starts where the frames in front of it end -- destination offsets 0..3 mod 4, a 16-bit frame's planes at the next
    even staging offset -- on the staged form and on the device form."""
    front = XC.frame_of(XC.built("random_97x131", "i444"), "jfif")
    names = [c[0] for c in XC.CASES if c[2] * c[3] <= 180][:14]
    builts = [XC.built(n, fmt[0]) for n in names]
    want = [XC.expected_bytes("random_97x131", "i444", XC.JFIF)] + [XC.expected_bytes(n, fmt[0], XC.BT2020) for n in names]
    dst = np.cumsum([97 * 131 * 3] + [b["h"] * b["w"] * 3 for b in builts])[:-1]
    assert {int(o) % 4 for o in dst} == {0, 1, 2, 3}
    for order in (slice(None), slice(None, None, -1)):
        bs, ws = builts[order], want[1:][order]
        got = post.op_yuvx_to_bgr([front] + [XC.frame_of(b, "bt2020") for b in bs])
        assert [g.tobytes() for g in got] == [want[0]] + ws
    front_dev = device_frame(XC.built("random_97x131", "i444"), "jfif")
    got = post.op_yuvx_to_bgr_device([front_dev] + [device_frame(b, "bt2020") for b in builts])
    assert [g.tobytes() for g in got] == want
    # position 1 alone: the case the issue names
    got = post.op_yuvx_to_bgr([front, XC.frame_of(XC.built("random_5x17", fmt[0]), "bt601")])
    assert got[1].tobytes() == XC.expected_bytes("random_5x17", fmt[0], XC.BT601) and got[0].tobytes() == want[0]


def test_clips_that_mix_old_and_new_formats(post):
    keep = [YC.build(YC.CASES[YC.CASE_NAMES.index("random_5x17")], YC.NV12), PC.built("random_5x17", PC.YUYV),
            XC.built("random_5x17", "p016"), XC.built("random_10x18", "yuv420p10le"), XC.built("random_3x4", "i444"),
            YC.build(YC.CASES[YC.CASE_NAMES.index("random_33x7")], YC.I420), XC.built("extremes_5x17", "yuv444p16"),
            PC.built("random_7x1", PC.UYVY)]
    frames = [YC.frame_of(keep[0], "bt601"), PC.frame_of(keep[1], "bt709"), XC.frame_of(keep[2], "bt2020"), XC.frame_of(keep[3], "bt2020"),
              XC.frame_of(keep[4], "jfif"), YC.frame_of(keep[5], "jfif"), XC.frame_of(keep[6], "bt709"), PC.frame_of(keep[7], "bt601")]
    alone = [post.op_yuvx_to_bgr([f])[0].tobytes() for f in frames]
    assert alone == [f.to_bgr().tobytes() for f in frames]
    for i in (0, 1, 5, 7):                              # the old formats: the old call's bytes
        assert alone[i] == post.op_yuv_to_bgr([frames[i]])[0].tobytes()
    for order in (list(range(8)), list(range(8))[::-1], [2, 2, 2], [4, 3, 2, 1, 0] * 3 + [6]):
        got = post.op_yuvx_to_bgr([frames[i] for i in order])
        assert [g.tobytes() for g in got] == [alone[i] for i in order], order
    with pytest.raises(ValueError, match="extended calls"):
        post.op_yuv_to_bgr([frames[0], frames[2]])


# ---- 4. the pipeline ------------------------------------------------------------------------------------------------------------------
def pictures():
    """Sample frame 1 (225 x 547) as a P016 frame (10 significant bits and a low-bit pattern) and as an 8-bit I444 frame."""
    h, w = XC.BIG
    Y, U, V = YC.sample_yuv(1)
    Y, U, V = (np.ascontiguousarray(p) for p in (Y[:h, :w], U[:(h + 1) // 2, :(w + 1) // 2], V[:(h + 1) // 2, :(w + 1) // 2]))
    assert Y.shape == (h, w) and U.shape == (113, 274)
    yy, xx = np.mgrid[0:h, 0:w]
    y16 = ((Y.astype(np.uint16) << 8) | ((yy * 37 + xx * 11) & 0xC0).astype(np.uint16)).astype("<u2")
    uv16 = (np.stack([U, V], axis=2).astype(np.uint16) << 8 | 0x40).astype("<u2").reshape(U.shape[0], -1)
    full = [np.ascontiguousarray(np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w]) for p in (U, V)]
    full[0][1::2] = np.clip(full[0][1::2].astype(np.int32) + 9, 0, 255).astype(np.uint8)      # (a 4:4:4 picture, not a 4:2:0 one in disguise)
    return dict(p016=YUVFrame.p016(y16, uv16, matrix="bt2020"), i444=YUVFrame.i444(Y, full[0], full[1], matrix="bt709"))


def run(fp, kw, begin):
    begin()
    canvas = fp.detector_input((416, 416), as_uint8=True)
    fp.detect_heads(**kw)
    return canvas, fp.collect(detections=True)


@pytest.mark.parametrize("key", ["p016", "i444"])
def test_a_submission_begun_from_the_frame_equals_one_begun_from_its_bgr_frame(model, kw, key):
    frame = pictures()[key]
    assert frame.needs_ext and (frame.h, frame.w) == XC.BIG
    bgr = frame.to_bgr()
    with FramePipeline(model, depth=1) as fp:
        want_canvas, want = run(fp, kw, lambda: fp.begin(bgr))
        canvas, got = run(fp, kw, lambda: fp.begin_yuv(frame))
        assert canvas.tobytes() == want_canvas.tobytes()
        assert_same(got, want)
        # the planes in device memory, on the caller's stream, their producer (the upload) enqueued on that stream
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            planes = [torch.from_numpy(np.ascontiguousarray(p)).to(DEV, non_blocking=True) for p in frame.planes]
            dev = YUVFrame(planes, frame.format, frame.matrix, frame.h, frame.w, container=frame.container, shift=frame.shift)
            assert dev.on_device
            canvas, got = run(fp, kw, lambda: fp.begin_yuv(dev, stream=s.cuda_stream))
            assert canvas.tobytes() == want_canvas.tobytes()
            assert_same(got, want)
            fp.begin_clip_yuv([dev, dev], stream=s.cuda_stream)
            fp.detect_heads_clip(**kw)
            clip, _ = fp.collect_clip(detections=True)
            assert_same(clip[1], want)
        s.synchronize()
        fp.begin_clip_yuv([frame, frame])                                   # a clip from host planes
        fp.detect_heads_clip(**kw)
        clip, _ = fp.collect_clip(detections=True)
        assert_same(clip[0], want), assert_same(clip[1], want)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_descriptors_leave_the_handle_usable_and_leak_no_slot(model, kw):
    h = model._handle
    lib, t = _lib.load(), C.c_int(-1)
    b = XC.built("random_10x18", "p016")
    good = XC.frame_of(b, "bt2020")
    dev_good = device_frame(b, "bt2020")
    landing = np.empty((64, 64, 3), np.uint8)
    bad = [(lambda d: d.plane.__setitem__(1, None), "plane 1 is NULL"), (lambda d: d.pitch.__setitem__(0, 34), "pitch 34 of plane 0"),
           (lambda d: setattr(d, "layout", 7), "unknown layout 7"), (lambda d: setattr(d, "container", 12), "unknown container 12"),
           (lambda d: setattr(d, "matrix", 4), "unknown matrix 4"), (lambda d: setattr(d, "shift", 9), "shift 9"),
           (lambda d: setattr(d, "w", 8193), "sides must be 1..8192"), (lambda d: d.pitch.__setitem__(1, 37), "is odd"),
           (lambda d: d.plane.__setitem__(0, d.plane[0] + 1), "odd address")]
    for _ in range(2):                                                     # (a refusal that took a slot would use them up)
        for fn, text in bad:
            d = good.descriptor()
            fn(d)
            assert lib.whenet_frame_begin_yuvx(h._h, d, C.byref(t)) == _lib.EINVAL
            msg = lib.whenet_last_error(h._h).decode()
            assert "frame 0" in msg and text in msg, msg
            arr = (_lib.YuvxFrameC * 2)(good.descriptor(), d)
            assert lib.whenet_clip_begin_yuvx(h._h, arr, 2, C.byref(t)) == _lib.EINVAL
            msg = lib.whenet_last_error(h._h).decode()
            assert "frame 1" in msg and text in msg, msg
            out = (C.c_void_p * 2)(*[landing.ctypes.data] * 2)
            assert lib.whenet_op_yuvx_to_bgr(h._h, arr, 2, out) == _lib.EINVAL
            assert "frame 1" in lib.whenet_last_error(h._h).decode()
            dd = dev_good.descriptor()
            fn(dd)
            for call in (lambda: h.frame_begin_yuvx_device(dd), lambda: h.clip_begin_yuvx_device([dev_good, dd]),
                         lambda: h.op_yuvx_to_bgr_device([dev_good, dd])):
                with pytest.raises(ValueError, match="frame [01]"):
                    call()
        hd = good.descriptor()                                             # a host pointer on the device calls
        for call in (lambda: h.frame_begin_yuvx_device(hd), lambda: h.clip_begin_yuvx_device([dev_good, hd])):
            with pytest.raises(ValueError, match="not device memory"):
                call()
    for n in (0, 17):
        arr = (_lib.YuvxFrameC * 17)(*[good.descriptor()] * 17)
        assert lib.whenet_clip_begin_yuvx(h._h, arr, n, C.byref(t)) == _lib.EINVAL
    assert lib.whenet_frame_begin_yuvx(h._h, None, C.byref(t)) == _lib.EINVAL
    # every slot is still there, and the handle converts
    tickets = [h.frame_begin_yuvx(good) for _ in range(_lib.MAX_INFLIGHT)]
    for tk in tickets:
        h.frame_heads(tk, np.zeros((0, 4), np.int32))
        h.collect(tk, 0)
    assert h.op_yuvx_to_bgr([good])[0].tobytes() == XC.expected_bytes("random_10x18", "p016", XC.BT2020)
    with FramePipeline(model, depth=1) as fp:
        fp.begin_yuv(good)
        got = fp.detector_input((32, 32), as_uint8=True)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
        fp.begin(good.to_bgr())
        want = fp.detector_input((32, 32), as_uint8=True)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
    assert got.tobytes() == want.tobytes()
