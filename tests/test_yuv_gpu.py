"""YUV 4:2:0 ingest on the GPU (csrc/yuv.hip; Engine::op_yuv_to_bgr / frame_begin_yuv / clip_begin_yuv of csrc/engine_post.cpp;
FramePipeline.begin_yuv / begin_clip_yuv).  Everything is bitwise, there is no tolerance: the kernel returns the bytes of the host
function (which tests/test_yuv_cpu.py holds to the numpy statement), frames packed back to back at unaligned offsets do not touch
each other, and a submission begun from planes returns what the same submission begun from the converted BGR frame returns."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import detector_cases as DC
from tests import yuv_cases as YC
from tests.test_clip_gpu import assert_same, hargs, kwargs
from whenet_hip import _lib, detector_weights as DW
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


def seeded_model():
    """A seeded f16 WHENet with the seeded tiny detector on its handle (as tests/test_mixed_clip_gpu.py builds it)."""
    import whenet
    m = whenet.WHENet(dtype="f16")
    m._handle.detector_load(DW.pack(DW.synthetic(1, DC.SEEDS[NAME])))
    return m


@pytest.fixture(scope="module")
def model():
    m = seeded_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def kw():
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        return kwargs(json.load(f)["detect"], NAME)


def built(name, fmt):
    return YC.build(YC.CASES[YC.CASE_NAMES.index(name)], fmt)


@pytest.fixture(scope="module")
def pictures():
    """Frames with content, cut from the committed sample frames: name -> YUVFrame (the built case is kept alive beside it)."""
    spec = dict(A=("sample0_224x528", YC.NV12, "bt601"), B=("sample1_225x547", YC.I420, "bt709"),
                A2=("sample0_224x528", YC.I420, "jfif"), W=("sample1_window_97x131", YC.NV12, "jfif"))
    out = {}
    for key, (name, fmt, matrix) in spec.items():
        b = built(name, fmt)
        out[key] = (YC.frame_of(b, matrix), b)
    return {k: v[0] for k, v in out.items()}, out


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
@pytest.mark.parametrize("mname,matrix", YC.MATRICES)
@pytest.mark.parametrize("fname,fmt", YC.FORMATS)
def test_kernel_equals_host_function_on_every_case(post, fname, fmt, mname, matrix):
    for case in YC.CASES:
        b = YC.build(case, fmt)
        frame = YC.frame_of(b, mname)
        got, = post.op_yuv_to_bgr([frame])
        want = frame.to_bgr()
        assert got.dtype == np.uint8 and got.shape == want.shape == (b["h"], b["w"], 3)
        assert got.tobytes() == want.tobytes(), (case[0], fname, mname)


@pytest.fixture(scope="module")
def triples():
    return YC.all_triples()


@pytest.mark.parametrize("mname,matrix", YC.MATRICES)
def test_kernel_equals_host_function_on_all_triples(post, triples, mname, matrix):
    yp, uv = triples
    frame = YUVFrame.nv12(yp, uv, matrix=mname)
    got, = post.op_yuv_to_bgr([frame])
    assert got.tobytes() == frame.to_bgr().tobytes()


# ---- 2. frames back to back at unaligned offsets -------------------------------------------------------------------------------
def test_packed_frames_do_not_touch_each_other(post):
    shapes = ((3, 5), (2, 2), (5, 17), (1, 1), (10, 18), (33, 7))
    offsets = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in shapes])])
    assert offsets[1:4].tolist() == [45, 57, 312] and offsets[1] % 4 and offsets[2] % 4 and offsets[3] % 16 and offsets[4] % 4
    keep, frames = [], []
    for i, (h, w) in enumerate(shapes):
        b = built(f"random_{h}x{w}", YC.FORMATS[i % 2][1])
        keep.append(b)
        frames.append(YC.frame_of(b, YC.MATRICES[i % 3][0]))
    alone = [post.op_yuv_to_bgr([f])[0] for f in frames]
    for f, a in zip(frames, alone):
        assert a.tobytes() == f.to_bgr().tobytes()
    for order in (list(range(len(frames))), list(range(len(frames)))[::-1]):
        got = post.op_yuv_to_bgr([frames[i] for i in order])
        for g, i in zip(got, order):
            assert g.tobytes() == alone[i].tobytes(), (order, i)
    # frames of ONE size, format and matrix (the launch with the frame as a grid dimension), 255 bytes apart
    bs = [built(n, YC.I420) for n in ("random_5x17", "extremes_5x17", "random_5x17")]
    same = [YC.frame_of(b, "bt709") for b in bs]
    got = post.op_yuv_to_bgr(same)
    for g, f in zip(got, same):
        assert g.tobytes() == f.to_bgr().tobytes()
    # sixteen frames, and the argument checks
    many = [frames[i % len(frames)] for i in range(16)]
    for g, f in zip(post.op_yuv_to_bgr(many), many):
        assert g.tobytes() == f.to_bgr().tobytes()
    for bad in ([], many + [frames[0]]):
        with pytest.raises(ValueError, match="1..16"):
            post.op_yuv_to_bgr(bad)
    assert post.op_yuv_to_bgr([frames[2]])[0].tobytes() == alone[2].tobytes()            # the handle stays usable


# ---- 3. the resident frame is the converted frame ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["A", "B"])
def test_detector_input_of_a_yuv_frame_equals_that_of_its_bgr_frame(model, pictures, key):
    frame = pictures[0][key]
    bgr = frame.to_bgr()
    with FramePipeline(model, depth=1) as fp:
        fp.begin_yuv(frame)
        got = fp.detector_input((64, 96), as_uint8=True)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
        fp.begin(bgr)
        want = fp.detector_input((64, 96), as_uint8=True)
    assert got.shape == (64, 96, 3) and got.tobytes() == want.tobytes()
    assert len(np.unique(got)) > 16                                        # a picture, not a flat canvas


# ---- 4. one submission per frame: begin_yuv; detect_heads; collect --------------------------------------------------------------
def test_submission_from_planes_equals_the_bgr_path(model, kw, pictures, single):
    frames = pictures[0]
    bgr = {k: f.to_bgr() for k, f in frames.items()}
    ref = {k: single(bgr[k]) for k in frames}
    for k in ("A", "B"):
        print(f"{k}: {len(ref[k][4])} detections, {len(ref[k][0])} heads with a window")
    assert sum(len(ref[k][4]) for k in frames) >= 1                        # (the seeded detector does fire on these pictures)
    with FramePipeline(model, depth=1) as fp:
        for k in ("A", "B", "A"):                                          # the third: a replay
            fp.begin_yuv(frames[k])
            fp.detect_heads(**kw)
            got = fp.collect(detections=True)
            assert len(got) == 8
            assert_same(got, ref[k])
        # planes and BGR frames alternating on one pipeline: every slot is reused both ways
        for _ in range(_lib.MAX_INFLIGHT + 1):
            for k, as_yuv in (("A", True), ("B", False), ("W", True), ("A2", False), ("B", True), ("A", False)):
                fp.begin_yuv(frames[k]) if as_yuv else fp.begin(bgr[k])
                fp.detect_heads(**kw)
                assert_same(fp.collect(detections=True), ref[k])
    with FramePipeline(model, depth=2) as fp:                              # two in flight
        order = [("A", True), ("B", True), ("A2", False), ("W", True), ("B", False), ("A", True), ("A", True)]
        got = []
        for i, (k, as_yuv) in enumerate(order):
            fp.begin_yuv(frames[k]) if as_yuv else fp.begin(bgr[k])
            fp.detect_heads(**kw)
            if i >= 1:
                got.append(fp.collect(detections=True))
        got.append(fp.collect(detections=True))
        for g, (k, _) in zip(got, order):
            assert_same(g, ref[k])
    # the other consumers of a resident frame: detect and heads
    with FramePipeline(model, depth=1) as fp:
        inside = ref["A"][7] != 0                                           # (heads() raises for a window that leaves the frame)
        fp.begin(bgr["A"])
        want_boxes = fp.detect(**kw)
        fp.heads(want_boxes[0][inside])
        want = fp.collect()
        fp.begin_yuv(frames["A"])
        got_boxes = fp.detect(**kw)
        fp.heads(got_boxes[0][inside])
        assert_same(fp.collect(), want)
        assert_same(got_boxes, want_boxes)


# ---- 5. clips -------------------------------------------------------------------------------------------------------------------
def run_clip(fp, frames, kw):
    fp.begin_clip_yuv(frames)
    fp.detect_heads_clip(**kw)
    return fp.collect_clip(detections=True)


def test_clip_of_same_size_frames_equals_its_frames_alone(model, kw, pictures, single):
    frames = pictures[0]
    flipped = built("sample0_224x528", YC.NV12)
    for v in flipped["views"]:
        v[...] = v[::-1].copy()
    other = YC.frame_of(flipped, "bt601")
    with FramePipeline(model, depth=1) as fp:
        # one size, format and matrix (the launch over a grid of frames); one size, two formats and matrices (the mixed launch)
        for clip in ([frames["A"], other], [frames["A"], frames["A2"]], [frames["A2"]]):
            got, (rows_used, overflow) = run_clip(fp, clip, kw)
            assert len(got) == len(clip) and overflow == 0
            for g, f in zip(got, clip):
                assert_same(g, single(f.to_bgr()))
    # the slot is a clip_begin slot: the same clip from the converted frames, through the handle, in every array
    h = model._handle
    pair = [frames["A"], other]
    t = h.clip_begin(np.stack([f.to_bgr() for f in pair]))
    want = h.collect_clip(t, 2, h.clip_detect_heads(t, *hargs(kw)), want_logits=True)
    t = h.clip_begin_yuv(pair)
    got = h.collect_clip(t, 2, h.clip_detect_heads(t, *hargs(kw)), want_logits=True)
    for g, w in zip(got, want):
        assert (g.tobytes() == w.tobytes()) if isinstance(w, np.ndarray) else g == w


def test_clip_of_different_sizes_formats_and_matrices_equals_its_frames_alone(model, kw, pictures, single):
    frames = pictures[0]
    clip = [frames["W"], frames["A"], frames["B"]]                        # 97 x 131 first: the frames behind it start unaligned
    assert (97 * 131 * 3) % 4 != 0
    assert len({(f.h, f.w) for f in clip}) == 3 and len({f.format for f in clip}) == 2 and len({f.matrix for f in clip}) == 3
    with FramePipeline(model, depth=1) as fp:
        for c in (clip, clip[::-1]):
            got, (rows_used, overflow) = run_clip(fp, c, kw)
            assert overflow == 0
            for g, f in zip(got, c):
                assert_same(g, single(f.to_bgr()))
    h = model._handle                                                      # a clip_begin_mixed slot
    t = h.clip_begin_mixed([f.to_bgr() for f in clip])
    want = h.collect_clip(t, 3, h.clip_detect_heads(t, *hargs(kw)), want_logits=True)
    t = h.clip_begin_yuv(clip)
    got = h.collect_clip(t, 3, h.clip_detect_heads(t, *hargs(kw)), want_logits=True)
    for g, w in zip(got, want):
        assert (g.tobytes() == w.tobytes()) if isinstance(w, np.ndarray) else g == w


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_more_sizes_than_the_letterbox_cache_is_refused_and_takes_no_slot(kw, pictures, single):
    frames = pictures[0]
    clip = [frames["W"], frames["A"], frames["B"]]
    m = seeded_model()
    try:
        h = m._handle
        h.set_option("letterbox_cache", 2)
        with FramePipeline(m, depth=1) as fp:
            for _ in range(_lib.MAX_INFLIGHT + 1):                        # (a leak would use up the slots)
                with pytest.raises(ValueError, match="letterbox_cache"):
                    fp.begin_clip_yuv(clip)
                with pytest.raises(ValueError, match="letterbox_cache"):
                    h.clip_begin_yuv(clip)
            assert fp.in_flight == 0
            tickets = [h.frame_begin_yuv(frames["W"]) for _ in range(_lib.MAX_INFLIGHT)]      # every slot is still there
            for t in tickets:
                h.frame_heads(t, np.zeros((0, 4), np.int32))
                h.collect(t, 0)
            got, _ = run_clip(fp, clip[:2], kw)                            # two sizes fit
            for g, f in zip(got, clip[:2]):
                assert_same(g, single(f.to_bgr()))
            got, _ = run_clip(fp, [frames["A"], frames["A2"], frames["A"]], kw)      # three frames of ONE size need no entry each
            assert_same(got[2], single(frames["A"].to_bgr()))
    finally:
        m.close()


def test_bad_frames_and_wrong_tickets_fail_and_the_handle_stays_usable(model, kw, pictures, single):
    frames, keep = pictures
    h = model._handle
    lib, t = _lib.load(), C.c_int(-1)
    args = hargs(kw)[:5]
    good = frames["A"]
    landing = np.empty((600, 600, 3), np.uint8)

    def spoiled(fn):
        d = frames["B"].descriptor()
        fn(d)
        return d

    bad = [(lambda d: d.plane.__setitem__(2, None), "plane 2 is NULL"), (lambda d: d.pitch.__setitem__(0, 546), "pitch"),
           (lambda d: setattr(d, "format", 7), "unknown format"), (lambda d: setattr(d, "matrix", -1), "unknown matrix"),
           (lambda d: setattr(d, "w", 8193), "sides must be 1..8192"), (lambda d: setattr(d, "h", 0), "sides must be 1..8192")]
    for _ in range(2):                                                     # (twelve refusals: a leak would use up the slots)
        for fn, text in bad:
            d = spoiled(fn)
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
    for n in (0, 17):
        arr = (_lib.YuvFrameC * 17)(*[good.descriptor()] * 17)
        assert lib.whenet_clip_begin_yuv(h._h, arr, n, C.byref(t)) == _lib.EINVAL
    assert lib.whenet_frame_begin_yuv(h._h, None, C.byref(t)) == _lib.EINVAL
    # wrong-ticket uses fail as they do for BGR tickets
    tk = h.frame_begin_yuv(good)
    with pytest.raises(ValueError, match="holds a single frame"):
        h.clip_detect_heads(tk, *args, 20)
    cap = h.frame_detect_heads(tk, *args, 20)
    with pytest.raises(ValueError, match="was not submitted by clip_detect_heads"):
        h.collect_clip(tk, 1, cap)
    res = h.collect_detect(tk, cap)
    assert res[0].tobytes() == single(good.to_bgr())[4].tobytes()
    tk = h.clip_begin_yuv([frames["W"], good])
    for call in (lambda: h.frame_detect_heads(tk, *args, 20), lambda: h.frame_detect(tk, *args, 20), lambda: h.frame_letterbox(tk, (64, 96)),
                 lambda: h.frame_heads(tk, np.array([[10, 10, 50, 50]], np.int32))):
        with pytest.raises(ValueError, match="holds a clip"):
            call()
    k = h.clip_detect_heads(tk, *args, 20)
    with pytest.raises(ValueError, match="collect_clip returns it"):
        h.collect(tk, 3)
    res = h.collect_clip(tk, 2, k)
    assert res[0][1] == len(single(good.to_bgr())[4])
    # the pipeline's state checks are begin's and begin_clip's
    with FramePipeline(model, depth=2) as fp:
        for wrong in (good.to_bgr(), None, [good]):
            with pytest.raises(ValueError, match="YUVFrame"):
                fp.begin_yuv(wrong)
        for wrong in ([], [good] * 17, [good, good.to_bgr()]):
            with pytest.raises(ValueError):
                fp.begin_clip_yuv(wrong)
        fp.begin_yuv(good)
        for call in (lambda: fp.begin_yuv(good), lambda: fp.begin_clip_yuv([good]), lambda: fp.begin(good.to_bgr()),
                     lambda: fp.detect_heads_clip(**kw)):
            with pytest.raises(ValueError):
                call()
        fp.detect_heads(**kw)
        fp.begin_clip_yuv([good, frames["W"]])
        for call in (lambda: fp.begin_yuv(good), lambda: fp.detect_heads(**kw), lambda: fp.heads(np.zeros((0, 4), np.float32))):
            with pytest.raises(ValueError):
                call()
        fp.detect_heads_clip(**kw)
        with pytest.raises(ValueError, match="frames already in flight"):
            fp.begin_yuv(good)
        assert_same(fp.collect(detections=True), single(good.to_bgr()))
        got, _ = fp.collect_clip(detections=True)
        assert_same(got[1], single(frames["W"].to_bgr()))
        fp.begin_yuv(good)                                                 # left without heads: released on exit
    with FramePipeline(model, depth=1) as fp:                              # no slot leaked: every one is taken in turn
        for _ in range(_lib.MAX_INFLIGHT + 1):
            fp.begin_yuv(frames["B"])
            fp.detect_heads(**kw)
            assert_same(fp.collect(detections=True), single(frames["B"].to_bgr()))
