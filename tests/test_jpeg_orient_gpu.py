"""The oriented JPEG decode on the GPU (csrc/jpeg_dec.hip: the oriented frame kernels and their clip forms; Engine::op_jpeg_decode,
frame_begin_jpeg, clip_begin_jpeg, op_jpeg_decode_clip of csrc/engine_post.cpp with `orient`).  There is no tolerance anywhere: the
kernels return the bytes and the status of `whenet_jpeg_decode_oriented_host`, which tests/test_jpeg_orient_cpu.py holds to the numpy
table and to executed Pillow; pitched destinations keep every byte outside the rows of the ORIENTED frame.  Streams are made at test
time (tests/jpeg_orient_cases.py)."""
import json
import os

import numpy as np
import pytest
import torch  # noqa: F401  (first, so there is exactly one HIP runtime in the process)

from tests import jpeg_decode_cases as DC
from tests import jpeg_orient_cases as OC
from tests import jpeg_prog_cases as PC
from tests.test_jpeg_decode_gpu import GAP, guarded_rows, untouched
from whenet_hip import _lib, jpeg

pytestmark = pytest.mark.gpu
RULES = ("own", "libjpeg")
OK = [_lib.OK, -1]


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


_REF = {}


def reference(data, rule="own", bgr=True, progressive=False):
    """(frame, status) of the oriented host statement: computed once per stream, shared, never modified"""
    key = (data, rule, bgr, progressive)
    if key not in _REF:
        i = _lib.jpeg_parse_scans(data)[0]
        frame = np.empty(jpeg.oriented_shape(i.h, i.w, jpeg.orientation(data)) + (3,), np.uint8)
        status = _lib.jpeg_decode_oriented_host(data, jpeg.packed_surface(frame), bgr, rule, progressive)
        frame.setflags(write=False)
        _REF[key] = (frame, status)
    return _REF[key]


def surface_of(view, pitch):
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
    return s


# ---- 1. the kernels alone are the host statement and the numpy table --------------------------------------------------------------
@pytest.mark.parametrize("name", OC.PICTURE_NAMES)
def test_the_oriented_kernels_are_the_host_statement_and_the_numpy_table(post, name):
    h, w = OC.PICTURES[name][:2]
    k = 0
    for progressive, forms in ((False, ((0, 128), (1, 16))), (True, ((-1, 128),))):
        plain = OC.stream(name, progressive)
        for rule in RULES:
            for bgr in (True, False):
                u = jpeg.decode_host(plain, bgr=bgr, rule=rule, progressive=progressive)
                for v in OC.VALUES:
                    d = OC.tagged(name, v, progressive, order="II" if v & 1 else "MM")
                    want = OC.transform(u, v)
                    host, host_status = reference(d, rule, bgr, progressive)
                    assert np.array_equal(host, want) and host_status.tolist() == OK
                    oh, ow = want.shape[:2]
                    for entropy, seg_bytes in forms:
                        k += 1
                        block, view, pitch = guarded_rows(oh, 3 * ow, 5 + k % 4, k % 4)
                        status, _, applied = post.op_jpeg_decode_oriented(d, surface_of(view, pitch), bgr, entropy, seg_bytes, rule, progressive, True)
                        where = (name, progressive, rule, bgr, v, entropy)
                        assert status.tolist() == OK and applied == v, where
                        assert np.array_equal(view.reshape(oh, ow, 3), want), where
                        assert untouched(block, view), where      # no byte outside 3 * w' of any row
    # the tight frame through the public function (value 1 of a 4:2:0 BGR stream under rule 0: the plane kernel of the YUV ingest)
    for v in (1, 2, 5, 8):
        d = OC.tagged(name, v)
        assert np.array_equal(jpeg.decode(d, handle=post, orient=True), reference(d)[0])
        assert np.array_equal(jpeg.decode(d, handle=post), jpeg.decode_host(OC.stream(name)))      # without the argument: today's bytes


def test_every_constructed_segment_through_the_kernels(post):
    """the value the kernels apply is the parser's, whatever form the APP1 takes; broken EXIF changes nothing"""
    base = OC.stream("420_17x35")
    u = jpeg.decode_host(base)
    for name, (segments, where, want) in OC.SEGMENTS.items():
        d = OC.splice(base, segments, where)
        got = np.empty(jpeg.oriented_shape(35, 17, want) + (3,), np.uint8)
        status, _, applied = post.op_jpeg_decode_oriented(d, jpeg.packed_surface(got), True)
        assert status.tolist() == OK and applied == want, name
        assert np.array_equal(got, OC.transform(u, want)), name


@pytest.mark.parametrize("progressive", [False, True])
def test_a_damaged_turned_stream_keeps_its_status(post, progressive):
    cut = PC.DAMAGED["truncated_in_scan_5"] if progressive else OC.baseline_cut()
    for rule in RULES:
        for v in (1, 3, 6, 7):
            d = OC.oriented(cut, v)
            want, want_status = reference(d, rule, True, progressive)
            assert want_status[0] == PC.EFORMAT
            block, view, pitch = guarded_rows(want.shape[0], 3 * want.shape[1], 3 + v, v % 4)
            status, _, applied = post.op_jpeg_decode_oriented(d, surface_of(view, pitch), True, -1, 128, rule, progressive, True)
            assert status.tolist() == want_status.tolist() and applied == v
            assert np.array_equal(view.reshape(want.shape), want) and untouched(block, view)
            with pytest.raises(jpeg.DecodeError) as err:
                jpeg.decode(d, handle=post, rule=rule, progressive=progressive, orient=True)
            assert err.value.interval == want_status[1] and np.array_equal(err.value.frame, want)


# ---- 2. clips ---------------------------------------------------------------------------------------------------------------------
def decode_clip_guarded(h, datas, rule="own", bgr=True, progressive=False, entropy=-1, seg_bytes=128, tight=()):
    """the clip into pitched destinations between guard bytes: frame f and its status are the oriented host statement's of stream f"""
    blocks, surfaces = [], []
    for f, d in enumerate(datas):
        want, _ = reference(d, rule, bgr, progressive)
        block, view, pitch = guarded_rows(want.shape[0], 3 * want.shape[1], 0 if f in tight else 5 + f % 4, f % 4)
        blocks.append((block, view)), surfaces.append(surface_of(view, pitch))
    status, applied = h.op_jpeg_decode_clip_oriented(datas, surfaces, bgr, entropy, seg_bytes, rule, progressive, True)
    for f, d in enumerate(datas):
        want, want_status = reference(d, rule, bgr, progressive)
        assert status[f].tolist() == want_status.tolist(), f
        assert applied[f] == jpeg.orientation(d), f
        assert np.array_equal(blocks[f][1].reshape(want.shape), want), f
        assert untouched(*blocks[f]), f
    return status


def eight_and_one():
    return [OC.tagged("420_17x35", v) for v in OC.VALUES] + [OC.stream("420_64x48")]


def test_the_eight_values_of_one_stream_and_an_untagged_one_in_two_orders(post):
    datas = eight_and_one()
    for rule in RULES:
        for bgr in (True, False):
            decode_clip_guarded(post, datas, rule, bgr)
            decode_clip_guarded(post, datas[::-1], rule, bgr, tight=range(0, 9, 2))
    decode_clip_guarded(post, datas, entropy=1, seg_bytes=16)
    frames, status = jpeg.decode_clip(datas, handle=post, orient=True, rule="libjpeg", bgr=False)
    assert all(np.array_equal(fr, reference(d, "libjpeg", False)[0]) for fr, d in zip(frames, datas)) and status.tolist() == [OK] * 9
    # without the argument the clip is the upright one
    frames, _ = jpeg.decode_clip(datas, handle=post)
    assert all(np.array_equal(fr, jpeg.decode_host(OC.stream("420_17x35"))) for fr in frames[:8])


def test_sixteen_frames_of_value_6(post):
    for name in ("420_17x35", "444_33x65"):
        for rule in RULES:
            decode_clip_guarded(post, [OC.tagged(name, 6)] * 16, rule, tight=range(16) if rule == "own" else ())


def test_progressive_and_baseline_turned_frames_in_one_clip(post):
    datas = [OC.tagged("420_33x65", 6, True), OC.tagged("422_35x50_blocks3", 8), OC.tagged("grey_9x7", 5, True), OC.stream("420_64x48"),
             OC.tagged("444_17x35", 3, True), OC.tagged("420_4x9_cw2", 7), OC.stream("422_64x48", True), OC.tagged("420_64x48", 2)]
    for rule in RULES:
        decode_clip_guarded(post, datas, rule, progressive=True)
        decode_clip_guarded(post, datas[::-1], rule, bgr=False, progressive=True, entropy=1, seg_bytes=16)


@pytest.mark.parametrize("progressive", [False, True])
def test_a_damaged_turned_stream_at_frame_2_of_4(post, progressive):
    cut = PC.DAMAGED["truncated_in_scan_5"] if progressive else OC.baseline_cut()
    datas = [OC.tagged("420_17x35", 6, progressive), OC.tagged("444_33x65", 4), OC.oriented(cut, 6), OC.tagged("422_35x50_blocks3", 7, progressive)]
    for rule in RULES:
        status = decode_clip_guarded(post, datas, rule, progressive=progressive)
        assert status[2, 0] == PC.EFORMAT and [s.tolist() for k, s in enumerate(status) if k != 2] == [OK] * 3
    with pytest.raises(jpeg.DecodeError, match="frame 2") as err:
        jpeg.decode_clip(datas, handle=post, progressive=progressive, orient=True)
    assert np.array_equal(err.value.frame, reference(datas[2], "own", True, progressive)[0])


# ---- 3. counters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 16])
def test_turned_frames_cost_a_clip_at_most_one_enqueue(post, F):
    for datas in ([OC.tagged("420_17x35", 1 + f % 8) for f in range(F)], [OC.tagged("444_33x65", 6)] * F,
                  [OC.stream("420_64x48")] + [OC.tagged("420_64x48", 6)] * (F - 1)):
        before = post.jpeg_clip_counters()
        jpeg.decode_clip(datas, handle=post)
        mid = post.jpeg_clip_counters()
        jpeg.decode_clip(datas, handle=post, orient=True)
        after = post.jpeg_clip_counters()
        upright, turned = mid["enqueues"] - before["enqueues"], after["enqueues"] - mid["enqueues"]
        print(f"F = {F}: {upright} enqueues upright, {turned} with turned frames")
        assert turned <= upright + 1
        assert after["h2d"] - mid["h2d"] == 1 and after["clips"] - mid["clips"] == 1 and after["frames"] - mid["frames"] == F
    # a clip whose frames all carry value 1 enqueues exactly what the upright one enqueues
    ones = [OC.tagged("420_17x35", 1)] * F
    a = post.jpeg_clip_counters()
    jpeg.decode_clip(ones, handle=post)
    b = post.jpeg_clip_counters()
    jpeg.decode_clip(ones, handle=post, orient=True)
    c = post.jpeg_clip_counters()
    assert c["enqueues"] - b["enqueues"] == b["enqueues"] - a["enqueues"]


def test_a_single_oriented_decode_counts_as_the_upright_one():
    for progressive in (False, True):
        d = OC.tagged("420_33x65", 6, progressive)
        with _lib.Handle.postproc(0) as up, _lib.Handle.postproc(0) as turned:
            jpeg.decode(d, handle=up, progressive=progressive)
            jpeg.decode(d, handle=turned, progressive=progressive, orient=True)
            assert up.jpeg_progressive_counters() == turned.jpeg_progressive_counters()
            assert up.jpeg_decode_counters() == turned.jpeg_decode_counters()
            assert sum(up.jpeg_decode_counters().values()) + up.jpeg_progressive_counters()["decodes"] == 1


# ---- 4. the pipeline --------------------------------------------------------------------------------------------------------------
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
        return kwargs(json.load(f)["detect"], "tiny", score=0.0)       # threshold 0: the seeded detector fires on small frames


@pytest.mark.parametrize("bgr,rule,progressive", [(True, None, False), (False, "libjpeg", True)])
def test_begin_jpeg_oriented_is_begin_of_the_turned_frame(model, kw, bgr, rule, progressive):
    """boxes, poses and annotated bytes on one 64 x 48 stream: the detector's own heads, then given boxes through the overlay"""
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    plain = OC.stream("420_64x48", progressive)
    u = jpeg.decode_host(plain, bgr=bgr, rule=rule or "own", progressive=progressive)
    with FramePipeline(model, depth=1, bgr=bgr) as fp:
        for v in (1, 3, 6, 8):
            d = OC.tagged("420_64x48", v, progressive)
            frame = OC.transform(u, v)
            assert frame.shape == ((64, 48, 3) if v >= 5 else (48, 64, 3))
            boxes = np.asarray([(8, 8, 30, 30), (12, 14, 36, 40)], np.float32)
            fp.begin(frame)
            want_input = fp.detector_input(kw["size"], as_uint8=True)
            fp.detect_heads(**kw)
            want = fp.collect(detections=True)
            fp.begin(frame)
            fp.heads(boxes)
            painted = np.zeros_like(frame)
            fp.annotate(painted, display="full")
            want_heads = fp.collect()
            st = fp.begin_jpeg(d, rule=rule, progressive=progressive, orient=True)
            got_input = fp.detector_input(kw["size"], as_uint8=True)
            fp.detect_heads(**kw)
            got = fp.collect(detections=True)
            assert np.array_equal(got_input, want_input)
            assert_same(got, want)
            assert st.ok and st.interval == -1 and st.orientation == v
            st = fp.begin_jpeg(d, rule=rule, progressive=progressive, orient=True)
            fp.heads(boxes)
            out = np.zeros_like(frame)
            fp.annotate(out, display="full")
            assert_same(fp.collect(), want_heads)
            assert np.array_equal(out, painted) and st.orientation == v
            # without the argument (and the option at 0): the upright frame, orientation 1
            st = fp.begin_jpeg(d, rule=rule, progressive=progressive)
            assert fp._last_sizes == [(48, 64)]
            fp.heads(np.zeros((0, 4), np.float32))
            fp.collect()
            assert st.ok and st.orientation == 1


def run_clip(fp, begin, clip, kw, **begin_kw):
    sts = begin(clip, **begin_kw)
    fp.detect_heads_clip(**kw)
    outs = [np.zeros(tuple(s) + (3,), np.uint8) for s in fp._last_sizes]
    fp.annotate_clip(outs, display="full")
    return fp.collect_clip(detections=True), outs, sts


def assert_same_clip(got, want):
    from tests.test_clip_gpu import assert_same
    (gf, gcount), gouts, _ = got
    (wf, wcount), wouts, _ = want
    assert gcount == wcount and len(gf) == len(wf)
    for g, w in zip(gf, wf):
        assert_same(g, w)
    for g, w in zip(gouts, wouts):
        assert g.shape == w.shape and g.tobytes() == w.tobytes()


@pytest.mark.parametrize("rule", RULES)
def test_begin_clip_jpeg_oriented_is_begin_clip_mixed_of_the_turned_frames(model, kw, rule):
    from whenet_hip.frames import FramePipeline
    datas = [OC.tagged("420_64x48", 1), OC.tagged("420_64x48", 3), OC.tagged("420_64x48", 6, True), OC.tagged("422_35x50_blocks3", 8),
             OC.stream("444_33x65", True)]
    frames = [np.array(reference(d, rule, True, True)[0]) for d in datas]
    assert [f.shape[:2] for f in frames] == [(48, 64), (48, 64), (64, 48), (35, 50), (65, 33)]
    with FramePipeline(model, depth=1) as fp:
        want = run_clip(fp, fp.begin_clip_mixed, frames, kw)
        for _ in range(2):                                               # (the slot's buffers reused)
            got = run_clip(fp, fp.begin_clip_jpeg, datas, kw, rule=rule, progressive=True, orient=True)
            assert_same_clip(got, want)
            assert [st.orientation for st in got[2]] == [1, 3, 6, 8, 1] and all(st.ok for st in got[2])
        assert sum(len(t[4]) for t in got[0][0]) > 0                    # the detector fired


def test_a_clip_is_one_size_by_its_oriented_sizes(model, kw):
    """64 x 48 upright next to 48 x 64 with value 6 and 8: one size after turning, the slot of begin_clip"""
    from whenet_hip.frames import FramePipeline
    datas = [OC.stream("420_64x48"), OC.tagged("420_48x64", 6), OC.tagged("420_48x64", 8), OC.tagged("420_64x48", 3)]
    frames = [np.array(reference(d)[0]) for d in datas]
    assert {f.shape for f in frames} == {(48, 64, 3)}
    with FramePipeline(model, depth=1) as fp:
        want = run_clip(fp, fp.begin_clip, frames, kw)
        got = run_clip(fp, fp.begin_clip_jpeg, datas, kw, orient=True)
        assert_same_clip(got, want)
        assert [st.orientation for st in got[2]] == [1, 6, 8, 3]


# ---- 5. the option and the errors -------------------------------------------------------------------------------------------------
def test_the_option_turns_the_single_stream_calls_and_leaves_clips_alone(model, kw):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    d = OC.tagged("420_64x48", 6)
    turned, upright = reference(d)[0], jpeg.decode_host(d)
    h = model._handle
    with pytest.raises(ValueError):
        h.set_option("jpeg_orient", 2)
    with FramePipeline(model, depth=1) as fp:
        fp.begin(np.array(turned))
        want_input = fp.detector_input(kw["size"], as_uint8=True)
        fp.detect_heads(**kw)
        want = fp.collect(detections=True)
        fp.begin(upright)
        want_upright_input = fp.detector_input(kw["size"], as_uint8=True)
        fp.detect_heads(**kw)
        want_upright = fp.collect(detections=True)
        h.set_option("jpeg_orient", 1)
        try:
            st = fp.begin_jpeg(d)
            assert fp._last_sizes == [(64, 48)]
            assert np.array_equal(fp.detector_input(kw["size"], as_uint8=True), want_input)
            fp.detect_heads(**kw)
            assert_same(fp.collect(detections=True), want)
            assert st.ok and st.orientation == 6
            got = np.empty_like(turned)
            assert h.op_jpeg_decode(d, jpeg.packed_surface(got), True).tolist() == OK and np.array_equal(got, turned)
            assert h.op_jpeg_decode_rule(d, jpeg.packed_surface(got), False, 1, 16, "libjpeg")[0].tolist() == OK
            assert np.array_equal(got, reference(d, "libjpeg", False)[0])
            # orient=False overrides the option: the SLOT holds the upright frame (its detector input and detections are those of
            # begin(upright)), and so does the destination of jpeg.decode on the same handle
            st = fp.begin_jpeg(d, orient=False)
            assert fp._last_sizes == [(48, 64)] and st.orientation == 1
            got_input = fp.detector_input(kw["size"], as_uint8=True)
            fp.detect_heads(**kw)
            got_upright = fp.collect(detections=True)
            assert np.array_equal(got_input, want_upright_input) and not np.array_equal(got_input, want_input)
            assert_same(got_upright, want_upright)
            assert np.array_equal(jpeg.decode(d, handle=h), upright) and np.array_equal(jpeg.decode(d, handle=h, rule="libjpeg", bgr=False),
                                                                                        jpeg.decode_host(d, rule="libjpeg", bgr=False))
            assert np.array_equal(jpeg.decode(d, handle=h, orient=True), turned)
            # clips do not read the option
            frames, _ = jpeg.decode_clip([d, d], handle=h)
            assert all(np.array_equal(f, upright) for f in frames)
            sts = fp.begin_clip_jpeg([d, d])
            assert fp._last_sizes == [(48, 64)] * 2 and [s.orientation for s in sts] == [1, 1]
            fp.detect_heads_clip(**kw)
            fp.collect_clip()
        finally:
            h.set_option("jpeg_orient", 0)
        st = fp.begin_jpeg(d)
        assert fp._last_sizes == [(48, 64)] and st.orientation == 1
        assert np.array_equal(fp.detector_input(kw["size"], as_uint8=True), want_upright_input)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
        got = np.empty_like(upright)
        assert h.op_jpeg_decode(d, jpeg.packed_surface(got), True).tolist() == OK and np.array_equal(got, upright)


def test_a_planar_destination_and_a_turned_stream(kw):
    """WHENET_EINVAL, nothing written, nothing enqueued or counted: the tickets are those of a twin handle that never saw the calls"""
    from tests.test_yuv_gpu import seeded_model
    good = OC.tagged("420_64x48", 6)

    def planar(fmt, h, w):
        ch, cw = (h + 1) // 2, (w + 1) // 2
        planes = [np.full((h, w), GAP, np.uint8)] + ([np.full((ch, cw), GAP, np.uint8)] * 2 if fmt == _lib.YUV_I420 else [np.full((ch, 2 * cw), GAP, np.uint8)])
        planes = [p.copy() for p in planes]
        s = _lib.SurfaceC()
        for k, p in enumerate(planes):
            s.plane[k], s.pitch[k] = p.ctypes.data, p.strides[0]
        s.format, s.matrix, s.on_device = fmt, _lib.YUV_JFIF, 0
        return s, planes

    def next_ticket(h):
        t, applied = h.frame_begin_jpeg_oriented(good, np.zeros(2, np.int32))
        assert applied == 6
        h.frame_heads(t, np.zeros((0, 4), np.int32))
        h.collect(t, 0)
        return t

    m, twin = seeded_model(), seeded_model()
    try:
        want = [next_ticket(twin._handle) for _ in range(2)]
        got = [next_ticket(m._handle)]
        before = (m._handle.jpeg_decode_counters(), m._handle.jpeg_clip_counters())
        for fmt in (_lib.YUV_I420, _lib.YUV_NV12):
            for hh, ww in ((48, 64), (64, 48)):
                s, planes = planar(fmt, hh, ww)
                with pytest.raises(ValueError, match="packed surfaces only"):
                    m._handle.op_jpeg_decode_oriented(good, s, True)
                with pytest.raises(ValueError, match="frame 1.*packed surfaces only"):
                    m._handle.op_jpeg_decode_clip_oriented([OC.stream("420_64x48"), good], [planar(fmt, 48, 64)[0], s], True)
                assert all((p == GAP).all() for p in planes)
        assert (m._handle.jpeg_decode_counters(), m._handle.jpeg_clip_counters()) == before
        # value 1 and an untagged stream keep the planar destinations they have today
        s, planes = planar(_lib.YUV_I420, 48, 64)
        assert m._handle.op_jpeg_decode_oriented(OC.tagged("420_64x48", 1), s, True)[0].tolist() == OK
        assert np.array_equal(planes[0], jpeg.decode_planes_host(OC.stream("420_64x48"))[0][0])
        got.append(next_ticket(m._handle))
        assert got == want
        # bad values of the argument itself
        lib = _lib.load()
        frame = np.full((64, 48, 3), GAP, np.uint8)
        a = np.frombuffer(good, np.uint8)
        rc = lib.whenet_op_jpeg_decode_oriented(m._handle._h, a.ctypes.data, a.size, jpeg.packed_surface(frame), _lib.BGR, -1, 128, -1, -1, 2,
                                                np.zeros(2, np.int32).ctypes.data, None, None)
        assert rc == _lib.EINVAL and (frame == GAP).all()
    finally:
        m.close()
        twin.close()
