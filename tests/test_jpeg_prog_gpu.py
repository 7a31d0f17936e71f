"""The progressive JPEG decoder on the GPU (csrc/jpeg_prog.hip; Engine::op_jpeg_decode / frame_begin_jpeg of csrc/engine_post.cpp with
progressive streams accepted).  There is no tolerance anywhere: the kernels return the bytes and the status of
`whenet_jpeg_decode_progressive_host`, which tests/test_jpeg_prog_cpu.py holds to the numpy statement, to the baseline twin and to
executed Pillow; pitched destinations keep every byte outside their rows.  Streams are made at test time."""
import json
import os

import numpy as np
import pytest
import torch  # noqa: F401  (first, so there is exactly one HIP runtime in the process)

from tests import jpeg_decode_cases as DC
from tests import jpeg_prog_cases as PC
from tests.test_jpeg_decode_gpu import GAP, guarded_rows, untouched
from whenet_hip import _lib, jpeg

pytestmark = pytest.mark.gpu

ALL = PC.PILLOW_NAMES + PC.CONSTRUCTED_NAMES + PC.DAMAGED_NAMES
SPECIAL = {"flat_grey_1024": PC.flat_grey_1024, "noisy_q100": PC.noisy_q100}


def stream_of(name):
    if name in SPECIAL:
        return SPECIAL[name]()
    if name in PC.PILLOW:
        return PC.pillow_case(name)
    if name in PC.DAMAGED:
        return PC.DAMAGED[name]
    return PC.constructed(name)


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


def host_reference(data, bgr, rule):
    i = _lib.jpeg_parse_scans(data)[0]
    frame = np.empty((i.h, i.w, 3), np.uint8)
    status = _lib.jpeg_decode_progressive_host(data, jpeg.packed_surface(frame), bgr, rule)
    return frame, status


# ---- 1. the kernels alone are the host statement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL + list(SPECIAL))
def test_op_jpeg_decode_progressive_equals_the_host_function(post, name):
    data = stream_of(name)
    i, scans = _lib.jpeg_parse_scans(data)
    for k, (bgr, rule) in enumerate(((True, "own"), (False, "libjpeg"), (False, "own"), (True, "libjpeg"))):
        want, want_status = host_reference(data, bgr, rule)
        block, view, pitch = guarded_rows(i.h, 3 * i.w, 7 + k, 1 + k)
        s = _lib.SurfaceC()
        s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
        status, stats = post.op_jpeg_decode_progressive(data, s, bgr, rule)
        assert status.tolist() == want_status.tolist(), (name, bgr, rule)
        assert np.array_equal(view.reshape(i.h, i.w, 3), want), (name, bgr, rule)
        assert untouched(block, view), name
        assert stats[:4].tolist() == [sum(sc.intervals for sc in scans), max(sc.level for sc in scans), len(scans), max(sc.level for sc in scans)]
    # the tight frame through the public function (for 4:2:0 BGR under rule 0: the plane kernel of the YUV ingest)
    assert np.array_equal(jpeg.decode(data, handle=post, strict=False, progressive=True), host_reference(data, True, "own")[0])
    if name in PC.DAMAGED:
        with pytest.raises(jpeg.DecodeError) as err:
            jpeg.decode(data, handle=post, progressive=True)
        assert err.value.interval == host_reference(data, True, "own")[1][1] >= 0


@pytest.mark.parametrize("name", [n for n in PC.PILLOW_NAMES + PC.CONSTRUCTED_NAMES if "_420_" in n] + ["noisy_q100"])
def test_a_420_stream_decodes_into_i420_and_nv12_surfaces(post, name):
    data = stream_of(name)
    i = _lib.jpeg_parse_scans(data)[0]
    h, w = i.h, i.w
    ch, cw = (h + 1) // 2, (w + 1) // 2
    planes = jpeg.decode_planes_host(data, progressive=True)[0]
    for fmt in ("i420", "nv12"):
        y = np.full((h, w + 5), GAP, np.uint8)
        s = _lib.SurfaceC()
        s.plane[0], s.pitch[0] = y.ctypes.data, w + 5
        if fmt == "i420":
            u, v = np.full((ch, cw + 3), GAP, np.uint8), np.full((ch, cw + 1), GAP, np.uint8)
            s.plane[1], s.pitch[1], s.plane[2], s.pitch[2] = u.ctypes.data, cw + 3, v.ctypes.data, cw + 1
            s.format = _lib.YUV_I420
        else:
            uv = np.full((ch, 2 * cw + 2), GAP, np.uint8)
            s.plane[1], s.pitch[1] = uv.ctypes.data, 2 * cw + 2
            s.format = _lib.YUV_NV12
        s.matrix, s.on_device = _lib.YUV_JFIF, 0
        status, _ = post.op_jpeg_decode_progressive(data, s, True, "own")
        assert status.tolist() == [PC.OK, -1]
        assert np.array_equal(y[:, :w], planes[0]) and (y[:, w:] == GAP).all()
        if fmt == "i420":
            assert np.array_equal(u[:, :cw], planes[1]) and np.array_equal(v[:, :cw], planes[2])
            assert (u[:, cw:] == GAP).all() and (v[:, cw:] == GAP).all()
        else:
            assert np.array_equal(uv[:, 0:2 * cw:2], planes[1]) and np.array_equal(uv[:, 1:2 * cw:2], planes[2]) and (uv[:, 2 * cw:] == GAP).all()


NAMES_BOTH_WAYS = ["pil_422_35x50_q75_blocks3", "pil_420_17x17_q100_blocks3", "pil_grey_64x48_q75_rows1", "levels14_420_17x17_ranked",
                   "dri_changes_420_17x17_fixed", "truncated_in_scan_5", "wrong_rst_scan_3", "ends_in_correction_bits", "noisy_q100"]


def test_a_launch_per_scan_gives_the_bytes_of_a_launch_per_level_and_the_counters_count():
    """option jpeg_prog_levels: 1 (default) one scan-kernel launch per level, 0 one per scan in stream order; the same bytes"""
    with _lib.Handle.postproc(0) as by_level, _lib.Handle.postproc(0) as by_scan:
        by_scan.set_option("jpeg_prog_levels", 0)
        with pytest.raises(ValueError):
            by_scan.set_option("jpeg_prog_levels", 2)
        decodes, launches, nscans = 0, [0, 0], 0
        for name in NAMES_BOTH_WAYS:
            data = stream_of(name)
            i, scans = _lib.jpeg_parse_scans(data)
            a, b = np.empty((i.h, i.w, 3), np.uint8), np.empty((i.h, i.w, 3), np.uint8)
            sa, ta = by_level.op_jpeg_decode_progressive(data, jpeg.packed_surface(a), True, "libjpeg")
            sb, tb = by_scan.op_jpeg_decode_progressive(data, jpeg.packed_surface(b), True, "libjpeg")
            assert np.array_equal(a, b) and sa.tolist() == sb.tolist() == host_reference(data, True, "libjpeg")[1].tolist(), name
            levels = max(sc.level for sc in scans)
            assert (ta[3], tb[3]) == (levels, len(scans)), name
            if name.startswith("pil_"):
                assert levels == 3 and len(scans) == (10 if i.components == 3 else 6)      # Pillow's script
            decodes, nscans = decodes + 1, nscans + len(scans)
            launches[0] += levels
            launches[1] += len(scans)
        assert by_level.jpeg_progressive_counters() == {"decodes": decodes, "launches": launches[0], "scans": nscans}
        assert by_scan.jpeg_progressive_counters() == {"decodes": decodes, "launches": launches[1], "scans": nscans}
        assert by_level.jpeg_decode_counters() == {"interval": 0, "segmented": 0}      # no baseline decode ran


@pytest.mark.parametrize("name", ["pil_420_17x17_q75_blocks3", "pil_444_35x50_q75_nodri", "pil_grey_9x7_q75_rows1"])
def test_a_baseline_stream_through_the_progressive_calls_is_the_existing_call(post, name):
    data = PC.pillow_twin(name)
    for rule in ("own", "libjpeg"):
        want = jpeg.decode(data, handle=post, rule=rule)
        assert np.array_equal(jpeg.decode(data, handle=post, rule=rule, progressive=True), want)
        assert np.array_equal(jpeg.decode(data, handle=post, rule=rule, progressive=True, entropy="segmented", seg_bytes=16), want)
        i = _lib.jpeg_parse(data)
        got = np.empty((i.h, i.w, 3), np.uint8)
        status, stats = post.op_jpeg_decode_progressive(data, jpeg.packed_surface(got), True, rule)
        assert status.tolist() == [PC.OK, -1] and np.array_equal(got, want)
    before = post.jpeg_progressive_counters()
    jpeg.decode(data, handle=post, progressive=True)
    assert post.jpeg_progressive_counters() == before            # a baseline stream is the baseline decoder's


def test_refusals_leave_the_handle_usable(post):
    good = PC.pillow_case("pil_420_17x17_q75_nodri")
    frame = np.full((17, 17, 3), GAP, np.uint8)
    for name, data in PC.REFUSED.items():
        with pytest.raises(ValueError):
            post.op_jpeg_decode_progressive(data, jpeg.packed_surface(frame), True, "own")
    assert (frame == GAP).all()
    # the defaults still refuse SOF2, in the words the earlier tests match
    for call in (lambda: post.op_jpeg_decode(good, jpeg.packed_surface(frame), True), lambda: jpeg.decode(good, handle=post),
                 lambda: jpeg.decode(good, handle=post, rule="libjpeg"), lambda: jpeg.decode_clip([good], handle=post)):
        with pytest.raises(ValueError, match="progressive"):
            call()
    assert (frame == GAP).all()
    assert np.array_equal(jpeg.decode(good, handle=post, progressive=True), host_reference(good, True, "own")[0])


def test_the_option_turns_the_plain_calls_into_their_progressive_twins():
    data = PC.pillow_case("pil_422_35x50_q75_blocks3")
    base = PC.pillow_twin("pil_422_35x50_q75_blocks3")
    with _lib.Handle.postproc(0) as h:
        h.set_option("jpeg_progressive", 1)
        for rule in ("own", "libjpeg"):
            want = host_reference(data, True, rule)[0]
            got = np.empty_like(want)
            assert h.op_jpeg_decode_rule(data, jpeg.packed_surface(got), True, -1, 128, rule)[0].tolist() == [PC.OK, -1]
            assert np.array_equal(got, want)
        got = np.empty_like(want)
        assert h.op_jpeg_decode(data, jpeg.packed_surface(got), True).tolist() == [PC.OK, -1]
        assert np.array_equal(got, host_reference(data, True, "own")[0])
        assert h.op_jpeg_decode_ex(data, jpeg.packed_surface(got), True, 1, 16)[0].tolist() == [PC.OK, -1]      # entropy: ignored for SOF2
        assert np.array_equal(got, host_reference(data, True, "own")[0])
        assert np.array_equal(jpeg.decode(base, handle=h), jpeg.decode_host(base))
        with pytest.raises(ValueError, match="frame 0.*progressive"):      # clips ignore the option
            jpeg.decode_clip([data], handle=h)
        h.set_option("jpeg_progressive", 0)
        with pytest.raises(ValueError, match="progressive"):
            h.op_jpeg_decode(data, jpeg.packed_surface(got), True)


# ---- 2. the pipeline: begin_jpeg -------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("bgr,rule", [(True, None), (False, "libjpeg")])
def test_begin_jpeg_progressive_is_begin_of_the_decoded_frame(model, kw, bgr, rule):
    """through detector, poses and overlay on one 64 x 48 stream, by the keyword and by the handle's option"""
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    data = PC.pillow_case("pil_420_64x48_q75_rows1")
    frame = jpeg.decode_host(data, bgr=bgr, rule=rule or "own", progressive=True)
    assert frame.shape == (48, 64, 3)
    boxes = np.asarray([(8, 8, 30, 30), (12, 14, 36, 40)], np.float32)
    with FramePipeline(model, depth=1, bgr=bgr) as fp:
        fp.begin(frame)
        want_input = fp.detector_input(kw["size"], as_uint8=True)
        fp.detect_heads(**kw)
        want = fp.collect(detections=True)
        fp.begin(frame)
        fp.heads(boxes)
        painted = np.zeros_like(frame)
        fp.annotate(painted, display="full")
        want_heads = fp.collect()
        for option in (0, 1):
            model._handle.set_option("jpeg_progressive", option)
            try:
                st = fp.begin_jpeg(data, rule=rule, progressive=None if option else True)
                got_input = fp.detector_input(kw["size"], as_uint8=True)
                fp.detect_heads(**kw)
                got = fp.collect(detections=True)
                assert np.array_equal(got_input, want_input)
                assert_same(got, want)
                assert st.ok and st.interval == -1
                fp.begin_jpeg(data, rule=rule, progressive=None if option else True)
                fp.heads(boxes)
                out = np.zeros_like(frame)
                fp.annotate(out, display="full")
                assert_same(fp.collect(), want_heads)
                assert np.array_equal(out, painted)
            finally:
                model._handle.set_option("jpeg_progressive", 0)
        with pytest.raises(ValueError, match="progressive"):      # the default still refuses, and takes no place
            fp.begin_jpeg(data)
        assert fp.in_flight == 0


def test_begin_jpeg_progressive_with_a_damaged_or_refused_stream(kw):
    """a damaged stream still yields a ticket and its defined frame; a refused one takes no slot: the tickets are those of a twin
    handle that saw the accepted submissions alone"""
    from tests.test_clip_gpu import assert_same
    from tests.test_yuv_gpu import seeded_model
    from whenet_hip.frames import FramePipeline
    good = PC.pillow_case("pil_420_64x48_q75_rows1")
    data = PC.DAMAGED["truncated_in_scan_5"]
    want_status = host_reference(data, True, "own")[1]
    frame = jpeg.decode_host(data, strict=False, progressive=True)

    def next_ticket(h):
        t = h.frame_begin_jpeg(good, np.zeros(2, np.int32), progressive=True)
        h.frame_heads(t, np.zeros((0, 4), np.int32))
        h.collect(t, 0)
        return t

    m, twin = seeded_model(), seeded_model()
    try:
        want = [next_ticket(twin._handle) for _ in range(3)]
        got = [next_ticket(m._handle)]
        for _ in range(_lib.MAX_INFLIGHT + 1):                    # (a leak would use up the slots)
            for refused in PC.REFUSED.values():
                with pytest.raises(ValueError):
                    m._handle.frame_begin_jpeg(refused, np.zeros(2, np.int32), progressive=True)
        got.append(next_ticket(m._handle))
        for _ in range(_lib.MAX_INFLIGHT + 1):
            with pytest.raises(ValueError, match="progressive"):
                m._handle.frame_begin_jpeg(good, np.zeros(2, np.int32))      # the default refuses SOF2
        got.append(next_ticket(m._handle))
        assert got == want
        with FramePipeline(m, depth=1) as fp:
            fp.begin(frame)
            fp.detect_heads(**kw)
            ref = fp.collect(detections=True)
            st = fp.begin_jpeg(data, progressive=True)
            fp.detect_heads(**kw)
            assert_same(fp.collect(detections=True), ref)
            assert not st.ok and st.interval == want_status[1]
            st = fp.begin_jpeg(good, progressive=True)
            fp.heads(np.zeros((0, 4), np.float32))
            fp.collect()
            assert st.ok and st.interval == -1
            with pytest.raises(ValueError, match="frame 1.*progressive"):      # clips still refuse SOF2
                fp.begin_clip_jpeg([PC.pillow_twin("pil_420_64x48_q75_rows1"), good])
            assert fp.in_flight == 0
    finally:
        m.close()
        twin.close()
