"""Rule 1 of the JPEG decoder (libjpeg's bytes) on the GPU: the rule-1 forms of the inverse DCT and frame kernels of
csrc/jpeg_dec.hip, alone, under the clip grid and behind `begin_jpeg`.  There is no tolerance anywhere: the kernels return the bytes
and the status of the host statement (`whenet_jpeg_decode_rule_host`), which tests/test_jpeg_exact_cpu.py holds to the numpy
statement and to executed Pillow.  The shapes are the smallest at which the kernels can go wrong: cw <= 2 (replication) and cw = 3
(the first filtered width), both vertical clamps, planes whose padding holds decoded samples, a row tail of 1, 2 and 3 pixels
behind a workgroup's item boundary, destinations at every address modulo 4."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import jpeg_decode_cases as DC
from tests import jpeg_exact_cases as EC
from tests.test_jpeg_decode_gpu import GAP, device_packed, guarded_rows, read_packed, untouched
from whenet_hip import _lib, jpeg, overlay
from whenet_hip.yuv import YUVFrame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (h, w): w = 1..4 replicate, w = 5, 6 filter (cw = 3); h = 1, 2, 3 clamp above and below; 17 x 17 is odd both ways; 8 x 33 and 70 x 50
# leave decoded samples in the planes' padding; 3 x 1029..1031: 258 items per row, so a row's tail of 1, 2, 3 pixels lies in the
# second workgroup and the next row starts inside it
SMALL = [(h, w) for h in (1, 2, 3) for w in (1, 2, 3, 4, 5, 6)] + [(17, 17), (8, 33), (70, 50), (3, 1029), (3, 1030), (3, 1031)]


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def stream(sampling, h, w):
    return EC.sweep_stream(sampling, h, w)


@functools.lru_cache(maxsize=None)
def host(data, bgr=True):
    """(frame, status) of the host statement under rule 1: computed once per stream and order, shared, never modified"""
    i = _lib.jpeg_parse(data)
    frame = np.empty((i.h, i.w, 3), np.uint8)
    status = _lib.jpeg_decode_rule_host(data, jpeg.packed_surface(frame), bgr, "libjpeg")
    frame.setflags(write=False)
    return frame, status.tolist()


def decode_pitched(post, data, bgr, extra, shift, entropy=-1, seg_bytes=128, rule="libjpeg"):
    """the kernels alone into rows `extra` bytes apart that start `shift` bytes into a guarded block: (frame, status, untouched)"""
    i = _lib.jpeg_parse(data)
    block, view, pitch = guarded_rows(i.h, 3 * i.w, extra, shift)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
    status, _ = post.op_jpeg_decode_rule(data, s, bgr, entropy, seg_bytes, rule)
    return view.reshape(i.h, i.w, 3).copy(), status.tolist(), untouched(block, view)


# ---- 1. the kernels alone are the host statement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("sampling", [1, 2], ids=["422", "420"])
def test_the_rule_1_kernels_equal_the_host_statement_at_the_small_shapes(post, sampling, bgr):
    for k, (h, w) in enumerate(SMALL):
        data = stream(sampling, h, w)
        want, want_status = host(data, bgr)
        got, status, clean = decode_pitched(post, data, bgr, extra=5 + k % 3, shift=1 + k % 3)      # addresses 1, 2, 3 mod 4
        assert status == want_status == [_lib.OK, -1], (h, w)
        assert np.array_equal(got, want), (h, w)
        assert clean, (h, w)
    # an aligned pitched destination, and the tight frame through the public function (under rule 0 the plane kernel of the YUV ingest)
    for h, w in ((3, 5), (17, 17), (70, 50), (3, 1031)):
        data = stream(sampling, h, w)
        got, status, clean = decode_pitched(post, data, bgr, extra=4 - (3 * w) % 4, shift=0)
        assert np.array_equal(got, host(data, bgr)[0]) and clean, (h, w)
        assert np.array_equal(jpeg.decode(data, handle=post, bgr=bgr, rule="libjpeg"), host(data, bgr)[0]), (h, w)


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("name", ["pil_444_17x17", "pil_grey_17x17"])
def test_444_and_grey_streams_under_rule_1(post, name, bgr):
    data = DC.case(name)
    want, want_status = host(data, bgr)
    for shift in (0, 1, 2, 3):
        got, status, clean = decode_pitched(post, data, bgr, extra=3, shift=shift)
        assert status == want_status and np.array_equal(got, want) and clean, shift
    assert np.array_equal(want, EC.statement_frame(name, bgr))      # (the host statement is the numpy statement here too)


@pytest.mark.parametrize("sampling", [1, 2], ids=["422", "420"])
def test_both_entropy_forms_give_one_frame(post, sampling):
    for data in (stream(sampling, 70, 50), DC.case("pil_420_rst_rows" if sampling == 2 else "pil_422_rst_rows")):
        want, want_status = host(data, True)
        for entropy, seg in ((0, 128), (1, 4), (1, 128)):
            got, status, clean = decode_pitched(post, data, True, extra=2, shift=3, entropy=entropy, seg_bytes=seg)
            assert status == want_status and np.array_equal(got, want) and clean, (entropy, seg)


@pytest.mark.parametrize("name", DC.DAMAGED_NAMES)
def test_damaged_streams_are_defined_and_keep_their_status(post, name):
    data, bad = DC.DAMAGED[name]()
    want, want_status = host(data, True)
    assert want_status == [_lib.EFORMAT, bad]
    for entropy in (0, 1):
        got, status, clean = decode_pitched(post, data, True, extra=1, shift=2, entropy=entropy, seg_bytes=16)
        assert status == want_status and np.array_equal(got, want) and clean, entropy


def test_rule_0_through_the_rule_entry_point_and_the_refusals(post):
    data = DC.case("pil_420_17x17")
    got, status, clean = decode_pitched(post, data, True, extra=3, shift=1, rule="own")
    assert np.array_equal(got, jpeg.decode_host(data)) and status == [_lib.OK, -1] and clean
    got, _, _ = decode_pitched(post, data, True, extra=3, shift=1, rule=None)      # None: the handle's option, whose default is rule 0
    assert np.array_equal(got, jpeg.decode_host(data))
    y, c = np.zeros((17, 17), np.uint8), np.zeros((9, 9), np.uint8)
    yuv = overlay.surface_of(YUVFrame.i420(y, c, c, "jfif"), 17, 17)[0]
    assert post.op_jpeg_decode_rule(data, yuv, True, -1, 128, "own")[0].tolist() == [_lib.OK, -1]
    with pytest.raises(ValueError, match="WHENET_SURF_PACKED only"):
        post.op_jpeg_decode_rule(data, yuv, True, -1, 128, "libjpeg")
    with pytest.raises(ValueError, match="WHENET_SURF_PACKED only"):
        post.op_jpeg_decode_clip_rule([data], [yuv], True, -1, 128, "libjpeg")
    with pytest.raises(ValueError, match="jpeg_rule"):
        post.set_option("jpeg_rule", 2)
    assert np.array_equal(jpeg.decode(data, handle=post, rule="libjpeg"), host(data, True)[0])      # the handle stays usable


# ---- 2. the option on the handle -------------------------------------------------------------------------------------------------
def test_the_option_is_read_by_every_decode_call_of_the_handle(post):
    data = DC.case("pil_420_rst_rows")
    info = _lib.jpeg_parse(data)
    want = host(data, True)[0]
    assert not np.array_equal(want, jpeg.decode_host(data))
    ent = torch.from_numpy(np.frombuffer(data, np.uint8)[info.data_offset:].copy()).to(DEV)
    status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    post.set_option("jpeg_rule", 1)
    try:
        frame = np.empty((info.h, info.w, 3), np.uint8)
        assert post.op_jpeg_decode(data, jpeg.packed_surface(frame), True).tolist() == [_lib.OK, -1] and np.array_equal(frame, want)
        frame = np.empty((info.h, info.w, 3), np.uint8)
        post.op_jpeg_decode_ex(data, jpeg.packed_surface(frame), True, 1, 16)
        assert np.array_equal(frame, want)
        frame = np.empty((info.h, info.w, 3), np.uint8)
        post.op_jpeg_decode_clip([data], [jpeg.packed_surface(frame)], True)
        assert np.array_equal(frame, want)
        buf, s_dst = device_packed(info.h, info.w, 2, 1)
        post.jpeg_decode_device(info, ent.data_ptr(), ent.numel(), s_dst, True, status.data_ptr())
        torch.cuda.synchronize()
        got, clean = read_packed(buf, info.h, info.w, 2, 1)
        assert status.cpu().tolist() == [_lib.OK, -1] and np.array_equal(got, want) and clean
        got, _, _ = decode_pitched(post, data, True, extra=0, shift=0, rule="own")              # the argument wins over the option
        assert np.array_equal(got, jpeg.decode_host(data))
    finally:
        post.set_option("jpeg_rule", 0)
    frame = np.empty((info.h, info.w, 3), np.uint8)
    post.op_jpeg_decode(data, jpeg.packed_surface(frame), True)
    assert np.array_equal(frame, jpeg.decode_host(data))


# ---- 3. clips --------------------------------------------------------------------------------------------------------------------
def test_a_clip_of_five_streams_with_a_damaged_one_is_the_five_single_decodes(post):
    damaged, bad = DC.DAMAGED["stray_marker"]()
    datas = [stream(2, 70, 50), stream(1, 8, 33), damaged, DC.case("pil_444_17x17"), stream(2, 3, 5)]
    for bgr in (True, False):
        singles = [jpeg.decode(d, handle=post, bgr=bgr, strict=False, rule="libjpeg") for d in datas]
        for entropy in (None, "interval", "segmented"):
            frames, status = jpeg.decode_clip(datas, bgr=bgr, entropy=entropy, seg_bytes=16, handle=post, strict=False, rule="libjpeg")
            for f, (got, one, d) in enumerate(zip(frames, singles, datas)):
                assert np.array_equal(got, one) and np.array_equal(got, host(d, bgr)[0]), (f, entropy)
                assert status[f].tolist() == host(d, bgr)[1]
            assert status[2].tolist() == [_lib.EFORMAT, bad] and [int(s) for s in status[:, 0]].count(_lib.OK) == 4
    with pytest.raises(jpeg.DecodeError, match="frame 2"):
        jpeg.decode_clip(datas, handle=post, rule="libjpeg")
    # pitched destinations at every address modulo 4: nothing outside any frame's rows is written
    blocks, surfaces = [], []
    for f, d in enumerate(datas):
        i = _lib.jpeg_parse(d)
        block, view, pitch = guarded_rows(i.h, 3 * i.w, 3 + f, f % 4)
        s = _lib.SurfaceC()
        s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
        blocks.append((block, view, i))
        surfaces.append(s)
    status = post.op_jpeg_decode_clip_rule(datas, surfaces, True, -1, 128, "libjpeg")
    for (block, view, i), d, st in zip(blocks, datas, status):
        assert np.array_equal(view.reshape(i.h, i.w, 3), host(d, True)[0]) and untouched(block, view) and st.tolist() == host(d, True)[1]


def test_a_clip_enqueues_no_more_under_rule_1(post):
    datas = [stream(2, 70, 50), stream(1, 8, 33), DC.case("pil_444_17x17"), DC.case("pil_grey_17x17")]
    counts = {}
    for rule in ("own", "libjpeg"):
        before = post.jpeg_clip_counters()
        jpeg.decode_clip(datas, handle=post, rule=rule)
        after = post.jpeg_clip_counters()
        assert after["clips"] - before["clips"] == 1 and after["frames"] - before["frames"] == 4 and after["h2d"] - before["h2d"] == 1
        counts[rule] = after["enqueues"] - before["enqueues"]
    assert counts["libjpeg"] <= counts["own"], counts      # (the tight 4:2:0 BGR frame takes the frame kernel, not a launch of its own)


# ---- 4. the pipeline: begin_jpeg -------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("name", ["sample_001", "sample_012"])
def test_begin_jpeg_under_jpeg_rule_1_is_begin_of_the_libjpeg_frame(model, kw, name, bgr):
    """The committed stills through detect_heads and collect, bit for bit; the frame is Pillow's own (tests/test_jpeg_exact_cpu.py)."""
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    data = DC.case(name)
    frame = jpeg.decode_host(data, bgr=bgr, rule="libjpeg")
    assert np.array_equal(frame[..., ::-1] if bgr else frame, EC.pillow(data))
    with FramePipeline(model, depth=1, bgr=bgr) as fp:
        fp.begin(frame)
        want_input = fp.detector_input(kw["size"], as_uint8=True)
        fp.detect_heads(**kw)
        want = fp.collect(detections=True)
        fp.begin(jpeg.decode_host(data, bgr=bgr))
        own_input = fp.detector_input(kw["size"], as_uint8=True)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
        assert not np.array_equal(own_input, want_input)                   # the two rules give the detector different pixels
        # the option's default leaves begin_jpeg's bytes those of rule 0 ...
        st = fp.begin_jpeg(data)
        assert np.array_equal(fp.detector_input(kw["size"], as_uint8=True), own_input)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
        assert st.ok
        # ... an override for one frame gives rule 1 ...
        st = fp.begin_jpeg(data, rule="libjpeg")
        assert np.array_equal(fp.detector_input(kw["size"], as_uint8=True), want_input)
        fp.detect_heads(**kw)
        assert_same(fp.collect(detections=True), want)
        assert st.ok and st.interval == -1
        # ... and so does the option, for single frames and for clips, until it is set back
        model._handle.set_option("jpeg_rule", 1)
        try:
            st = fp.begin_jpeg(data)
            assert np.array_equal(fp.detector_input(kw["size"], as_uint8=True), want_input)
            fp.detect_heads(**kw)
            assert_same(fp.collect(detections=True), want)
            assert st.ok and st.interval == -1
            st = fp.begin_jpeg(data, rule="own")
            assert np.array_equal(fp.detector_input(kw["size"], as_uint8=True), own_input)
            fp.heads(np.zeros((0, 4), np.float32))
            fp.collect()
        finally:
            model._handle.set_option("jpeg_rule", 0)


def test_begin_clip_jpeg_follows_the_rule(model, kw):
    """A mixed clip (two sizes, two samplings): the annotated frames are the decoded frames with their overlay, byte for byte."""
    from tests.test_jpeg_clip_gpu import assert_same_clip, run_clip
    from whenet_hip.frames import FramePipeline
    datas = [stream(2, 70, 50), stream(1, 17, 17)]
    frames = [jpeg.decode_host(d, rule="libjpeg") for d in datas]
    assert not np.array_equal(frames[0], jpeg.decode_host(datas[0]))
    with FramePipeline(model, depth=1) as fp:
        want = run_clip(fp, fp.begin_clip_mixed, frames, kw)
        got = run_clip(fp, functools.partial(fp.begin_clip_jpeg, rule="libjpeg"), datas, kw)
        assert_same_clip(got, want)
        assert all(st.ok and st.interval == -1 for st in got[2])
        model._handle.set_option("jpeg_rule", 1)
        try:
            assert_same_clip(run_clip(fp, fp.begin_clip_jpeg, datas, kw), want)
        finally:
            model._handle.set_option("jpeg_rule", 0)
