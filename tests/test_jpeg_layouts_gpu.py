"""The JPEG decoder's LAYOUTS section on the GPU (csrc/jpeg_dec.hip: frame_group for luma hs = 4 and for 4:4:0 under rule 1, the
entropy kernels of both forms at up to 10 blocks per MCU; csrc/jpeg_prog.hip: the sequential scan kernel; the engine's calls with
the accept bits).  There is no tolerance anywhere: the kernels return the bytes and the status of the host statement
(`jpeg.decode_host(..., layouts=True)`), which tests/test_jpeg_layouts_cpu.py holds to the numpy statement and to executed Pillow.
Pitched destinations keep every byte outside the frame's rows.  Streams are made at test time (tests/jpeg_layout_cases.py); nothing
is larger than 65 x 65."""
import json
import os

import numpy as np
import pytest
import torch  # noqa: F401  (first, so there is exactly one HIP runtime in the process)

from tests import jpeg_layout_cases as LC
from tests import jpeg_orient_cases as OC
from tests.test_jpeg_decode_gpu import guarded_rows, untouched
from whenet_hip import _lib, jpeg

pytestmark = pytest.mark.gpu
RULES = ("own", "libjpeg")
OK = [_lib.OK, -1]
BOTH = _lib.JPEG_ACCEPT_PROGRESSIVE | _lib.JPEG_ACCEPT_LAYOUTS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


_REF = {}


def reference(data, rule="own", bgr=True, orient=False):
    """(frame, status) of the host statement with both accept bits: computed once per stream, shared, never modified"""
    key = (data, rule, bgr, orient)
    if key not in _REF:
        i = _lib.jpeg_parse_scans_accept(data, BOTH)[0]
        frame = np.empty((jpeg.oriented_shape(i.h, i.w, jpeg.orientation(data)) if orient else (i.h, i.w)) + (3,), np.uint8)
        status, _ = _lib.jpeg_decode_accept_host(data, jpeg.packed_surface(frame), bgr, rule, BOTH, orient)
        frame.setflags(write=False)
        _REF[key] = (frame, status)
    return _REF[key]


def surface_of(view, pitch):
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
    return s


def decode_guarded(h, data, k, rule="own", bgr=True, entropy=-1, seg_bytes=128, accept=BOTH, orient=False):
    """the kernels into a pitched destination between guard bytes: (frame, status, statistics)"""
    want, _ = reference(data, rule, bgr, orient)
    block, view, pitch = guarded_rows(want.shape[0], 3 * want.shape[1], 5 + k % 4, k % 4)
    status, stats, _ = h.op_jpeg_decode_accept(data, surface_of(view, pitch), bgr, entropy, seg_bytes, rule, accept, orient)
    assert untouched(block, view)
    return view.reshape(want.shape), status, stats


FORMS = ((0, 128), (1, 4), (1, 16))      # "interval", "segmented" with seg_bytes 4 and 16


# ---- 1. the kernels against the host statement: every new sampling, both rules, both orders, both entropy forms ---------------------
@pytest.mark.parametrize("sampling", list(LC.SAMPLINGS))
def test_the_kernels_are_the_host_statement_at_every_new_sampling(post, sampling):
    k = 0
    for h, w in LC.GPU_SHAPES:
        data = LC.single(LC._name(sampling, h, w))
        for rule in RULES:
            for bgr in (True, False):
                want, want_status = reference(data, rule, bgr)
                assert want_status.tolist() == OK
                for entropy, seg_bytes in FORMS:
                    k += 1
                    got, status, _ = decode_guarded(post, data, k, rule, bgr, entropy, seg_bytes, accept=_lib.JPEG_ACCEPT_LAYOUTS)
                    where = (sampling, h, w, rule, bgr, entropy, seg_bytes)
                    assert status.tolist() == OK, where
                    assert np.array_equal(got, want), where
        # the public function, which sizes the frame itself
        assert np.array_equal(jpeg.decode(data, handle=post, layouts=True), reference(data)[0])
        assert np.array_equal(jpeg.decode(data, handle=post, layouts=True, entropy="segmented", seg_bytes=8, rule="libjpeg", bgr=False),
                              reference(data, "libjpeg", False)[0])


def test_the_output_does_not_depend_on_the_lanes_of_the_segmented_form():
    for lanes in (16, 64):
        with _lib.Handle.postproc(0) as h:
            h.set_option("jpeg_seg_lanes", lanes)
            for k, sampling in enumerate(LC.SAMPLINGS):
                data = LC.single(LC._name(sampling, 33, 65))
                got, status, _ = decode_guarded(h, data, k, "libjpeg", True, 1, 4)
                assert status.tolist() == OK and np.array_equal(got, reference(data, "libjpeg")[0]), (lanes, sampling)


@pytest.mark.parametrize("name", LC.DAMAGED_NAMES)
def test_a_damaged_stream_keeps_its_status_and_its_defined_frame(post, name):
    data = LC.DAMAGED[name]
    for k, rule in enumerate(RULES):
        want, want_status = reference(data, rule)
        assert want_status[0] == LC.EFORMAT
        for entropy, seg_bytes in FORMS:
            got, status, _ = decode_guarded(post, data, k, rule, True, entropy, seg_bytes)
            assert status.tolist() == want_status.tolist(), (name, rule, entropy, seg_bytes)
            assert np.array_equal(got, want), (name, rule, entropy, seg_bytes)
    with pytest.raises(jpeg.DecodeError) as err:
        jpeg.decode(data, handle=post, layouts=True)
    assert err.value.interval == reference(data)[1][1] and np.array_equal(err.value.frame, reference(data)[0])


# ---- 2. the scan-plan path: SOF1, SOF2 with the new samplings, multi-scan sequential frames -----------------------------------------
@pytest.mark.parametrize("name", LC.SOF1_NAMES)
def test_a_sof1_stream_that_qualifies_takes_the_baseline_decoder(post, name):
    data = LC.sof1(name)
    before = post.jpeg_decode_counters()
    for k, rule in enumerate(RULES):
        got, status, _ = decode_guarded(post, data, k, rule, True, 0, 128)
        assert status.tolist() == OK and np.array_equal(got, reference(data, rule)[0]), (name, rule)
    got, status, _ = decode_guarded(post, data, 3, "own", False, 1, 16)
    assert status.tolist() == OK and np.array_equal(got, reference(data, "own", False)[0])
    after = post.jpeg_decode_counters()
    assert (after["interval"] - before["interval"], after["segmented"] - before["segmented"]) == (2, 1)


@pytest.mark.parametrize("name", [n for n in LC.SOF2_NAMES if "33x17" in n])
def test_a_sof2_stream_of_a_new_sampling(post, name):
    data = LC.sof2(name)
    for k, rule in enumerate(RULES):
        for bgr in (True, False):
            got, status, stats = decode_guarded(post, data, k, rule, bgr)
            assert status.tolist() == OK and np.array_equal(got, reference(data, rule, bgr)[0]), (name, rule, bgr)
    with pytest.raises(ValueError, match="progressive DCT"):      # the LAYOUTS bit alone does not accept SOF2
        decode_guarded(post, data, 0, accept=_lib.JPEG_ACCEPT_LAYOUTS)


NS2 = [("411", (0, 1)), ("440", (1, 2)), ("410", (0, 2)), ("420", (0, 1))]      # the SOF2 streams of the CPU file whose DC scans hold two components


@pytest.mark.parametrize("sampling,first", NS2)
def test_a_sof2_stream_whose_dc_scans_hold_two_components(post, sampling, first):
    """the general (component, block) loops of the DC first and DC refinement scans in the progressive scan kernel"""
    data = LC.sof2_ns2(sampling, 17, 33, first)
    scans = jpeg.info(data, progressive=True, layouts=True)["scans"]
    assert [s["components"] for s in scans[:4]] == [first, tuple(c for c in range(3) if c not in first)] * 2
    for k, rule in enumerate(RULES):
        for bgr in (True, False):
            want, want_status = reference(data, rule, bgr)
            got, status, stats = decode_guarded(post, data, k, rule, bgr)
            assert want_status.tolist() == OK and status.tolist() == OK and np.array_equal(got, want), (sampling, first, rule, bgr)
    # the same picture as the sequential stream of the same quantised blocks
    b, hs, vs = LC._blocks(sampling, 17, 33)
    assert np.array_equal(reference(data)[0], reference(LC.write(b, 17, 33, hs, vs))[0])
    # without the LAYOUTS bit: today's text, the first thing the parser meets (a new sampling in the SOF, else the two-component SOS)
    with pytest.raises(ValueError, match="a scan of two components" if sampling == "420" else "luma sampling must be"):
        decode_guarded(post, data, 0, accept=_lib.JPEG_ACCEPT_PROGRESSIVE)


@pytest.mark.parametrize("name", [n for n in LC.MULTI_NAMES if "33x17" in n] + LC.MULTI_DAMAGED_NAMES)      # (17 x 33: three MCU columns of 4:1:1)
def test_a_sequential_frame_of_several_scans_is_one_scan_kernel_launch(post, name):
    data = LC.multi(name)
    nscans = len(jpeg.info(data, layouts=True)["scans"])
    for k, rule in enumerate(RULES):
        want, want_status = reference(data, rule)
        before = post.jpeg_progressive_counters()
        got, status, stats = decode_guarded(post, data, k, rule, True, accept=_lib.JPEG_ACCEPT_LAYOUTS)
        after = post.jpeg_progressive_counters()
        assert status.tolist() == want_status.tolist(), (name, rule)
        assert np.array_equal(got, want), (name, rule)
        assert [after[key] - before[key] for key in ("decodes", "launches", "scans")] == [1, 1, nscans], name
        assert stats[1] == 1 and stats[2] == nscans and stats[3] == 1      # levels, scans, launches of the scan kernel
    assert (want_status[0] == LC.EFORMAT) == (name in LC.MULTI_DAMAGED_NAMES)


# ---- 3. a clip -----------------------------------------------------------------------------------------------------------------------
def the_clip():
    """16 frames: 4:2:0 baseline, the three new samplings, a three-scan 4:2:2, SOF1, a SOF2 4:4:0, a SOF2 with two-component DC scans,
    damaged ones"""
    return [LC.plain("420", 17, 33), LC.single("440_33x17"), LC.single("411_33x17"), LC.single("410_33x17"), LC.multi("422_33x17_y_cb_cr"),
            LC.sof1("440_33x17_sof1"), LC.sof2("440_33x17_minimal"), LC.DAMAGED["411_truncated"], LC.single("410_65x33"),
            LC.multi("440_33x17_cb_cr_y"), LC.multi("411_33x17_y_cbcr_ids23"), LC.MULTI_DAMAGED["truncated_in_scan_2"], LC.sof2_ns2("411", 17, 33, (0, 1)),
            LC.sof2("411_33x17_dri_changes"), LC.single("411_2x17"), LC.single("410_1x1")]


def test_a_clip_of_sixteen_mixed_streams(post):
    datas = the_clip()
    assert len(datas) == 16
    for rule in RULES:
        blocks, surfaces = [], []
        for f, d in enumerate(datas):
            want, _ = reference(d, rule)
            block, view, pitch = guarded_rows(want.shape[0], 3 * want.shape[1], 0 if f % 3 == 0 else 5 + f % 4, f % 4)
            blocks.append((block, view)), surfaces.append(surface_of(view, pitch))
        before = post.jpeg_progressive_counters()
        status, _ = post.op_jpeg_decode_clip_accept(datas, surfaces, True, -1, 128, rule, BOTH, False)
        after = post.jpeg_progressive_counters()
        for f, d in enumerate(datas):
            want, want_status = reference(d, rule)
            assert status[f].tolist() == want_status.tolist(), (rule, f)
            assert np.array_equal(blocks[f][1].reshape(want.shape), want), (rule, f)
            assert untouched(*blocks[f]), (rule, f)
        # the SOF2 frames' levels, and ONE launch of the sequential scan kernel for the four multi-scan frames together
        levels = max(max(s["level"] for s in jpeg.info(d, progressive=True, layouts=True)["scans"]) for d in (datas[6], datas[12], datas[13]))
        assert after["launches"] - before["launches"] == levels + 1 and after["decodes"] - before["decodes"] == 7
    frames, status = jpeg.decode_clip(datas, handle=post, progressive=True, layouts=True, strict=False)
    for f, d in enumerate(datas):
        assert np.array_equal(frames[f], reference(d)[0]) and status[f].tolist() == reference(d)[1].tolist(), f
    with pytest.raises(ValueError, match="frame 1: .*luma sampling must be"):      # without the argument: the first such frame
        jpeg.decode_clip(datas, handle=post, progressive=True)


# ---- 4. orientation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["440", "411"])
def test_the_oriented_kernels_inherit_both_rules(post, sampling):
    plain = LC.single(LC._name(sampling, 17, 33))
    k = 0
    for rule in RULES:
        u = jpeg.decode_host(plain, rule=rule, layouts=True)
        for v in (3, 6):
            data = OC.oriented(plain, v, where="soi")
            want, want_status = reference(data, rule, True, True)
            assert np.array_equal(want, OC.transform(u, v)) and want_status.tolist() == OK
            for entropy, seg_bytes in ((0, 128), (1, 16)):
                k += 1
                got, status, _ = decode_guarded(post, data, k, rule, True, entropy, seg_bytes, orient=True)
                assert status.tolist() == OK and np.array_equal(got, want), (sampling, rule, v, entropy)
            assert np.array_equal(jpeg.decode(data, handle=post, rule=rule, orient=True, layouts=True), want)


# ---- 5. the resident frame -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from tests.test_yuv_gpu import seeded_model
    m = seeded_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def kw():
    from tests.test_clip_gpu import kwargs
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        return kwargs(json.load(f)["detect"], "tiny", score=0.0)       # threshold 0: the seeded detector fires on small frames


def test_begin_jpeg_leaves_the_slot_that_begin_of_the_host_frame_leaves(model, kw):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    with FramePipeline(model, depth=1) as fp:
        fired = 0
        for data, extra in ((LC.single("411_65x33"), {}), (LC.single("440_65x33"), {}), (LC.single("410_65x33"), {}),
                            (LC.multi("422_33x17_y_cb_cr"), {}), (LC.sof2("440_33x17_minimal"), {"progressive": True}),
                            (LC.strip_dht(LC.annexk_411()), {"default_tables": True})):
            for rule in RULES:
                host = jpeg.decode_host(data, rule=rule, layouts=True, **extra)
                fp.begin(host)
                fp.detect_heads(**kw)
                want = fp.collect(detections=True)
                st = fp.begin_jpeg(data, rule=rule, layouts=True, **extra)
                fp.detect_heads(**kw)
                got = fp.collect(detections=True)
                assert_same(got, want)      # the detector's input, the windows, the crops' angles and logits: bit for bit
                assert (st.ok, st.interval) == (True, -1)
                fired += len(want[4])
        assert fired > 0
        with pytest.raises(ValueError, match="luma sampling must be"):
            fp.begin_jpeg(LC.single("411_65x33"))
        with pytest.raises(ValueError, match="missing Huffman table"):
            fp.begin_jpeg(LC.strip_dht(LC.annexk_411()), layouts=True)
        assert fp.in_flight == 0


def test_begin_clip_jpeg_leaves_the_slots_of_the_host_frames(model, kw):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    datas = [LC.single("411_33x17"), LC.single("440_33x17"), LC.multi("422_33x17_y_cb_cr"), LC.sof2("440_33x17_minimal"), LC.single("410_65x33"),
             LC.DAMAGED["411_truncated"]]
    with FramePipeline(model, depth=1) as fp:
        hosts = [jpeg.decode_host(d, progressive=True, layouts=True, strict=False) for d in datas]
        fp.begin_clip_mixed(hosts)
        fp.detect_heads_clip(**kw)
        want, wcount = fp.collect_clip(detections=True)
        sts = fp.begin_clip_jpeg(datas, progressive=True, layouts=True)
        fp.detect_heads_clip(**kw)
        got, gcount = fp.collect_clip(detections=True)
        assert gcount == wcount and len(got) == len(want) == len(datas)
        for g, w in zip(got, want):
            assert_same(g, w)
        assert [(s.ok, s.interval) for s in sts] == [(True, -1)] * 5 + [(False, int(reference(datas[5])[1][1]))]
        with pytest.raises(ValueError, match="frame 0: .*luma sampling must be"):
            fp.begin_clip_jpeg(datas, progressive=True)
        assert fp.in_flight == 0 and fp._begun_clip is None


# ---- 6. the defaults -------------------------------------------------------------------------------------------------------------------
def test_a_handle_with_its_defaults_refuses_every_stream_of_the_file_and_the_option_accepts_them():
    # every stream this file decodes anywhere: sequential ones, then the SOF2 ones
    streams = [LC.single(n) for n in LC.SINGLE_NAMES] + [LC.sof1(n) for n in LC.SOF1_NAMES] + [LC.multi(n) for n in LC.MULTI_NAMES if "33x17" in n]
    streams += [LC.multi(n) for n in LC.MULTI_DAMAGED_NAMES] + [LC.DAMAGED[n] for n in LC.DAMAGED_NAMES] + [LC.annexk_411()]
    streams += [OC.oriented(LC.single(LC._name(s, 17, 33)), v, where="soi") for s in ("440", "411") for v in (3, 6)]
    sof2 = [LC.sof2(n) for n in LC.SOF2_NAMES] + [LC.sof2_ns2(s, 17, 33, first) for s, first in NS2]
    old = LC.plain("420", 17, 33)
    with _lib.Handle.postproc(0) as h:
        before = jpeg.decode(old, handle=h)
        assert np.array_equal(before, jpeg.decode_host(old))
        for d in streams + sof2:
            i = _lib.jpeg_parse_scans_accept(d, BOTH)[0]
            frame = np.full((i.h, i.w, 3), 0xC3, np.uint8)
            for call in (lambda s: h.op_jpeg_decode_oriented(d, s, True), lambda s: h.op_jpeg_decode_accept(d, s, True),
                         lambda s: h.op_jpeg_decode_accept(d, s, True, accept=0), lambda s: h.op_jpeg_decode_accept(d, s, True, accept=1),
                         lambda s: h.op_jpeg_decode_clip_accept([old, d], [jpeg.packed_surface(np.empty_like(before)), s], True, accept=1)):
                with pytest.raises(ValueError, match="luma sampling must be|SOF1|several scans|SOF2|id above 1|two components"):
                    call(jpeg.packed_surface(frame))
                assert (frame == 0xC3).all()
        h.set_option("jpeg_layouts", 1)
        for d in streams:      # the option stands for the argument of the single-stream calls
            i = _lib.jpeg_parse_scans_accept(d, BOTH)[0]
            frame = np.empty((i.h, i.w, 3), np.uint8)
            status, _, _ = h.op_jpeg_decode_oriented(d, jpeg.packed_surface(frame), True, orient=False)
            assert status.tolist() == reference(d)[1].tolist() and np.array_equal(frame, reference(d)[0])
        for d in sof2:      # SOF2 needs its own option beside it
            i = _lib.jpeg_parse_scans_accept(d, BOTH)[0]
            frame = np.full((i.h, i.w, 3), 0xC3, np.uint8)
            with pytest.raises(ValueError, match="progressive DCT"):
                h.op_jpeg_decode_oriented(d, jpeg.packed_surface(frame), True, orient=False)
            assert (frame == 0xC3).all()
        h.set_option("jpeg_progressive", 1)
        for d in sof2:
            i = _lib.jpeg_parse_scans_accept(d, BOTH)[0]
            frame = np.empty((i.h, i.w, 3), np.uint8)
            status, _, _ = h.op_jpeg_decode_oriented(d, jpeg.packed_surface(frame), True, orient=False)
            assert status.tolist() == reference(d)[1].tolist() and np.array_equal(frame, reference(d)[0])
        assert np.array_equal(jpeg.decode(old, handle=h), before)      # a 4:2:0 stream's bytes are what they were
