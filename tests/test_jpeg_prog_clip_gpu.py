"""Progressive JPEG streams in clips on the GPU (csrc/jpeg_prog.hip: the clip forms of the scan and finish kernels;
Engine::clip_begin_jpeg / Engine::op_jpeg_decode_clip with progressive = 1): no tolerance anywhere.  Frame f of a clip is what the
host statement `jpeg.decode_host(datas[f], rule=..., progressive=True)` makes of stream f alone -- bytes and status --, whether the
stream is progressive, baseline or the clip a mix, damaged streams included; a refused stream takes no place; a clip slot behaves as
the slot `begin_clip` / `begin_clip_mixed` leave for the decoded frames; the launches follow the deepest frame, not the frame count.
Every stream comes from tests/jpeg_prog_cases.py or tests/jpeg_decode_cases.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import jpeg_decode_cases as DC
from tests import jpeg_prog_cases as PC
from whenet_hip import _lib, jpeg

pytestmark = pytest.mark.gpu
GAP = 0xC3

# 4:2:0 / 4:2:2 / 4:4:4 / grey at 1 x 1, 9 x 7, 17 x 17, 35 x 50 with 3-block intervals and 64 x 48 with row intervals
SINGLES = ["pil_420_1x1_q75_nodri", "pil_grey_1x1_q75_nodri", "pil_444_9x7_q75_nodri", "pil_422_9x7_q75_blocks3", "pil_420_17x17_q75_nodri",
           "pil_422_17x17_q95_blocks3", "pil_grey_17x17_q30_nodri", "pil_420_35x50_q75_blocks3", "pil_444_35x50_q100_blocks3",
           "pil_grey_35x50_q75_blocks3", "pil_420_64x48_q75_rows1", "pil_422_64x48_q75_rows1", "pil_444_64x48_q75_rows1"]
SIXTEEN_SIZES = ["pil_420_1x1_q75_nodri", "pil_444_8x8_q75_blocks3", "pil_422_9x7_q75_rows1", "pil_grey_17x17_q95_blocks3",
                 "pil_420_33x18_q75_rows1", "pil_444_35x50_q30_nodri", "pil_422_64x48_q75_blocks3", "pil_grey_1x1_q75_rows1",
                 "pil_420_8x8_q75_nodri", "pil_444_9x7_q75_blocks3", "pil_422_17x17_q100_nodri", "pil_grey_33x18_q75_blocks3",
                 "pil_420_35x50_q95_blocks3", "pil_444_64x48_q75_nodri", "pil_422_35x50_q75_rows1", "pil_grey_64x48_q75_blocks3"]
RULES = ("own", "libjpeg")


def stream_of(name):
    if name.startswith("twin:"):
        return PC.pillow_twin(name[5:])
    if name in PC.PILLOW:
        return PC.pillow_case(name)
    if name in PC.CONSTRUCTED_NAMES:
        return PC.constructed(name)
    if name in PC.DAMAGED:
        return PC.DAMAGED[name]
    if name == "grey_17_intervals":
        return grey_17_intervals()
    return DC.case(name)


def grey_17_intervals():
    """56 x 56 grey with 3-block intervals: 49 blocks, so every scan has 17 intervals -- two workgroups of the padded lists.  (17
    intervals do not occur up to 64 x 48: a scan has at most 8 x 6 units there, and 17 r - j, j < r, is 17 for r = 1, 33 or 34 for
    r = 2, 49..51 for r = 3 and above 48 from r = 4 on; none of 17, 33, 34 is a product a x b with a <= 8 and b <= 6.)"""
    return PC.pillow_stream(56, 56, "grey", 75, restart_marker_blocks=3)


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


_REF = {}


def reference(name, rule="own", bgr=True):
    """(stream, frame, status) of the host statement: computed once, shared, never modified"""
    key = (name, rule, bgr)
    if key not in _REF:
        data = stream_of(name)
        i = _lib.jpeg_parse_scans(data)[0]
        frame = np.empty((i.h, i.w, 3), np.uint8)
        status = _lib.jpeg_decode_progressive_host(data, jpeg.packed_surface(frame), bgr, rule)
        assert np.array_equal(frame, jpeg.decode_host(data, bgr=bgr, strict=False, rule=rule, progressive=True))      # (the public name of it)
        frame.setflags(write=False)
        _REF[key] = (data, frame, status)
    return _REF[key]


def guarded_rows(rows, row_bytes, extra, shift):
    pitch = row_bytes + extra
    block = np.full(shift + rows * pitch + 16, GAP, np.uint8)
    view = np.lib.stride_tricks.as_strided(block[shift:], (rows, row_bytes), (pitch, 1))
    return block, view, pitch


def untouched(block, view):
    mask = np.ones(block.size, bool)
    start = view.ctypes.data - block.ctypes.data
    for r in range(view.shape[0]):
        mask[start + r * view.strides[0]:start + r * view.strides[0] + view.shape[1]] = False
    return bool((block[mask] == GAP).all())


def decode_clip_guarded(h, names, rule="own", bgr=True, entropy=-1, seg_bytes=128, tight=()):
    """the clip into pitched destinations between guard bytes (frames in `tight`: at the tight pitch): every frame and status is the
    host statement's.  Returns the status words."""
    datas, blocks, surfaces = [], [], []
    for f, name in enumerate(names):
        data, want, _ = reference(name, rule, bgr)
        hh, ww = want.shape[:2]
        block, view, pitch = guarded_rows(hh, 3 * ww, 0 if f in tight else 5 + f % 4, f % 4)
        s = _lib.SurfaceC()
        s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
        datas.append(data), blocks.append((block, view)), surfaces.append(s)
    status = h.op_jpeg_decode_clip_progressive(datas, surfaces, bgr, entropy, seg_bytes, rule)
    for f, name in enumerate(names):
        _, want, want_status = reference(name, rule, bgr)
        assert status[f].tolist() == want_status.tolist(), (f, name)
        assert np.array_equal(blocks[f][1].reshape(want.shape), want), (f, name)
        assert untouched(*blocks[f]), (f, name)
    return status


def counters(h):
    return dict(h.jpeg_clip_counters(), **{"p_" + k: v for k, v in h.jpeg_progressive_counters().items()})


def delta(h, before):
    after = counters(h)
    return {k: after[k] - before[k] for k in after}


# ---- 1. a clip of one ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLES)
def test_a_clip_of_one_progressive_stream(post, name):
    for rule in RULES:
        for bgr in (True, False):
            status = decode_clip_guarded(post, [name], rule, bgr)
            assert status[0].tolist() == [_lib.OK, -1]
    decode_clip_guarded(post, [name], tight=[0])
    frames, status = jpeg.decode_clip([stream_of(name)], handle=post, progressive=True, rule="libjpeg", bgr=False)
    assert np.array_equal(frames[0], reference(name, "libjpeg", False)[1]) and status.tolist() == [[_lib.OK, -1]]


# ---- 2. mixed clips: where the grid arithmetic can go wrong ---------------------------------------------------------------------
MIXED_A = ["pil_420_35x50_q75_blocks3", "twin:pil_422_35x50_q75_blocks3", "levels14_420_17x17_ranked", "twin:pil_444_64x48_q75_rows1",
           "pil_grey_1x1_q75_nodri"]


@pytest.mark.parametrize("rule", RULES)
def test_frames_drop_out_of_later_launches_and_baseline_frames_sit_between(post, rule):
    """(a) a 3-level Pillow stream, a baseline stream, the 14-level script, a baseline stream, grey 1 x 1 progressive: launches 3..13
    have one live frame between frames without workgroups.  Once with the baseline frames in form 0, once forced segmented with
    seg_bytes = 16."""
    levels = [max(s["level"] for s in jpeg.info(stream_of(n), progressive=True)["scans"]) for n in MIXED_A]
    assert levels == [3, 1, 14, 1, 3]
    for entropy, seg_bytes in ((0, 128), (1, 16)):
        before = counters(post)
        decode_clip_guarded(post, MIXED_A, rule, entropy=entropy, seg_bytes=seg_bytes, tight=[0, 1] if entropy else ())
        d = delta(post, before)
        nscans = [len(jpeg.info(stream_of(n), progressive=True)["scans"]) for n in (MIXED_A[0], MIXED_A[2], MIXED_A[4])]
        assert (d["clips"], d["frames"], d["h2d"]) == (1, 5, 1)
        assert (d["p_decodes"], d["p_launches"], d["p_scans"]) == (3, 14, sum(nscans))      # the largest level count, not 3 + 14 + 3
    # the same clip in the order that puts the deepest frame last and first
    decode_clip_guarded(post, MIXED_A[::-1], rule)
    decode_clip_guarded(post, [MIXED_A[2]] + MIXED_A[:2] + MIXED_A[3:], rule)


def test_a_baseline_frame_keeps_the_form_the_options_pick(post):
    """auto on a handle with jpeg_seg_bytes = 16: the camera still takes the segmented form, the small baseline stream form 0, in one
    clip with progressive frames"""
    names = [MIXED_A[0], "sample_001", MIXED_A[2], "twin:pil_422_35x50_q75_blocks3", MIXED_A[4]]
    plan = _lib.jpeg_clip_plan_progressive([stream_of(n) for n in names], 2, 16)
    assert [f["form"] for f in plan["frames"]] == [2, 1, 2, 0, 2]
    h = _lib.Handle.postproc(0)
    try:
        h.set_option("jpeg_seg_bytes", 16)
        before, forms = counters(h), h.jpeg_decode_counters()
        decode_clip_guarded(h, names)
        after = h.jpeg_decode_counters()
        assert (after["interval"] - forms["interval"], after["segmented"] - forms["segmented"]) == (1, 1)
        assert delta(h, before)["p_decodes"] == 3
    finally:
        h.close()


def test_sixteen_progressive_frames_of_different_sizes(post):
    assert len({reference(n)[1].shape for n in SIXTEEN_SIZES}) == 7
    for rule in RULES:
        decode_clip_guarded(post, SIXTEEN_SIZES, rule)
    decode_clip_guarded(post, SIXTEEN_SIZES[::-1], bgr=False, tight=range(0, 16, 2))


def test_sixteen_copies_of_one_stream(post):
    for name in ("pil_420_64x48_q75_rows1", "levels14_grey_9x7_fixed"):
        decode_clip_guarded(post, [name] * 16)
        decode_clip_guarded(post, [name] * 16, "libjpeg", tight=range(16))


def test_sixteen_items_next_to_seventeen(post):
    """(d) the padded lists at the workgroup boundary: the luma AC scans of 64 x 48 4:2:0 with 3-block intervals have 48 / 3 = 16
    items -- one workgroup, no padding --, the scans of `grey_17_intervals` 17 -- two workgroups --, 64 x 48 grey with row intervals 6"""
    def intervals(name):
        return [s["intervals"] for s in jpeg.info(stream_of(name), progressive=True)["scans"]]

    sixteen, seventeen, six = "pil_420_64x48_q75_blocks3", "grey_17_intervals", "pil_grey_64x48_q75_rows1"
    assert 16 in intervals(sixteen) and set(intervals(seventeen)) == {17} and set(intervals(six)) == {6}
    lists = _lib.jpeg_clip_plan_progressive([stream_of(n) for n in (sixteen, seventeen, six)])["frames"]
    assert lists[1]["list"] == 32 * lists[1]["nscans"] and lists[2]["list"] == 16 * lists[2]["nscans"]
    assert lists[0]["list"] == 16 * lists[0]["nscans"]                   # (4 or 16 intervals per scan: one workgroup each)
    for names in ([sixteen, seventeen], [seventeen, sixteen], [sixteen, seventeen, six, seventeen, sixteen]):
        for rule in RULES:
            decode_clip_guarded(post, names, rule)


# ---- 3. damaged streams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.DAMAGED_NAMES)
def test_a_damaged_stream_damages_its_own_frame_only(post, name):
    clean = ["pil_422_35x50_q75_blocks3", "twin:pil_420_17x17_q75_nodri", "pil_444_17x17_q75_blocks3"]
    names = clean[:2] + [name] + clean[2:]
    for rule in RULES:
        status = decode_clip_guarded(post, names, rule)                  # (every frame against the host statement: the clean ones too)
        want = reference(name, rule)[2]
        assert want[0] == PC.EFORMAT and status[2].tolist() == want.tolist()
        assert [s.tolist() for k, s in enumerate(status) if k != 2] == [[_lib.OK, -1]] * 3
    with pytest.raises(jpeg.DecodeError, match="frame 2") as err:
        jpeg.decode_clip([stream_of(n) for n in names], handle=post, progressive=True)
    assert err.value.interval == int(reference(name)[2][1]) and np.array_equal(err.value.frame, reference(name)[1])


# ---- 4. refused streams take no place -------------------------------------------------------------------------------------------
def test_refused_streams_take_no_slot_and_write_nothing():
    from tests.test_yuv_gpu import seeded_model
    good, base = stream_of("pil_420_17x17_q75_nodri"), stream_of("twin:pil_420_17x17_q75_nodri")
    lib = _lib.load()

    def raw(h, datas):
        """whenet_clip_begin_jpeg_progressive itself: (return code, the error text, the ticket and the status words it left)"""
        arrs = [np.frombuffer(d, np.uint8) for d in datas]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        sz = np.array([a.size for a in arrs], np.int64)
        status = np.full((len(arrs), 2), 77, np.int32)
        t = C.c_int(-5)
        rc = lib.whenet_clip_begin_jpeg_progressive(h._h, ptrs, sz.ctypes.data_as(C.c_void_p), len(arrs), _lib.BGR, 0, C.byref(t),
                                                    status.ctypes.data_as(C.c_void_p))
        return rc, lib.whenet_last_error(h._h).decode(), t.value, status

    def next_ticket(h):
        t = h.frame_begin_jpeg(good, np.zeros(2, np.int32), progressive=True)
        h.frame_heads(t, np.zeros((0, 4), np.int32))
        h.collect(t, 0)
        return t

    m, twin = seeded_model(), seeded_model()                 # the twin sees the accepted submissions alone
    try:
        want = [next_ticket(twin._handle) for _ in range(len(PC.REFUSED) + 1)]
        got = [next_ticket(m._handle)]
        for name, bad in PC.REFUSED.items():
            with pytest.raises(ValueError) as why:
                jpeg.info(bad, progressive=True)
            reason = str(why.value).split("jpeg_parse_scans: ", 1)[-1]
            for _ in range(_lib.MAX_INFLIGHT + 1):            # (a leak would use up the slots)
                rc, err, ticket, status = raw(m._handle, [good, base, bad, good])
                assert rc == PC.EFORMAT and f"frame 2: {reason}" in err, (name, rc, err)
                assert ticket == -5 and (status == 77).all(), name      # nothing is written
            got.append(next_ticket(m._handle))                # the ticket it would have got without the refused calls
        assert got == want
        before = counters(m._handle)
        with pytest.raises(ValueError, match="frame 2"):
            m._handle.op_jpeg_decode_clip_progressive([good, base, PC.REFUSED["ns_2"], good], [jpeg.packed_surface(np.zeros((17, 17, 3), np.uint8))] * 4,
                                                      True)
        assert delta(m._handle, before) == {k: 0 for k in before}       # refused before anything was counted or enqueued
    finally:
        m.close()
        twin.close()


# ---- 5. the pipeline ------------------------------------------------------------------------------------------------------------
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


def run_clip(fp, begin, clip, kw, **begin_kw):
    """(collect_clip's result, the annotated frames, what begin returned) of a clip begun by `begin`"""
    sts = begin(clip, **begin_kw)
    fp.detect_heads_clip(**kw)
    outs = [np.zeros(s + (3,), np.uint8) for s in fp._last_sizes]
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
        assert g.tobytes() == w.tobytes()


@pytest.mark.parametrize("rule", RULES)
def test_begin_clip_jpeg_progressive_is_begin_clip_of_the_decoded_frames(model, kw, rule):
    from whenet_hip.frames import FramePipeline
    names = ["pil_420_35x50_q75_blocks3", "twin:pil_422_35x50_q75_blocks3", "pil_444_35x50_q75_nodri", "truncated_in_scan_6"]      # 35 x 50 all
    datas = [stream_of(n) for n in names]
    for bgr in (True, False):
        frames = [np.array(reference(n, rule, bgr)[1]) for n in names]
        with FramePipeline(model, depth=1, bgr=bgr) as fp:
            want = run_clip(fp, fp.begin_clip, frames, kw)
            got = run_clip(fp, fp.begin_clip_jpeg, datas, kw, progressive=True, rule=rule)
            assert_same_clip(got, want)
            assert sum(len(t[4]) for t in got[0][0]) > 0                # the detector fired: windows, angles and logits were compared
            sts = got[2]
            assert [st.ok for st in sts] == [True, True, True, False]
            assert sts[3].interval == int(reference(names[3], rule, bgr)[2][1])


def test_begin_clip_jpeg_progressive_is_begin_clip_mixed_of_the_decoded_frames(model, kw):
    from whenet_hip.frames import FramePipeline
    names = ["pil_444_17x17_q75_nodri", "twin:pil_420_33x18_q75_rows1", "pil_420_35x50_q75_blocks3", "levels14_grey_9x7_ranked"]
    datas = [stream_of(n) for n in names]
    frames = [np.array(reference(n)[1]) for n in names]
    assert [f.shape[:2] for f in frames] == [(17, 17), (18, 33), (50, 35), (7, 9)]      # every frame after the first starts at an odd byte
    with FramePipeline(model, depth=1) as fp:
        want = run_clip(fp, fp.begin_clip_mixed, frames, kw)
        for _ in range(2):                                               # (the slot's buffers reused)
            got = run_clip(fp, fp.begin_clip_jpeg, datas, kw, progressive=True)
            assert_same_clip(got, want)
            assert all(st.ok and st.interval == -1 for st in got[2])
        with pytest.raises(ValueError, match="frame 0.*progressive"):   # without the flag the clip is refused and takes no place
            fp.begin_clip_jpeg(datas)
        assert fp.in_flight == 0 and fp._begun_clip is None


# ---- 6. counters ----------------------------------------------------------------------------------------------------------------
def test_the_launches_follow_the_levels_not_the_frame_count(post):
    name = "pil_444_35x50_q75_blocks3"
    data = stream_of(name)
    plan = _lib.jpeg_clip_plan_progressive([data])
    nscans, levels = plan["frames"][0]["nscans"], plan["scan_launches"]
    assert levels == max(s["level"] for s in jpeg.info(data, progressive=True)["scans"]) == plan["frames"][0]["levels"]
    # one memset; a scan launch per level; the finish; the inverse DCT; one colour kernel (4:4:4: the frame kernel) -- no marker
    # scan, no entropy launch: the clip holds no baseline frame
    want = 1 + levels + 1 + 1 + 1
    for F in (1, 16):
        assert _lib.jpeg_clip_plan_progressive([data] * F)["scan_launches"] == levels
        before, forms = counters(post), post.jpeg_decode_counters()
        decode_clip_guarded(post, [name] * F)
        d = delta(post, before)
        print(f"F = {F}: {d}")
        assert (d["clips"], d["frames"], d["h2d"]) == (1, F, 1)
        assert d["enqueues"] == want
        assert (d["p_decodes"], d["p_launches"], d["p_scans"]) == (F, levels, F * nscans)
        assert post.jpeg_decode_counters() == forms                      # no baseline decode was counted


# ---- 7. defaults ----------------------------------------------------------------------------------------------------------------
def test_without_the_flag_nothing_changes():
    prog = stream_of("pil_420_17x17_q75_nodri")
    names = ["pil_420_50x70", "pil_444_q50", "pil_grey_rst_blocks3", "pil_420_rst_rows"]
    datas = [DC.case(n) for n in names]
    h = _lib.Handle.postproc(0)
    try:
        for option in (0, 1):                                            # clips ignore the option
            h.set_option("jpeg_progressive", option)
            with pytest.raises(ValueError, match="frame 0.*progressive"):
                jpeg.decode_clip([prog], handle=h)
            surf = [jpeg.packed_surface(np.zeros((17, 17, 3), np.uint8))]
            with pytest.raises(ValueError, match="frame 0.*progressive"):
                h.op_jpeg_decode_clip([prog], surf, True)
            with pytest.raises(ValueError, match="frame 0.*progressive"):
                h.op_jpeg_decode_clip_rule([prog], surf, True, rule="libjpeg")
        # a clip of baseline streams through the new call: the bytes and statuses of the old call, the same launches, no progressive count
        for rule in RULES:
            for entropy, seg_bytes in ((None, None), ("interval", None), ("segmented", 8)):
                before = counters(h)
                old, old_status = jpeg.decode_clip(datas, handle=h, rule=rule, entropy=entropy, seg_bytes=seg_bytes)
                mid = delta(h, before)
                new, new_status = jpeg.decode_clip(datas, handle=h, rule=rule, entropy=entropy, seg_bytes=seg_bytes, progressive=True)
                d = delta(h, before)
                assert all(np.array_equal(a, b) for a, b in zip(old, new)) and np.array_equal(old_status, new_status)
                assert d["enqueues"] == 2 * mid["enqueues"] and d["clips"] == 2 and d["h2d"] == 2
                assert (d["p_decodes"], d["p_launches"], d["p_scans"]) == (0, 0, 0)
    finally:
        h.close()
