"""Clips of JPEG streams on the GPU (csrc/jpeg_dec.hip, csrc/jpeg_dec_seg.hip: the clip kernels; Engine::clip_begin_jpeg,
Engine::op_jpeg_decode_clip): no tolerance anywhere.  Frame f of a clip is what the host statement `whenet_jpeg_decode_host` makes of
stream f alone -- bytes and status, in either entropy form, damaged streams included -- and a clip slot behaves as the slot
`begin_clip` / `begin_clip_mixed` leave for the decoded frames.  Every stream is a small one of tests/jpeg_decode_cases.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import jpeg_decode_cases as DC
from whenet_hip import _lib, jpeg

pytestmark = pytest.mark.gpu
GAP = 0xC3

MIXED = ["pil_420_50x70", "pil_422_50x70", "pil_444_q50", "pil_grey_50x70", "pil_420_rst_rows", "pil_444_rst_blocks3", "pil_420_optimize",
         "pil_grey_optimize", "pil_420_q10", "pil_444_q100", "own_17x17", "pil_grey_rst_blocks3", "pil_422_33x8", "pil_420_8x8",
         "pil_420_16x16", "pil_grey_1x1"]
CLIPS = {
    "one": ["pil_420_17x17"],
    "two": ["pil_420_50x70", "pil_444_17x17"],
    "one_by_one_between": ["pil_420_50x70", "pil_420_1x1", "pil_420_q50"],      # 70 x 50, one workgroup's worth, 70 x 50
    "sixteen_copies": ["pil_420_rst_rows"] * 16,
    "mixed": MIXED,
    "mixed_reversed": MIXED[::-1],
}
MODES = {"interval": (0, 128), "segmented_4": (1, 4), "segmented_8": (1, 8), "segmented_128": (1, 128), "auto": (-1, 128)}


def stream_of(name):
    return DC.DAMAGED[name]()[0] if name in DC.DAMAGED else DC.case(name)


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


_REF = {}


def reference(name):
    """(stream, frame, status) of the host statement: computed once, shared, never modified"""
    if name not in _REF:
        data = stream_of(name)
        i = _lib.jpeg_parse(data)
        frame = np.empty((i.h, i.w, 3), np.uint8)
        status = _lib.jpeg_decode_host(data, jpeg.packed_surface(frame), True)
        frame.setflags(write=False)
        _REF[name] = (data, frame, status)
    return _REF[name]


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


def decode_clip_guarded(post, names, entropy, seg_bytes, tight=()):
    """the clip into pitched destinations between guard bytes (frames in `tight`: at the tight pitch): every frame and status is the
    host statement's"""
    datas, blocks, surfaces = [], [], []
    for f, name in enumerate(names):
        data, want, _ = reference(name)
        h, w = want.shape[:2]
        block, view, pitch = guarded_rows(h, 3 * w, 0 if f in tight else 5 + f % 4, f % 4)
        s = _lib.SurfaceC()
        s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
        datas.append(data), blocks.append((block, view)), surfaces.append(s)
    status = post.op_jpeg_decode_clip(datas, surfaces, True, entropy, seg_bytes)
    for f, name in enumerate(names):
        _, want, want_status = reference(name)
        assert status[f].tolist() == want_status.tolist(), (f, name)
        assert np.array_equal(blocks[f][1].reshape(want.shape), want), (f, name)
        assert untouched(*blocks[f]), (f, name)
    return status


# ---- 1. decode_clip = decode_host per stream --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("clip", list(CLIPS))
def test_decode_clip_equals_decode_host_per_stream(post, clip, mode):
    names = CLIPS[clip]
    entropy, seg_bytes = MODES[mode]
    decode_clip_guarded(post, names, entropy, seg_bytes)
    decode_clip_guarded(post, names, entropy, seg_bytes, tight=range(0, len(names), 2))      # the plane kernel of the YUV ingest for some
    # the public function: tight frames
    frames, status = jpeg.decode_clip([reference(n)[0] for n in names], handle=post,
                                      entropy={0: "interval", 1: "segmented", -1: None}[entropy], seg_bytes=seg_bytes)
    for f, name in enumerate(names):
        assert np.array_equal(frames[f], reference(name)[1]) and status[f].tolist() == [_lib.OK, -1]
    rgb, _ = jpeg.decode_clip([reference(n)[0] for n in names[:3]], handle=post, bgr=False)
    for f, name in enumerate(names[:3]):
        assert np.array_equal(rgb[f][..., ::-1], reference(name)[1])


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
@pytest.mark.parametrize("mode", ["interval", "segmented_8"])
def test_decode_clip_into_i420_and_nv12_surfaces(post, fmt, mode):
    names = ["pil_420_50x70", "pil_420_1x1", "pil_420_rst_rows", "own_17x17", "pil_420_33x8"]
    entropy, seg_bytes = MODES[mode]
    datas, all_blocks, surfaces, wants = [], [], [], []
    for f, name in enumerate(names):
        data = stream_of(name)
        i = _lib.jpeg_parse(data)
        h, w, ch, cw = i.h, i.w, (i.h + 1) // 2, (i.w + 1) // 2
        geo = [(h, w, 3, 1), (ch, cw, 5, 2), (ch, cw, 2, 3)] if fmt == "i420" else [(h, w, 5, 3), (ch, 2 * cw, 3, 1)]
        blocks = [guarded_rows(*g) for g in geo]
        s = _lib.SurfaceC()
        for p, (_, view, pitch) in enumerate(blocks):
            s.plane[p], s.pitch[p] = view.ctypes.data, pitch
        s.format, s.matrix, s.on_device = (_lib.YUV_I420 if fmt == "i420" else _lib.YUV_NV12), _lib.YUV_JFIF, 0
        datas.append(data), all_blocks.append(blocks), surfaces.append(s), wants.append(jpeg.decode_planes_host(data))
    status = post.op_jpeg_decode_clip(datas, surfaces, True, entropy, seg_bytes)
    for f, (blocks, (planes, want_status)) in enumerate(zip(all_blocks, wants)):
        assert status[f].tolist() == want_status.tolist()
        assert np.array_equal(blocks[0][1], planes[0])
        if fmt == "i420":
            assert np.array_equal(blocks[1][1], planes[1]) and np.array_equal(blocks[2][1], planes[2])
        else:
            assert np.array_equal(blocks[1][1][:, 0::2], planes[1]) and np.array_equal(blocks[1][1][:, 1::2], planes[2])
        for block, view, _ in blocks:
            assert untouched(block, view), (f, fmt)


# ---- 2. both forms in one clip ----------------------------------------------------------------------------------------------------
def test_auto_puts_both_forms_into_one_clip():
    # auto takes the segmented form from 4096 bytes per interval on: the two camera stills (one interval of 21 KB and more) take form
    # 1, the small streams and the one with restart intervals form 0
    names = ["pil_420_50x70", "sample_001", "pil_420_rst_rows", "sample_012", "pil_grey_1x1"]
    datas = [reference(n)[0] for n in names]
    infos = [_lib.jpeg_parse(d) for d in datas]
    plan = _lib.jpeg_clip_plan(infos, [len(d) - i.data_offset for d, i in zip(datas, infos)], 2, 8)
    forms = [f["form"] for f in plan["frames"]]
    assert forms == [0, 1, 0, 1, 0]
    h = _lib.Handle.postproc(0)
    try:
        h.set_option("jpeg_seg_bytes", 8)
        before = h.jpeg_decode_counters()
        decode_clip_guarded(h, names, -1, 128)
        after = h.jpeg_decode_counters()
        assert after["interval"] - before["interval"] == forms.count(0) and after["segmented"] - before["segmented"] == forms.count(1)
    finally:
        h.close()


# ---- 3. damaged streams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["interval", "segmented_8"])
@pytest.mark.parametrize("name", DC.DAMAGED_NAMES)
def test_a_damaged_stream_keeps_to_its_own_frame(post, name, mode):
    entropy, seg_bytes = MODES[mode]
    clean = ["pil_420_50x70", "pil_444_q50", "pil_420_rst_rows", "pil_grey_50x70"]
    want_interval = DC.DAMAGED[name]()[1]
    for at in (0, 2, 4):
        names = clean[:at] + [name] + clean[at:]
        status = decode_clip_guarded(post, names, entropy, seg_bytes)      # (every frame against decode_host: the clean ones too)
        assert status[at].tolist() == [DC.EFORMAT, want_interval]
        assert [s.tolist() for k, s in enumerate(status) if k != at] == [[_lib.OK, -1]] * 4
    with pytest.raises(jpeg.DecodeError, match="frame 1") as err:
        jpeg.decode_clip([reference(clean[0])[0], reference(name)[0]], handle=post)
    assert err.value.interval == want_interval and np.array_equal(err.value.frame, reference(name)[1])


# ---- 4 .. 7: the pipeline ---------------------------------------------------------------------------------------------------------
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


def run_clip(fp, begin, clip, kw, annotate=True):
    """(collect_clip's result, the annotated frames) of a clip begun by `begin`"""
    sts = begin(clip)
    fp.detect_heads_clip(**kw)
    outs = [np.zeros(s + (3,), np.uint8) for s in fp._last_sizes] if annotate else None
    if annotate:
        fp.annotate_clip(outs, display="full")
    return fp.collect_clip(detections=True), outs, sts


def assert_same_clip(got, want):
    from tests.test_clip_gpu import assert_same
    (gf, gcount), gouts, _ = got
    (wf, wcount), wouts, _ = want
    assert gcount == wcount and len(gf) == len(wf)
    for g, w in zip(gf, wf):
        assert_same(g, w)
    if wouts is not None:
        for g, w in zip(gouts, wouts):
            assert g.tobytes() == w.tobytes()


def test_begin_clip_jpeg_is_begin_clip_of_the_decoded_frames(model, kw):
    from whenet_hip.frames import FramePipeline
    names = ["pil_420_50x70", "pil_422_50x70", "pil_420_rst_rows"]      # three streams of 70 x 50
    datas = [reference(n)[0] for n in names]
    frames = [jpeg.decode_host(d) for d in datas]
    with FramePipeline(model, depth=1) as fp:
        want = run_clip(fp, fp.begin_clip, frames, kw)
        sts = fp.begin_clip_jpeg(datas)
        with pytest.raises(ValueError, match="not collected"):
            sts[0].ok
        fp.detect_heads_clip(**kw)
        outs = [np.zeros_like(f) for f in frames]
        fp.annotate_clip(outs, display="full")
        got = (fp.collect_clip(detections=True), outs, sts)
        assert_same_clip(got, want)
        assert sum(len(t[4]) for t in got[0][0]) > 0                    # the detector fired: windows, angles and logits were compared
        assert all(st.ok and st.interval == -1 for st in sts)
        # the annotated clip as JPEG streams
        fp.begin_clip(frames)
        fp.detect_heads_clip(**kw)
        a = fp.annotate_clip_jpeg(quality=90)
        fp.collect_clip()
        fp.begin_clip_jpeg(datas)
        fp.detect_heads_clip(**kw)
        b = fp.annotate_clip_jpeg(quality=90)
        fp.collect_clip()
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b]
    with FramePipeline(model, depth=1, bgr=False) as fp:               # the other channel order
        rgb = [jpeg.decode_host(d, bgr=False) for d in datas]
        assert_same_clip(run_clip(fp, fp.begin_clip_jpeg, datas, kw), run_clip(fp, fp.begin_clip, rgb, kw))


def test_begin_clip_jpeg_is_begin_clip_mixed_of_the_decoded_frames(model, kw):
    from whenet_hip.frames import FramePipeline
    names = ["pil_444_17x17", "pil_420_33x8", "pil_420_50x70", "pil_420_16x16"]      # every frame after the first starts at an odd byte
    datas = [reference(n)[0] for n in names]
    frames = [jpeg.decode_host(d) for d in datas]
    assert [f.shape[:2] for f in frames] == [(17, 17), (8, 33), (70, 50), (16, 16)]
    with FramePipeline(model, depth=1) as fp:
        want = run_clip(fp, fp.begin_clip_mixed, frames, kw)
        got = run_clip(fp, fp.begin_clip_jpeg, datas, kw)
        assert_same_clip(got, want)
        assert all(st.ok for st in got[2])
        # no heads: the annotated frame is the slot's frame buffer, byte for byte
        fp.begin_clip_jpeg(datas)
        fp.detect_heads_clip(**dict(kw, score=2.0))
        outs = [np.zeros_like(f) for f in frames]
        fp.annotate_clip(outs)
        res, _ = fp.collect_clip(detections=True)
        assert all(len(t[4]) == 0 for t in res)
        for o, f in zip(outs, frames):
            assert np.array_equal(o, f)


def test_slots_are_reused_both_ways(model, kw):
    from tests.test_clip_gpu import assert_same
    from whenet_hip.frames import FramePipeline
    names = ["pil_420_50x70", "pil_444_17x17", "pil_420_rst_rows"]
    datas = [reference(n)[0] for n in names]
    frames = [jpeg.decode_host(d) for d in datas]
    big = np.ascontiguousarray(DC.picture(120, 160, seed=9)[..., ::-1])      # a raw frame larger than every frame of the clip
    with FramePipeline(model, depth=1) as fp:                 # ONE slot: a JPEG clip, a larger raw frame, a JPEG clip
        want = run_clip(fp, fp.begin_clip_mixed, frames, kw)
        fp.begin(big)
        fp.detect_heads(**kw)
        want_big = fp.collect(detections=True)
        for _ in range(2):
            assert_same_clip(run_clip(fp, fp.begin_clip_jpeg, datas, kw), want)
            fp.begin(big)
            fp.detect_heads(**kw)
            assert_same(fp.collect(detections=True), want_big)
        assert_same_clip(run_clip(fp, fp.begin_clip_jpeg, datas, kw), want)
    with FramePipeline(model, depth=2) as fp:                 # the slots cycling: a clip and a frame in flight side by side
        for _ in range(3):
            fp.begin_clip_jpeg(datas)
            fp.detect_heads_clip(**kw)
            fp.begin(big)
            fp.detect_heads(**kw)
            got = (fp.collect_clip(detections=True), None, None)
            assert_same(fp.collect(detections=True), want_big)
            assert_same_clip(got, (want[0], None, None))
            fp.begin(big)                                     # shifts the clip to the other slot next time round
            fp.detect_heads(**kw)
            assert_same(fp.collect(detections=True), want_big)


def test_refusals_take_no_slot(kw):
    from tests.test_yuv_gpu import seeded_model
    from whenet_hip.frames import FramePipeline
    good = reference("pil_420_50x70")[0]
    lib = _lib.load()

    def raw(h, datas, sizes=None):
        """whenet_clip_begin_jpeg itself: (return code, the error text)"""
        arrs = [np.frombuffer(d, np.uint8) for d in datas]
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        sz = np.array([a.size for a in arrs] if sizes is None else sizes, np.int64)
        status = np.zeros((max(len(arrs), 1), 2), np.int32)
        t = C.c_int(-1)
        rc = lib.whenet_clip_begin_jpeg(h._h, ptrs, sz.ctypes.data_as(C.c_void_p), len(arrs), _lib.BGR, C.byref(t),
                                        status.ctypes.data_as(C.c_void_p))
        return rc, lib.whenet_last_error(h._h).decode()

    def next_ticket(h):
        t = h.frame_begin_jpeg(good, np.zeros(2, np.int32))
        h.frame_heads(t, np.zeros((0, 4), np.int32))
        h.collect(t, 0)
        return t

    refused = DC.REFUSED["progressive"]()
    calls = (([], None, _lib.EINVAL, "1..16"), ([good] * 17, None, _lib.EINVAL, "1..16"),
             ([good, good], [len(good), 0], _lib.EINVAL, "frame 1"), ([good, good, refused, good], None, DC.EFORMAT, "frame 2"))
    m, twin = seeded_model(), seeded_model()                 # the twin sees the accepted submissions alone
    try:
        want = [next_ticket(twin._handle) for _ in range(len(calls) + 1)]
        got = [next_ticket(m._handle)]
        for datas, sizes, code, text in calls:
            for _ in range(_lib.MAX_INFLIGHT + 1):            # (a leak would use up the slots)
                rc, err = raw(m._handle, datas, sizes)
                assert rc == code and text in err, (rc, err)
            got.append(next_ticket(m._handle))                # the ticket it would have got without the refused calls
        assert got == want
        with pytest.raises(ValueError, match="frame 2.*progressive"):
            jpeg.decode_clip([good, good, refused, good], handle=m._handle)
        m._handle.set_option("letterbox_cache", 2)
        three_sizes = [reference(n)[0] for n in ("pil_420_50x70", "pil_444_17x17", "pil_420_16x16")]
        with FramePipeline(m, depth=1) as fp:
            for name, make in DC.REFUSED.items():
                with pytest.raises(ValueError, match="frame 2"):
                    fp.begin_clip_jpeg([good, good, make(), good])
            for _ in range(_lib.MAX_INFLIGHT + 1):
                with pytest.raises(ValueError, match="letterbox_cache"):
                    fp.begin_clip_jpeg(three_sizes)
            with pytest.raises(ValueError, match="1..16"):
                fp.begin_clip_jpeg([])
            with pytest.raises(ValueError, match="1..16"):
                fp.begin_clip_jpeg([good] * 17)
            assert fp.in_flight == 0 and fp._begun_clip is None
            (res, _), _, sts = run_clip(fp, fp.begin_clip_jpeg, three_sizes[:2], kw, annotate=False)      # two sizes fit
            assert len(res) == 2 and all(st.ok for st in sts)
            run_clip(fp, fp.begin_clip_jpeg, [good] * 3, kw, annotate=False)                              # one size needs no entry each
    finally:
        m.close()
        twin.close()


# ---- 8. the enqueues do not grow with the frame count -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["interval", "segmented_8"])
def test_enqueues_do_not_grow_with_the_frame_count(post, mode):
    entropy, seg_bytes = MODES[mode]
    deltas = []
    for F in (2, 16):
        before = post.jpeg_clip_counters()
        decode_clip_guarded(post, ["pil_420_rst_rows"] * F, entropy, seg_bytes)      # one stream repeated: the same forms and colour path
        after = post.jpeg_clip_counters()
        d = {k: after[k] - before[k] for k in after}
        assert d["clips"] == 1 and d["frames"] == F and d["h2d"] == 1
        deltas.append(d["enqueues"])
    print(f"{mode}: launches plus memsets per clip {deltas}")
    # one memset, scan, the entropy stage (one kernel, or the segmented form's six), idct, one colour kernel
    assert deltas[0] == deltas[1] == (5 if entropy == 0 else 10)
