"""Mixed clips on the GPU: frames of DIFFERENT sizes as one submission (begin_clip_mixed -> detect_heads_clip -> collect_clip; the
mixed kernels of csrc/letterbox.hip, csrc/yolo.hip, csrc/headplan.hip and csrc/frame.hip, Engine::clip_begin_mixed and the
letterbox geometry cache of csrc/engine_post.cpp).  The contract is bitwise and has no tolerance: frame f of a mixed clip returns
the bytes that begin; detect_heads; collect returns for that frame alone, every stage alone equals its single-frame form, and a
set of sizes that the cache holds costs no miss and no wait."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import detector_cases as DC
from tests.test_clip_gpu import assert_same, assert_slots_equal_frame, hargs, kwargs, seeded_maps
from whenet_hip import _lib, detector_weights as DW
from whenet_hip.frames import FramePipeline

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def detect_args():
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        return json.load(f)["detect"]


def seeded_model(name, kind):
    import whenet
    m = whenet.WHENet(dtype="f16")
    m._handle.detector_load(DW.pack(DW.synthetic(kind, DC.SEEDS[name])))
    return m


@pytest.fixture(scope="module")
def models():
    """One seeded f16 WHENet per detector body, the seeded detector attached to its handle (as tests/test_clip_gpu.py)."""
    ms = {name: seeded_model(name, kind) for name, kind in DC.KINDS}
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def tagged():
    """The frames of the issue's table, cut from the two committed sample frames."""
    f0, f1 = DC.sample_frame(0), DC.sample_frame(1)
    assert f0.shape == (224, 528, 3) and f1.shape == (226, 548, 3)
    cut = dict(A=f0, B=f1, C=f0[::2, ::2], D=f1[:, 100:327], E=f0[60:157, 200:331], G=np.rot90(f0), T=f1[40:190, 250:290])
    frames = {k: np.ascontiguousarray(v) for k, v in cut.items()}
    assert [frames[k].shape[:2] for k in "CDEGT"] == [(112, 264), (226, 227), (97, 131), (528, 224), (150, 40)]
    assert (97 * 131 * 3) % 16 != 0 and (131 * 3) % 16 != 0          # E: odd pitch, and the frame behind it starts unaligned
    return frames


@pytest.fixture(scope="module")
def single(models, detect_args):
    """The single-frame path of (detector, frame), computed once per pair and shared: `eight` = begin; detect_heads;
    collect(detections=True) at depth 1, `slots` = the same submission through the handle with argmax and logits."""
    memo = {}

    def get(name, frame):
        key = (name, frame.shape, frame.tobytes())
        if key not in memo:
            kw = kwargs(detect_args, name)
            h = models[name]._handle
            with FramePipeline(models[name], depth=1) as fp:
                fp.begin(frame)
                fp.detect_heads(**kw)
                eight = fp.collect(detections=True)
                t = h.frame_begin(frame)
                slots = h.collect_detect(t, h.frame_detect_heads(t, *hargs(kw)), want_logits=True)
            memo[key] = (eight, slots)
        return memo[key]

    return get


def run_mixed(fp, frames, kw, max_heads=None):
    fp.begin_clip_mixed(frames)
    fp.detect_heads_clip(max_heads=max_heads, **kw)
    return fp.collect_clip(detections=True)


def handle_mixed(h, frames, kw, max_heads=None):
    t = h.clip_begin_mixed(frames)
    k = h.clip_detect_heads(t, *hargs(kw), max_heads=max_heads)
    return h.collect_clip(t, len(frames), k, want_logits=True)


def assert_clip_is_per_frame(name, frames, clip, single):
    """Every frame's eight arrays against its single-frame submission; prints and returns (detections, heads with a window)."""
    got, (rows_used, overflow) = clip
    assert len(got) == len(frames)
    for g, frame in zip(got, frames):
        assert len(g) == 8
        assert_same(g, single(name, frame)[0])
    counts = [len(t[4]) for t in got]
    heads = [int((t[7] != 0).sum()) for t in got]
    print(f"{name}: sizes {[f.shape[:2] for f in frames]}, detections per frame {counts}, with a window {heads}, "
          f"rows_used {rows_used}, overflow {overflow}")
    assert overflow == 0 and rows_used == sum(heads)
    return counts, heads


# ---- 1. mixed clip = per-frame path, bitwise ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_mixed_clip_is_bitwise_the_per_frame_path(models, detect_args, tagged, single, name, kind):
    kw = kwargs(detect_args, name)
    frames = [tagged[k] for k in "EATB"]
    F, K = len(frames), kw["max_boxes"]
    with FramePipeline(models[name], depth=1) as fp:
        clip = run_mixed(fp, frames, kw, max_heads=F * K)
    counts, heads = assert_clip_is_per_frame(name, frames, clip, single)
    assert min(heads) >= 1 and sum(heads) >= 8
    got = clip[0]
    assert any(got[i][4].tobytes() != got[j][4].tobytes() for i in range(F) for j in range(i))       # not one frame four times
    # the slot arrays through the handle, argmax and logits included
    res = handle_mixed(models[name]._handle, frames, kw, max_heads=F * K)
    assert res[-2:] == clip[1]
    for f in range(F):
        slots = single(name, frames[f])[1]
        assert_slots_equal_frame(res, f, slots, slots[4] != 0)
    live = np.flatnonzero((res[6] >= 0).reshape(-1))
    assert res[6].reshape(-1)[live].tolist() == list(range(clip[1][0]))              # rows in (frame, detection) order


# ---- 2. frames of one size through the mixed entry point ---------------------------------------------------------------------
def test_same_sizes_equal_the_uniform_clip(models, detect_args, tagged):
    name = "tiny"
    kw = kwargs(detect_args, name)
    a = tagged["A"]
    frames = [np.ascontiguousarray(v) for v in (a, a[::-1], a[:, ::-1])]
    h = models[name]._handle
    t = h.clip_begin(np.stack(frames))
    want = h.collect_clip(t, 3, h.clip_detect_heads(t, *hargs(kw)), want_logits=True)
    got = handle_mixed(h, frames, kw)
    assert len(got) == len(want) == 12
    for g, w in zip(got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
        else:
            assert g == w
    assert want[-2] >= 3


# ---- 3. sixteen distinct sizes -----------------------------------------------------------------------------------------------
def test_sixteen_distinct_sizes(models, detect_args, tagged, single):
    name = "tiny"
    kw = kwargs(detect_args, name)
    f0 = tagged["A"]
    frames = [np.ascontiguousarray(f0[:224 - 3 * i, :528 - 5 * i]) for i in range(16)]
    assert len({f.shape for f in frames}) == 16
    with FramePipeline(models[name], depth=1) as fp:
        clip = run_mixed(fp, frames, kw, max_heads=256)
    counts, heads = assert_clip_is_per_frame(name, frames, clip, single)
    assert sum(heads) >= 16


# ---- 4. overflow across sizes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_overflow_across_sizes(models, detect_args, tagged, single, name, kind):
    kw = kwargs(detect_args, name)
    frames = [tagged[k] for k in "GED"]
    F = len(frames)
    slots = [single(name, f)[1] for f in frames]
    valid = [s[4] != 0 for s in slots]
    total = int(sum(v.sum() for v in valid))
    print(f"{name}: heads with a window per frame {[int(v.sum()) for v in valid]}")
    assert total >= 3
    h = models[name]._handle
    for max_heads in (1, total - 1):
        res = handle_mixed(h, frames, kw, max_heads=max_heads)
        assert res[-2:] == (max_heads, total - max_heads)
        seen = 0
        for f in range(F):
            order = seen + np.cumsum(valid[f]) - 1                                   # number of each head in (frame, detection) order
            assert_slots_equal_frame(res, f, slots[f], valid[f] & (order < max_heads))
            seen += int(valid[f].sum())


# ---- 5. the mixed letterbox alone --------------------------------------------------------------------------------------------
def letterbox_cases(tagged):
    a = tagged["A"]
    return [([tagged[k] for k in "ETA"], (64, 96)),
            ([tagged[k] for k in "TD"], (64, 64)),
            ([np.ascontiguousarray(a[:3, :5]), np.ascontiguousarray(a[100:101, 200:201]), tagged["C"]], (32, 32))]


@pytest.mark.parametrize("case", range(3))
def test_mixed_letterbox_equals_the_single_frame_letterbox(post, tagged, case):
    frames, size = letterbox_cases(tagged)[case]
    if case == 2:
        assert frames[0].shape == (3, 5, 3) and frames[1].shape == (1, 1, 3)       # rows shorter than one 16-byte chunk
    F = len(frames)
    u8, f32 = post.op_letterbox_mixed(frames, size)
    assert u8.shape == (F,) + size + (3,) and f32.shape == u8.shape and u8.dtype == np.uint8 and f32.dtype == np.float32
    for f in range(F):
        w8, w32 = post.op_letterbox(frames[f], size)
        assert u8[f].tobytes() == w8.tobytes() and f32[f].tobytes() == w32.tobytes()
    assert u8[0].tobytes() != u8[-1].tobytes()
    only8, none32 = post.op_letterbox_mixed(frames, size, want_f32=False)
    none8, only32 = post.op_letterbox_mixed(frames, size, bgr=False, want_u8=False)
    assert none32 is None and none8 is None and only8.tobytes() == u8.tobytes()
    assert only32.tobytes() == np.stack([post.op_letterbox(f, size, bgr=False)[1] for f in frames]).tobytes()


# ---- 6. the selection alone, every image its own shape -----------------------------------------------------------------------
def test_mixed_selection_equals_the_single_image_selection(post):
    anchors = np.array(DC.ANCHORS["full"], np.float32).reshape(-1, 2)
    grids = [(2, 3), (4, 6), (8, 12)]                                                # a 64 x 96 input
    maps = seeded_maps(21, grids, 2, conf=(0.0, -40.0, 4.0, 0.5))                   # some, none, nearly every box, some
    shapes = [(224, 528), (528, 224), (97, 131), (1, 1)]
    kw = dict(max_boxes=5, score_threshold=0.3, iou_threshold=0.45)
    got = post.yolo_eval_mixed(maps, anchors, 2, shapes, **kw)
    assert len(got) == 4
    counts = []
    for f, g in enumerate(got):
        want = post.yolo_eval([m[f] for m in maps], anchors, 2, shapes[f], debug=True, **kw)[:4]
        assert_same(g, want)
        counts.append([int((g[2] == c).sum()) for c in range(2)])
    print(f"selected per image and class {counts}")
    assert counts[1] == [0, 0] and counts[2] == [5, 5] and sum(counts[0]) > 0 and sum(counts[3]) > 0
    # the same maps under one shape give other boxes: the correction is the image's own
    one = post.yolo_eval_mixed(maps, anchors, 2, [shapes[0]] * 4, **kw)
    assert one[2][0].tobytes() != got[2][0].tobytes()
    assert_same(one[0], got[0])


# ---- 7. the geometry cache ---------------------------------------------------------------------------------------------------
def cache_pass(fp, kw, A, E, T, A2):
    """Single frames A, E, A, E, then a mixed clip [A, E, T], then a uniform clip of A, two submissions in flight; the results
    in submission order."""
    out = []
    fp.begin(A)
    fp.detect_heads(**kw)
    for frame in (E, A, E):
        fp.begin(frame)
        fp.detect_heads(**kw)
        out.append(fp.collect(detections=True))
    fp.begin_clip_mixed([A, E, T])
    fp.detect_heads_clip(**kw)
    out.append(fp.collect(detections=True))
    fp.begin_clip([A, A2])
    fp.detect_heads_clip(**kw)
    out.append(fp.collect_clip(detections=True))
    out.append(fp.collect_clip(detections=True))
    return out


def test_cache_keeps_alternating_sizes_enqueue_only(models, detect_args, tagged, single):
    name = "tiny"
    kw = kwargs(detect_args, name)
    A, E, T = (tagged[k] for k in "AET")
    A2 = np.ascontiguousarray(A[::-1])
    want = [single(name, f)[0] for f in (A, E, A, E)]
    want_mixed = [single(name, f)[0] for f in (A, E, T)]
    want_uniform = [single(name, f)[0] for f in (A, A2)]
    h = models[name]._handle

    def check(out):
        assert len(out) == 6
        for g, w in zip(out[:4], want):
            assert_same(g, w)
        for clip, ws in ((out[4], want_mixed), (out[5], want_uniform)):
            assert len(clip[0]) == len(ws) and clip[1][1] == 0
            for g, w in zip(clip[0], ws):
                assert_same(g, w)

    with FramePipeline(models[name], depth=2) as fp:
        check(cache_pass(fp, kw, A, E, T, A2))
        s1 = h.letterbox_cache_stats()
        check(cache_pass(fp, kw, A, E, T, A2))
        s2 = h.letterbox_cache_stats()
    print(f"cache after the first pass {s1}, after the second {s2}")
    assert s2["misses"] == s1["misses"] and s2["host_waits"] == s1["host_waits"] and s2["hits"] > s1["hits"]
    assert 3 <= s2["entries"] == s1["entries"]
    # two entries for three sizes: every frame re-stages its tables, the bytes stay
    m = seeded_model(name, 1)
    try:
        m._handle.set_option("letterbox_cache", 2)
        with FramePipeline(m, depth=2) as fp:
            cycle = (A, E, T, A, E, T)
            got = []
            fp.begin(cycle[0])
            fp.detect_heads(**kw)
            for frame in cycle[1:]:
                fp.begin(frame)
                fp.detect_heads(**kw)
                got.append(fp.collect(detections=True))
            got.append(fp.collect(detections=True))
            for g, frame in zip(got, cycle):
                assert_same(g, single(name, frame)[0])
            s3 = m._handle.letterbox_cache_stats()
            print(f"two entries, three sizes: {s3}")
            assert s3["misses"] >= 6 and s3["entries"] <= 4
            with pytest.raises(ValueError, match="letterbox_cache"):                # three sizes at once do not fit
                fp.begin_clip_mixed([A, E, T])
            assert fp.in_flight == 0
            clip = run_mixed(fp, [A, E], kw)                                         # the pipeline stays usable
            assert_same(clip[0][1], single(name, E)[0])
        for bad in (0, 33):
            with pytest.raises(ValueError, match="letterbox_cache"):
                m._handle.set_option("letterbox_cache", bad)
    finally:
        m.close()


# ---- 8. misuse ---------------------------------------------------------------------------------------------------------------
def test_misuse_is_reported_and_no_slot_leaks(models, detect_args, tagged, single):
    name = "tiny"
    kw = kwargs(detect_args, name)
    args = hargs(kw)[:5]
    A, E = tagged["A"], tagged["E"]
    h = models[name]._handle
    with FramePipeline(models[name], depth=2) as fp:
        for bad in ([], [A] * 17, [A, np.zeros((0, 5, 3), np.uint8)], [A, np.zeros((8193, 1, 3), np.uint8)], [A, E.astype(np.float32)],
                    [A, E[:, :, 0]], [A, E[None]]):
            with pytest.raises(ValueError):
                fp.begin_clip_mixed(bad)
            with pytest.raises(ValueError):
                h.clip_begin_mixed(bad)
        assert fp.in_flight == 0
    # the library's own checks: F, NULL frames and sides, each naming the frame
    lib, t = _lib.load(), C.c_int(-1)
    ptrs = (C.c_void_p * 17)(*([A.ctypes.data] * 17))
    sides = lambda v: (C.c_int * 17)(*v)
    ok_h, ok_w = [224] * 17, [528] * 17
    for n in (0, 17):
        assert lib.whenet_clip_begin_mixed(h._h, ptrs, n, sides(ok_h), sides(ok_w), _lib.BGR, C.byref(t)) == _lib.EINVAL
    for fh, fw in (([224, 0] + ok_h[2:], ok_w), (ok_h, [528, 8193] + ok_w[2:])):
        assert lib.whenet_clip_begin_mixed(h._h, ptrs, 2, sides(fh), sides(fw), _lib.BGR, C.byref(t)) == _lib.EINVAL
        assert b"frame 1" in lib.whenet_last_error(h._h)
    null = (C.c_void_p * 2)(A.ctypes.data, None)
    assert lib.whenet_clip_begin_mixed(h._h, null, 2, sides(ok_h), sides(ok_w), _lib.BGR, C.byref(t)) == _lib.EINVAL
    assert b"frame 1" in lib.whenet_last_error(h._h)
    canvas = np.empty((2, 64, 96, 3), np.uint8)
    assert lib.whenet_op_letterbox_mixed(h._h, ptrs, 2, sides([224, 8193]), sides(ok_w), _lib.BGR, 64, 96, canvas.ctypes.data,
                                         None) == _lib.EINVAL
    # a frame whose resized image would be empty at this detector input: reported by the heads, the ticket stays releasable
    thin = np.zeros((1, 400, 3), np.uint8)
    tk = h.clip_begin_mixed([A, thin])
    with pytest.raises(ValueError, match="frame 1"):
        h.clip_detect_heads(tk, *args, 20)
    h.frame_heads(tk, np.zeros((0, 4), np.int32))
    h.collect(tk, 0)
    # the calls for ONE frame on a mixed ticket, and the wrong collects
    tk = h.clip_begin_mixed([E, A])
    for call in (lambda: h.frame_detect_heads(tk, *args, 20), lambda: h.frame_detect(tk, *args, 20),
                 lambda: h.frame_letterbox(tk, (64, 96)), lambda: h.frame_heads(tk, np.array([[10, 10, 50, 50]], np.int32))):
        with pytest.raises(ValueError, match="holds a clip"):
            call()
    k = h.clip_detect_heads(tk, *args, 20)
    with pytest.raises(ValueError, match="collect_clip returns it"):
        h.collect(tk, 3)
    with pytest.raises(ValueError, match="not submitted by frame_detect_heads"):
        h.collect_detect(tk, k)
    res = h.collect_clip(tk, 2, k)
    assert res[0][0] == len(single(name, E)[0][4])
    with FramePipeline(models[name], depth=2) as fp:
        fp.begin_clip_mixed([E, A])
        for call in (lambda: fp.detect_heads(**kw), lambda: fp.detect(**kw), lambda: fp.heads(np.zeros((0, 4), np.float32)),
                     lambda: fp.begin(A), lambda: fp.begin_clip_mixed([A, E]), lambda: fp.collect()):
            with pytest.raises(ValueError):
                call()
        fp.detect_heads_clip(**kw)
        with pytest.raises(ValueError, match="collect_clip"):
            fp.collect(detections=True)
        got = fp.collect_clip(detections=True)
        assert_same(got[0][0], single(name, E)[0])
        fp.begin_clip_mixed([A, E])                                                  # left without heads: released on exit
    # afterwards a clip runs and returns the bytes of test 1: no slot leaked (every one of them is taken in turn)
    frames = [tagged[k] for k in "EATB"]
    with FramePipeline(models[name], depth=1) as fp:
        for _ in range(_lib.MAX_INFLIGHT + 1):
            clip = run_mixed(fp, frames, kw)
            for g, frame in zip(clip[0], frames):
                assert_same(g, single(name, frame)[0])
