"""Clips on the GPU: F frames of one size as ONE submission (begin_clip -> detect_heads_clip -> collect_clip; the batched passes of
csrc/letterbox.hip, csrc/yolo.hip and csrc/headplan.hip, the compaction kernel, the gathering crop kernel of csrc/frame.hip,
Engine::clip_detect_heads).  The contract is bitwise: every frame of a clip returns the bytes that begin; detect_heads; collect
returns for that frame alone, every stage alone equals its single-frame form, and the numbering of the heads equals a cumsum."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import detector_cases as DC
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


@pytest.fixture(scope="module")
def models():
    """One seeded f16 WHENet per detector body, the seeded detector attached to its handle (as tests/test_frame_async_gpu.py)."""
    import whenet
    ms = {}
    for name, kind in DC.KINDS:
        m = whenet.WHENet(dtype="f16")
        m._handle.detector_load(DW.pack(DW.synthetic(kind, DC.SEEDS[name])))
        ms[name] = m
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def variants():
    """Four frames of one size with different content: the sample frame, its vertical flip, horizontal flip and a 100-column roll."""
    a = DC.sample_frame(0)
    assert a.shape == (224, 528, 3)
    return [np.ascontiguousarray(v) for v in (a, a[::-1], a[:, ::-1], np.roll(a, 100, axis=1))]


def kwargs(detect_args, name, **over):
    d = detect_args[name]
    assert tuple(d["size"]) == (64, 96)
    kw = dict(size=tuple(d["size"]), score=d["score"], iou=d["iou"], max_boxes=d["max_boxes"],
              anchors=np.array(DC.ANCHORS[name], np.float32).reshape(-1, 2), num_classes=1)
    kw.update(over)
    return kw


def hargs(kw):
    return (kw["anchors"], kw["num_classes"], kw["size"], kw["score"], kw["iou"], kw["max_boxes"])


@pytest.fixture(scope="module")
def per_frame(models, detect_args, variants):
    """The single-frame path of every (detector, variant), computed once: `eight` = begin; detect_heads; collect(detections=True),
    `slots` = the same submission through the handle with argmax and logits (boxes, scores, classes, rects, valid, ypr, argmax,
    logits over the detections)."""
    ref = {}
    for name, _ in DC.KINDS:
        kw = kwargs(detect_args, name)
        h = models[name]._handle
        with FramePipeline(models[name], depth=1) as fp:
            for v, frame in enumerate(variants):
                fp.begin(frame)
                fp.detect_heads(**kw)
                eight = fp.collect(detections=True)
                t = h.frame_begin(frame)
                slots = h.collect_detect(t, h.frame_detect_heads(t, *hargs(kw)), want_logits=True)
                ref[name, v] = (eight, slots)
    return ref


def run_clip(fp, frames, kw, max_heads=None):
    fp.begin_clip(frames)
    fp.detect_heads_clip(max_heads=max_heads, **kw)
    return fp.collect_clip(detections=True)


def handle_clip(h, frames, kw, max_heads=None):
    t = h.clip_begin(np.stack(frames))
    k = h.clip_detect_heads(t, *hargs(kw), max_heads=max_heads)
    return h.collect_clip(t, len(frames), k, want_logits=True)


def assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def assert_slots_equal_frame(res, f, slots, rows_expected):
    """Frame f of a handle-level clip result against the single-frame submission's arrays; rows_expected [n]: whether detection i
    must have a forward row."""
    counts, boxes, scores, classes, rects, valid, row, ypr, amax, logits, _, _ = res
    n = len(slots[0])
    assert counts[f] == n
    for g, w in zip((boxes, scores, classes, rects, valid), slots[:5]):
        assert g[f, :n].tobytes() == w.tobytes()
    assert not boxes[f, n:].any() and (classes[f, n:] == -1).all() and not valid[f, n:].any() and (row[f, n:] == -1).all()
    has = row[f, :n] >= 0
    assert np.array_equal(has, rows_expected)
    for g, w in zip((ypr, amax, logits), slots[5:]):
        assert g[f, :n][has].tobytes() == w[has].tobytes()
    lost = ~has
    assert np.isnan(ypr[f, :n][lost]).all() and (amax[f, :n][lost] == -1).all() and np.isnan(logits[f, :n][lost]).all()
    assert np.isnan(ypr[f, n:]).all() and (amax[f, n:] == -1).all() and np.isnan(logits[f, n:]).all()


# ---- 1. clip = per-frame path, bitwise ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_clip_is_bitwise_the_per_frame_path(models, detect_args, variants, per_frame, name, kind):
    kw = kwargs(detect_args, name)
    F, K = 3, kw["max_boxes"]
    with FramePipeline(models[name], depth=1) as fp:
        frames, (rows_used, overflow) = run_clip(fp, variants[:F], kw, max_heads=F * K)
    want = [per_frame[name, v][0] for v in range(F)]
    counts = [len(t[4]) for t in frames]
    heads = [int((t[7] != 0).sum()) for t in frames]
    print(f"{name}: detections per frame {counts}, with a window {heads}, rows_used {rows_used}, overflow {overflow}")
    assert len(frames) == F
    for got, w in zip(frames, want):
        assert len(got) == 8
        assert_same(got, w)
    assert overflow == 0 and rows_used == sum(heads) and sum(heads) >= 3
    assert any(frames[i][4].tobytes() != frames[j][4].tobytes() for i in range(F) for j in range(i))     # not frame 0 three times
    # the slot arrays through the handle, argmax and logits included
    res = handle_clip(models[name]._handle, variants[:F], kw, max_heads=F * K)
    assert res[-2:] == (rows_used, overflow)
    for f in range(F):
        slots = per_frame[name, f][1]
        assert_slots_equal_frame(res, f, slots, slots[4] != 0)
    live = np.flatnonzero((res[6] >= 0).reshape(-1))
    assert res[6].reshape(-1)[live].tolist() == list(range(rows_used))            # rows in (frame, detection) order


# ---- 2. F = 1 and F = 16 -----------------------------------------------------------------------------------------------------
def test_one_frame_and_sixteen_frames(models, detect_args, variants, per_frame):
    name = "tiny"
    kw = kwargs(detect_args, name)
    with FramePipeline(models[name], depth=1) as fp:
        one, (used1, over1) = run_clip(fp, variants[:1], kw)
        few, (used1b, over1b) = run_clip(fp, [variants[2]], kw, max_heads=max(1, len(per_frame[name, 2][0][0])))   # without the padding
        four, (used4, over4) = run_clip(fp, variants, kw)
        sixteen, (used16, over16) = run_clip(fp, variants * 4, kw)
    assert len(one) == 1 and len(four) == 4 and len(sixteen) == 16
    assert_same(one[0], per_frame[name, 0][0])
    assert_same(few[0], per_frame[name, 2][0])
    assert (over1, over1b, over4, over16) == (0, 0, 0, 0)
    assert used1 == len(one[0][0]) and used1b == len(few[0][0]) and used4 == sum(len(t[0]) for t in four) and used16 == 4 * used4
    for v in range(4):
        assert_same(four[v], per_frame[name, v][0])
    for f in range(16):
        assert_same(sixteen[f], four[f % 4])


# ---- 3. overflow -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_overflow_keeps_the_first_heads_and_reports_the_rest(models, detect_args, variants, per_frame, name, kind):
    kw = kwargs(detect_args, name)
    F = 3
    valid = [per_frame[name, v][1][4] != 0 for v in range(F)]
    total = int(sum(v.sum() for v in valid))
    assert total >= 3
    h = models[name]._handle
    for max_heads in (1, total - 1):
        res = handle_clip(h, variants[:F], kw, max_heads=max_heads)
        assert res[-2:] == (max_heads, total - max_heads)
        seen = 0
        for f in range(F):
            order = seen + np.cumsum(valid[f]) - 1                                   # number of each head in (frame, detection) order
            assert_slots_equal_frame(res, f, per_frame[name, f][1], valid[f] & (order < max_heads))
            seen += int(valid[f].sum())
        # the pipeline's view: detections, windows and valid unchanged, the heads those that have a row
        with FramePipeline(models[name], depth=1) as fp:
            frames, (used, over) = run_clip(fp, variants[:F], kw, max_heads=max_heads)
        assert (used, over) == (max_heads, total - max_heads)
        left = max_heads
        for f in range(F):
            w = per_frame[name, f][0]
            assert_same(frames[f][4:], w[4:])
            k = min(left, len(w[0]))
            assert_same(frames[f][:4], tuple(a[:k] for a in w[:4]))
            left -= k


# ---- 4. the compaction kernel alone ------------------------------------------------------------------------------------------
def compact_ref(valid, count, max_heads):
    F, K = valid.shape
    live = ((valid != 0) & (np.arange(K)[None, :] < np.clip(count, 0, K)[:, None])).reshape(-1)
    number = np.cumsum(live) - 1
    row = np.where(live & (number < max_heads), number, -1).astype(np.int32)
    slot_of_row = np.full(max_heads, -1, np.int32)
    slot_of_row[row[row >= 0]] = np.flatnonzero(row >= 0)
    total = int(live.sum())
    used = min(total, max_heads)
    return row.reshape(F, K), slot_of_row, used, total - used


def compact_cases():
    rng = np.random.default_rng(11)
    full = lambda F, K: np.full(F, K, np.int32)
    last = np.zeros((16, 64), np.int32)
    last[-1, -1] = 1
    beyond = np.ones((3, 20), np.int32)
    return [
        ("all_zero", np.zeros((3, 20), np.int32), full(3, 20), 60),
        ("all_one", np.ones((3, 20), np.int32), full(3, 20), 60),
        ("all_one_1024", np.ones((16, 64), np.int32), full(16, 64), 256),
        ("alternating", (np.arange(5 * 37).reshape(5, 37) % 2).astype(np.int32), full(5, 37), 185),
        ("alternating_tight", (np.arange(5 * 37).reshape(5, 37) % 2).astype(np.int32), full(5, 37), 92),      # exactly the live count
        ("only_last", last, full(16, 64), 256),
        ("random_1024", (rng.random((16, 64)) < 0.4).astype(np.int32), rng.integers(0, 65, 16).astype(np.int32), 256),
        ("random_odd", (rng.random((7, 13)) < 0.5).astype(np.int32) * 3, rng.integers(0, 14, 7).astype(np.int32), 17),
        ("beyond_count", beyond, np.array([4, 0, 20], np.int32), 60),
        ("count_out_of_range", beyond, np.array([-3, 99, 2], np.int32), 60),
        ("max_heads_1", np.ones((3, 20), np.int32), full(3, 20), 1),
        ("max_heads_1_none", np.zeros((3, 20), np.int32), full(3, 20), 1),
        ("one_slot_live", np.ones((1, 1), np.int32), full(1, 1), 1),
        ("one_slot_dead", np.zeros((1, 1), np.int32), full(1, 1), 3),
        ("wave_edge", (np.arange(1 * 130).reshape(1, 130) % 64 >= 62).astype(np.int32), full(1, 130), 256),
    ]


@pytest.mark.parametrize("case", compact_cases(), ids=lambda c: c[0])
def test_compaction_kernel_equals_a_cumsum(post, case):
    _, valid, count, max_heads = case
    row, slot_of_row, used, overflow = post.op_head_compact(valid, count, max_heads)
    w_row, w_sor, w_used, w_over = compact_ref(valid, count, max_heads)
    assert row.dtype == np.int32 and slot_of_row.dtype == np.int32 and row.shape == valid.shape
    assert np.array_equal(row, w_row) and np.array_equal(slot_of_row, w_sor) and (used, overflow) == (w_used, w_over)


# ---- 5. the batched selection alone ------------------------------------------------------------------------------------------
def seeded_maps(seed, grids, num_classes, conf):
    """[F, gh, gw, 3 * (5 + C)] per grid: normal logits, image f's confidence logits drawn around conf[f]."""
    rng = np.random.default_rng(seed)
    maps = []
    for gh, gw in grids:
        m = rng.normal(0.0, 1.0, (len(conf), gh, gw, 3, 5 + num_classes)).astype(np.float32)
        for f, c in enumerate(conf):
            m[f, ..., 4] = rng.normal(c, 1.5, (gh, gw, 3))
        maps.append(m.reshape(len(conf), gh, gw, 3 * (5 + num_classes)))
    return maps


def assert_batch_is_per_image(post, maps, anchors, num_classes, image_shape, **kw):
    batch = post.yolo_eval_batch(maps, anchors, num_classes, image_shape, **kw)
    assert len(batch) == maps[0].shape[0]
    counts = []
    for f, got in enumerate(batch):
        want = post.yolo_eval([m[f] for m in maps], anchors, num_classes, image_shape, debug=True, **kw)[:4]
        assert_same(got, want)
        counts.append([int((got[2] == c).sum()) for c in range(num_classes)])
    return batch, counts


def test_batched_selection_equals_the_single_image_selection(post):
    anchors = np.array(DC.ANCHORS["full"], np.float32).reshape(-1, 2)
    grids = [(2, 3), (4, 6), (8, 12)]                                                # a 64 x 96 input
    n_all = sum(gh * gw * 3 for gh, gw in grids)
    maps = seeded_maps(21, grids, 2, conf=(0.0, -40.0, 4.0))                        # some, none, nearly every box a candidate
    kw = dict(max_boxes=5, score_threshold=0.3, iou_threshold=0.45)
    batch, counts = assert_batch_is_per_image(post, maps, anchors, 2, (224, 528), **kw)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    cand = []                                                                       # candidates per (image, class), in float64
    for f in range(3):
        t = np.concatenate([m[f].reshape(-1, 7) for m in maps])
        cand.append(((sig(t[:, 4:5]) * sig(t[:, 5:])) >= 0.35).sum(axis=0).tolist())
    print(f"selected per image and class {counts}, candidates (score >= 0.35) {cand}, of {n_all} boxes")
    assert counts[1] == [0, 0] and len(batch[1][0]) == 0                             # the image without a candidate
    assert min(cand[2]) > 5 and counts[2] == [5, 5]                                  # more candidates than max_boxes
    assert 0 < sum(counts[0]) and batch[0][0].tobytes() != batch[2][0][:len(batch[0][0])].tobytes()
    # tiny layout (2 maps, 6 anchors), one class, max_boxes beyond the boxes the maps hold
    tiny = np.array(DC.ANCHORS["tiny"], np.float32).reshape(-1, 2)
    assert_batch_is_per_image(post, seeded_maps(22, grids[:2], 1, conf=(3.0, 0.0)), tiny, 1, (224, 528), max_boxes=1000,
                              score_threshold=0.3, iou_threshold=0.45)


def test_batched_selection_sorts_in_global_memory_at_threshold_zero(post):
    anchors = np.array(DC.ANCHORS["full"], np.float32).reshape(-1, 2)
    maps = seeded_maps(23, [(13, 13), (26, 26), (52, 52)], 2, conf=(0.0, 1.0))       # 416 x 416: 10,647 candidates per class > 4096
    batch, counts = assert_batch_is_per_image(post, maps, anchors, 2, (720, 1280), max_boxes=20, score_threshold=0.0, iou_threshold=0.45)
    assert counts == [[20, 20], [20, 20]] and batch[0][3].tobytes() != batch[1][3].tobytes()


# ---- 6. the batched letterbox alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fh,fw,size", [(97, 131, (64, 96)), (150, 40, (64, 64))])
def test_batched_letterbox_equals_the_single_frame_letterbox(post, variants, fh, fw, size):
    frames = np.stack([np.ascontiguousarray(v[:fh, :fw]) for v in variants[:3]])
    assert (fh * fw * 3) % 16 != 0 or fw * 3 % 16 != 0                              # odd frame stride or row pitch
    u8, f32 = post.op_letterbox_batch(frames, size)
    assert u8.shape == (3,) + size + (3,) and f32.shape == u8.shape and u8.dtype == np.uint8 and f32.dtype == np.float32
    for f in range(3):
        w8, w32 = post.op_letterbox(frames[f], size)
        assert u8[f].tobytes() == w8.tobytes() and f32[f].tobytes() == w32.tobytes()
    assert u8[0].tobytes() != u8[1].tobytes() and u8[0].tobytes() != u8[2].tobytes()
    if size == (64, 64):
        assert (u8[:, :, 0] == 128).all() and (u8[:, :, -1] == 128).all() and (u8[:, 32, 32] != 128).any()      # pasted with an x offset
    only8, none32 = post.op_letterbox_batch(frames, size, want_f32=False)
    none8, only32 = post.op_letterbox_batch(frames, size, bgr=False, want_u8=False)
    assert none32 is None and none8 is None and only8.tobytes() == u8.tobytes()
    assert only32.tobytes() == np.stack([post.op_letterbox(f, size, bgr=False)[1] for f in frames]).tobytes()


# ---- 7. order, replay and depth ----------------------------------------------------------------------------------------------
def test_order_replay_and_depth(models, detect_args, variants, per_frame):
    name = "tiny"
    kw = kwargs(detect_args, name)
    B = DC.sample_frame(1)
    assert B.shape != variants[0].shape                                              # (the letterbox tables are re-staged in between)
    clipB = [B, np.ascontiguousarray(B[::-1])]
    a0 = per_frame[name, 0][0]
    with FramePipeline(models[name], depth=1) as fp:
        cA1 = run_clip(fp, variants[:3], kw)
        cB1 = run_clip(fp, clipB, kw)
        fp.begin(B)
        fp.detect_heads(**kw)
        b1 = fp.collect(detections=True)
        fp.submit(variants[0], a0[4][a0[7] != 0])
        s1 = fp.collect()
    assert_same(cB1[0][0], b1)
    with FramePipeline(models[name], depth=2) as fp:
        fp.begin_clip(variants[:3])
        fp.detect_heads_clip(**kw)
        fp.begin(B)
        fp.detect_heads(**kw)
        assert fp.in_flight == 2
        cA2, b2 = fp.collect_clip(detections=True), fp.collect(detections=True)
        fp.begin_clip(clipB)
        fp.detect_heads_clip(**kw)
        fp.submit(variants[0], a0[4][a0[7] != 0])
        cB3, s3 = fp.collect_clip(detections=True), fp.collect()
        fp.begin(variants[1])
        fp.detect_heads(**kw)
        fp.begin_clip(variants[:3])
        fp.detect_heads_clip(**kw)
        a4, cA4 = fp.collect(detections=True), fp.collect_clip(detections=True)
        fp.begin_clip(clipB)
        fp.detect_heads_clip(**kw)
        fp.begin_clip(variants[:3])
        fp.detect_heads_clip(**kw)
        cB5, cA5 = fp.collect_clip(detections=True), fp.collect_clip(detections=True)
    for want, gots in ((cA1, (cA2, cA4, cA5)), (cB1, (cB3, cB5))):
        for got in gots:
            assert got[1] == want[1] and len(got[0]) == len(want[0])
            for g, w in zip(got[0], want[0]):
                assert_same(g, w)
    assert_same(b2, b1)
    assert_same(s3, s1)
    assert_same(a4, per_frame[name, 1][0])
    for f in range(3):
        assert_same(cA1[0][f], per_frame[name, f][0])


# ---- 8. score 1.0 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_a_clip_without_detections(models, detect_args, variants, per_frame, name, kind):
    with FramePipeline(models[name], depth=1) as fp:
        frames, (rows_used, overflow) = run_clip(fp, variants[:3], kwargs(detect_args, name, score=1.0))
        assert len(frames) == 3 and (rows_used, overflow) == (0, 0)
        for t in frames:
            assert [len(a) for a in t] == [0] * 8 and t[0].shape == (0, 4) and t[4].shape == (0, 4)
        again, _ = run_clip(fp, variants[:2], kwargs(detect_args, name))          # the handle stays usable
        assert_same(again[1], per_frame[name, 1][0])


# ---- 9. misuse ---------------------------------------------------------------------------------------------------------------
def test_misuse_is_reported_and_the_handle_stays_usable(models, detect_args, variants, per_frame, post):
    import whenet
    name = "tiny"
    kw = kwargs(detect_args, name)
    args = hargs(kw)[:5]
    clip = np.stack(variants[:2])
    crops = np.load(os.path.join(GOLDEN, "golden_crops.npy"))[:2]
    h = models[name]._handle
    # frames of different shapes or dtypes, F outside 1..16 (the checks of the binding, then the library's own)
    with FramePipeline(models[name], depth=2) as fp:
        for bad in ([variants[0], variants[0][:100]], [variants[0], variants[0].astype(np.float32)], [], [variants[0]] * 17):
            with pytest.raises(ValueError):
                fp.begin_clip(bad)
        assert fp.in_flight == 0
    lib, t = _lib.load(), C.c_int(-1)
    seventeen = np.zeros((17, 8, 8, 3), np.uint8)
    for n in (17, 0):
        assert lib.whenet_clip_begin(h._h, seventeen.ctypes.data, n, 8, 8, _lib.BGR, C.byref(t)) == _lib.EINVAL
    # F x K > 1024 and max_heads outside 1..256, then the same ticket with legal values
    t16 = h.clip_begin(np.stack(variants * 4))
    with pytest.raises(ValueError, match="1..1024"):
        h.clip_detect_heads(t16, *args, 65)
    k = C.c_int(0)
    for bad in (257, -1):
        assert lib.whenet_clip_detect_heads(h._h, t16, 64, 96, kw["anchors"].ctypes.data, 6, kw["score"], kw["iou"], 20, bad,
                                            C.byref(k)) == _lib.EINVAL
    with pytest.raises(ValueError, match="max_heads"):
        h.clip_detect_heads(t16, *args, 20, max_heads=0)
    # the calls for ONE frame on a clip ticket
    for call in (lambda: h.frame_detect(t16, *args, 20), lambda: h.frame_detect_heads(t16, *args, 20),
                 lambda: h.frame_letterbox(t16, (64, 96)), lambda: h.frame_heads(t16, np.array([[10, 10, 100, 100]], np.int32))):
        with pytest.raises(ValueError, match="holds a clip"):
            call()
    assert h.clip_detect_heads(t16, *args, 64) == 64                                 # 16 x 64 = 1024 slots
    with pytest.raises(ValueError, match="clip_detect_heads"):                       # its heads are already enqueued
        h.clip_detect_heads(t16, *args, 64)
    # collect / collect_detect on a clip, a capacity below the submission's, then the right call
    with pytest.raises(ValueError, match="collect_clip returns it"):
        h.collect(t16, 3)
    with pytest.raises(ValueError, match="not submitted by frame_detect_heads"):
        h.collect_detect(t16, 64)
    with pytest.raises(ValueError, match="capacity"):
        h.collect_clip(t16, 16, 20)
    res = h.collect_clip(t16, 16, 64)
    assert res[0][0] == len(per_frame[name, 0][0][4]) and res[0][4:].tolist() == res[0][:12].tolist() and res[-1] == 0
    with pytest.raises(ValueError, match="unknown or already collected"):
        h.collect_clip(t16, 16, 64)
    # clip_detect_heads on a frame ticket, collect_clip on frame tickets
    t = h.frame_begin(variants[0])
    with pytest.raises(ValueError, match="single frame"):
        h.clip_detect_heads(t, *args, 20)
    with pytest.raises(ValueError, match="not submitted by clip_detect_heads"):
        h.collect_clip(t, 1, 20)
    cap = h.frame_detect_heads(t, *args, 20)
    with pytest.raises(ValueError, match="not submitted by clip_detect_heads"):
        h.collect_clip(t, 1, 20)
    assert_same(h.collect_detect(t, cap)[:5], per_frame[name, 0][1][:5])
    # a clip that never gets its heads is released like a frame
    t = h.clip_begin(clip)
    h.frame_heads(t, np.zeros((0, 4), np.int32))
    h.collect(t, 0)
    # the pipeline: the wrong call for what was begun, the wrong collect for what is in flight
    with FramePipeline(models[name], depth=2) as fp:
        fp.begin_clip(clip)
        for call in (lambda: fp.detect(**kw), lambda: fp.detect_heads(**kw), lambda: fp.detector_input((64, 96)),
                     lambda: fp.heads(np.zeros((0, 4), np.float32)), lambda: fp.begin(variants[0]), lambda: fp.begin_clip(clip)):
            with pytest.raises(ValueError):
                call()
        fp.detect_heads_clip(**kw)
        fp.begin(variants[0])
        with pytest.raises(ValueError, match="single frame"):
            fp.detect_heads_clip(**kw)
        fp.detect_heads(**kw)
        with pytest.raises(ValueError, match="collect_clip"):
            fp.collect(detections=True)
        got = fp.collect_clip(detections=True)
        with pytest.raises(ValueError, match="not a clip"):
            fp.collect_clip()
        assert_same(fp.collect(detections=True), per_frame[name, 0][0])
        assert_same(got[0][1], per_frame[name, 1][0])
        fp.begin_clip(clip)                                                          # left without heads: released on exit
    # no detector on the handle
    bare = whenet.WHENet(dtype="f16")
    try:
        b = bare._handle
        t = b.clip_begin(clip)
        with pytest.raises(ValueError, match="no detector is loaded"):
            b.clip_detect_heads(t, *args, 20)
        b.frame_heads(t, np.zeros((0, 4), np.int32))
        b.collect(t, 0)
        assert b.forward(crops)[0].shape == (2, 3)
    finally:
        bare.close()
    # a post-processing handle: no network to run the heads through
    t = post.clip_begin(clip)
    with pytest.raises(ValueError, match="without a network"):
        post.clip_detect_heads(t, *args, 20)
    post.frame_heads(t, np.zeros((0, 4), np.int32))
    post.collect(t, 0)
    assert post.op_head_compact(np.ones((1, 2), np.int32), np.array([2], np.int32), 2)[2] == 2
    for valid, count, max_heads in ((np.zeros((17, 64), np.int32), np.zeros(17, np.int32), 8),):
        with pytest.raises(ValueError, match="op_head_compact"):
            post.op_head_compact(valid, count, max_heads)
    assert h.forward(crops)[0].shape == (2, 3)
