"""One submission per video frame on the GPU (begin -> detect_heads -> collect; csrc/headplan.hip, the masked crop kernel of
csrc/frame.hip, Engine::frame_detect_heads): the device's windows and crop plans bit for bit the host's, the fused submission
bit for bit the two-step path (begin; detect; heads; collect), heads without a window, an empty frame, order / replay / depth,
and misuse."""
import json
import os

import numpy as np
import pytest

from tests import detector_cases as DC
from whenet_hip import _lib, detector_weights as DW
from whenet_hip.frames import FramePipeline

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def check_rects(fh, fw, r):
    """check_rects of csrc/engine_post.cpp: the window is non-empty and inside the frame."""
    return (r[:, 0] >= 0) & (r[:, 1] >= 0) & (r[:, 2] <= fh) & (r[:, 3] <= fw) & (r[:, 0] < r[:, 2]) & (r[:, 1] < r[:, 3])


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
    """One seeded f16 WHENet per detector body, the seeded detector attached to its handle."""
    import whenet
    ms = {}
    for name, kind in DC.KINDS:
        m = whenet.WHENet(dtype="f16")
        m._handle.detector_load(DW.pack(DW.synthetic(kind, DC.SEEDS[name])))
        ms[name] = m
    yield ms
    for m in ms.values():
        m.close()


def kwargs(detect_args, name, **over):
    d = detect_args[name]
    kw = dict(size=tuple(d["size"]), score=d["score"], iou=d["iou"], max_boxes=d["max_boxes"],
              anchors=np.array(DC.ANCHORS[name], np.float32).reshape(-1, 2), num_classes=1)
    kw.update(over)
    return kw


def fused(fp, frame, kw):
    fp.begin(frame)
    fp.detect_heads(**kw)
    return fp.collect(detections=True)


def two_step(fp, frame, kw, valid):
    """begin; detect -> boxes; heads(boxes[valid]); collect -> ((boxes, scores, classes), (rects, yaw, pitch, roll))."""
    fp.begin(frame)
    det = fp.detect(**kw)
    fp.heads(det[0][valid != 0])
    return det, fp.collect()


def assert_fused_is_two_step(got, det, heads):
    rects, yaw, pitch, roll, boxes, scores, classes, valid = got
    for g, w in zip((boxes, scores, classes), det):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    for g, w in zip((rects, yaw, pitch, roll), heads):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


# ---- 1. windows and valid flags, bitwise -------------------------------------------------------------------------------------
def test_rects_and_valid_equal_the_executed_reference_and_the_host(post):
    with np.load(os.path.join(GOLDEN, "reference_rects.npz")) as z:
        boxes, hw, want = z["boxes"], z["frame_hw"], z["rects"]
    sizes = np.unique(hw, axis=0)
    assert len(sizes) == 4 and len(boxes) == 1220
    n_valid = n_invalid = 0
    for fh, fw in sizes:
        m = (hw[:, 0] == fh) & (hw[:, 1] == fw)
        rects, valid, plans = post.op_head_plan(int(fh), int(fw), boxes[m], want_plans=False)
        assert plans is None and rects.dtype == np.int32 and valid.dtype == np.int32
        host = _lib.frame_rects(int(fh), int(fw), boxes[m])
        assert rects.tobytes() == host.tobytes()                                   # every row, valid or not
        ok = check_rects(fh, fw, host)
        assert np.array_equal(valid, ok.astype(np.int32))
        assert np.array_equal(rects[ok], want[m][ok])                              # what the executed process_detection sliced
        n_valid += int(ok.sum())
        n_invalid += int((~ok).sum())
    assert (n_valid, n_invalid) == (1213, 7)


# ---- 2. crop plans, bitwise ----------------------------------------------------------------------------------------------------
SIDES = (1, 2, 3, 7, 111, 112, 223, 224, 225, 447, 448, 449, 1079, 1919)


def boxes_for_window_sides(limit, axis, sides):
    """For each side s <= limit a box interval (lo, hi) whose window along `axis` (0: rows, margin 1/10; 1: columns, 1/5) is
    exactly s pixels long on a frame of `limit` pixels, found with the host's own arithmetic (whenet_frame_rects).  The candidate
    lengths go in quarter pixels up to the frame's own (at least 2000 pixels), so every side up to `limit` is found."""
    steps = max(8000, 4 * limit)
    lo = np.repeat(np.array([0.0, 3.25, 40.5], np.float32), steps)
    hi = lo + np.tile(np.arange(1, steps + 1, dtype=np.float32) * np.float32(0.25), 3)
    b = np.zeros((len(lo), 4), np.float32)
    b[:, axis], b[:, axis + 2] = lo, hi
    b[:, 1 - axis], b[:, 3 - axis] = 10.0, 20.0
    r = _lib.frame_rects(limit if axis == 0 else 64, limit if axis == 1 else 64, b)
    length = r[:, axis + 2] - r[:, axis]
    out = {}
    for s in sides:
        if s <= limit:
            i = np.flatnonzero(length == s)
            assert len(i), (axis, s)
            out[s] = (float(lo[i[-1]]), float(hi[i[-1]]))          # (the candidate farthest from the origin)
    return out


def test_plans_equal_the_host_crop_plan_bitwise(post):
    fh, fw = 1080, 1920
    ys, xs = boxes_for_window_sides(fh, 0, SIDES), boxes_for_window_sides(fw, 1, SIDES)
    assert sorted(ys) == [s for s in SIDES if s <= fh] and sorted(xs) == list(SIDES)
    boxes = np.array([[ys[h][0], xs[w][0], ys[h][1], xs[w][1]] for h in ys for w in xs], np.float32)
    rects, valid, plans = post.op_head_plan(fh, fw, boxes)                       # one launch
    assert rects.tobytes() == _lib.frame_rects(fh, fw, boxes).tobytes() and valid.all()
    got = {(int(r[2] - r[0]), int(r[3] - r[1])) for r in rects}
    assert got == {(h, w) for h in ys for w in xs} and (448, 448) in got
    for r, p in zip(rects, plans):
        want = _lib.crop_plan(r)
        assert p.tobytes() == want.tobytes(), (r.tolist(), np.flatnonzero(p != want)[:8].tolist())
    assert sum(int(p[4]) for p in plans) == 1                                      # the 2x-shrink flag: the 448 x 448 window alone
    # a window that fails check_rects: zeros in the place of its plan
    rects, valid, plans = post.op_head_plan(fh, fw, np.array([[2000, 10, 2100, 50], [10, 10, 50, 50]], np.float32))
    assert valid.tolist() == [0, 1] and not plans[0].any() and plans[1].tobytes() == _lib.crop_plan(rects[1]).tobytes()


def test_plans_equal_the_host_crop_plan_for_every_source_size(post):
    """Every source size 1..2048 on both axes in one launch of 2048 boxes (op_head_plan's limit): box i has a window of 2049 - s rows
    by s columns, the pairing of tests/test_head_plan_cpu.py, which holds the host's tables to the oracle for the same sizes."""
    fh = fw = 2304
    sizes = list(range(1, 2049))
    ys, xs = boxes_for_window_sides(fh, 0, sizes), boxes_for_window_sides(fw, 1, sizes)
    assert sorted(ys) == sizes and sorted(xs) == sizes                          # the search found every size on both axes
    boxes = np.array([[ys[2049 - s][0], xs[s][0], ys[2049 - s][1], xs[s][1]] for s in sizes], np.float32)
    rects, valid, plans = post.op_head_plan(fh, fw, boxes)                       # one launch
    assert rects.tobytes() == _lib.frame_rects(fh, fw, boxes).tobytes() and valid.all()
    assert [(int(r[2] - r[0]), int(r[3] - r[1])) for r in rects] == [(2049 - s, s) for s in sizes]
    bad = [(int(r[2] - r[0]), int(r[3] - r[1])) for r, p in zip(rects, plans) if p.tobytes() != _lib.crop_plan(r).tobytes()]
    assert not bad, bad[:8]
    # The FMA-sensitive entry: source size 32, d = 3.  float((3 + 0.5) * (32 / 224) - 0.5) is 0.0 with every operation rounded on its
    # own and -2.8e-17 as one fused multiply-add, the only (size, d) pair of 1..4096 x 0..223 where the two differ.  Vertically that
    # flips (yofs, b0, b1) from (0, 2048, 0) to (-1, 0, 2048); horizontally the s < 0 clamp hides it.
    tall = plans[sizes.index(2049 - 32)]
    assert tall[2] == 32
    yofs, b0, b1 = tall[8:].reshape(6, 224)[3:]
    assert (int(yofs[3]), int(b0[3]), int(b1[3])) == (0, 2048, 0)


# ---- 3. fused = two-step, bitwise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_fused_submission_is_bitwise_the_two_step_path(models, detect_args, name, kind):
    kw = kwargs(detect_args, name)
    frame = DC.sample_frame(0)
    assert frame.shape == (224, 528, 3)
    with FramePipeline(models[name], depth=1) as fp:
        got = fused(fp, frame, kw)
        valid = got[7]
        det, heads = two_step(fp, frame, kw, valid)
    count = len(got[4])
    print(f"{name}: {count} detections, {int((valid != 0).sum())} with a window, sides "
          f"{[(int(r[2] - r[0]), int(r[3] - r[1])) for r in got[0]]}")
    assert 3 <= count <= kw["max_boxes"] and (valid != 0).sum() >= 1
    assert np.array_equal(valid != 0, check_rects(224, 528, _lib.frame_rects(224, 528, got[4])))
    assert_fused_is_two_step(got, det, heads)
    assert not np.isnan(got[1]).any()


# ---- 4. heads without a window, and an empty frame ----------------------------------------------------------------------------
def test_heads_without_a_window_are_skipped_and_reported(models, detect_args):
    """Smaller and smaller top-left corners of the sample frame: the seeded detectors' boxes are scaled to the frame, and some
    of them end up with an empty window.  Every (detector, frame) is compared with the two-step path; at least one of them has
    to hold a detection without a window."""
    seen = 0
    for name, _ in DC.KINDS:
        kw = kwargs(detect_args, name)
        h = models[name]._handle
        fp = FramePipeline(models[name], depth=1)
        for fh, fw in ((97, 131), (61, 83), (40, 150), (33, 33)):
            frame = np.ascontiguousarray(DC.sample_frame(0)[:fh, :fw])
            t = h.frame_begin(frame)
            cap = h.frame_detect_heads(t, kw["anchors"], 1, kw["size"], kw["score"], kw["iou"], kw["max_boxes"])
            boxes, scores, classes, rects, valid, ypr, amax, logits = h.collect_detect(t, cap, want_logits=True)
            ok = check_rects(fh, fw, _lib.frame_rects(fh, fw, boxes)) if len(boxes) else np.zeros(0, bool)
            print(f"{name} {fh}x{fw}: {len(boxes)} detections, {int((~ok).sum())} without a window")
            assert np.array_equal(valid != 0, ok)
            assert np.isnan(ypr[~ok]).all() and (amax[~ok] == -1).all() and np.isnan(logits[~ok]).all()
            assert not np.isnan(ypr[ok]).any() and not np.isnan(logits[ok]).any()
            seen += int((~ok).sum())
            got = fused(fp, frame, kw)
            assert got[7].tobytes() == valid.tobytes() and got[1].tobytes() == ypr[ok, 0].tobytes()
            det, heads = two_step(fp, frame, kw, valid)
            assert_fused_is_two_step(got, det, heads)
    if seen == 0:
        pytest.skip("no seeded detection fell outside any of the shrunken frames")


@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_a_frame_without_detections(models, detect_args, name, kind):
    kw = kwargs(detect_args, name, score=1.0)
    frame = DC.sample_frame(0)
    with FramePipeline(models[name], depth=1) as fp:
        got = fused(fp, frame, kw)
        assert [len(g) for g in got] == [0] * 8 and got[0].shape == (0, 4) and got[4].shape == (0, 4)
        fp.begin(frame)
        assert len(fp.detect(**kw)[0]) == 0
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
        again = fused(fp, frame, kwargs(detect_args, name))                       # the handle stays usable
        assert len(again[4]) >= 3


# ---- 5. order, replay and depth ----------------------------------------------------------------------------------------------
def test_order_replay_and_depth(models, detect_args):
    name = "tiny"
    kw = kwargs(detect_args, name)
    A, B = DC.sample_frame(0), DC.sample_frame(1)
    assert A.shape != B.shape                                                      # (the letterbox tables are re-staged in between)
    with FramePipeline(models[name], depth=1) as fp:
        a1, b1 = fused(fp, A, kw), fused(fp, B, kw)
        sub = two_step(fp, A, kw, a1[7])[1]
    assert len(a1[4]) >= 3 and len(b1[4]) >= 1
    with FramePipeline(models[name], depth=2) as fp:
        fp.begin(A)
        fp.detect_heads(**kw)
        fp.begin(B)
        fp.detect_heads(**kw)
        assert fp.in_flight == 2
        a2, b2 = fp.collect(detections=True), fp.collect(detections=True)
        # A again, a plain submission in between, B, A: collected in submission order
        fp.begin(A)
        fp.detect_heads(**kw)
        fp.submit(A, a1[4][a1[7] != 0])
        a3, s3 = fp.collect(detections=True), fp.collect()
        fp.begin(B)
        fp.detect_heads(**kw)
        fp.begin(A)
        fp.detect_heads(**kw)
        b4, a4 = fp.collect(detections=True), fp.collect(detections=True)
    for want, gots in ((a1, (a2, a3, a4)), (b1, (b2, b4))):
        for got in gots:
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes()
    for g, w in zip(s3, sub):
        assert g.tobytes() == w.tobytes()


# ---- 6. misuse ----------------------------------------------------------------------------------------------------------------
def test_misuse_is_reported_and_the_handle_stays_usable(models, detect_args, post):
    import whenet
    kw = kwargs(detect_args, "tiny")
    args = (kw["anchors"], 1, kw["size"], kw["score"], kw["iou"])
    frame = DC.sample_frame(0)
    crops = np.load(os.path.join(GOLDEN, "golden_crops.npy"))[:2]
    # no detector on the handle
    bare = whenet.WHENet(dtype="f16")
    try:
        h = bare._handle
        t = h.frame_begin(frame)
        with pytest.raises(ValueError, match="no detector is loaded"):
            h.frame_detect_heads(t, *args, 20)
        h.frame_heads(t, np.zeros((0, 4), np.int32))
        h.collect(t, 0)
        assert h.forward(crops)[0].shape == (2, 3)
    finally:
        bare.close()
    # a post-processing handle: no network to run the heads through
    t = post.frame_begin(frame)
    with pytest.raises(ValueError, match="without a network"):
        post.frame_detect_heads(t, *args, 20)
    post.frame_heads(t, np.zeros((0, 4), np.int32))
    post.collect(t, 0)
    assert post.op_head_plan(224, 528, np.array([[10, 10, 50, 50]], np.float32))[1].tolist() == [1]
    with pytest.raises(ValueError, match="op_head_plan"):
        post.op_head_plan(224, 528, np.zeros((2049, 4), np.float32))
    with pytest.raises(ValueError, match="op_head_plan"):
        post.op_head_plan(224, 528, np.zeros((0, 4), np.float32))
    # classes x max_boxes beyond the forward's capacity, then the same ticket with a legal one
    h = models["tiny"]._handle
    t = h.frame_begin(frame)
    for bad in (65, 0):
        with pytest.raises(ValueError, match="must be 1..64"):
            h.frame_detect_heads(t, *args, bad)
    cap = h.frame_detect_heads(t, *args, 64)
    assert cap == 64
    # a ticket whose heads are already enqueued
    with pytest.raises(ValueError, match="frame_detect_heads"):
        h.frame_detect_heads(t, *args, 64)
    with pytest.raises(ValueError, match="frame_heads"):
        h.frame_heads(t, np.zeros((0, 4), np.int32))
    # whenet_collect on a detect ticket, a capacity below the submission's, then the right call
    with pytest.raises(ValueError, match="collect_detect returns it"):
        h.collect(t, 3)
    with pytest.raises(ValueError, match="capacity"):
        h.collect_detect(t, 20)
    res64 = h.collect_detect(t, cap)
    t = h.frame_begin(frame)
    res20 = h.collect_detect(t, h.frame_detect_heads(t, *args, 20))
    for a, b in zip(res64[:7], res20[:7]):                                         # (7 detections either way: the padding changes nothing)
        assert a.tobytes() == b.tobytes()
    # whenet_collect_detect on plain tickets
    t = h.frame_begin(frame)
    with pytest.raises(ValueError, match="not submitted by frame_detect_heads"):
        h.collect_detect(t, 20)
    h.frame_heads(t, _lib.frame_rects(224, 528, np.array([[10, 10, 100, 100]], np.float32)))
    with pytest.raises(ValueError, match="not submitted by frame_detect_heads"):
        h.collect_detect(t, 20)
    assert h.collect(t, 1)[0].shape == (1, 3)
    with pytest.raises(ValueError, match="unknown or already collected"):
        h.collect_detect(t, 20)
    assert h.forward(crops)[0].shape == (2, 3)
