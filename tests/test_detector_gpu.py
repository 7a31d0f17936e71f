"""The detector body on the GPU (csrc/dconv.hip, csrc/detector.cpp): single layers bitwise on exact integers and against float64
on random operands, the whole bodies against the executed reference (tests/golden/reference_detector.*), batch invariance, the
composition letterbox -> body -> yolo_eval, replays and misuse."""
import json
import os

import numpy as np
import pytest

from tests import detector_cases as DC
from tests import detector_ref as R
from whenet_hip import _lib, detector_weights as DW

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "reference_detector.npz")) as z:
        return meta, {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def detectors():
    """One handle per body with the fixture's synthetic detector attached."""
    hs = {}
    for name, kind in DC.KINDS:
        h = _lib.Handle.postproc(0)
        h.detector_load(DW.pack(DW.synthetic(kind, DC.SEEDS[name])))
        hs[name] = h
    yield hs
    for h in hs.values():
        h.close()


def run_conv(h, c, x, x2, kernel, bias, skip, leaky):
    return h.op_dconv(x, kernel, bias, stride=c["stride"], leaky=leaky, x2=x2, skip=skip, f32_out=c["f32_out"])


# ---- 6. exact integers, bitwise ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,c", DC.CONV_CASES, ids=[n for n, _ in DC.CONV_CASES])
def test_conv_exact_integers_bitwise(post, name, c):
    x, x2, kernel, bias, skip = DC.integer_operands(c)
    leaky = not c["f32_out"]
    want, bound = DC.integer_expected(c, x, x2, kernel, bias, skip, leaky)
    assert bound < 2048, bound                   # every partial sum is exact in binary16 and float32, in any order
    assert np.abs(want).max() > 3 and len(np.unique(want)) > 8            # (the case says something)
    got = run_conv(post, c, x, x2, kernel, bias, skip, leaky)
    assert got.shape == want.shape and np.array_equal(got, want), (name, np.abs(got - want).max(), np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name,shape", DC.POOL_CASES, ids=[n for n, _ in DC.POOL_CASES])
@pytest.mark.parametrize("negative", [False, True])
def test_pool_bitwise(post, name, shape, negative):
    n, h, w, c, stride = shape
    rng = np.random.RandomState(DC.case_seed(name))
    x = rng.normal(0, 2, (n, h, w, c)).astype(np.float16).astype(np.float32)
    if negative:
        x = (-np.abs(x) - 1).astype(np.float16).astype(np.float32)          # padding (zeros, were it read) must not win the max
    got = post.op_dpool(x, stride)
    assert np.array_equal(got, R.pool(x, stride))


# ---- 7. random operands against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,c", DC.CONV_CASES, ids=[n for n, _ in DC.CONV_CASES])
def test_conv_random_against_float64(post, fixture, name, c):
    """|got - ref| <= 2^-10 |ref| + 4 e32 per element: one binary16 ulp of the expected value for the one output rounding, and
    four times the deviation of a float32 CPU evaluation from the float64 one (measured when the fixture was made) for the
    matrix cores' other summation order."""
    x, x2, kernel, bias, skip = DC.random_operands(c, DC.case_seed(name))
    leaky = not c["f32_out"]
    ref = R.conv(x, kernel, bias, c["stride"], leaky, x2=x2, skip=skip, dtype=np.float64)
    got = run_conv(post, c, x, x2, kernel, bias, skip, leaky).astype(np.float64)
    e32 = fixture[0]["e32"][name]
    excess = np.abs(got - ref) - (2.0 ** -10 * np.abs(ref) + 4 * e32)
    print(f"{name}: max |got - ref| = {np.abs(got - ref).max():.3e}, e32 = {e32:.3e}, worst excess = {excess.max():.3e}")
    assert excess.max() <= 0, (name, float(excess.max()))


# ---- 8. whole bodies against the executed reference ----------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
@pytest.mark.parametrize("size", DC.SIZES, ids=["32x32", "64x96"])
def test_body_against_the_executed_reference(detectors, fixture, name, kind, size):
    """Per map max |got - ref| / rms(ref) <= 3 x the same figure of the CPU emulation of binary16 storage (the 3 is for another
    summation order through up to 75 layers)."""
    meta, arrays = fixture
    h, w = size
    maps = detectors[name].detector_forward(DC.fixture_image(h, w), kind, 18)
    assert len(maps) == (3 if kind == 0 else 2)
    for l, m in enumerate(maps):
        ref = arrays[f"{name}/{h}x{w}/map{l}"]
        err = float(np.abs(m - ref).max() / np.sqrt(np.mean(ref ** 2)))
        emu = meta["emu_err"][f"{name}/{h}x{w}"][l]
        print(f"{name} {h}x{w} map {l}: gpu {err:.3e}, emulation {emu:.3e}, ratio {err / emu:.2f}")
        assert m.shape == ref.shape and err <= 3 * emu, (name, size, l, err, emu)


# ---- 9. batch invariance, bitwise ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_batch_invariance_bitwise(detectors, name, kind):
    h = detectors[name]
    a, b = DC.fixture_image(64, 96, 0), DC.fixture_image(64, 96, 1)
    c = np.ascontiguousarray(a[:, ::-1])
    alone = h.detector_forward(a, kind, 18)
    first = h.detector_forward(np.concatenate([a, b, c]), kind, 18)
    last = h.detector_forward(np.concatenate([b, c, a]), kind, 18)
    for m0, m1, m2 in zip(alone, first, last):
        assert m0[0].tobytes() == m1[0].tobytes() == m2[2].tobytes()
        assert m1[1].tobytes() == m2[0].tobytes() and m1[1].tobytes() != m1[0].tobytes()


# ---- 10. composition, bitwise --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_detect_is_letterbox_body_yolo_eval(detectors, fixture, name, kind):
    h = detectors[name]
    d = fixture[0]["detect"][name]
    size, kw = tuple(d["size"]), dict(max_boxes=d["max_boxes"])
    anchors = np.array(DC.ANCHORS[name], np.float32).reshape(-1, 2)
    frame = DC.sample_frame(0)
    _, image = h.op_letterbox(frame, size, bgr=True, want_u8=False)
    maps = h.detector_forward(image[None], kind, 18)
    want = h.yolo_eval(maps, anchors, 1, frame.shape[:2], score_threshold=d["score"], iou_threshold=d["iou"], **kw)
    got = h.op_detect(frame, anchors, 1, size, d["score"], d["iou"], bgr=True, **kw)
    assert 3 <= len(got[0]) <= d["max_boxes"]
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    # replay: the same call again, and after another size in between
    again = h.op_detect(frame, anchors, 1, size, d["score"], d["iou"], bgr=True, **kw)
    h.op_detect(frame, anchors, 1, (32, 32), d["score"], d["iou"], bgr=True, **kw)
    third = h.op_detect(frame, anchors, 1, size, d["score"], d["iou"], bgr=True, **kw)
    for g, a, t in zip(got, again, third):
        assert g.tobytes() == a.tobytes() == t.tobytes()
    # the resident frame
    ticket = h.frame_begin(frame, bgr=True)
    res = h.frame_detect(ticket, anchors, 1, size, d["score"], d["iou"], **kw)
    h.frame_heads(ticket, np.zeros((0, 4), np.int32))
    h.collect(ticket, 0)
    for g, r in zip(got, res):
        assert g.tobytes() == r.tobytes()


def test_frame_pipeline_detect_then_heads():
    """fp.begin; fp.detect; fp.heads; fp.collect returns the windows and angles of fp.submit(frame, boxes)."""
    import whenet
    from whenet_hip.detector import YOLO
    from whenet_hip.frames import FramePipeline
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        d = json.load(f)["detect"]["tiny"]
    m = whenet.WHENet(dtype="f16")
    try:
        yolo = YOLO(model_path=DW.synthetic(1, DC.SEEDS["tiny"]), anchors_path=DC.ANCHORS["tiny"], classes_path=["head"],
                    score=d["score"], iou=d["iou"], model_image_size=tuple(d["size"]), handle=m)
        frame = DC.sample_frame(0)
        want_boxes = yolo.detect(np.ascontiguousarray(frame[:, :, ::-1]))[0]
        assert 3 <= len(want_boxes) <= 20

        def inside(b):                           # random-weight boxes may lie outside the frame: keep what has a window
            lo = np.maximum(b[:, :2], 0)
            hi = np.minimum(b[:, 2:], np.array(frame.shape[:2], np.float32))
            return np.ascontiguousarray(np.concatenate([lo, hi], 1)[(hi > lo + 1).all(1)])

        for depth in (1, 2):
            with FramePipeline(m, depth=depth) as fp:
                if depth == 1:
                    fp.attach_detector(yolo)         # (depth 2: found on the model's handle)
                fp.begin(frame)
                b, s, c = fp.detect(size=tuple(d["size"]), score=d["score"], iou=d["iou"])
                assert b.tobytes() == want_boxes.tobytes() and len(s) == len(c) == len(b)
                fp.heads(inside(b))
                got = fp.collect()
                fp.submit(frame, inside(b))
                want = fp.collect()
            assert len(got[0]) >= 1
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes()
    finally:
        m.close()


# ---- 11. misuse ----------------------------------------------------------------------------------------------------------
def test_misuse_is_reported_and_the_handle_stays_usable(post, detectors):
    frame = DC.sample_frame(0)
    anchors = np.array(DC.ANCHORS["tiny"], np.float32)
    img = DC.fixture_image(32, 32)
    with pytest.raises(ValueError, match="no detector is loaded"):
        post.detector_forward(img, 1, 18)
    with pytest.raises(ValueError, match="no detector is loaded"):
        post.op_detect(frame, anchors, 1, (32, 32))
    t = post.frame_begin(frame)
    with pytest.raises(ValueError, match="no detector is loaded"):
        post.frame_detect(t, anchors, 1, (32, 32))
    post.frame_heads(t, np.zeros((0, 4), np.int32))
    post.collect(t, 0)
    w = DW.synthetic(1, DC.SEEDS["tiny"])
    names = DW.tensors(1)
    with pytest.raises(ValueError, match="dbn005/gamma"):
        post.detector_load(DW.pack_named([n for n in names if n[0] != "dbn005/gamma"], w))
    bad = dict(w)
    bad["dconv007/kernel"] = np.zeros((3, 3, 256, 500), np.float32)
    with pytest.raises(ValueError, match="dconv007/kernel"):
        post.detector_load(DW.pack_named([(n, bad[n].shape) for n, _ in names], bad))
    with pytest.raises(ValueError, match="not a WHNPACK1"):
        post.detector_load(b"x" * 64)
    assert post.op_letterbox(frame, (32, 32))[0].shape == (32, 32, 3)              # still usable, still without a detector
    h = detectors["tiny"]
    with pytest.raises(ValueError):
        h._check(h._lib.whenet_detector_forward(h._h, _lib._ptr(np.zeros((1, 48, 32, 3), np.float32)), 1, 48, 32, None))
    with pytest.raises(ValueError, match="3 maps with 9 anchors or 2 maps with 6"):
        h.op_detect(frame, np.array(DC.ANCHORS["full"], np.float32), 1, (32, 32))
    t = h.frame_begin(frame)
    h.frame_heads(t, np.zeros((0, 4), np.int32))
    with pytest.raises(ValueError, match="frame_detect"):
        h.frame_detect(t, anchors, 1, (32, 32))
    h.collect(t, 0)
    assert len(h.detector_forward(img, 1, 18)) == 2
