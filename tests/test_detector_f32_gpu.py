"""The float32 detector body on the GPU (option "detector_dtype" = 1: csrc/dconv.hip on v_mfma_f32_32x32x2_f32, csrc/detector.cpp):
single layers bitwise on exact integers -- small ones, and wide ones that binary16 cannot hold --, pools bitwise, random operands
and the whole bodies against float64 at float32-grade bounds (tests/golden/reference_detector_f32.json), batch invariance, the
boxes and crop windows of the float64 oracle, the compositions of the frame / clip paths on the f32 detector, and the option's
default and misuse."""
import numpy as np
import pytest

from tests import detector_cases as DC
from tests import detector_f32_cases as FC
from tests import detector_ref as R
from whenet_hip import _lib, detector_weights as DW
from whenet_hip.frames import FramePipeline

pytestmark = pytest.mark.gpu
FRAME_HW = (224, 528)


@pytest.fixture(scope="module")
def metas():
    return FC.load_meta()


@pytest.fixture(scope="module")
def arrays():
    return FC.load_maps()


@pytest.fixture(scope="module")
def post32():
    h = _lib.Handle.postproc(0)
    h.set_option("detector_dtype", 1)
    yield h
    h.close()


@pytest.fixture(scope="module")
def detectors32():
    """One handle per body with the fixture's synthetic detector attached as float32."""
    hs = {}
    for name, kind in DC.KINDS:
        h = _lib.Handle.postproc(0)
        h.detector_load(DW.pack(DW.synthetic(kind, DC.SEEDS[name])), dtype="f32")
        hs[name] = h
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def tiny_model():
    """A seeded f16 pose model with the tiny detector attached as float32 (the compositions)."""
    import whenet
    m = whenet.WHENet(dtype="f16")
    m._handle.detector_load(DW.pack(DW.synthetic(1, DC.SEEDS["tiny"])), dtype="f32")
    yield m
    m.close()


def run_conv(h, c, x, x2, kernel, bias, skip, leaky):
    return h.op_dconv(x, kernel, bias, stride=c["stride"], leaky=leaky, x2=x2, skip=skip, f32_out=c["f32_out"])


def detect_kw(metas, name):
    d = metas[0]["detect"][name]
    return dict(size=tuple(d["size"]), score=d["score"], iou=d["iou"], max_boxes=d["max_boxes"],
                anchors=np.array(DC.ANCHORS[name], np.float32).reshape(-1, 2), num_classes=1)


def hargs(kw):
    return (kw["anchors"], kw["num_classes"], kw["size"], kw["score"], kw["iou"], kw["max_boxes"])


def check_rects(fh, fw, r):
    return (r[:, 0] >= 0) & (r[:, 1] >= 0) & (r[:, 2] <= fh) & (r[:, 3] <= fw) & (r[:, 0] < r[:, 2]) & (r[:, 1] < r[:, 3])


def assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


# ---- 1. exact integers, bitwise ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,c", DC.CONV_CASES, ids=[n for n, _ in DC.CONV_CASES])
def test_conv_exact_integers_bitwise(post32, name, c):
    x, x2, kernel, bias, skip = DC.integer_operands(c)
    leaky = not c["f32_out"]
    want, bound = FC.expected_f32(c, x, x2, kernel, bias, skip, leaky)
    assert bound < 2048, bound
    assert np.abs(want).max() > 3 and len(np.unique(want)) > 8
    got = run_conv(post32, c, x, x2, kernel, bias, skip, leaky)
    assert got.shape == want.shape and np.array_equal(got, want), (name, np.abs(got - want).max(), np.argwhere(got != want)[:4])


# ---- 2. wide integers, bitwise -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.WIDE_CASES)
def test_conv_wide_integers_bitwise(post32, name):
    """Operands binary16 cannot hold: fails on the binary16 kernels (and on a library without the option)."""
    c = FC.CASES[name]
    x, x2, kernel, bias, skip = FC.wide_operands(c)
    want, bound = FC.expected_f32(c, x, x2, kernel, bias, skip, True)
    assert bound < 2 ** 24, bound                # sum |w||x| + |bias| + |skip|: every partial sum is an exact float32 integer
    with np.errstate(over="ignore"):
        assert (R.r16(x) != x).any() and np.abs(x).max() > 65504
    got = run_conv(post32, c, x, x2, kernel, bias, skip, True)
    assert got.shape == want.shape and np.array_equal(got, want), (name, np.abs(got - want).max(), np.argwhere(got != want)[:4])


# ---- 3. pools, bitwise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", DC.POOL_CASES, ids=[n for n, _ in DC.POOL_CASES])
@pytest.mark.parametrize("negative", [False, True])
def test_pool_bitwise(post32, name, shape, negative):
    n, h, w, c, stride = shape
    rng = np.random.RandomState(DC.case_seed(name))
    x = (rng.normal(0, 2, (n, h, w, c)) * (1 + 2.0 ** -13)).astype(np.float32)
    if negative:
        x = (-np.abs(x) - 1).astype(np.float32)             # padding (zeros, were it read) must not win the max
    assert (R.r16(x) != x).mean() > 0.5                     # values binary16 would round
    got = post32.op_dpool(x, stride)
    assert np.array_equal(got, R.pool(x, stride))


# ---- 4. random operands against float64 ----------------------------------------------------------------------------------
RANDOM = [(n, "random") for n, _ in DC.CONV_CASES] + [(n, "wide") for n in FC.WIDE_CASES]


@pytest.mark.parametrize("name,kind", RANDOM, ids=[f"{n}-{k}" for n, k in RANDOM])
def test_conv_against_float64(post32, metas, name, kind):
    """|got - ref| <= 2^-23 |ref| + 4 e32 per element: one float32 ulp of the expected value, and four times the deviation of a
    float32 CPU evaluation from the float64 one (recorded when the fixtures were made) for the matrix cores' other summation
    order.  The random operands are those of the binary16 test; the wide ones are tests/detector_f32_cases.py's."""
    c = FC.CASES[name]
    x, x2, kernel, bias, skip = DC.random_operands(c, DC.case_seed(name)) if kind == "random" else FC.wide_operands(c)
    leaky = not c["f32_out"]
    e32 = metas[0]["e32"][name] if kind == "random" else metas[1]["e32"][name]
    ref = R.conv(x, kernel, bias, c["stride"], leaky, x2=x2, skip=skip, dtype=np.float64)
    got = run_conv(post32, c, x, x2, kernel, bias, skip, leaky).astype(np.float64)
    excess = np.abs(got - ref) - (2.0 ** -23 * np.abs(ref) + 4 * e32)
    err = np.abs(got - ref).max()
    print(f"F32FIG conv {name}-{kind}: max |got - ref| = {err:.3e}, e32 = {e32:.3e}, ratio to 4 e32 = {err / (4 * e32):.3f}, "
          f"worst excess = {excess.max():.3e}")
    assert excess.max() <= 0, (name, float(excess.max()))


# ---- 5. whole bodies against the executed reference ----------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
@pytest.mark.parametrize("size", DC.SIZES, ids=["32x32", "64x96"])
def test_body_against_the_executed_reference(detectors32, metas, arrays, name, kind, size):
    """Per map max |got - ref| / rms(ref) <= 4 x the same figure of a float32 CPU evaluation (the 4 is for another summation order,
    as in the single layers): about 200 x below the binary16 emulation's figure."""
    h, w = size
    maps = detectors32[name].detector_forward(DC.fixture_image(h, w), kind, 18)
    assert len(maps) == (3 if kind == 0 else 2)
    for l, m in enumerate(maps):
        ref = arrays[f"{name}/{h}x{w}/map{l}"]
        err, e32 = FC.body_error(m, ref), metas[1]["e32_body"][f"{name}/{h}x{w}"][l]
        print(f"F32FIG body {name} {h}x{w} map {l}: gpu {err:.3e}, cpu float32 {e32:.3e}, ratio to 4 e32_body = {err / (4 * e32):.3f}, "
              f"binary16 emulation {metas[0]['emu_err'][f'{name}/{h}x{w}'][l]:.3e}")
        assert m.shape == ref.shape and err <= 4 * e32, (name, size, l, err, e32)


# ---- 6. batch invariance, bitwise ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,size", [("tiny", 1, (64, 96)), ("full", 0, (32, 32))])
def test_batch_invariance_bitwise(detectors32, name, kind, size):
    h = detectors32[name]
    a, b = DC.fixture_image(*size, 0), DC.fixture_image(*size, 1)
    c = np.ascontiguousarray(a[:, ::-1])
    alone = h.detector_forward(a, kind, 18)
    batch = h.detector_forward(np.concatenate([a, b, a]), kind, 18)
    other = h.detector_forward(np.concatenate([b, c, c]), kind, 18)
    for m0, m1, m2 in zip(alone, batch, other):
        assert m0[0].tobytes() == m1[0].tobytes() == m1[2].tobytes()
        assert m1[1].tobytes() == m2[0].tobytes() and m1[1].tobytes() != m1[0].tobytes()


# ---- 7. boxes and windows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_boxes_and_windows_are_the_oracles(detectors32, metas, name, kind):
    meta, rec = metas
    d, r = meta["detect"][name], rec["detect"][name]
    kw = detect_kw(metas, name)
    boxes, scores, classes = detectors32[name].op_detect(DC.sample_frame(0), *hargs(kw), bgr=True)
    assert len(boxes) == d["oracle_count"] and not classes.any()
    dist = FC.box_distance(boxes, r["oracle_boxes"])
    ds = float(np.abs(scores.astype(np.float64) - np.array(r["oracle_scores"])).max())
    print(f"F32FIG detect {name}: {len(boxes)} boxes, max distance {dist:.3e} px (cpu float32 {r['f32_box_px']:.3e}, ratio to 4 x = "
          f"{dist / (4 * r['f32_box_px']):.3f}), max score difference {ds:.3e} (cpu float32 {r['f32_score']:.3e}, ratio to 4 x = "
          f"{ds / (4 * r['f32_score']):.3f})")
    assert dist <= 4 * r["f32_box_px"] and ds <= 4 * r["f32_score"]
    assert _lib.frame_rects(*FRAME_HW, boxes).tolist() == r["oracle_windows"]


# ---- 8. composition, bitwise, on the f32 detector ------------------------------------------------------------------------
def test_compositions_bitwise(tiny_model, metas):
    m, h = tiny_model, tiny_model._handle
    kw = detect_kw(metas, "tiny")
    frame, frame1 = DC.sample_frame(0), DC.sample_frame(1)
    # op_detect = yolo_eval(detector_forward(op_letterbox))
    _, image = h.op_letterbox(frame, kw["size"], bgr=True, want_u8=False)
    maps = h.detector_forward(image[None], 1, 18)
    want = h.yolo_eval(maps, kw["anchors"], 1, frame.shape[:2], score_threshold=kw["score"], iou_threshold=kw["iou"], max_boxes=kw["max_boxes"])
    got = h.op_detect(frame, *hargs(kw), bgr=True)
    assert 3 <= len(got[0]) <= kw["max_boxes"]
    assert_same(got, want)
    # frame_detect = op_detect
    t = h.frame_begin(frame, bgr=True)
    res = h.frame_detect(t, *hargs(kw))
    h.frame_heads(t, np.zeros((0, 4), np.int32))
    h.collect(t, 0)
    assert_same(res, got)
    with FramePipeline(m, depth=1) as fp:
        # detect_heads = detect + heads
        singles = []
        for f in (frame, frame1[:224, :528], frame1):
            f = np.ascontiguousarray(f)
            fp.begin(f)
            fp.detect_heads(**kw)
            fused = fp.collect(detections=True)
            singles.append(fused)
            fp.begin(f)
            det = fp.detect(**kw)
            fp.heads(det[0][fused[7] != 0])
            heads = fp.collect()
            assert_same(fused[4:7], det)
            assert_same(fused[:4], heads)
        assert_same(singles[0][4:7], got)
        assert len(singles[0][0]) >= 1
        # a clip of 2 = its frames one by one
        fp.begin_clip(np.stack([frame, np.ascontiguousarray(frame1[:224, :528])]))
        fp.detect_heads_clip(**kw)
        clip, (used, over) = fp.collect_clip(detections=True)
        assert over == 0 and len(clip) == 2
        assert_same(clip[0], singles[0])
        assert_same(clip[1], singles[1])
        # a mixed clip of 2 sizes = its frames one by one
        fp.begin_clip_mixed([frame, frame1])
        fp.detect_heads_clip(**kw)
        mixed, (used, over) = fp.collect_clip(detections=True)
        assert over == 0 and len(mixed) == 2
        assert_same(mixed[0], singles[0])
        assert_same(mixed[1], singles[2])
        assert singles[0][4].tobytes() != singles[2][4].tobytes()


# ---- 9. whole frame ------------------------------------------------------------------------------------------------------
def test_whole_frame_windows_and_angles(metas):
    """FramePipeline.detect_heads with the f32 detector and the default pose dtype: the windows are the float64 oracle's, and the
    angles are, bitwise, get_angle of the crops whenet_op_crop_resize cuts at those windows."""
    import whenet
    from whenet_hip.detector import YOLO
    d, r = metas[0]["detect"]["tiny"], metas[1]["detect"]["tiny"]
    frame = DC.sample_frame(0)
    m = whenet.WHENet()
    try:
        yolo = YOLO(model_path=DW.synthetic(1, DC.SEEDS["tiny"]), anchors_path=DC.ANCHORS["tiny"], classes_path=["head"], score=d["score"],
                    iou=d["iou"], model_image_size=tuple(d["size"]), handle=m, dtype="f32")
        assert yolo.dtype == "f32"
        with FramePipeline(m, depth=1) as fp:
            fp.begin(frame)
            fp.detect_heads(size=tuple(d["size"]), score=d["score"], iou=d["iou"], max_boxes=d["max_boxes"])
            rects, yaw, pitch, roll, boxes, scores, classes, valid = fp.collect(detections=True)
        windows = np.array(r["oracle_windows"], np.int32)
        ok = check_rects(*FRAME_HW, windows)
        assert len(boxes) == d["oracle_count"] and np.array_equal(valid != 0, ok) and ok.sum() >= 1
        assert np.array_equal(rects, windows[ok])
        crops = m._handle.op_crop_resize(frame, windows[ok], bgr=True)
        want = m.get_angle(crops)
        assert yaw.tobytes() == np.asarray(want[0], np.float32).tobytes() and pitch.tobytes() == np.asarray(want[1], np.float32).tobytes() \
            and roll.tobytes() == np.asarray(want[2], np.float32).tobytes()
        assert not np.isnan(yaw).any()
    finally:
        m.close()


# ---- 10. default unchanged and misuse ------------------------------------------------------------------------------------
def test_default_is_binary16_and_misuse_is_reported(detectors32):
    blob = DW.pack(DW.synthetic(1, DC.SEEDS["tiny"]))
    img = DC.fixture_image(32, 32)
    c = FC.CASES["k3s1_5x7"]
    ops = DC.random_operands(c, 5)
    plain, explicit = _lib.Handle.postproc(0), _lib.Handle.postproc(0)
    try:
        explicit.set_option("detector_dtype", 0)
        outs = []
        for h in (plain, explicit):
            h.detector_load(blob)
            outs.append(h.detector_forward(img, 1, 18) + [run_conv(h, c, *ops, True), h.op_dpool(ops[0], 2)])
        for a, b in zip(*outs):
            assert a.tobytes() == b.tobytes()
        f32 = detectors32["tiny"].detector_forward(img, 1, 18)
        assert all(a.tobytes() != b.tobytes() for a, b in zip(outs[0], f32))                 # the option selects other kernels
        assert np.array_equal(outs[0][2], R.r16(outs[0][2]))                                 # the default layer stores binary16
        # value 2; a change with a detector attached; the handle stays usable and keeps its dtype
        with pytest.raises(ValueError, match="detector_dtype must be 0"):
            plain.set_option("detector_dtype", 2)
        with pytest.raises(ValueError, match="load again"):
            plain.set_option("detector_dtype", 1)
        with pytest.raises(ValueError, match="load again"):
            plain.detector_load(blob, dtype="f32")
        with pytest.raises(ValueError, match="load again"):
            detectors32["tiny"].set_option("detector_dtype", 0)
        plain.set_option("detector_dtype", 0)                                                 # (the value it has: accepted)
        again = plain.detector_forward(img, 1, 18)
        for a, b in zip(again, outs[0]):
            assert a.tobytes() == b.tobytes()
        for a, b in zip(detectors32["tiny"].detector_forward(img, 1, 18), f32):
            assert a.tobytes() == b.tobytes()
    finally:
        plain.close()
        explicit.close()
    from whenet_hip.detector import YOLO
    with pytest.raises(ValueError, match="dtype"):
        YOLO(model_path=DW.synthetic(1, DC.SEEDS["tiny"]), anchors_path=DC.ANCHORS["tiny"], classes_path=["head"], dtype="f64")
