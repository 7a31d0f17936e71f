"""The detector's pre-processing (yolo_v3/utils.py:23-34 `letterbox_image` + yolo_postprocess.py:191-195 `/ 255.`):
the fixture recorded from the executed reference, the numpy restatement of Pillow's 8-bit BICUBIC resample against it,
the library's host tables against the restatement (CPU), and the kernels and the resident-frame pipeline on the GPU --
bit for bit everywhere: it is integer arithmetic."""
import hashlib
import os

import numpy as np
import pytest

from whenet_hip import _lib, synth

from tests import letterbox_cases as LC
from tests import letterbox_ref as R

REF_UTILS = "/root/reference/yolo_v3/utils.py"


@pytest.fixture(scope="module")
def fixture():
    return np.load(LC.FIXTURE)


_expected_cache = {}


def expected_canvas(case):
    """The whole uint8 canvas of a case: the restatement, which test 1 pins to the executed reference."""
    if case.name not in _expected_cache:
        _expected_cache[case.name] = R.letterbox_u8(LC.make_frame(case), *case.box_hw)
    return _expected_cache[case.name]


def check_against_fixture(fixture, case, canvas):
    assert canvas.dtype == np.uint8 and canvas.shape == (*case.box_hw, 3)
    assert hashlib.sha256(canvas.tobytes()).hexdigest() == str(fixture[case.name + "/sha256"]), case.name
    assert np.array_equal(canvas[::8, ::8], fixture[case.name + "/sub"]), case.name
    if case.full:
        assert np.array_equal(canvas, fixture[case.name + "/full"]), case.name


# ------------------------------------------------------------------ CPU
def test_case_list_covers_what_the_fixture_must_hold(fixture):
    pairs = {(c.frame_hw, c.box_hw) for c in LC.GOOD_CASES}
    assert all((f, b) in pairs for f in LC.FRAME_SIZES for b in LC.BOX_SIZES) and len(LC.FRAME_SIZES) * len(LC.BOX_SIZES) == 33
    assert any(c.box_hw[0] != c.box_hw[1] and c.box_hw[0] % 32 and c.box_hw[1] % 32 for c in LC.GOOD_CASES)
    assert [c.frame_hw[0] for c in LC.BAD_CASES] == [1]
    assert {c.recipe for c in LC.CASES} == {"noise", "gradient", "sample0", "sample1"}
    for c in LC.GOOD_CASES:
        assert c.full == (c.name + "/full" in fixture.files)
        assert c.full == (max(c.box_hw) <= 160 or c.recipe.startswith("sample"))
    assert os.path.getsize(LC.FIXTURE) <= 1024 * 1024
    assert str(fixture["pillow_version"])


def test_restatement_reproduces_the_executed_reference(fixture):
    """Hash, subsample and -- where stored -- the whole canvas of every case; the geometry; the float form."""
    for case in LC.GOOD_CASES:
        assert list(R.geometry(*case.frame_hw, *case.box_hw)) == fixture[case.name + "/geom"].tolist(), case.name
        canvas = expected_canvas(case)
        check_against_fixture(fixture, case, canvas)
        x = R.image_data(canvas)
        assert x.dtype == np.float32 and x.shape == (1, *case.box_hw, 3)
        assert np.array_equal(x[0], canvas.astype(np.float32) / 255)
    for case in LC.BAD_CASES:
        assert str(fixture[case.name + "/error"]) == "ValueError"
        with pytest.raises(ValueError):
            R.letterbox_u8(LC.make_frame(case), *case.box_hw)


def test_reference_function_executed_again_reproduces_the_fixture(fixture):
    if not os.path.exists(REF_UTILS):
        pytest.skip("no reference checkout on this machine")
    pytest.importorskip("PIL")
    pytest.importorskip("matplotlib")          # utils.py imports it at module level
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location("reference_yolo_v3_utils", REF_UTILS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for case in LC.GOOD_CASES:
        boxed = mod.letterbox_image(Image.fromarray(LC.make_frame(case), "RGB"), tuple(reversed(case.box_hw)))
        check_against_fixture(fixture, case, np.array(boxed))
    for case in LC.BAD_CASES:
        with pytest.raises(ValueError):
            mod.letterbox_image(Image.fromarray(LC.make_frame(case), "RGB"), tuple(reversed(case.box_hw)))


def test_library_plan_equals_the_restatement():
    """whenet_letterbox_plan is pure host code inside libwhenet_hip.so: geometry and both axes' integer tables of every
    case; a resized side of zero pixels and sizes beyond the documented limits are WHENET_EINVAL."""
    seen = set()
    for case in LC.GOOD_CASES:
        key = (case.frame_hw, case.box_hw)
        if key in seen:
            continue
        seen.add(key)
        (ih, iw), (oh, ow) = key
        geom, axes = _lib.letterbox_plan(ih, iw, oh, ow)
        nw, nh, x0, y0 = R.geometry(ih, iw, oh, ow)
        assert geom == (nw, nh, x0, y0), case.name
        for (ks, bounds, coeffs), (n_in, n_out) in zip(axes, ((iw, nw), (ih, nh))):
            rks, rb, rc = R.axis_tables(n_in, n_out)
            assert ks == rks and np.array_equal(bounds, rb) and np.array_equal(coeffs, rc), (case.name, n_in, n_out)
            # what keeps the kernels inside their buffers
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all()
            assert (bounds[:, 1] <= ks).all()
    for case in LC.BAD_CASES:
        with pytest.raises(ValueError):
            _lib.letterbox_plan(*case.frame_hw, *case.box_hw)
    for bad in [(1, 5000, 416, 416), (5000, 1, 416, 416), (R.MAX_FRAME_SIDE + 1, 100, 416, 416),
                (100, R.MAX_FRAME_SIDE + 1, 416, 416), (100, 100, R.MAX_BOX_SIDE + 1, 416), (100, 100, 416, R.MAX_BOX_SIDE + 1),
                (0, 100, 416, 416), (100, 100, 0, 416), (100, 100, 416, -1)]:
        with pytest.raises(ValueError):
            _lib.letterbox_plan(*bad)
    # the limits themselves are accepted
    geom, _ = _lib.letterbox_plan(R.MAX_FRAME_SIDE, R.MAX_FRAME_SIDE, R.MAX_BOX_SIDE, R.MAX_BOX_SIDE)
    assert geom == (R.MAX_BOX_SIDE, R.MAX_BOX_SIDE, 0, 0)
    # a coefficient array that is too small is refused, not overrun
    import ctypes as C
    g, ks = (C.c_int32 * 4)(), C.c_int(0)
    b, c = np.empty((416, 2), np.int32), np.empty(16, np.int32)
    rc = _lib.load().whenet_letterbox_plan(720, 1280, 416, 416, C.byref(g), 0, b.ctypes.data_as(C.c_void_p),
                                           c.ctypes.data_as(C.c_void_p), c.size, C.byref(ks))
    assert rc == _lib.EINVAL


def test_python_letterbox_asserts_multiples_of_32_like_the_reference():
    from whenet_hip import yolo
    for size in [(416, 400), (250, 333), (0, 416), (416,)]:
        with pytest.raises(ValueError):
            yolo.letterbox(object(), np.zeros((10, 10, 3), np.uint8), size=size)     # refused before the handle is touched


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def model():
    import whenet
    m = whenet.WHENet(dtype="f32")
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["postproc", "model"])
@pytest.mark.parametrize("bgr", [True, False])
def test_op_letterbox_bit_exact(post, model, fixture, which, bgr):
    h = post if which == "postproc" else model._handle
    for case in LC.GOOD_CASES:
        rgb = LC.make_frame(case)
        frame = np.ascontiguousarray(rgb[:, :, ::-1]) if bgr else rgb
        want = expected_canvas(case)
        u8, f32 = h.op_letterbox(frame, case.box_hw, bgr=bgr)
        assert np.array_equal(u8, want), case.name
        check_against_fixture(fixture, case, u8)
        assert f32.dtype == np.float32 and f32.tobytes() == (want.astype(np.float32) / 255).tobytes(), case.name
        # either output alone
        only_u8, none = h.op_letterbox(frame, case.box_hw, bgr=bgr, want_f32=False)
        assert none is None and np.array_equal(only_u8, want)
        none, only_f32 = h.op_letterbox(frame, case.box_hw, bgr=bgr, want_u8=False)
        assert none is None and only_f32.tobytes() == f32.tobytes()
    for case in LC.BAD_CASES:
        with pytest.raises(ValueError):
            h.op_letterbox(LC.make_frame(case), case.box_hw, bgr=bgr)
    # the handle is fine afterwards
    case = LC.GOOD_CASES[0]
    assert np.array_equal(h.op_letterbox(LC.make_frame(case), case.box_hw, bgr=False)[0], expected_canvas(case))


@pytest.mark.gpu
def test_yolo_letterbox_is_the_image_data_of_detect(model):
    from whenet_hip import yolo
    case = next(c for c in LC.GOOD_CASES if c.recipe == "sample0")
    bgr = np.ascontiguousarray(LC.make_frame(case)[:, :, ::-1])
    want = R.image_data(expected_canvas(case))
    for h in (model, model._handle, None):
        got = yolo.letterbox(h, bgr, size=case.box_hw)
        assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert np.array_equal(yolo.letterbox(model, bgr, size=case.box_hw, as_uint8=True), expected_canvas(case))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f32s", "f16"])
def test_resident_frame_equals_submit_frame(dtype):
    """begin -> detector_input -> heads -> collect against FramePipeline.process / submit_frame on the same frames: angles,
    argmax and rects bitwise equal, the canvas equal to the stage alone; depths 1..4 with frames interleaved, k = 0, and two
    detector inputs of different sizes on one frame."""
    import whenet
    from whenet_hip.frames import FramePipeline
    m = whenet.WHENet(dtype=dtype)
    try:
        h = m._handle
        frames = [synth.video_frame(360, 640, seed=s) for s in range(6)]
        boxes = [synth.head_boxes(k, 360, 640, seed=10 + k) for k in (3, 0, 1, 5, 2, 4)]
        want, want_am = [], []
        with FramePipeline(m, depth=1) as fp:
            for f, b in zip(frames, boxes):
                want.append(fp.process(f, b))
        for f, (rects, _, _, _) in zip(frames, want):                      # argmax: the handle's own submit_frame
            t = h.submit_frame(f, rects, bgr=True)
            ypr, am, _ = h.collect(t, rects.shape[0])
            want_am.append((ypr, am))
        canvases = {}
        for i, f in enumerate(frames):
            for size in ((416, 416), (320, 608)):
                canvases[i, size] = R.letterbox_u8(f[:, :, ::-1], *size)
                assert np.array_equal(h.op_letterbox(f, size, bgr=True)[0], canvases[i, size])

        # the handle's entry points: one frame at a time, argmax too
        h.set_option("inflight", 1)
        for i, (f, (rects, yaw, pitch, roll)) in enumerate(zip(frames, want)):
            t = h.frame_begin(f, bgr=True)
            u8, f32 = h.frame_letterbox(t, (416, 416))
            assert np.array_equal(u8, canvases[i, (416, 416)])
            assert f32.tobytes() == (canvases[i, (416, 416)].astype(np.float32) / 255).tobytes()
            u8b, _ = h.frame_letterbox(t, (320, 608), want_f32=False)      # another size, same resident frame
            assert np.array_equal(u8b, canvases[i, (320, 608)])
            h.frame_heads(t, rects)
            ypr, am, _ = h.collect(t, rects.shape[0])
            assert ypr.tobytes() == want_am[i][0].tobytes() and np.array_equal(am, want_am[i][1])
            assert np.array_equal(ypr[:, 0], yaw) and np.array_equal(ypr[:, 1], pitch) and np.array_equal(ypr[:, 2], roll)

        # the pipeline, depths 1..4, frames interleaved: begin the next one while earlier ones are in flight
        for depth in (1, 2, 3, 4):
            got = []
            with FramePipeline(m, depth=depth) as fp:
                for i, (f, b) in enumerate(zip(frames, boxes)):
                    if fp.in_flight == depth:
                        got.append(fp.collect())
                    fp.begin(f)
                    x = fp.detector_input((416, 416))
                    assert x.shape == (1, 416, 416, 3) and x.dtype == np.float32
                    assert x.tobytes() == R.image_data(canvases[i, (416, 416)]).tobytes()
                    if i % 2:
                        assert np.array_equal(fp.detector_input((320, 608), as_uint8=True), canvases[i, (320, 608)])
                    fp.heads(b)
                while fp.in_flight:
                    got.append(fp.collect())
            assert len(got) == len(frames)
            for g, w in zip(got, want):
                assert g[0].dtype == w[0].dtype and np.array_equal(g[0], w[0])
                for a, b_ in zip(g[1:], w[1:]):
                    assert a.tobytes() == b_.tobytes()
        # the two forms mixed in one pipeline keep their order
        with FramePipeline(m, depth=2) as fp:
            fp.begin(frames[0])
            fp.heads(boxes[0])
            fp.submit(frames[3], boxes[3])
            a, b_ = fp.collect(), fp.collect()
        assert np.array_equal(a[1], want[0][1]) and np.array_equal(b_[1], want[3][1])
    finally:
        m.close()


@pytest.mark.gpu
def test_resident_frame_misuse_is_einval_and_the_handle_stays_usable(model, post):
    from whenet_hip.frames import FramePipeline
    h = model._handle
    h.set_option("inflight", 1)
    frame = synth.video_frame(360, 640)
    boxes = synth.head_boxes(3, 360, 640)
    rects = _lib.frame_rects(360, 640, boxes)
    with FramePipeline(model, depth=1) as fp:
        want = fp.process(frame, boxes)
    with pytest.raises(ValueError):
        h.frame_letterbox(12345, (416, 416))                       # unknown ticket
    with pytest.raises(ValueError):
        h.frame_heads(12345, rects)
    with pytest.raises(ValueError):
        h.frame_heads(-1, rects)
    t = h.frame_begin(frame)
    with pytest.raises(ValueError):
        h.frame_letterbox(t, (5000, 416))                           # beyond the documented limit: the ticket survives
    with pytest.raises(ValueError):
        h.frame_heads(t, np.array([[0, 0, 361, 50]], np.int32))     # outside the frame: the ticket survives
    h.frame_heads(t, rects)
    with pytest.raises(ValueError):
        h.frame_heads(t, rects)                                     # heads twice
    with pytest.raises(ValueError):
        h.frame_letterbox(t, (416, 416))                            # letterbox after the heads
    ypr, _, _ = h.collect(t, 3)
    assert np.array_equal(ypr[:, 0], want[1])
    with pytest.raises(ValueError):
        h.frame_heads(t, rects)                                     # collected: unknown again
    with pytest.raises(ValueError):
        h.collect(t, 3)
    # a submit_frame ticket is not a resident frame
    t2 = h.submit_frame(frame, rects)
    with pytest.raises(ValueError):
        h.frame_letterbox(t2, (416, 416))
    with pytest.raises(ValueError):
        h.frame_heads(t2, rects)
    h.collect(t2, 3)
    # a ticket that never gets heads: released by k = 0 + collect; all four slots come back
    for _ in range(2):
        ts = [h.frame_begin(frame) for _ in range(_lib.MAX_INFLIGHT)]
        with pytest.raises(ValueError):
            h.frame_begin(frame)                                    # WHENET_MAX_INFLIGHT held
        for t in ts:
            h.frame_heads(t, np.zeros((0, 4), np.int32))
            assert h.collect(t, 0)[0].shape == (0, 3)
    # the pipeline's own ordering rules
    with FramePipeline(model, depth=2) as fp:
        with pytest.raises(ValueError):
            fp.detector_input()
        with pytest.raises(ValueError):
            fp.heads(boxes)
        fp.begin(frame)
        with pytest.raises(ValueError):
            fp.begin(frame)
        with pytest.raises(ValueError):
            fp.detector_input((416, 400))                           # not a multiple of 32
        fp.heads(boxes)
        with pytest.raises(ValueError):
            fp.detector_input()
        got = fp.collect()
    assert np.array_equal(got[1], want[1])
    # a handle without a network: begin / letterbox / no heads work, heads do not
    t = post.frame_begin(frame)
    assert np.array_equal(post.frame_letterbox(t, (416, 416), want_f32=False)[0], R.letterbox_u8(frame[:, :, ::-1], 416, 416))
    with pytest.raises(ValueError):
        post.frame_heads(t, rects)
    post.frame_heads(t, np.zeros((0, 4), np.int32))
    post.collect(t, 0)
    # and a normal frame afterwards
    with FramePipeline(model, depth=1) as fp:
        again = fp.process(frame, boxes)
    for a, b in zip(again, want):
        assert np.array_equal(a, b)
