"""The float32 detector body without a GPU: the figures of tests/golden/reference_detector_f32.json derived again, the condition
the GPU tests rest on (CPU-float32 boxes give the float64 oracle's crop windows; binary16 storage does not), the wide-operand
cases' preconditions, and the Python surface of the dtype."""
import numpy as np
import pytest

from tests import detector_cases as DC
from tests import detector_f32_cases as FC
from tests import detector_ref as R
from tests.golden import make_detector_f32_fixture as MK
from whenet_hip import _lib, detector_weights as DW


@pytest.fixture(scope="module")
def metas():
    return FC.load_meta()


@pytest.fixture(scope="module")
def live():
    return MK.measure()


def test_fixture_is_what_the_cpu_computes_now(metas, live):
    """Float32 sums may be taken in another order on another CPU: the error figures agree within a factor of 4 (the factor the GPU
    bounds allow for the same reason); the float64 oracle's selection agrees to 1e-3 px and its windows exactly."""
    _, rec = metas
    assert set(rec) == {"e32_body", "e32", "detect"} and set(rec["e32"]) == set(FC.WIDE_CASES)
    assert set(rec["e32_body"]) == {f"{n}/{h}x{w}" for n, _ in DC.KINDS for h, w in DC.SIZES}
    for tag, errs in rec["e32_body"].items():
        print(tag, "recorded", errs, "live", live["e32_body"][tag])
        assert len(errs) == len(live["e32_body"][tag])
        for a, b in zip(errs, live["e32_body"][tag]):
            assert 0 < a < 1e-5 and a <= 4 * b and b <= 4 * a, (tag, a, b)
    for name, _ in DC.KINDS:
        r, l = rec["detect"][name], live["detect"][name]
        assert r["oracle_windows"] == l["oracle_windows"]
        assert np.abs(np.array(r["oracle_boxes"]) - np.array(l["oracle_boxes"])).max() <= 1e-3
        assert np.abs(np.array(r["oracle_scores"]) - np.array(l["oracle_scores"])).max() <= 1e-6
    for cname in FC.WIDE_CASES:
        print(cname, "e32 recorded", rec["e32"][cname], "live", live["e32"][cname])
        assert 0 < rec["e32"][cname] < 0.01 and live["e32"][cname] <= 4 * rec["e32"][cname]


@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_float32_boxes_give_the_oracle_windows(metas, live, name, kind):
    """What tests 7 and 9 of the GPU suite rest on: at the committed configuration the CPU-float32 maps select oracle_count boxes,
    hundredths of a pixel from the float64 oracle's, and `whenet_frame_rects` of them is the oracle's integer windows."""
    meta, rec = metas
    d, l = meta["detect"][name], live["detect"][name]
    assert l["f32_count"] == d["oracle_count"] == rec["detect"][name]["f32_count"] == len(l["oracle_windows"])
    assert l["f32_box_px"] is not None and l["f32_box_px"] <= 0.01 and l["f32_score"] <= 1e-5
    assert l["f32_windows"] == l["oracle_windows"]
    # every window is one a crop can be cut from or is rejected the same way by both: the library's windows of the ORACLE's boxes
    fh, fw = DC.sample_frame(0).shape[:2]
    assert _lib.frame_rects(fh, fw, np.array(l["oracle_boxes"], np.float32)).tolist() == l["oracle_windows"]
    # recorded distances are of the same kind (the GPU bound is 4 x the recorded figure)
    r = rec["detect"][name]
    assert 0 < r["f32_box_px"] <= 0.01 and l["f32_box_px"] <= 4 * r["f32_box_px"] and l["f32_score"] <= 4 * r["f32_score"]


@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_binary16_storage_does_not_give_the_oracle_windows(metas, name, kind):
    """Why the dtype exists: the CPU emulation of binary16 storage selects boxes whose windows differ from the oracle's."""
    meta, rec = metas
    d = meta["detect"][name]
    arrays = FC.load_maps()
    emu = [arrays[f"{name}/64x96/emu{l}"] for l in range(3 if kind == 0 else 2)]
    b, s, c, i = FC.oracle_detect(name, d, emu)
    assert len(b) == d["oracle_count"]
    fh, fw = DC.sample_frame(0).shape[:2]
    assert _lib.frame_rects(fh, fw, b).tolist() != rec["detect"][name]["oracle_windows"]
    # and its maps lie two orders of magnitude further from the reference than float32's: an f16 body cannot pass 4 x e32_body
    for h, w in DC.SIZES:
        for e16, e32 in zip(meta["emu_err"][f"{name}/{h}x{w}"], rec["e32_body"][f"{name}/{h}x{w}"]):
            assert e16 > 100 * e32


@pytest.mark.parametrize("cname", FC.WIDE_CASES)
def test_wide_operands_are_exact_in_float32_and_not_in_binary16(cname):
    c = FC.CASES[cname]
    x, x2, kernel, bias, skip = FC.wide_operands(c)
    want, bound = FC.expected_f32(c, x, x2, kernel, bias, skip, True)
    assert bound < 2 ** 24, bound
    for a in (x, x2, skip):
        if a is None:
            continue
        nz = a[a != 0]
        assert np.array_equal(a, np.rint(a)) and np.array_equal(a.astype(np.float32).astype(np.float64), a)
        assert np.abs(a).max() > 65504 and ((np.abs(nz) > 2048) & (np.abs(nz) % 2 == 1)).any()
        with np.errstate(over="ignore"):
            assert (R.r16(a) != a).any()
    assert np.abs(kernel).max() <= 2 and np.abs(want).max() > 2048 and len(np.unique(want)) > 8


def test_python_surface_of_the_dtype():
    from whenet_hip import detector
    assert _lib.DETECTOR_DTYPES == {"f16": 0, "f32": 1}
    kw = dict(model_path=DW.synthetic(1, DC.SEEDS["tiny"]), anchors_path=DC.ANCHORS["tiny"], classes_path=["head"])
    for bad in ("f64", "f32s", 1, None):
        with pytest.raises(ValueError, match="dtype"):
            detector.YOLO(dtype=bad, handle=object(), **kw)          # raised before the handle (or the library) is touched
    with pytest.raises(TypeError):
        detector.YOLO("f32", **kw)                                     # keyword-only
    import inspect
    assert inspect.signature(_lib.Handle.detector_load).parameters["dtype"].default == "f16"
    assert inspect.signature(detector.YOLO.__init__).parameters["dtype"].default == "f16"
