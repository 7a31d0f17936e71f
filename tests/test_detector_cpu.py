"""The detector body without a GPU: the engine's layer table against the EXECUTED reference (tests/golden/reference_detector.*,
made by tests/golden/make_detector_fixture.py from yolo_v3/model.py run under stand-ins), the synthetic weights, the snapshot
packer and the shape of the Python interface."""
import json
import os

import numpy as np
import pytest

from tests import detector_cases as DC
from tests import detector_harness as Hn
from tests import detector_ref as R
from whenet_hip import _lib, detector_weights as DW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROW_KEYS = ("op", "k", "stride", "cin", "cout", "bn", "leaky")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "reference_detector.npz")) as z:
        return meta, {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def synthetic():
    return {name: DW.synthetic(kind, DC.SEEDS[name]) for name, kind in DC.KINDS}


@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_layer_table_reproduces_the_executed_reference(fixture, synthetic, name, kind):
    """Routes, skips, padding sides and the upsample / concatenate order: a float64 evaluation driven by whenet_detector_spec
    alone gives the maps the reference's own yolo_body / tiny_yolo_body gave when run (1e-10 of each map's max |x|), and the rows
    equal the recorded layer list."""
    meta, arrays = fixture
    rows = _lib.detector_spec(kind)
    assert len(rows) == (75 if kind == 0 else 19) and sum(r["op"] == 0 for r in rows) == (75 if kind == 0 else 13)
    assert [[r[k] for k in ROW_KEYS] for r in rows] == meta["rows"][name]
    if kind == 0:
        assert meta["routes"][name] == [["Add", 512], ["Add", 256]]                 # darknet.layers[152], [92]
        cat = [r for r in rows if r["src1"] >= 0]
        assert [(rows[r["src1"]]["cout"], rows[r["src1"]]["skip"] >= 0, r["cin0"]) for r in cat] == [(512, True, 256), (256, True, 128)]
    for h, w in DC.SIZES:
        maps = R.forward(rows, synthetic[name], DC.fixture_image(h, w), "f64")
        assert len(maps) == (3 if kind == 0 else 2)
        for l, m in enumerate(maps):
            ref = arrays[f"{name}/{h}x{w}/map{l}"]
            assert m.shape == ref.shape == (1, (h // 32) << l, (w // 32) << l, 18)
            assert np.abs(m - ref).max() <= 1e-10 * np.abs(ref).max(), (name, h, w, l)


@pytest.mark.skipif(not Hn.available(), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("name,kind", DC.KINDS)
def test_reference_executed_again_reproduces_the_fixture(fixture, synthetic, name, kind):
    meta, arrays = fixture
    run = Hn.run(kind, synthetic[name], DC.fixture_image(64, 96))
    assert [[r[k] for k in ROW_KEYS] for r in run["rows"]] == meta["rows"][name]
    assert all(r["padded_top_left"] == (r["stride"] == 2 and r["op"] == 0) for r in run["rows"])      # ZeroPadding2D(((1,0),(1,0)))
    for l, m in enumerate(run["maps"]):
        ref = arrays[f"{name}/64x96/map{l}"]
        assert np.abs(m - ref).max() <= 1e-12 * np.abs(ref).max()


def test_synthetic_weights_keep_every_layer_in_range(fixture):
    """The precondition of the binary16 comparison: no layer of the fixture runs away or dies."""
    meta, _ = fixture
    assert set(meta["stats"]) == {f"{n}/{h}x{w}" for n, _ in DC.KINDS for h, w in DC.SIZES}
    for tag, stats in meta["stats"].items():
        assert all(0.1 <= rms <= 10 and mx < 1000 for rms, mx in stats), tag


def test_fixture_records_what_the_gpu_tests_need(fixture):
    meta, arrays = fixture
    assert set(meta["e32"]) == {n for n, _ in DC.CONV_CASES}
    assert all(0 < v < 1e-4 for v in meta["e32"].values())
    for name, _ in DC.KINDS:
        d = meta["detect"][name]
        assert 3 <= d["oracle_count"] <= d["max_boxes"] and d["size"] == [64, 96]
        for h, w in DC.SIZES:
            assert all(0 < e < 0.05 for e in meta["emu_err"][f"{name}/{h}x{w}"])
    assert sum(a.nbytes for a in arrays.values()) < 200_000


def test_spec_for_other_heads_and_bad_arguments():
    rows = _lib.detector_spec(0, 3, 80)
    assert [r["cout"] for r in rows if r["is_output"]] == [255, 255, 255]
    assert [r["cout"] for r in _lib.detector_spec(1, 2, 4) if r["is_output"]] == [18, 18]
    for bad in ((2, 3, 1), (0, 0, 1), (0, 3, 0), (-1, 3, 1)):
        with pytest.raises(ValueError):
            _lib.detector_spec(*bad)
    # the first layer is the only one whose Cin is no multiple of 16; binary16 outputs are multiples of 16
    for kind in (0, 1):
        rows = _lib.detector_spec(kind)
        assert [i for i, r in enumerate(rows) if r["cin"] % 16] == [0] and rows[0]["cin"] == 3
        assert all(r["cout"] % 16 == 0 for r in rows if not r["is_output"])


def test_tensor_list_and_pack_round_trip(synthetic):
    for name, kind in DC.KINDS:
        names = DW.tensors(kind)
        assert len(names) == (75 * 5 - 3 * 3 if kind == 0 else 13 * 5 - 2 * 3)          # kernel + 4 BN arrays, output convs kernel + bias
        w = synthetic[name]
        assert set(w) == {n for n, _ in names}
        if kind == 1:
            blob = DW.pack(w)
            back = DW.parse(blob)
            assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
            assert DW.kind_of(back) == (1, 18)
    w = dict(synthetic["tiny"])
    del w["dbn003/beta"]
    with pytest.raises(ValueError, match="dbn003/beta"):
        DW.pack(w)
    w = dict(synthetic["tiny"])
    w["dconv004/kernel"] = w["dconv004/kernel"][:, :, :, :-1]
    with pytest.raises(ValueError, match="dconv004/kernel"):
        DW.pack(w)
    with pytest.raises(ValueError, match="not a detector snapshot"):
        DW.pack({"dconv000/kernel": np.zeros((3, 3, 3, 16), np.float32)})


def test_yolo_class_has_the_reference_interface(tmp_path, synthetic):
    from whenet_hip import detector
    d = detector.YOLO._defaults
    assert list(d) == ["model_path", "anchors_path", "classes_path", "score", "iou", "model_image_size", "gpu_num"]
    assert (d["score"], d["iou"], d["model_image_size"], d["gpu_num"]) == (0.3, 0.45, (416, 416), 1)
    assert [os.path.basename(d[k]) for k in ("model_path", "anchors_path", "classes_path")] == ["head_detect.h5", "yolo_anchors.txt", "head_classes.txt"]
    assert detector.YOLO.get_defaults("score") == 0.3 and detector.YOLO.get_defaults("x") == "Unrecognized attribute name 'x'"
    kw = dict(model_path=synthetic["tiny"], anchors_path=DC.ANCHORS["tiny"], classes_path=["head"])
    with pytest.raises(ValueError, match="Multiples of 32"):
        detector.YOLO(model_image_size=(100, 96), **kw)
    with pytest.raises(ValueError, match=r"Keras \.h5 of the detector is not read"):
        detector.YOLO(**dict(kw, model_path=str(tmp_path / "head_detect.h5")))
    with pytest.raises(ValueError, match="Mismatch between model and given anchor and class sizes"):
        detector.YOLO(**dict(kw, classes_path=["head", "hand"]))
    with pytest.raises(TypeError):
        detector.YOLO(threshold=0.5, **kw)
    import torch
    if not torch.cuda.is_available():          # no CPU fallback: nothing computes without a gfx950 device
        with pytest.raises(_lib.WhenetError) as e:
            detector.YOLO(model_image_size=(64, 96), **kw).detect(np.zeros((48, 64, 3), np.uint8))
        assert e.value.code == _lib.ENODEV


def test_package_stays_numpy_and_ctypes_only():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import whenet_hip.detector, whenet_hip.detector_weights, whenet_hip.frames; "
            "bad = [m for m in ('torch', 'cv2', 'oracle', 'tensorflow', 'keras') if m in sys.modules]; assert not bad, bad"
            % os.path.join(os.path.dirname(GOLDEN), "..", "headposeestimation-whenet_amd"))
    subprocess.run([sys.executable, "-c", code], check=True)
