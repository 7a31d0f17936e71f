"""The oracle has no reference-side vectors to be pinned against ("parity unpinned");
these tests pin it the only ways available here:
  * committed self-generated goldens (regression),
  * an independent float32 torch/oneDNN restatement agrees to float32 noise,
  * an independent third-party implementation of EfficientNet-B0 (HuggingFace
    transformers, torch) fed the same weights produces the same 7x7x1280 features,
  * the reference's own pre/post-processing lines are EXECUTED, not restated: tests/test_reference_run.py
    (whenet.py:22-34 and utils.py:7-11 run from /root/reference under module stand-ins; their outputs are the
    committed fixtures tests/golden/reference_*.npz that the oracle -- and the HIP path -- are checked against).
"""
import os

import numpy as np
import pytest

from oracle import whenet_oracle as O
from oracle.whenet_torch import TorchWHENet
from whenet_hip import spec


def test_golden_regression(weights, golden):
    crops = golden["crops"][:3]
    r = O.forward(crops, weights, np.float64)
    np.testing.assert_allclose(r["logits"], golden["expected"]["logits"][:3], rtol=0, atol=1e-9)
    ang = np.stack([r["yaw"], r["pitch"], r["roll"]], axis=1)
    np.testing.assert_allclose(ang, golden["expected"]["angles"][:3], rtol=0, atol=1e-9)
    assert np.array_equal(r["argmax"], golden["expected"]["argmax"][:3])


def test_block_is_the_backbone_s_arithmetic(weights, golden):
    """backbone() chains block(): every tap of every block, recomputed by block() from the tap before it, is bit for bit the tap
    backbone() recorded, and so is the feature map (the per-block tests feed block() inputs of their own: they must be checking the
    arithmetic the end-to-end goldens check)."""
    x = O.normalise(golden["crops"][:1]).astype(np.float64)
    t = {}
    feat = O.backbone(x, weights, taps=t)
    cur = t["stem"]
    for b in spec.blocks():
        mine = {}
        got = O.block(t["stem"] if b.index == 1 else t[f"b{b.index - 1}/out"], weights, b.index, taps=mine)
        assert mine and all(np.array_equal(v, t[k]) for k, v in mine.items()), b.index
        assert np.array_equal(got, t[f"b{b.index}/out"]), b.index
        cur = O.block(cur, weights, b.index)
    head = O.swish(O.batchnorm(O.conv2d(cur, weights["head/conv/kernel"], 1), weights, "head/bn"))
    assert np.array_equal(head, feat)
    np.testing.assert_allclose(O.heads(feat, weights), golden["expected"]["logits"][:1], rtol=0, atol=1e-9)


def test_torch_restatement_agrees(weights, golden):
    """float32 torch (NCHW, oneDNN) vs float64 numpy: <= 1e-3 deg, the north-star bar."""
    crops = golden["crops"]
    tw = TorchWHENet(weights)
    y, p, r = tw.get_angle(crops.copy())
    ang = np.stack([y, p, r], axis=1)
    err = np.abs(ang - golden["expected"]["angles"]).max()
    assert err < 1e-3, err
    lg = np.concatenate(tw.predict_logits(O.normalise(crops)), axis=1)
    am = O.argmax_bins(lg)
    safe = golden["expected"]["margins"] > 5e-3
    assert np.array_equal(am[safe], golden["expected"]["argmax"][safe])


def test_numpy_f32_noise_floor(weights, golden):
    r = O.forward(golden["crops"][:4], weights, np.float32)
    ang = np.stack([r["yaw"], r["pitch"], r["roll"]], axis=1)
    assert np.abs(ang - golden["expected"]["angles"][:4]).max() < 1e-3


def test_conv_same_padding_against_torch():
    """TF-SAME asymmetric pads (bottom/right only for even sizes at stride 2)."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(0)
    for (h, k, s) in ((8, 3, 2), (10, 5, 2), (7, 5, 1), (6, 3, 1), (9, 3, 2)):
        x = rng.normal(size=(2, h, h, 5))
        w = rng.normal(size=(k, k, 5, 1))
        got = O.depthwise(x, w, s)
        out, pb, pa = spec.same_pad(h, k, s)
        xt = F.pad(torch.from_numpy(x).permute(0, 3, 1, 2), (pb, pa, pb, pa))
        wt = torch.from_numpy(w).permute(2, 3, 0, 1)
        ref = F.conv2d(xt, wt, stride=s, groups=5).permute(0, 2, 3, 1).numpy()
        assert got.shape == (2, out, out, 5)
        np.testing.assert_allclose(got, ref, atol=1e-12)
        # a one-pixel shift of the padding must be detectable
        if pb != pa:
            xt2 = F.pad(torch.from_numpy(x).permute(0, 3, 1, 2), (pa, pb, pa, pb))
            bad = F.conv2d(xt2, wt, stride=s, groups=5).permute(0, 2, 3, 1).numpy()
            assert np.abs(bad - got).max() > 1e-3


def test_hf_efficientnet_cross_check(weights, golden):
    """Independent implementation: transformers' EfficientNet (B0 config) with our weights must give
    the same 7x7x1280 feature map as oracle.backbone().  A HARD requirement where this suite runs
    (the build box has transformers): a missing package is a failure, not a skip -- this is the only
    third-party check the oracle's backbone has."""
    try:
        import transformers  # noqa: F401
    except ImportError as e:          # pragma: no cover
        pytest.fail(f"transformers is required for the oracle's independent cross-check: {e}")
    from tests.hf_reference import hf_backbone_features
    crops = golden["crops"][:2]
    x = O.normalise(crops).astype(np.float64)
    ours = O.backbone(x, weights)
    hf = hf_backbone_features(weights, x)
    assert hf.shape == ours.shape == (2, 7, 7, 1280)
    np.testing.assert_allclose(hf, ours, rtol=0, atol=1e-9)
    # and the committed fixture (what the GPU box checks against) is this very tensor
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "hf_features.npz"))
    assert np.array_equal(fx["crop_index"], [0, 1])
    np.testing.assert_allclose(fx["features"], hf.astype(np.float32), rtol=0, atol=0)


def test_oracle_matches_committed_hf_fixture(weights, golden):
    """The same check without transformers: oracle backbone vs the committed HuggingFace features
    (tests/golden/hf_features.npz, float32, written by tests/golden/make_hf_fixture.py)."""
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "hf_features.npz"))
    x = O.normalise(golden["crops"][fx["crop_index"]]).astype(np.float64)
    ours = O.backbone(x, weights)
    scale = np.abs(ours).max()
    assert np.abs(ours - fx["features"]).max() <= 2e-7 * scale + 1e-7      # float32 storage rounding only


def test_oracle_class_surface(weights, golden):
    m = O.OracleWHENet(weights)
    y, p, r = m.get_angle(golden["crops"][:1])
    assert y.shape == p.shape == r.shape == (1,)
    with pytest.raises(ValueError):
        m.get_angle(np.zeros((224, 224, 3), np.uint8))


def test_f16_set_fixture_is_the_oracle(weights):
    """tests/golden/f16_set_expected.npz (the 48-crop accuracy contract of the GPU suite) is what
    oracle/whenet_oracle.py computes for those seeded crops: re-derived here for a sample of them."""
    import os
    from whenet_hip import synth
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "f16_set_expected.npz"))
    crops = np.concatenate([synth.scene_crops(24, seed=5), synth.noise_crops(24, seed=6)])
    idx = [0, 23, 24, 47]
    ref = O.forward(crops[idx], weights, np.float64)
    assert np.abs(np.stack([ref["yaw"], ref["pitch"], ref["roll"]], 1) - fx["angles"][idx]).max() < 1e-9
    assert np.allclose(ref["logits"], fx["logits"][idx], rtol=1e-6, atol=1e-5)          # (stored as float32)
    assert np.array_equal(ref["argmax"], fx["argmax"][idx])
    assert fx["angles"].shape == (48, 3) and fx["logits"].shape == (48, 252)
    # round 4: the 512-crop set of the f16 DISTRIBUTION contract is the oracle's too (it used to be the f32 HIP path)
    fx5 = np.load(os.path.join(os.path.dirname(__file__), "golden", "f16_set512_expected.npz"))
    big = np.concatenate([synth.scene_crops(256, seed=41), synth.noise_crops(256, seed=42)])
    idx5 = [0, 255, 256, 511]
    ref5 = O.forward(big[idx5], weights, np.float64)
    assert np.abs(np.stack([ref5["yaw"], ref5["pitch"], ref5["roll"]], 1) - fx5["angles"][idx5]).max() < 1e-9
    assert np.allclose(ref5["logits"], fx5["logits"][idx5], rtol=1e-6, atol=1e-5)
    assert np.array_equal(ref5["argmax"], fx5["argmax"][idx5])
    assert fx5["angles"].shape == (512, 3) and fx5["margins"].shape == (512, 3) and (fx5["margins"] >= 0).all()


def test_block1_project_composed_with_block2_expand_is_the_same_function(weights, golden):
    """The algebra behind the engine's option fold12 (csrc/snapshot.cpp, HostModel::fold12), restated in numpy float64
    on the oracle's own tensors: block 1's project conv + BN is linear, block 2 has no skip and nothing else reads
    block 1's output (efficientnet MBConvBlock, whenet.py:8), so
        expand2(project1(a)) = a . (Wp1 . We2) + (bp1 . We2 + be2),       a = gate1 * depthwise1,
    with both BatchNorms folded into their convs.  Checked against the oracle's block-2 expanded tensor."""
    from oracle import b0_spec as G
    w = weights
    x = O.normalise(golden["crops"][:1]).astype(np.float64)
    taps = {}
    O.backbone(x, w, taps=taps)

    def folded(conv, bn):
        k = w[f"{conv}/kernel"][0, 0].astype(np.float64)                      # [K][N]
        s = w[f"{bn}/gamma"].astype(np.float64) / np.sqrt(w[f"{bn}/var"].astype(np.float64) + G.BN_EPSILON)
        return k * s, w[f"{bn}/beta"].astype(np.float64) - w[f"{bn}/mean"].astype(np.float64) * s

    wp, bp = folded("b1/project", "b1/project_bn")                           # 32 -> 16
    we, be = folded("b2/expand", "b2/expand_bn")                             # 16 -> 96
    wc, bc = wp @ we, bp @ we + be
    assert wc.shape == (32, 96)
    a = taps["b1/dw"] * taps["b1/gate"]
    two_step = (a @ wp + bp)
    np.testing.assert_allclose(two_step, taps["b1/out"], rtol=0, atol=1e-10)    # block 1 has no skip
    np.testing.assert_allclose(O.swish(a @ wc + bc), taps["b2/expand"], rtol=0, atol=1e-10)
