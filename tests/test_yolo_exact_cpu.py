"""The premises of tests/yolo_exact_cases.py, with the oracle alone (no GPU): what the builders claim about their maps is what
oracle/yolo_oracle.py computes.  tests/test_yolo_exact_gpu.py then holds csrc/yolo.hip to the same cases."""
import numpy as np
import pytest

from oracle import yolo_oracle as Y
from tests import yolo_exact_cases as X

F = np.float32


def test_the_logit_set_is_exact():
    with np.errstate(over="ignore"):
        assert Y.sigmoid(X.EXACT).tobytes() == np.array([0.5, 1.0, 0.0], F).tobytes()
        assert np.exp(X.EXACT).tobytes() == np.array([1.0, np.inf, 0.0], F).tobytes()
        assert np.exp(-X.EXACT).tobytes() == np.array([1.0, 0.0, np.inf], F).tobytes()


@pytest.mark.parametrize("case", X.DECODE_CASES, ids=[c[0] for c in X.DECODE_CASES])
def test_decode_cases_hold_only_exact_logits_and_no_nan(case):
    maps, anchors, nc, image = X.decode_case(case)
    assert [m.shape for m in maps] == [(2 << l, 3 << l, 3 * (5 + nc)) for l in range(len(maps))]
    assert X.num_boxes(maps) == (378 if len(maps) == 3 else 90)
    seen = set()
    for m in maps:
        assert m.dtype == F and np.isin(m, X.EXACT).all()
        t = m.reshape(-1, 5 + nc)
        assert {0.0, 128.0, -128.0} == set(np.unique(t[:, :2])) == set(np.unique(t[:, 4:]))       # xy, confidence and classes: all three
        assert (t[:, 2:4] == X.POS).sum() >= 1                                                     # a box of infinite extent
        seen |= set(np.unique(t[:, 2:4]))
    assert seen == {0.0, 128.0, -128.0}
    boxes, scores = X.oracle_decode(maps, anchors, nc, image)
    assert boxes.dtype == F and boxes.shape == (X.num_boxes(maps), 4) and scores.shape == (X.num_boxes(maps), nc)
    assert not np.isnan(boxes).any() and np.isinf(boxes).any()
    assert set(np.unique(scores)) <= {0.0, 0.25, 0.5, 1.0}
    assert (boxes[:, 2] - boxes[:, 0] == 0).any()                                                  # zero extents too
    # the selection is not empty, so the batched / mixed comparisons have rows to compare
    assert len(X.oracle_eval(maps, anchors, nc, image, **X.DECODE_KW)[0]) >= 2


def test_half_to_even_case_gives_a_new_width_of_2():
    # image (128, 5) in a 64 x 96 input: image * min(input / image) = (64, 2.5); K.round is half to even
    inp, image = np.array([64, 96], F), np.array([128, 5], F)
    scaled = image * np.min(inp / image)
    assert scaled.tolist() == [64.0, 2.5] and np.round(scaled).tolist() == [64.0, 2.0]
    # and that is what the oracle's boxes are made of: a box at the centre, one input wide, is new_w / 96 of the image wide.
    # Zero logits on a 2 x 3 map: anchor (w, h) = (96, 64) -> bw = 1, scale_x = 96 / 2 = 48 -> width 48 * 5 = 240 pixels (160 with 3)
    maps = [np.zeros((2 << l, 3 << l, 18), F) for l in range(3)]
    anchors = np.tile(np.array([[96, 64]], F), (9, 1))
    boxes, _ = X.oracle_decode(maps, anchors, 1, (128, 5))
    assert 239.9 < float(boxes[0, 3] - boxes[0, 1]) < 240.1


@pytest.mark.parametrize("image", X.EDGE_IMAGES)
def test_edge_pair_has_an_iou_of_exactly_one_half(image):
    thr = X.edge_pair_iou(image)
    assert thr.dtype == F and thr == F(0.5)
    boxes, scores = X.oracle_decode(X.edge_maps(), X.EDGE_ANCHORS, 1, image)
    assert len(boxes) == X.EDGE_N and scores[:2, 0].tolist() == [1.0, 0.5] and not scores[2:].any()
    assert Y.non_max_suppression(boxes[:2], scores[:2, 0], 20, thr) == [0, 1]
    assert Y.non_max_suppression(boxes[:2], scores[:2, 0], 20, np.nextafter(thr, F(0))) == [0]


EDGE = X.edge_cases()


@pytest.mark.parametrize("case", EDGE, ids=[c[0] for c in EDGE])
def test_edge_cases_keep_what_is_written_down(case):
    _, maps, image, kw, expect, anchors = case
    boxes, scores, classes, index = X.oracle_eval(maps, anchors, 1, image, **kw)
    assert index.tolist() == expect and not np.isnan(boxes).any()


def test_rounded_union_pair_tells_a_fused_union_from_an_unfused_one():
    """IOU() with inter's product fused into `area_a + area_b - inter` (one rounding of the exact difference), in exact rational
    arithmetic, against the oracle's operation-by-operation value: the fused one is larger, so a kernel that contracts suppresses
    box 1 at the threshold the oracle's own IoU sets."""
    from fractions import Fraction
    b, s = X.oracle_decode(X.edge_maps(), X.ROUNDED_ANCHORS, 1, (32, 32))
    a, c = b[0], b[1]
    assert c[0] < a[0] < a[2] < c[2] and c[1] < a[1] < a[3] < c[3]                                  # box 0 inside box 1
    area_a, area_c = F(F(a[2] - a[0]) * F(a[3] - a[1])), F(F(c[2] - c[0]) * F(c[3] - c[1]))
    dy, dx = F(a[2] - a[0]), F(a[3] - a[1])                                                         # the intersection is box 0
    exact = Fraction(float(F(area_a + area_c))) - Fraction(float(dy)) * Fraction(float(dx))
    lo = F(float(exact))                                                                            # (float64 holds the nearest float32's neighbourhood)
    fused = F(F(dy * dx) / lo)
    unfused = Y.iou(a, c)
    assert unfused == X.edge_pair_iou((32, 32), X.ROUNDED_ANCHORS) and F(0.3) < unfused < fused
    assert Fraction(float(lo)) != Fraction(float(F(F(area_a + area_c) - F(dy * dx))))


def test_edge_case_premises():
    cases = {c[0]: c for c in EDGE}
    dec = lambda name: X.oracle_decode(cases[name][1], cases[name][5], 1, cases[name][2])
    b, s = dec("zero-area-on-top")
    assert b[1, 3] == b[1, 1] and b[1, 2] > b[1, 0] and s[:2, 0].tolist() == [0.5, 1.0]             # zero width, top score
    assert b[0, 1] < b[1, 1] < b[0, 3] and b[0, 0] <= b[1, 0] and b[1, 2] <= b[0, 2]                # inside box 0
    b, s = dec("infinite-extent")
    assert b[0, 1] == -np.inf and b[0, 3] == np.inf and b[1, 1] == -np.inf and np.isfinite(b[:2, [0, 2]]).all()
    with np.errstate(invalid="ignore"):
        assert np.isnan(Y.iou(b[0], b[1]))
    b, s = dec("score-at-threshold")
    assert s[0, 0].tobytes() == F(0.25).tobytes() and s[1, 0] == 1
    assert float(X.QUARTER_UP) > 0.25 and F(float(X.QUARTER_UP)) == X.QUARTER_UP
    b, s = dec("score-threshold-zero")
    assert s[:2, 0].tolist() == [1.0, 0.5] and not s[2:].any() and not np.signbit(s).any()
    assert ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) == 0).all()
    b, s = dec("equal-scores-max-1")
    assert s[0, 0] == s[1, 0] == 0.5


@pytest.mark.parametrize("pattern", X.SORT_PATTERNS)
@pytest.mark.parametrize("n", X.SORT_SIZES + (0,))
def test_sort_cases_have_exactly_n_candidates(n, pattern):
    maps, chosen = X.sort_maps(n, pattern)
    assert X.num_boxes(maps) == X.SORT_N and len(chosen) == n == len(set(chosen.tolist()))
    boxes, scores = X.oracle_decode(maps, X.synth.YOLO_ANCHORS, 1, X.SORT_IMAGE)
    cand = np.flatnonzero(scores[:, 0] >= F(X.SORT_SCORE))
    assert np.array_equal(cand, chosen) and not scores[np.setdiff1d(np.arange(X.SORT_N), chosen)].any()
    assert ((boxes[:, 2] - boxes[:, 0]) == 0).all() and ((boxes[:, 3] - boxes[:, 1]) == 0).all()  # zero areas: nothing is suppressed
    if n:
        if pattern == "equal":
            assert (scores[chosen, 0] == 0.5).all()
        else:
            assert (scores[chosen, 0] >= 0.5).all() and len(np.unique(scores[chosen, 0])) > 0.99 * n - 1
    assert 300 <= X.sort_max_boxes(n) or X.sort_max_boxes(n) == max(n, 1)


@pytest.mark.parametrize("pattern", X.SORT_PATTERNS)
@pytest.mark.parametrize("n", [n for n in X.SORT_SIZES if n <= 65])
def test_oracle_nms_keeps_the_plain_sorted_order_on_sort_cases(n, pattern):
    """Why the GPU test may state the expected order directly (the Python loop is too slow beyond these sizes)."""
    maps, chosen = X.sort_maps(n, pattern)
    boxes, scores = X.oracle_decode(maps, X.synth.YOLO_ANCHORS, 1, X.SORT_IMAGE)
    s = scores[:, 0]
    want = sorted(chosen.tolist(), key=lambda i: (-float(s[i]), i))
    assert X.expected_order(s, chosen, n).tolist() == want
    keep = Y.non_max_suppression(boxes[chosen], s[chosen], n, 0.5)
    assert chosen[keep].tolist() == want
    got = X.oracle_eval(maps, X.synth.YOLO_ANCHORS, 1, X.SORT_IMAGE, max_boxes=X.sort_max_boxes(n), score_threshold=X.SORT_SCORE,
                        iou_threshold=0.5)
    assert got[3].tolist() == want


def test_three_class_sort_case():
    maps, chosen = X.sort_maps_three_classes()
    boxes, scores = X.oracle_decode(maps, X.synth.YOLO_ANCHORS, 3, X.SORT_IMAGE)
    cand = [np.flatnonzero(scores[:, c] >= F(X.SORT_SCORE)) for c in range(3)]
    assert [len(c) for c in cand] == [4097, 4096, 0]
    assert np.array_equal(cand[0], chosen) and np.array_equal(cand[1], chosen[1:])
    assert (scores[chosen, 0] == 0.5).all() and len(np.unique(scores[chosen[1:], 1])) > 4000
