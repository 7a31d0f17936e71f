"""csrc/yolo.hip held to the exact cases of tests/yolo_exact_cases.py (premises: tests/test_yolo_exact_cpu.py).  Every comparison is
bitwise or exact-integer: the decode against the oracle on logits where expf is exact, the selection against the oracle's NMS on the
device's own decoded rows, the sorted order at the sizes where the bitonic sort changes shape or moves from LDS to global keys."""
import numpy as np
import pytest

from tests import yolo_exact_cases as X
from whenet_hip import _lib, synth

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


def assert_same(got, want):
    """(boxes, scores, classes, index) of two calls, bitwise."""
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def ids(cases):
    return [c[0] for c in cases]


# ---- 1. the premise on the device: expf(0), expf(+-128) and the sigmoid are exact on gfx950 ------------------------------------------
@pytest.mark.parametrize("case", X.DECODE_CASES[::5], ids=ids(X.DECODE_CASES[::5]))
def test_premise_scores_are_exact_on_the_exact_set(post, case):
    maps, anchors, nc, image = X.decode_case(case)
    _, want = X.oracle_decode(maps, anchors, nc, image)
    all_scores = post.yolo_eval(maps, anchors, nc, image, debug=True, **X.DECODE_KW)[5]
    assert all_scores.dtype == F and all_scores.shape == want.shape
    assert set(np.unique(all_scores)) == {0.0, 0.25, 0.5, 1.0}                 # every product of {0, 0.5, 1} occurs
    assert all_scores.tobytes() == want.tobytes()


# ---- 2. the decode, bitwise -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.DECODE_CASES, ids=ids(X.DECODE_CASES))
def test_decode_is_bitwise_the_oracle(post, case):
    maps, anchors, nc, image = X.decode_case(case)
    want_b, want_s = X.oracle_decode(maps, anchors, nc, image)
    got = post.yolo_eval(maps, anchors, nc, image, debug=True, **X.DECODE_KW)
    all_boxes, all_scores = got[4], got[5]
    assert np.isinf(want_b).any() and not np.isnan(want_b).any()               # infinities are part of the comparison, NaN is not
    diff = np.flatnonzero((all_boxes.view(np.uint32) != want_b.view(np.uint32)).any(axis=1))
    assert all_boxes.tobytes() == want_b.tobytes(), (diff[:8].tolist(), all_boxes[diff[:4]].tolist(), want_b[diff[:4]].tolist())
    assert all_scores.tobytes() == want_s.tobytes()
    # and the selection made from them is the oracle's, on bitwise the oracle's rows
    X.assert_selection_is_oracle_nms(got, nc, **X.DECODE_KW)
    rb, rs, rc, ri = X.oracle_eval(maps, anchors, nc, image, **X.DECODE_KW)
    assert_same(got[:4], (rb, rs, rc, ri))


@pytest.mark.parametrize("config", range(len(X.CONFIGS)), ids=[c[0] for c in X.CONFIGS])
def test_batched_decode_is_bitwise_the_oracle(post, config):
    """F = 3 different exact maps of one image shape."""
    name, layers, anchors, nc = X.CONFIGS[config]
    image = X.IMAGES[2]                                                        # (1080, 607)
    per = [X.exact_maps(1000 + 10 * config + f, nc, num_layers=layers) for f in range(3)]
    assert per[0][0].tobytes() != per[1][0].tobytes() != per[2][0].tobytes()
    maps = [np.stack([per[f][l] for f in range(3)]) for l in range(layers)]
    batch = post.yolo_eval_batch(maps, anchors, nc, image, **X.DECODE_KW)
    assert len(batch) == 3
    for f, got in enumerate(batch):
        want_b, want_s = X.oracle_decode(per[f], anchors, nc, image)
        single = post.yolo_eval(per[f], anchors, nc, image, debug=True, **X.DECODE_KW)
        assert_same(got, single[:4])
        boxes, scores, classes, index = got
        assert len(index) >= 2
        assert boxes.tobytes() == want_b[index].tobytes() and scores.tobytes() == want_s[index, classes].tobytes()


@pytest.mark.parametrize("config", range(len(X.CONFIGS)), ids=[c[0] for c in X.CONFIGS])
def test_mixed_decode_is_bitwise_the_oracle(post, config):
    """F = 3 images of three shapes, the half-to-even one among them."""
    name, layers, anchors, nc = X.CONFIGS[config]
    images = [X.IMAGES[4], X.IMAGES[1], X.IMAGES[3]]                           # (128, 5), (720, 1280), (97, 131)
    per = [X.exact_maps(2000 + 10 * config + f, nc, num_layers=layers) for f in range(3)]
    maps = [np.stack([per[f][l] for f in range(3)]) for l in range(layers)]
    mixed = post.yolo_eval_mixed(maps, anchors, nc, images, **X.DECODE_KW)
    assert len(mixed) == 3
    for f, got in enumerate(mixed):
        want_b, want_s = X.oracle_decode(per[f], anchors, nc, images[f])
        single = post.yolo_eval(per[f], anchors, nc, images[f], debug=True, **X.DECODE_KW)
        assert_same(got, single[:4])
        boxes, scores, classes, index = got
        assert len(index) >= 2
        assert boxes.tobytes() == want_b[index].tobytes() and scores.tobytes() == want_s[index, classes].tobytes()


# ---- 3. NMS in isolation: the edge cases, the keep-lists written out in yolo_exact_cases.edge_cases() --------------------------------
EDGE = X.edge_cases()


@pytest.mark.parametrize("case", EDGE, ids=ids(EDGE))
def test_nms_edge_cases(post, case):
    """`>` and not `>=` at the IoU threshold, a zero-area box is kept, equal scores go to the lower index, infinite extents, `>=` at the
    score threshold, zero scores at threshold 0, an IoU whose last bit needs the union rounded operation by operation.  Boxes with NaN
    coordinates (anchor 0 times inf) are out of scope."""
    _, maps, image, kw, expect, anchors = case
    got = post.yolo_eval(maps, anchors, 1, image, debug=True, **kw)
    want_b, want_s = X.oracle_decode(maps, anchors, 1, image)
    assert got[4].tobytes() == want_b.tobytes() and got[5].tobytes() == want_s.tobytes()      # exact logits here too
    assert got[3].tolist() == expect
    assert X.assert_selection_is_oracle_nms(got, 1, **kw) == expect
    assert not got[2].any() and len(got[0]) == len(got[1]) == len(expect)


# ---- 4. sort sizes -----------------------------------------------------------------------------------------------------------------
def sort_kw(n):
    return dict(max_boxes=X.sort_max_boxes(n), score_threshold=X.SORT_SCORE, iou_threshold=0.5)


def assert_sorted_selection(got, num_classes, counts, max_boxes):
    """Nothing is suppressed (zero areas), so class c's rows are its candidates in (-score, index) order, cut at max_boxes."""
    gb, gs, gc, gi, all_boxes, all_scores = got
    first = 0
    for c in range(num_classes):
        cand = np.flatnonzero(all_scores[:, c] >= F(X.SORT_SCORE))
        assert len(cand) == counts[c]
        want = X.expected_order(all_scores[:, c], cand, max_boxes)
        k = min(counts[c], max_boxes)
        assert len(want) == k
        index = gi[first:first + k]
        assert index.tolist() == want.tolist(), (c, np.flatnonzero(index != want)[:8].tolist())
        assert (gc[first:first + k] == c).all()
        assert gs[first:first + k].tobytes() == all_scores[want, c].tobytes()
        assert gb[first:first + k].tobytes() == all_boxes[want].tobytes()
        first += k
    assert len(gi) == len(gs) == len(gc) == len(gb) == first                  # the class-by-class concatenation and nothing else


@pytest.mark.parametrize("pattern", X.SORT_PATTERNS)
@pytest.mark.parametrize("n", X.SORT_SIZES)
def test_sorted_order_at_every_sort_size(post, n, pattern):
    maps, chosen = X.sort_maps(n, pattern)
    kw = sort_kw(n)
    got = post.yolo_eval(maps, synth.YOLO_ANCHORS, 1, X.SORT_IMAGE, debug=True, **kw)
    assert np.array_equal(np.flatnonzero(got[5][:, 0] >= F(X.SORT_SCORE)), chosen)
    if pattern == "equal":                                                     # the index half of the key alone decides
        assert got[3].tolist() == chosen[:kw["max_boxes"]].tolist()
    assert len(got[3]) == min(n, kw["max_boxes"])
    assert_sorted_selection(got, 1, [n], kw["max_boxes"])


def test_sorted_order_in_lds_and_in_global_memory_side_by_side(post):
    """Three classes in one launch: 4097 candidates (global keys), 4096 (the LDS limit), none."""
    maps, chosen = X.sort_maps_three_classes()
    kw = sort_kw(4097)
    got = post.yolo_eval(maps, synth.YOLO_ANCHORS, 3, X.SORT_IMAGE, debug=True, **kw)
    assert_sorted_selection(got, 3, [4097, 4096, 0], kw["max_boxes"])
    assert got[2].tolist() == [0] * 600 + [1] * 600
    assert got[3][:600].tolist() == chosen[:600].tolist()


@pytest.mark.parametrize("pattern", X.SORT_PATTERNS)
def test_batched_sort_chooses_lds_or_global_keys_per_image(post, pattern):
    """F = 3 images with 4097, 1 and 0 candidates in one call: each bitwise the single-image result."""
    sizes = (4097, 1, 0)
    per = [X.sort_maps(n, pattern)[0] for n in sizes]
    maps = [np.stack([per[f][l] for f in range(3)]) for l in range(3)]
    kw = sort_kw(4097)
    batch = post.yolo_eval_batch(maps, synth.YOLO_ANCHORS, 1, X.SORT_IMAGE, **kw)
    assert [len(b[3]) for b in batch] == [600, 1, 0]
    for f, n in enumerate(sizes):
        single = post.yolo_eval(per[f], synth.YOLO_ANCHORS, 1, X.SORT_IMAGE, debug=True, **kw)
        assert_sorted_selection(single, 1, [n], kw["max_boxes"])
        assert_same(batch[f], single[:4])
