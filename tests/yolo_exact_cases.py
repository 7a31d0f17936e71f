"""Exact cases for the YOLO post-processing kernels (csrc/yolo.hip): feature maps on which the float32 decode has ONE right answer,
and candidate lists whose selection order can be written down.  Pure numpy + the oracle, importable without a GPU;
tests/test_yolo_exact_cpu.py checks every claim made here with the oracle alone, tests/test_yolo_exact_gpu.py holds the kernels to them.

The exact logit set.  `expf` is the decode's only inexact step, and it is exact on three logits:
    0     -> sigmoid 0.5, exp 1
    +128  -> sigmoid 1,   exp +inf     (exp(-128) = 2.6e-56 is below the smallest float32 subnormal: 1 / (1 + 0))
    -128  -> sigmoid 0,   exp 0        (1 / (1 + inf))
Every logit of the maps built here is one of the three, so every box coordinate is a chain of individually rounded float32
operations (the anchors are not powers of two: every division rounds) and the kernel's boxes must be BITWISE the oracle's.
A w/h logit of +128 gives a box of infinite extent (-inf .. +inf); anchors are positive, so no coordinate is NaN.
"""
import numpy as np

from oracle import yolo_oracle as Y
from whenet_hip import synth

F = np.float32
ZERO, POS, NEG = F(0), F(128), F(-128)
EXACT = np.array([ZERO, POS, NEG], F)
MASK3 = [[6, 7, 8], [3, 4, 5], [0, 1, 2]]              # model.py:203
MASK2 = [[3, 4, 5], [1, 2, 3]]


def num_boxes(maps):
    return int(sum(m.shape[-3] * m.shape[-2] * 3 for m in maps))


def oracle_decode(maps, anchors, num_classes, image):
    """`Y.yolo_boxes_and_scores` per layer, concatenated: boxes [N,4], scores [N,C] in the kernel's box order."""
    anchors = np.asarray(anchors, F).reshape(-1, 2)
    mask = MASK3 if len(maps) == 3 else MASK2
    inp = (maps[0].shape[0] * 32, maps[0].shape[1] * 32)
    with np.errstate(over="ignore", invalid="ignore"):       # exp(128) = inf is the point
        out = [Y.yolo_boxes_and_scores(m, anchors[mask[l]], num_classes, inp, image) for l, m in enumerate(maps)]
    return np.concatenate([b for b, _ in out]), np.concatenate([s for _, s in out])


def oracle_eval(maps, anchors, num_classes, image, **kw):
    with np.errstate(over="ignore", invalid="ignore"):
        return Y.yolo_eval(maps, anchors, num_classes, image, return_index=True, **kw)


# ---- exact decode cases ---------------------------------------------------------------------------------------------------------
def exact_maps(seed, num_classes, grid_hw=(2, 3), num_layers=3, infinite=4):
    """Maps [gh << l, gw << l, 3 * (5 + C)]: xy, confidence and class logits drawn from all three exact values, w/h logits from
    {0, -128}, and `infinite` boxes per map with a w or h logit of +128."""
    rng = np.random.default_rng(seed)
    maps = []
    for l in range(num_layers):
        gh, gw = grid_hw[0] << l, grid_hw[1] << l
        m = EXACT[rng.integers(0, 3, (gh, gw, 3, 5 + num_classes))]
        m[..., 2:4] = np.array([ZERO, NEG], F)[rng.integers(0, 2, (gh, gw, 3, 2))]
        for _ in range(infinite):
            m[rng.integers(gh), rng.integers(gw), rng.integers(3), 2 + rng.integers(2)] = POS
        maps.append(np.ascontiguousarray(m.reshape(gh, gw, 3 * (5 + num_classes))))
    return maps


IMAGES = ((64, 96), (720, 1280), (1080, 607), (97, 131), (128, 5))       # (128, 5): new width 2.5 -> 2, round half to even
# (name, number of maps, anchors, classes): input 64 x 96 -> maps 2x3, 4x6, 8x12 (N = 378); the tiny configuration has two
CONFIGS = (("full-1", 3, synth.YOLO_ANCHORS, 1), ("full-3", 3, synth.YOLO_ANCHORS, 3), ("tiny-1", 2, synth.YOLO_ANCHORS[:6], 1))
DECODE_CASES = [(f"{name}-{image[0]}x{image[1]}", 100 * k + i, layers, anchors, nc, image)
                for k, (name, layers, anchors, nc) in enumerate(CONFIGS) for i, image in enumerate(IMAGES)]
DECODE_KW = dict(max_boxes=20, score_threshold=0.3, iou_threshold=0.45)


def decode_case(case):
    _, seed, layers, anchors, nc, image = case
    return exact_maps(seed, nc, num_layers=layers), anchors, nc, image


# ---- NMS edge cases: input 32 x 32, maps 1x1, 2x2, 4x4 (N = 63); boxes 0 and 1 are anchors 0 and 1 of the 1x1 map -----------------
EDGE_ANCHORS = synth.YOLO_ANCHORS.copy()
EDGE_ANCHORS[6], EDGE_ANCHORS[7] = (16, 16), (32, 16)       # (w, h): box 0 is 16 x 16, box 1 is 32 x 16 around the same centre
EDGE_N = 63


def edge_maps(wh=((ZERO, ZERO), (ZERO, ZERO)), conf=(POS, POS), cls=(POS, ZERO), all_wh=ZERO):
    """Every confidence logit -128 but those of boxes 0 and 1; xy logits 0 (the two boxes share the centre of the input)."""
    maps = []
    for g in (1, 2, 4):
        m = np.zeros((g, g, 3, 6), F)
        m[..., 2:4] = all_wh
        m[..., 4] = NEG
        maps.append(m)
    for b in (0, 1):
        maps[0][0, 0, b, 2:4] = wh[b]
        maps[0][0, 0, b, 4] = conf[b]
        maps[0][0, 0, b, 5] = cls[b]
    return [m.reshape(m.shape[0], m.shape[1], 18) for m in maps]


# Anchors whose pair has an IoU that depends on how the union is rounded: the box sides are not integers, so inter = dy * dx rounds,
# and (area_a + area_b) - inter with inter's product fused into the subtraction gives 0.37329757 where TensorFlow's IOU(), every
# operation rounded on its own, gives 0.37329754 (tests/test_yolo_exact_cpu.py computes both).  Image = input: the decode is exact.
ROUNDED_ANCHORS = EDGE_ANCHORS.copy()
ROUNDED_ANCHORS[6], ROUNDED_ANCHORS[7] = (7.806, 13.021), (18.38, 14.814)


def edge_pair_iou(image, anchors=EDGE_ANCHORS, **kw):
    """Y.iou of the oracle's boxes 0 and 1."""
    b, _ = oracle_decode(edge_maps(**kw), anchors, 1, image)
    with np.errstate(invalid="ignore"):
        return Y.iou(b[0], b[1])


EDGE_IMAGES = ((32, 32), (720, 1280), (1080, 607))
QUARTER_UP = np.nextafter(F(0.25), F(1))


def edge_cases():
    """(name, maps, image, kwargs, expected index, anchors): the keep-lists are written out here; the CPU test holds the oracle to them, the
    GPU test the kernel."""
    cases = []
    for image in EDGE_IMAGES:
        tag = f"{image[0]}x{image[1]}"
        thr = edge_pair_iou(image)                           # exactly 0.5 (checked on the CPU): `>` keeps the pair, one ulp less does not
        pair = edge_maps()                                   # scores 1 and 0.5
        cases.append((f"iou-at-threshold-{tag}", pair, image, dict(max_boxes=20, score_threshold=0.3, iou_threshold=thr), [0, 1]))
        cases.append((f"iou-above-threshold-{tag}", pair, image,
                      dict(max_boxes=20, score_threshold=0.3, iou_threshold=np.nextafter(thr, F(0))), [0]))
    image = (720, 1280)
    tie = edge_maps(cls=(ZERO, ZERO))                        # equal scores 0.5: the lower index first
    cases.append(("equal-scores-max-1", tie, image, dict(max_boxes=1, score_threshold=0.3, iou_threshold=0.9), [0]))
    cases.append(("equal-scores-max-2", tie, image, dict(max_boxes=2, score_threshold=0.3, iou_threshold=0.9), [0, 1]))
    # box 1 has zero width, the top score and lies inside box 0: IoU 0 by definition, both kept even at threshold 0
    flat = edge_maps(wh=((ZERO, ZERO), (NEG, ZERO)), cls=(ZERO, POS))
    cases.append(("zero-area-on-top", flat, image, dict(max_boxes=20, score_threshold=0.3, iou_threshold=0.0), [1, 0]))
    # two boxes of infinite width: inter / (area + area - inter) = inf / (inf - inf) = NaN, and NaN > threshold is false -> both kept
    # (TensorFlow's IOU() does the same arithmetic).  Boxes with NaN COORDINATES (anchor 0 times inf) are out of scope.
    wide = edge_maps(wh=((POS, ZERO), (POS, ZERO)))
    cases.append(("infinite-extent", wide, image, dict(max_boxes=20, score_threshold=0.3, iou_threshold=0.0), [0, 1]))
    # score threshold at equality: box 0 scores 0.5 * 0.5 = 0.25 exactly, box 1 scores 1
    quarter = edge_maps(conf=(ZERO, POS), cls=(ZERO, POS))
    cases.append(("score-at-threshold", quarter, image, dict(max_boxes=20, score_threshold=0.25, iou_threshold=0.9), [1, 0]))
    cases.append(("score-below-threshold", quarter, image, dict(max_boxes=20, score_threshold=QUARTER_UP, iou_threshold=0.9), [1]))
    # threshold 0 and exact-zero scores: all 63 boxes are candidates; zero areas, so nothing is suppressed: scores 1, 0.5, then the
    # zeros in index order
    zeros = edge_maps(wh=((NEG, NEG), (NEG, NEG)), all_wh=NEG)
    cases.append(("score-threshold-zero", zeros, image, dict(max_boxes=EDGE_N, score_threshold=0.0, iou_threshold=0.5),
                  list(range(EDGE_N))))
    cases = [c + (EDGE_ANCHORS,) for c in cases]
    # an IoU whose last bit depends on the union being rounded operation by operation: at the threshold, and one ulp below it
    thr = edge_pair_iou((32, 32), ROUNDED_ANCHORS)
    cases.append(("rounded-union-at-threshold", edge_maps(), (32, 32), dict(max_boxes=20, score_threshold=0.3, iou_threshold=thr),
                  [0, 1], ROUNDED_ANCHORS))
    cases.append(("rounded-union-above-threshold", edge_maps(), (32, 32),
                  dict(max_boxes=20, score_threshold=0.3, iou_threshold=np.nextafter(thr, F(0))), [0], ROUNDED_ANCHORS))
    return cases


# ---- sort sizes: grid 9, input 288 x 288, maps 9 / 18 / 36, N = 5103 (the smallest above 4097) -------------------------------------
SORT_GRID = 9
SORT_N = 5103
SORT_SIZES = (1, 2, 3, 64, 65, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 5103)
SORT_PATTERNS = ("equal", "normal")
SORT_SCORE = 0.3
SORT_IMAGE = (720, 1280)


def sort_max_boxes(n):
    """The whole sorted order up to 1025 (across the 256-entry LDS selection list); 600 beyond: across the list, a short serial walk."""
    return max(n, 1) if n <= 1025 else 600


def sort_maps(n, pattern, seed=0, num_classes=1):
    """Every w/h logit -128: zero areas, nothing is ever suppressed.  A seeded subset of exactly n boxes has confidence +128, the
    rest -128.  Class logits: all 0 ("equal": n scores of 0.5), or |normal(0, 1)| ("normal": mostly distinct scores, each >= 0.5)."""
    rng = np.random.default_rng([seed, n, SORT_PATTERNS.index(pattern)])
    chosen = np.sort(rng.choice(SORT_N, n, replace=False))
    flat = np.zeros((SORT_N, 5 + num_classes), F)
    flat[:, 0:2] = EXACT[rng.integers(0, 3, (SORT_N, 2))]
    flat[:, 2:4] = NEG
    flat[:, 4] = NEG
    flat[chosen, 4] = POS
    if pattern == "normal":
        flat[:, 5:] = np.abs(rng.normal(0.0, 1.0, (SORT_N, num_classes))).astype(F)
    return split_sort_maps(flat), chosen


def split_sort_maps(flat):
    maps, first = [], 0
    for l in range(3):
        g = SORT_GRID << l
        maps.append(np.ascontiguousarray(flat[first:first + g * g * 3].reshape(g, g, 3 * flat.shape[1])))
        first += g * g * 3
    assert first == SORT_N
    return maps


def sort_maps_three_classes(seed=0):
    """One launch that sorts in LDS and in global memory side by side: class 0 has 4097 candidates (equal scores 0.5), class 1 has
    4096 of them (|normal| logits; the lowest-indexed candidate's class-1 logit is -128), class 2 has none."""
    rng = np.random.default_rng([seed, 3])
    chosen = np.sort(rng.choice(SORT_N, 4097, replace=False))
    flat = np.zeros((SORT_N, 8), F)
    flat[:, 2:4] = NEG
    flat[:, 4] = NEG
    flat[chosen, 4] = POS
    flat[:, 6] = np.abs(rng.normal(0.0, 1.0, SORT_N)).astype(F)
    flat[chosen[0], 6] = NEG
    flat[:, 7] = NEG
    return split_sort_maps(flat), chosen


def expected_order(scores, candidates, max_boxes):
    """sorted(candidates, key=(-score, index))[:max_boxes]: what greedy NMS keeps when nothing is suppressed."""
    s = scores[candidates]
    return candidates[np.lexsort((candidates, -s))][:max_boxes]


# ---- the selection in isolation --------------------------------------------------------------------------------------------------
def assert_selection_is_oracle_nms(result, num_classes, max_boxes, score_threshold, iou_threshold):
    """`result` = yolo_eval(..., debug=True).  The oracle's NMS on the DEVICE's own decoded boxes and scores: index and classes equal,
    returned boxes / scores bitwise the decoded rows.  Nothing here depends on how the decode rounds."""
    gb, gs, gc, gi, all_boxes, all_scores = result
    want_i, want_c = [], []
    for c in range(num_classes):
        cand = np.flatnonzero(all_scores[:, c] >= F(score_threshold))
        with np.errstate(invalid="ignore"):
            keep = Y.non_max_suppression(all_boxes[cand], all_scores[cand, c], max_boxes, iou_threshold)
        want_i += cand[keep].tolist()
        want_c += [c] * len(keep)
    assert gi.tolist() == want_i and gc.tolist() == want_c, (gi.tolist(), want_i)
    assert gb.dtype == F and gs.dtype == F
    assert gb.tobytes() == all_boxes[gi].tobytes() and gs.tobytes() == all_scores[gi, gc].tobytes()
    return want_i
