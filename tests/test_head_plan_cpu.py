"""Host side of the one-submission frame path (begin -> detect_heads -> collect), no GPU: the crop plan the library exposes
(`whenet_crop_plan`, what `frame_heads` uploads and csrc/headplan.hip reproduces on the device) against the pre-processing
oracle for every source size, and FramePipeline's bookkeeping over a fake handle."""
import numpy as np
import pytest

from oracle import preprocess_oracle as P
from whenet_hip import _lib
from whenet_hip.frames import FramePipeline

OUT = 224


@pytest.fixture(scope="module")
def oracle_tables():
    """linear_tables of every source size 1..2048, both axes: [src-1] -> (xofs, a0, a1, xmax, yofs, b0, b1)."""
    rows = []
    for src in range(1, 2049):
        xo, xc, xmax = P.linear_tables(src, OUT, True)
        yo, yc, _ = P.linear_tables(src, OUT, False)
        rows.append((xo, xc[:, 0], xc[:, 1], xmax, yo, yc[:, 0], yc[:, 1]))
    return rows


def test_crop_plan_tables_equal_the_oracle_for_every_source_size(oracle_tables):
    assert _lib.CROP_PLAN_INTS == 8 + 6 * OUT
    for src in range(1, 2049):
        # width src with another height and the other way round: the two axes are independent tables
        other = 2049 - src
        plan = _lib.crop_plan([3, 5, 3 + other, 5 + src])
        T = plan[8:].reshape(6, OUT)
        xo, a0, a1, xmax, _, _, _ = oracle_tables[src - 1]
        _, _, _, _, yo, b0, b1 = oracle_tables[other - 1]
        assert plan[:8].tolist() == [3, 5, other, src, 0, xmax, 0, 0], src
        for got, want in zip(T, (xo, a0, a1, yo, b0, b1)):
            assert np.array_equal(got, want), src


def test_crop_plan_header_and_the_2x_shrink_flag():
    for h in (1, 223, 224, 447, 448, 449, 896):
        for w in (1, 223, 224, 447, 448, 449, 896):
            plan = _lib.crop_plan([7, 11, 7 + h, 11 + w])
            assert plan[:4].tolist() == [7, 11, h, w] and plan[6] == 0 and plan[7] == 0
            assert plan[4] == (1 if (h, w) == (448, 448) else 0), (h, w)
    assert _lib.crop_plan([0, 0, 9, 1])[5] == 0                    # a 1-pixel-wide window: every column reads a single sample
    for empty in ([5, 5, 5, 9], [5, 5, 9, 5], [9, 9, 5, 5]):
        with pytest.raises(ValueError, match="empty crop window"):
            _lib.crop_plan(empty)
    h = _lib.load()
    assert h.whenet_crop_plan(None, None) == _lib.EINVAL


class FakeHandle:
    """The calls FramePipeline makes, recorded; results carry the ticket so that the collection order can be read back."""

    def __init__(self):
        self.calls, self.next, self.kind = [], 0, {}

    def set_option(self, k, v):
        self.calls.append(("set_option", k, v))

    def _ticket(self, kind):
        t, self.next = self.next, self.next + 1
        self.kind[t] = kind
        return t

    def submit_frame(self, frame, rects, bgr=True):
        return self._ticket("plain")

    def frame_begin(self, frame, bgr=True):
        return self._ticket("begun")

    def frame_heads(self, ticket, rects):
        assert self.kind[ticket] == "begun"
        self.kind[ticket] = "plain"

    def frame_detect_heads(self, ticket, anchors, num_classes, size, score, iou, max_boxes):
        assert self.kind[ticket] == "begun"
        self.kind[ticket] = "detect"
        self.calls.append(("frame_detect_heads", ticket, np.asarray(anchors).size, num_classes, tuple(size), score, iou, max_boxes))
        return num_classes * max_boxes

    def collect(self, ticket, n, want_logits=False):
        assert self.kind.pop(ticket) == "plain"
        return np.full((n, 3), float(ticket), np.float32), np.zeros((n, 3), np.int32), None

    def collect_detect(self, ticket, capacity, want_logits=False):
        assert self.kind.pop(ticket) == "detect" and capacity == 20
        k = 3                                                      # three detections, the middle one without a window
        boxes = np.arange(k * 4, dtype=np.float32).reshape(k, 4)
        rects = np.arange(k * 4, dtype=np.int32).reshape(k, 4) + 100
        valid = np.array([1, 0, 1], np.int32)
        ypr = np.full((k, 3), float(ticket), np.float32)
        ypr[1] = np.nan
        return boxes, np.ones(k, np.float32), np.zeros(k, np.int32), rects, valid, ypr, np.zeros((k, 3), np.int32), None


class FakeModel:
    def __init__(self):
        self._handle = FakeHandle()


FRAME = np.zeros((48, 64, 3), np.uint8)
BOXES = np.array([[8, 8, 30, 30], [10, 30, 40, 60]], np.float32)
ANCHORS = np.arange(12, dtype=np.float32)


def test_detect_heads_without_begin_raises():
    fp = FramePipeline(FakeModel(), depth=2)
    with pytest.raises(ValueError, match="begin"):
        fp.detect_heads(anchors=ANCHORS)
    fp.begin(FRAME)
    with pytest.raises(ValueError, match="Multiples of 32"):
        fp.detect_heads(size=(40, 64), anchors=ANCHORS)
    with pytest.raises(ValueError, match="anchors"):
        fp.detect_heads()                                          # no YOLO on the handle and no anchors given
    fp.detect_heads(size=(64, 96), score=.5, iou=.4, max_boxes=20, anchors=ANCHORS)
    assert fp._h.calls[-1] == ("frame_detect_heads", 0, 12, 1, (64, 96), .5, .4, 20)
    with pytest.raises(ValueError, match="begin"):                 # its heads are enqueued: neither form may follow
        fp.detect_heads(anchors=ANCHORS)
    with pytest.raises(ValueError, match="begin"):
        fp.heads(BOXES)
    assert fp.in_flight == 1
    rects, yaw, pitch, roll = fp.collect()
    assert rects.tolist() == [[100, 101, 102, 103], [108, 109, 110, 111]] and yaw.tolist() == [0.0, 0.0] and len(pitch) == len(roll) == 2


def test_collect_detections_after_submit_raises_and_keeps_the_frame():
    fp = FramePipeline(FakeModel(), depth=2)
    fp.submit(FRAME, BOXES)
    with pytest.raises(ValueError, match="detect_heads"):
        fp.collect(detections=True)
    assert fp.in_flight == 1
    assert len(fp.collect()[0]) == 2
    fp.begin(FRAME)
    fp.heads(BOXES)
    with pytest.raises(ValueError, match="detect_heads"):
        fp.collect(detections=True)
    fp.collect()
    fp.begin(FRAME)
    fp.detect_heads(anchors=ANCHORS)
    res = fp.collect(detections=True)
    assert len(res) == 8
    rects, yaw, pitch, roll, boxes, scores, classes, valid = res
    assert valid.tolist() == [1, 0, 1] and boxes.shape == (3, 4) and len(scores) == len(classes) == 3
    assert rects.shape == (2, 4) and not np.isnan(yaw).any() and len(yaw) == len(pitch) == len(roll) == 2


def test_mixed_submissions_collect_in_order():
    m = FakeModel()
    with FramePipeline(m, depth=4) as fp:
        fp.begin(FRAME)
        fp.detect_heads(anchors=ANCHORS)                           # ticket 0
        fp.submit(FRAME, BOXES)                                    # ticket 1
        fp.begin(FRAME)
        fp.heads(BOXES[:1])                                        # ticket 2
        fp.begin(FRAME)
        fp.detect_heads(anchors=ANCHORS)                           # ticket 3
        with pytest.raises(ValueError, match="in flight"):
            fp.begin(FRAME)
        got = [fp.collect(), fp.collect(), fp.collect(), fp.collect(detections=True)]
        assert [float(g[1][0]) for g in got] == [0.0, 1.0, 2.0, 3.0]
        assert [len(g[0]) for g in got] == [2, 2, 1, 2] and [len(g) for g in got] == [4, 4, 4, 8]
        fp.begin(FRAME)
        fp.detect_heads(anchors=ANCHORS)                           # left in flight: the context manager collects it
    assert m._handle.kind == {}
