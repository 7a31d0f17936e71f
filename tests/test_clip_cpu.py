"""Clips (several frames per submission), the parts that need no GPU: the header declares and the library exports the new entry
points, the Python argument checks raise before the library is touched, and the result scatter of `collect_clip` as a pure
function on synthetic arrays."""
import os
import re
from collections import deque

import numpy as np
import pytest

from whenet_hip import _lib, frames as FR
from whenet_hip.frames import FramePipeline

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CLIP_SYMBOLS = ("whenet_clip_begin", "whenet_clip_detect_heads", "whenet_collect_clip", "whenet_op_letterbox_batch",
                "whenet_yolo_eval_batch", "whenet_op_head_compact")
TINY_ANCHORS = np.array([10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319], np.float32).reshape(-1, 2)


def test_header_declares_and_library_exports_the_clip_entry_points():
    text = open(os.path.join(ROOT, "include", "whenet_hip.h")).read()
    declared = re.findall(r"WHENET_API\s+[\w\s\*]+?\b(whenet_\w+)\s*\(", text)
    lib = _lib.load()
    for s in CLIP_SYMBOLS:
        assert s in declared, s
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert re.search(r"#define WHENET_ABI_VERSION 6\b", text)                   # additions only
    # every new entry point is described next to the reference lines it stands for
    block = text[text.index("CLIPS: several frames per submission"):]
    for cite in ("demo_video.py:49-53", "demo_video.py:54-58", "yolo_v3/utils.py:23-34", "yolo_v3/model.py:193-232"):
        assert cite in block, cite


class Untouchable:
    """In the place of a handle: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were checked")


def pipeline(begun=None, begun_clip=None, pending=()):
    fp = FramePipeline.__new__(FramePipeline)
    fp._h, fp._depth, fp._bgr, fp._detector = Untouchable(), 2, True, None
    fp._pending, fp._begun, fp._begun_clip = deque(pending), begun, begun_clip
    return fp


def test_clip_frames_are_checked_and_stacked_before_the_library_is_touched():
    a, b = np.zeros((5, 7, 3), np.uint8), np.ones((5, 7, 3), np.uint8)
    got = _lib.clip_u8([a, b])
    assert got.shape == (2, 5, 7, 3) and got.dtype == np.uint8 and got.flags.c_contiguous and got[1].all() and not got[0].any()
    assert _lib.clip_u8(np.zeros((16, 5, 7, 3), np.uint8)[:, ::-1]).flags.c_contiguous
    bad = ([a, np.zeros((5, 8, 3), np.uint8)],                 # different shapes
           [a, np.zeros((5, 7, 3), np.float32)],               # different dtypes
           [a, np.zeros((5, 7, 3), np.int8)],
           [a.astype(np.float32)] * 2,
           [],                                                 # F outside 1..16
           [a] * 17,
           np.zeros((17, 5, 7, 3), np.uint8),
           np.zeros((0, 5, 7, 3), np.uint8),
           np.zeros((5, 7, 3), np.uint8),                      # one frame is not a clip array
           np.zeros((2, 5, 7, 4), np.uint8))
    for frames in bad:
        with pytest.raises(ValueError):
            _lib.clip_u8(frames)
        with pytest.raises(ValueError):
            pipeline().begin_clip(frames)
        h = _lib.Handle.__new__(_lib.Handle)                   # no device needed: the checks come first
        with pytest.raises(ValueError):
            _lib.Handle.clip_begin(h, frames)
        with pytest.raises(ValueError):
            _lib.Handle.op_letterbox_batch(h, frames, (64, 96))


def test_detect_heads_clip_checks_its_arguments_before_the_library_is_touched():
    kw = dict(size=(64, 96), anchors=TINY_ANCHORS, num_classes=1)
    assert FR.clip_slots((64, 96), TINY_ANCHORS, 1, 20) == 20
    assert FR.clip_slots((64, 96), TINY_ANCHORS, 2, 1000) == 2 * 90              # cut to the (2*3 + 4*6) * 3 boxes the maps hold
    assert FR.clip_slots((416, 416), np.zeros((9, 2)), 1, 20000) == 10647
    for max_heads in (0, 257, -1):
        with pytest.raises(ValueError, match="max_heads"):
            pipeline(begun_clip=(0, 3)).detect_heads_clip(max_heads=max_heads, **kw)
        with pytest.raises(ValueError, match="max_heads"):
            _lib.Handle.clip_detect_heads(_lib.Handle.__new__(_lib.Handle), 0, TINY_ANCHORS, 1, (64, 96), max_heads=max_heads)
        with pytest.raises(ValueError, match="max_heads"):
            _lib.Handle.op_head_compact(_lib.Handle.__new__(_lib.Handle), np.zeros((2, 3), np.int32), np.zeros(2, np.int32), max_heads)
    with pytest.raises(ValueError, match="1..1024"):                             # 16 x 65 slots
        pipeline(begun_clip=(0, 16)).detect_heads_clip(max_boxes=65, **kw)
    with pytest.raises(ValueError, match="max_boxes"):
        pipeline(begun_clip=(0, 2)).detect_heads_clip(max_boxes=0, **kw)
    with pytest.raises(ValueError, match="Multiples of 32"):
        pipeline(begun_clip=(0, 2)).detect_heads_clip(size=(64, 100), anchors=TINY_ANCHORS)
    with pytest.raises(ValueError, match="no clip begun"):
        pipeline().detect_heads_clip(**kw)
    with pytest.raises(ValueError, match="single frame"):                        # a frame ticket
        pipeline(begun=(0, 10, 10)).detect_heads_clip(**kw)
    # the calls that work on one frame refuse a clip
    for call in (lambda fp: fp.detect(**kw), lambda fp: fp.detect_heads(**kw), lambda fp: fp.detector_input((64, 96)),
                 lambda fp: fp.heads(np.zeros((0, 4), np.float32))):
        with pytest.raises(ValueError, match="a clip was begun last"):
            call(pipeline(begun_clip=(0, 3)))
    # one thing at a time between begin and the heads
    frames = np.zeros((2, 5, 7, 3), np.uint8)
    with pytest.raises(ValueError, match="has no heads yet"):
        pipeline(begun_clip=(0, 3)).begin_clip(frames)
    with pytest.raises(ValueError, match="has no heads yet"):
        pipeline(begun_clip=(0, 3)).begin(frames[0])
    with pytest.raises(ValueError, match="has no heads yet"):
        pipeline(begun=(0, 5, 7)).begin_clip(frames)
    with pytest.raises(ValueError, match="already in flight"):
        pipeline(pending=[(0, None, 20), (1, None, 20)]).begin_clip(frames)
    # collect and collect_clip each refuse the other's submissions and leave them in flight
    fp = pipeline(pending=[(0, FR._CLIP, (3, 20))])
    with pytest.raises(ValueError, match="collect_clip"):
        fp.collect()
    with pytest.raises(ValueError, match="collect_clip"):
        fp.collect(detections=True)
    assert fp.in_flight == 1
    for entry in ((0, None, 20), (0, np.zeros((0, 4), np.int32), 0)):
        fp = pipeline(pending=[entry])
        with pytest.raises(ValueError, match="not a clip"):
            fp.collect_clip()
        assert fp.in_flight == 1
    with pytest.raises(ValueError, match="nothing in flight"):
        pipeline().collect_clip()


def test_scatter_clip_row_minus_one_counts_and_filtering():
    F, K = 3, 4
    rng = np.random.default_rng(5)
    boxes = rng.normal(size=(F, K, 4)).astype(np.float32)
    scores = rng.random((F, K)).astype(np.float32)
    classes = np.zeros((F, K), np.int32)
    rects = rng.integers(0, 100, (F, K, 4)).astype(np.int32)
    ypr = rng.normal(size=(F, K, 3)).astype(np.float32)
    counts = np.array([3, 0, 4], np.int32)
    # frame 0: slot 1 has no window; slot 3 lies beyond the count although its flags are set.  frame 1: nothing.
    # frame 2: every slot has a window, slot 2 and 3 got no row (overflow)
    valid = np.array([[1, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]], np.int32)
    row = np.array([[0, -1, 1, 7], [5, 5, 5, 5], [2, 3, -1, -1]], np.int32)
    ypr[row < 0] = np.nan
    plain = FR.scatter_clip(counts, boxes, scores, classes, rects, valid, row, ypr)
    full = FR.scatter_clip(counts, boxes, scores, classes, rects, valid, row, ypr, detections=True)
    assert len(plain) == len(full) == F and all(len(t) == 4 for t in plain) and all(len(t) == 8 for t in full)
    keep = ([0, 2], [], [0, 1])
    for f in range(F):
        n = int(counts[f])
        for t in (plain[f], full[f][:4]):
            assert t[0].dtype == np.int32 and t[0].shape == (len(keep[f]), 4) and np.array_equal(t[0], rects[f, keep[f]])
            for j in range(3):
                assert t[1 + j].dtype == np.float32 and t[1 + j].shape == (len(keep[f]),)
                assert t[1 + j].tobytes() == ypr[f, keep[f], j].tobytes() and not np.isnan(t[1 + j]).any()
        b, s, c, v = full[f][4:]
        assert b.shape == (n, 4) and s.shape == c.shape == v.shape == (n,)
        assert b.tobytes() == boxes[f, :n].tobytes() and s.tobytes() == scores[f, :n].tobytes()
        assert np.array_equal(v, valid[f, :n]) and np.array_equal(c, classes[f, :n])
    # the results do not alias the slot arrays
    full[2][4][:] = 0
    assert boxes[2].any()
