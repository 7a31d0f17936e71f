"""Mixed clips (frames of different sizes in one submission), the parts that need no GPU: the header declares and the library
exports the new entry points, the binding's argument checks raise before the library is touched, and the pipeline's calls reach
the handle in the right order (a recording fake handle in its place)."""
import os
import re
from collections import deque

import numpy as np
import pytest

from whenet_hip import _lib, frames as FR
from whenet_hip.frames import FramePipeline

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MIXED_SYMBOLS = ("whenet_clip_begin_mixed", "whenet_op_letterbox_mixed", "whenet_yolo_eval_mixed", "whenet_letterbox_cache_stats")
TINY_ANCHORS = np.array([10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319], np.float32).reshape(-1, 2)


def test_header_declares_and_library_exports_the_mixed_entry_points():
    text = open(os.path.join(ROOT, "include", "whenet_hip.h")).read()
    declared = re.findall(r"WHENET_API\s+[\w\s\*]+?\b(whenet_\w+)\s*\(", text)
    lib = _lib.load()
    for s in MIXED_SYMBOLS:
        assert s in declared, s
        assert s in _lib.EXPORTS and hasattr(lib, s), s
    assert re.search(r"#define WHENET_ABI_VERSION 6\b", text)                   # additions only
    block = text[text.index("MIXED CLIPS: frames of different sizes"):]
    for cite in ("demo_video.py:49-53", "demo_video.py:54-58", "yolo_v3/utils.py:23-34", "yolo_v3/model.py:193-232",
                 "yolo_v3/model.py:153-178"):
        assert cite in block, cite


class Recorder:
    """In the place of a handle: records every call; tickets count up from 40."""

    def __init__(self):
        self.calls, self.next = [], 40

    def clip_begin_mixed(self, frames, bgr=True):
        self.calls.append(("clip_begin_mixed", [f.shape for f in frames], [f.flags.c_contiguous and f.dtype == np.uint8 for f in frames], bgr))
        self.next += 1
        return self.next - 1

    def clip_detect_heads(self, ticket, anchors, num_classes, size, score, iou, max_boxes, max_heads):
        self.calls.append(("clip_detect_heads", ticket, num_classes, tuple(size), max_boxes, max_heads))
        return num_classes * max_boxes

    def collect_clip(self, ticket, frames, slots_per_frame):
        self.calls.append(("collect_clip", ticket, frames, slots_per_frame))
        F, K = frames, slots_per_frame
        z = lambda *s, dt=np.int32: np.zeros(s, dt)
        return (z(F), z(F, K, 4, dt=np.float32), z(F, K, dt=np.float32), z(F, K), z(F, K, 4), z(F, K), np.full((F, K), -1, np.int32),
                np.full((F, K, 3), np.nan, np.float32), z(F, K, 3), None, 0, 0)

    def frame_heads(self, ticket, rects):
        self.calls.append(("frame_heads", ticket, rects.shape))

    def collect(self, ticket, n):
        self.calls.append(("collect", ticket, n))
        return np.zeros((n, 3), np.float32), np.zeros((n, 3), np.int32), None


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were checked")


def pipeline(handle, bgr=True):
    fp = FramePipeline.__new__(FramePipeline)
    fp._h, fp._depth, fp._bgr, fp._detector = handle, 2, bgr, None
    fp._pending, fp._begun, fp._begun_clip = deque(), None, None
    return fp


def frames_of(*shapes):
    return [np.full(s + (3,), i, np.uint8) for i, s in enumerate(shapes)]


def test_mixed_frames_are_checked_before_the_library_is_touched():
    a, b = frames_of((5, 7), (3, 11))
    got = _lib.mixed_u8([a, b[:, ::-1]])
    assert [g.shape for g in got] == [(5, 7, 3), (3, 11, 3)] and all(g.flags.c_contiguous and g.dtype == np.uint8 for g in got)
    assert len(_lib.mixed_u8([a] * 16)) == 16
    assert len(_lib.mixed_u8(np.zeros((2, 5, 7, 3), np.uint8))) == 2           # an array of frames of one size is a list of them
    bad = ([], [a] * 17,
           [a, np.zeros((0, 7, 3), np.uint8)], [a, np.zeros((5, 0, 3), np.uint8)],          # a side of 0
           [a, np.zeros((8193, 1, 3), np.uint8)], [np.zeros((1, 8193, 3), np.uint8)],       # a side above 8192
           [a, b.astype(np.float32)], [a, b.astype(np.int8)],                               # dtype
           [a, b[:, :, 0]], [a, b[None]], [a, np.zeros((3, 11, 4), np.uint8)],              # rank, channels
           a, None, 7)
    for frames in bad:
        with pytest.raises(ValueError):
            _lib.mixed_u8(frames)
        with pytest.raises(ValueError):
            pipeline(Untouchable()).begin_clip_mixed(frames)
        h = _lib.Handle.__new__(_lib.Handle)                   # no device needed: the checks come first
        with pytest.raises(ValueError):
            _lib.Handle.clip_begin_mixed(h, frames)
        with pytest.raises(ValueError):
            _lib.Handle.op_letterbox_mixed(h, frames, (64, 96))
    h = _lib.Handle.__new__(_lib.Handle)
    with pytest.raises(ValueError, match="size"):
        _lib.Handle.op_letterbox_mixed(h, [a, b], (0, 96))
    maps = [np.zeros((2, 2, 3, 18), np.float32), np.zeros((2, 4, 6, 18), np.float32)]
    for shapes in ([(5, 7)], [(5, 7), (3, 11), (2, 2)], [(5, 7), (0, 11)], [(5, 7), (3,)], (5, 7)):
        with pytest.raises(ValueError, match="image_shapes"):
            _lib.Handle.yolo_eval_mixed(h, maps, TINY_ANCHORS, 1, shapes)
    with pytest.raises(ValueError, match="max_boxes"):
        _lib.Handle.yolo_eval_mixed(h, maps, TINY_ANCHORS, 1, [(5, 7), (3, 11)], max_boxes=0)
    with pytest.raises(ValueError, match="feature map"):
        _lib.Handle.yolo_eval_mixed(h, [maps[0], maps[1][:1]], TINY_ANCHORS, 1, [(5, 7), (3, 11)])


def test_begin_clip_still_rejects_frames_of_different_shapes():
    a, b = frames_of((5, 7), (3, 11))
    for call in (lambda: _lib.clip_u8([a, b]), lambda: pipeline(Untouchable()).begin_clip([a, b]),
                 lambda: _lib.Handle.clip_begin(_lib.Handle.__new__(_lib.Handle), [a, b])):
        with pytest.raises(ValueError, match="one size"):
            call()


def test_begin_clip_mixed_calls_the_handle_in_order():
    rec = Recorder()
    a, b, c = frames_of((5, 7), (3, 11), (9, 2))
    kw = dict(size=(64, 96), anchors=TINY_ANCHORS, num_classes=1)
    fp = pipeline(rec, bgr=False)
    fp.begin_clip_mixed([a, b[:, ::-1], c])
    assert fp.in_flight == 0 and fp._begun_clip == (40, 3)
    # one thing at a time between begin and the heads; the calls for one frame refuse a clip
    for call in (lambda: fp.begin_clip_mixed([a, b]), lambda: fp.begin_clip(np.stack([a, a])), lambda: fp.begin(a)):
        with pytest.raises(ValueError, match="has no heads yet"):
            call()
    for call in (lambda: fp.detect_heads(**kw), lambda: fp.detect(**kw), lambda: fp.heads(np.zeros((0, 4), np.float32))):
        with pytest.raises(ValueError, match="a clip was begun last"):
            call()
    with pytest.raises(ValueError, match="max_heads"):
        fp.detect_heads_clip(max_heads=257, **kw)
    fp.detect_heads_clip(max_boxes=7, max_heads=9, **kw)
    assert fp.in_flight == 1 and fp._begun_clip is None
    fp.begin_clip_mixed([c, a])
    fp.detect_heads_clip(max_boxes=5, **kw)
    with pytest.raises(ValueError, match="already in flight"):
        fp.begin_clip_mixed([a, b])
    with pytest.raises(ValueError, match="collect_clip"):
        fp.collect()
    frames, (used, over) = fp.collect_clip(detections=True)
    assert len(frames) == 3 and all(len(t) == 8 and len(t[0]) == 0 for t in frames) and (used, over) == (0, 0)
    assert len(fp.collect_clip()[0]) == 2
    assert rec.calls == [("clip_begin_mixed", [(5, 7, 3), (3, 11, 3), (9, 2, 3)], [True] * 3, False),
                         ("clip_detect_heads", 40, 1, (64, 96), 7, 9),
                         ("clip_begin_mixed", [(9, 2, 3), (5, 7, 3)], [True] * 2, False),
                         ("clip_detect_heads", 41, 1, (64, 96), 5, None),
                         ("collect_clip", 40, 3, 7), ("collect_clip", 41, 2, 5)]
    # F x K beyond the slots of the compaction kernel: refused before the handle sees it
    fp.begin_clip_mixed([a] * 16)
    n = len(rec.calls)
    with pytest.raises(ValueError, match="1..1024"):
        fp.detect_heads_clip(max_boxes=65, **kw)
    assert len(rec.calls) == n


def test_exit_releases_a_mixed_clip_that_never_got_its_heads():
    rec = Recorder()
    a, b = frames_of((5, 7), (3, 11))
    with pipeline(rec) as fp:
        fp.begin_clip_mixed([a, b])
        fp.detect_heads_clip(size=(64, 96), anchors=TINY_ANCHORS, num_classes=1)
        fp.begin_clip_mixed([b, a])
    assert fp.in_flight == 0 and fp._begun_clip is None
    assert [c[0] for c in rec.calls] == ["clip_begin_mixed", "clip_detect_heads", "clip_begin_mixed", "frame_heads", "collect_clip",
                                         "collect"]
    assert rec.calls[3] == ("frame_heads", 41, (0, 4)) and rec.calls[5] == ("collect", 41, 0)
