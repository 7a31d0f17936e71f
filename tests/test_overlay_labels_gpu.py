"""The labels of the pose overlay on the GPU (csrc/overlay.hip: the plan kernel's label records, the draw kernel's
WHENET_DISPLAY_FULL instantiation; Engine::op_annotate / frame_annotate; FramePipeline.annotate(display="full")).  No tolerance
anywhere: the kernels return the bytes of `whenet_annotate_host_ex`, which tests/test_overlay_labels_cpu.py holds to the numpy
statement; a device destination keeps every byte outside its rows; the collect calls return what they return without an annotate."""
import os

import numpy as np
import pytest

from tests import label_cases as LC
from tests import overlay_cases as OC
from tests.test_clip_gpu import assert_same
from tests.test_overlay_gpu import FMT_NAME, MAT_NAME, DeviceSurface, frames, kw, model, planes_of, post, ypr_of  # noqa: F401  (fixtures)
from whenet_hip import overlay
from whenet_hip.frames import FramePipeline

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def host_statement(frame, rects, ypr, fmt, matrix, valid=None, bgr=True, display="full"):
    ypr = np.asarray(ypr, np.float32).reshape(-1, 3)
    out = overlay.annotate_host(frame, rects, ypr[:, 0], ypr[:, 1], ypr[:, 2], format=FMT_NAME[fmt], matrix=MAT_NAME[matrix], valid=valid,
                                bgr=bgr, display=display)
    return planes_of(out)


def op_equals_host(post, frame, order, heads, fmt, matrix, tag, display="full"):
    rects, valid, ypr = heads
    got = overlay.annotate(post, frame, rects, ypr[:, 0], ypr[:, 1], ypr[:, 2], format=FMT_NAME[fmt], matrix=MAT_NAME[matrix], valid=valid,
                           bgr=order == OC.BGR, display=display)
    want = host_statement(frame, rects, ypr, fmt, matrix, valid, bgr=order == OC.BGR, display=display)
    for p, (g, wnt) in enumerate(zip(planes_of(got), want)):
        assert g.shape == wnt.shape and g.tobytes() == wnt.tobytes(), (tag, frame.shape, FMT_NAME[fmt], MAT_NAME[matrix], order, p)
    return want


# ---- the kernels alone are the host statement ------------------------------------------------------------------------------------
def test_op_annotate_full_equals_the_host_function_on_the_head_set(post, frames):
    frame = frames["W"]                                              # 97 x 131
    heads = LC.label_heads(*frame.shape[:2])
    plain = None
    for _, fmt in OC.FORMATS:
        for _, matrix in OC.MATRICES:
            for order in (OC.BGR, OC.RGB):
                want = op_equals_host(post, frame, order, heads, fmt, matrix, "head set")
                if fmt == OC.PACKED and order == OC.BGR:
                    plain = want[0]
    assert (plain.reshape(-1, 3) == LC.COLOUR_BGR).all(axis=1).sum() > 300          # text was painted
    for key, fmt, matrix in (("A", OC.NV12, OC.BT709), ("B", OC.I420, OC.JFIF)):    # 128 x 160 and 75 x 101
        op_equals_host(post, frames[key], OC.BGR, LC.label_heads(*frames[key].shape[:2]), fmt, matrix, key)


def test_lines_across_tile_seams(post):
    heads = LC.seam_heads()
    frame = OC.frame_for(48, 160, 5)
    for _, fmt in OC.FORMATS:
        want = op_equals_host(post, frame, OC.BGR, heads, fmt, OC.BT601, "seams")
    # the cases are what their names say: text on both sides of x = 128, and in all three tile rows
    packed = host_statement(frame, heads[0][:1], heads[2][:1], OC.PACKED, 0)[0].reshape(48, 160, 3)
    text = (packed == LC.COLOUR_BGR).all(axis=2) & ~(frame == LC.COLOUR_BGR).all(axis=2)
    assert text[:, :128].any() and text[:, 128:].any() and text[:16].any() and text[16:32].any() and text[32:].any()
    third = host_statement(frame, heads[0][2:], heads[2][2:], OC.PACKED, 0)[0].reshape(48, 160, 3)
    text = (third == LC.COLOUR_BGR).all(axis=2) & ~(frame == LC.COLOUR_BGR).all(axis=2)
    assert text[15].any() and text[16].any() and text[31].any() and text[32].any()
    assert heads[0][1][1] == 127 and want is not None


@pytest.mark.parametrize("same", [True, False])
def test_256_labelled_heads_on_one_tile(post, same):
    heads = LC.capacity_heads(same)
    assert len(heads[0]) == 256 and all(LC.labels(r, *a)[2] == 7 for r, a in zip(heads[0][::17], heads[2][::17]))
    frame = OC.frame_for(48, 128, 9)
    for fmt in (OC.PACKED, OC.NV12):
        op_equals_host(post, frame, OC.RGB, heads, fmt, OC.BT709, ("capacity", same))


def test_plan_kernels_label_records_on_the_fixtures_angles(post):
    """One head per frame, every angle triple of tests/golden/reference_labels.npz: the picture holds the head's three lines whole,
    every pair of glyphs differs in it (tests/test_overlay_labels_cpu.py), so equal bytes are equal label records."""
    with np.load(os.path.join(GOLDEN, "reference_labels.npz")) as z:
        angles, texts = z["ypr"], z["text"]
    frame = np.zeros((56, 104, 3), np.uint8)
    rect = np.asarray([(40, 2, 54, 30)], np.int32)
    seen = {}
    for i, a in enumerate(angles):
        want = op_equals_host(post, frame, OC.BGR, (rect, None, a.reshape(1, 3)), OC.PACKED, 0, ("angles", i, a.tolist()))[0]
        text = (want.reshape(56, 104, 3) == LC.COLOUR_BGR).all(axis=2)               # on a black frame only the lines have this colour
        key = tuple(t.decode() for t in texts[i]) if all(LC.in_range(v) for v in a) else None
        assert text.any() == (key is not None), (i, a)
        assert seen.setdefault(key, text).tobytes() == text.tobytes(), (i, key)      # the same text is the same pixels ...
    assert len({v.tobytes() for v in seen.values()}) == len(seen) >= 70              # ... and another text other ones


def test_simple_display_gives_the_bytes_of_today(post, frames):
    frame = frames["B"]
    heads = LC.label_heads(*frame.shape[:2])
    rects, valid, ypr = heads
    for _, fmt in OC.FORMATS:
        want = op_equals_host(post, frame, OC.BGR, heads, fmt, OC.BT601, "simple", display="simple")
        got = overlay.annotate(post, frame, rects, *ypr.T, format=FMT_NAME[fmt], valid=valid)          # no keyword at all
        assert all(g.tobytes() == w.tobytes() for g, w in zip(planes_of(got), want))
        assert any(w.tobytes() != f.tobytes() for w, f in zip(want, host_statement(frame, rects, ypr, fmt, OC.BT601, valid)))
    with pytest.raises(ValueError, match="display"):
        post.op_annotate(frame, rects, valid, ypr, overlay.surface_of(np.zeros_like(frame), *frame.shape[:2])[0], display=2)
    out = overlay.annotate(post, frame, rects, *ypr.T, valid=valid, display="full")                    # the handle is usable
    assert out.tobytes() == host_statement(frame, rects, ypr, OC.PACKED, 0, valid)[0].tobytes()


# ---- device destinations -------------------------------------------------------------------------------------------------------------
BOXES = [(30, 8, 70, 50), (45, 70, 90, 128)]          # on 97 x 131: the second one's lines run into the right edge


@pytest.mark.parametrize("fname,fmt", OC.FORMATS)
def test_device_destination_of_width_131_at_every_base_alignment(model, frames, fname, fmt):
    frame = frames["W"]
    h, w = frame.shape[:2]
    assert w == 131
    with FramePipeline(model, depth=1) as fp:
        for base in range(4):
            matrix, extra = base % 3, (0, 1, 5, 64)[base]
            s = DeviceSurface(h, w, fmt, matrix, extra, base)
            fp.begin(frame)
            fp.heads(np.asarray(BOXES, np.float32))
            fp.annotate(s.out, display="full")
            res = fp.collect()
            assert len(res[0]) == 2
            s.check(host_statement(frame, res[0], ypr_of(res), fmt, matrix), (fname, base, extra))      # rows equal, gaps still 0xC3


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def test_pipeline_annotate_full_host_device_and_nv12(model, kw, frames):
    heads_painted = 0
    with FramePipeline(model, depth=1) as fp:
        for i, (key, frame) in enumerate(frames.items()):
            h, w = frame.shape[:2]
            fp.begin(frame)
            fp.detect_heads(**kw)
            plain = fp.collect()
            heads_painted += len(plain[0])
            full = host_statement(frame, plain[0], ypr_of(plain), OC.PACKED, 0)
            simple = host_statement(frame, plain[0], ypr_of(plain), OC.PACKED, 0, display="simple")
            if len(plain[0]):
                assert full[0].tobytes() != simple[0].tobytes(), key
            # a host array
            out = np.zeros_like(frame)
            fp.begin(frame)
            fp.detect_heads(**kw)
            fp.annotate(out, display="full")
            assert_same(fp.collect(), plain)                       # collect returns what it returns without annotate
            assert out.tobytes() == full[0].tobytes(), (key, "host")
            # a device BGR tensor
            s = DeviceSurface(h, w, OC.PACKED, 0, extra=5, base=i + 1)
            fp.begin(frame)
            fp.detect_heads(**kw)
            fp.annotate(s.out, display="full")
            assert_same(fp.collect(), plain)
            s.check(full, (key, "device bgr"))
            # a device NV12 YUVFrame
            matrix = i % 3
            s = DeviceSurface(h, w, OC.NV12, matrix, extra=1, base=2)
            fp.begin(frame)
            fp.detect_heads(**kw)
            fp.annotate(s.out, display="full")
            assert_same(fp.collect(), plain)
            s.check(host_statement(frame, plain[0], ypr_of(plain), OC.NV12, matrix), (key, "device nv12"))
            # display="simple" gives today's bytes
            out = np.zeros_like(frame)
            fp.begin(frame)
            fp.detect_heads(**kw)
            fp.annotate(out, display="simple")
            assert_same(fp.collect(), plain)
            assert out.tobytes() == simple[0].tobytes(), (key, "simple")
    assert heads_painted >= 3


def test_annotate_clip_full_on_a_two_frame_clip(model, kw, frames):
    clip = [frames["A"], np.ascontiguousarray(frames["A"][:, ::-1])]
    with FramePipeline(model, depth=1) as fp:
        fp.begin_clip(clip)
        fp.detect_heads_clip(**kw)
        plain = fp.collect_clip()
        outs = [np.zeros_like(clip[0]), DeviceSurface(clip[1].shape[0], clip[1].shape[1], OC.I420, OC.BT709, 5, 3)]
        fp.begin_clip(clip)
        fp.detect_heads_clip(**kw)
        fp.annotate_clip([outs[0], outs[1].out], display="full")
        got = fp.collect_clip()
        assert got[1] == plain[1]
        for g, p in zip(got[0], plain[0]):
            assert_same(g, p)
        assert sum(len(r[0]) for r in got[0]) >= 1
        assert outs[0].tobytes() == host_statement(clip[0], got[0][0][0], ypr_of(got[0][0]), OC.PACKED, 0)[0].tobytes()
        outs[1].check(host_statement(clip[1], got[0][1][0], ypr_of(got[0][1]), OC.I420, OC.BT709), "clip frame 1")
