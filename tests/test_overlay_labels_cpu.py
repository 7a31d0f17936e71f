"""The labels of the pose overlay without a GPU: `whenet_overlay_labels` against the EXECUTED reference (demo_video.process_detection
with --display full under tests/refharness.py, committed as tests/golden/reference_labels.npz) and against Python's own formatting
on a sweep of float32 angles; the font against this suite's copy of it; the thin raster rule; `whenet_annotate_host_ex` against the
numpy statement of tests/label_cases.py byte for byte; the plumbing."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import label_cases as LC
from tests import overlay_cases as OC
from tests import refharness
from whenet_hip import _lib, overlay
from whenet_hip.frames import FramePipeline

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_labels.npz")
HEADER = os.path.join(ROOT, "include", "whenet_hip.h")
WINDOW = np.asarray((40, 20, 90, 80), np.int32)


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(GOLDEN))


# ---- 1. text and origins against executed reference code ------------------------------------------------------------------------
def test_fixture_holds_the_case_set_and_the_putText_arguments(recorded):
    assert recorded["ypr"].tobytes() == LC.fixture_angles().tobytes()
    for a in LC.DESIGNED_ANGLES:                                   # (-0.0 == 0.0: compare the bits)
        assert np.float32(a).tobytes() in {v.tobytes() for v in recorded["ypr"][:, 0]}, a
    # what the reference passes besides text and origin (demo_video.py:32-34): FONT_HERSHEY_SIMPLEX, 0.4, (100, 255, 0), 1
    assert (recorded["font"] == refharness.Cv2Recorder.FONT_HERSHEY_SIMPLEX).all() and (recorded["scale"] == 0.4).all()
    assert (recorded["colour"] == np.array(LC.COLOUR_BGR)).all() and (recorded["thickness"] == 1).all()


def test_labels_equal_the_recorded_putText_calls(recorded):
    labelled = 0
    for i, (window, a) in enumerate(zip(recorded["window"], recorded["ypr"])):
        texts, origins, flags = overlay.labels(window, *a)
        want = [t.decode() for t in recorded["text"][i]]
        assert origins.tolist() == recorded["origin"][i].tolist(), i
        assert want == [n + LC.number(v) for n, v in zip(LC.NAMES, a)], i          # (the numpy statement says the same)
        if all(LC.in_range(v) for v in a):
            assert flags == 7 and texts == want, (i, a, texts, want)
            labelled += 1
        else:                                                      # the reference prints 10000.0; the overlay paints no line
            assert flags == 3 and texts == ["", "", ""] and any("10000.0" in t for t in want), (i, a)
    assert labelled >= len(recorded["ypr"]) - 4 and labelled < len(recorded["ypr"])


@pytest.mark.skipif(not refharness.available(), reason="the reference tree is not present")
def test_live_reference_run_reproduces_the_fixture(recorded):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_label_fixture", os.path.join(ROOT, "tests", "golden", "make_label_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    boxes, frame_hw, ypr = mod.cases()
    assert boxes.tobytes() == recorded["boxes"].tobytes() and np.array_equal(frame_hw, recorded["frame_hw"])
    live = mod.run_reference(boxes, frame_hw, ypr)
    for key, value in live.items():
        assert np.array_equal(value, recorded[key]), key


# ---- 2. the format sweep -----------------------------------------------------------------------------------------------------
class Labels:
    """whenet_overlay_labels on one window, without the Python layer's allocations."""

    def __init__(self):
        self.lib = _lib.load()
        self.text = C.create_string_buffer(48)
        self.origin = np.zeros((3, 2), np.int32)
        self.flags = C.c_int32(0)

    def __call__(self, y, p, r):
        rc = self.lib.whenet_overlay_labels(_lib._ptr(WINDOW), float(y), float(p), float(r), self.text, _lib._ptr(self.origin), C.byref(self.flags))
        assert rc == _lib.OK
        raw = self.text.raw
        return [raw[16 * i:16 * i + 16].split(b"\0", 1)[0].decode() for i in range(3)], self.flags.value


def sweep_values():
    f32 = np.float32
    eighths = (np.arange(-80200, 80201, dtype=np.int64) / 8).astype(f32)
    halves = (np.arange(-400, 400, 2, dtype=np.int64) + 1).astype(f32) / f32(2)                # every half-integer in [-200, 200]
    assert halves[0] == -199.5 and halves[-1] == 199.5 and len(halves) == 400
    edge = np.asarray([9999.5, -9999.5], f32)
    around = [np.nextafter(v, f32(np.inf)) for v in (halves, edge)] + [np.nextafter(v, f32(-np.inf)) for v in (halves, edge)]
    tiny = np.asarray([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38], f32)
    return np.concatenate([eighths, halves, edge] + around + [tiny])


def test_text_and_the_no_labels_flag_on_a_sweep_of_float32_angles():
    call = Labels()
    values = sweep_values()
    ok = np.asarray([LC.in_range(v) for v in values])
    assert ok.sum() > 159000 and (~ok).sum() > 400
    good = values[ok]
    good = np.concatenate([good, good[:(-len(good)) % 3]]).reshape(-1, 3)                      # three angles per call
    for y, p, r in good:
        texts, flags = call(y, p, r)
        assert flags == 7 and texts == [n + LC.number(a) for n, a in zip(LC.NAMES, (y, p, r))], (y, p, r, texts)
        assert max(len(t) for t in texts) <= LC.MAX_CHARS
    for slot, v in zip(itertools.cycle(range(3)), values[~ok]):                               # one angle out of range: no line at all
        a = [1.0, 2.0, 3.0]
        a[slot] = v
        assert call(*a) == (["", "", ""], 3), (v, slot)
    for v in (np.inf, -np.inf, np.nan):                                                        # not finite: the rectangle only
        assert call(v, 0, 0) == (["", "", ""], 1) and call(0, 0, v) == (["", "", ""], 1)
    assert call(9999.4, -9999.4, np.nextafter(np.float32(9999.5), np.float32(0)))[0] == ["yaw: 9999.0", "pitch: -9999.0", "roll: 9999.0"]
    assert LC.number(9999.5) == "10000.0" and LC.number(-0.3) == "-0.0" and LC.number(2.5) == "2.0" and LC.number(99.49999) == "99.0"


def test_labels_flags_origins_and_range():
    texts, origins, flags = overlay.labels((40, 20, 90, 80), 10.2, -5.5, 2.5)
    assert (texts, origins.tolist(), flags) == (["yaw: 10.0", "pitch: -6.0", "roll: 2.0"], [[20, 40], [20, 25], [20, 10]], 7)
    assert overlay.labels((40, 20, 90, 80), 10.2, -5.5, 2.5) [0] == LC.labels((40, 20, 90, 80), 10.2, -5.5, 2.5)[0]
    assert overlay.labels((-40, -20, 90, 80), 1, 2, 3)[1].tolist() == [[-20, -40], [-20, -55], [-20, -70]]
    with pytest.raises(ValueError, match="-4096..8192"):
        overlay.labels((0, 0, 10, 8193), 0, 0, 0)
    lib = _lib.load()
    text, origin = C.create_string_buffer(48), np.zeros((3, 2), np.int32)
    assert lib.whenet_overlay_labels(None, 0, 0, 0, text, _lib._ptr(origin), None) == _lib.EINVAL
    assert lib.whenet_overlay_labels(_lib._ptr(WINDOW), 0, 0, 0, None, _lib._ptr(origin), None) == _lib.EINVAL
    assert lib.whenet_overlay_labels(_lib._ptr(WINDOW), 0, 0, 0, text, None, None) == _lib.EINVAL
    assert lib.whenet_overlay_labels(_lib._ptr(WINDOW), 0, 0, 0, text, _lib._ptr(origin), None) == _lib.OK


# ---- 3. the font ---------------------------------------------------------------------------------------------------------------
def test_glyphs_equal_the_suites_table_and_stay_in_their_box():
    assert len(LC.GLYPHS) == 25 and set(LC.GLYPHS) == set(LC.FONT) == set("achiloprtwy: -.0123456789") and _lib.OVERLAY_GLYPHS == LC.GLYPHS
    pixels = {}
    for ch in LC.GLYPHS:
        segs = overlay.glyph(ch)
        assert segs.dtype == np.int32 and [tuple(s) for s in segs.tolist()] == LC.FONT[ch], ch
        assert len(segs) <= 8 and (len(segs) >= 1 or ch == " "), ch
        for x0, y0, x1, y1 in segs.tolist():
            assert LC.BOX_X[0] <= min(x0, x1) and max(x0, x1) <= LC.BOX_X[1] and LC.BOX_Y[0] <= min(y0, y1) and max(y0, y1) <= LC.BOX_Y[1], ch
        pixels[ch] = frozenset(LC.glyph_pixels(ch, [tuple(s) for s in segs.tolist()]))       # searched 3 pixels beyond the box
        assert all(LC.BOX_X[0] <= x <= LC.BOX_X[1] and LC.BOX_Y[0] <= y <= LC.BOX_Y[1] for x, y in pixels[ch]), ch
        if ch not in "py":
            assert all(y <= 0 for _, y in pixels[ch]), (ch, "goes below the baseline")
    assert len(set(pixels.values())) == 25                          # pairwise different
    for a, b in itertools.combinations(LC.GLYPHS, 2):               # ... and by more than a pixel
        assert len(pixels[a] ^ pixels[b]) >= 2, (a, b)
    with pytest.raises(ValueError, match="not one of"):
        overlay.glyph("b")
    with pytest.raises(ValueError):
        overlay.glyph("yaw")
    lib = _lib.load()
    assert lib.whenet_overlay_glyph(ord("0"), None) == _lib.EINVAL and lib.whenet_overlay_glyph(0, _lib._ptr(np.zeros((8, 4), np.int32))) == _lib.EINVAL


def test_header_states_the_font_the_library_returns():
    text = open(HEADER).read()
    assert re.search(r'#define WHENET_OVERLAY_GLYPHS "([^"]+)"', text).group(1) == LC.GLYPHS
    m = re.search(r"#define WHENET_OVERLAY_FONT \{ \\\n((?:.*\\\n)*.*)\n", text)
    rows = [[int(v) for v in re.findall(r"-?\d+", r)] for r in re.findall(r"\{([^{}]+)\}", m.group(1))]
    assert len(rows) == 25 and all(len(r) == 33 for r in rows)
    for ch, row in zip(LC.GLYPHS, rows):
        n = row[0]
        assert [tuple(row[1 + 4 * s:5 + 4 * s]) for s in range(n)] == LC.FONT[ch] and not any(row[1 + 4 * n:]), ch
    assert "restated, unpinned" in text and "#define WHENET_ABI_VERSION 6" in text
    assert int(re.search(r"#define WHENET_DISPLAY_SIMPLE (\d+)", text).group(1)) == _lib.DISPLAY_SIMPLE == LC.SIMPLE
    assert int(re.search(r"#define WHENET_DISPLAY_FULL (\d+)", text).group(1)) == _lib.DISPLAY_FULL == LC.FULL
    lib = _lib.load()
    for name in ("whenet_overlay_labels", "whenet_overlay_glyph", "whenet_annotate_host_ex", "whenet_op_annotate_ex", "whenet_frame_annotate_ex"):
        assert re.search(r"WHENET_API int " + name + r"\(", text), name
        assert name in _lib.EXPORTS and getattr(lib, name)


# ---- 4. the thin rule ------------------------------------------------------------------------------------------------------------
def test_thin_rule_on_every_segment_of_the_glyph_box():
    points = [(x, y) for x in range(LC.BOX_X[0], LC.BOX_X[1] + 1) for y in range(LC.BOX_Y[0], LC.BOX_Y[1] + 1)]
    grid = [(x, y) for x in range(LC.BOX_X[0] - 2, LC.BOX_X[1] + 3) for y in range(LC.BOX_Y[0] - 2, LC.BOX_Y[1] + 3)]
    for (px, py), (qx, qy) in itertools.combinations_with_replacement(points, 2):
        thin = {g for g in grid if LC.hit(px, py, qx, qy, *g)}
        assert thin == {g for g in grid if LC.hit(qx, qy, px, py, *g)}                            # symmetric
        assert all(LC.hit(px, py, qx, qy, *g, reach=2) for g in thin)                            # a subset of the reach-1 rule
        assert (px, py) in thin and (qx, qy) in thin
        assert all(LC.BOX_X[0] <= x <= LC.BOX_X[1] and LC.BOX_Y[0] <= y <= LC.BOX_Y[1] for x, y in thin)
        if abs(qy - py) >= abs(qx - px):                                                          # steep: a pixel on every row
            assert {y for _, y in thin} == set(range(min(py, qy), max(py, qy) + 1)), (px, py, qx, qy)
        else:                                                                                     # shallow: on every column
            assert {x for x, _ in thin} == set(range(min(px, qx), max(px, qx) + 1)), (px, py, qx, qy)


def test_thin_rule_is_the_distance_statement_in_exact_rationals():
    from fractions import Fraction
    for px, py, qx, qy in ((0, -8, 4, -8), (4, -8, 1, 0), (0, -5, 2, 0), (4, -5, 1, 3), (2, -7, 2, -7), (1, -6, 2, -8), (0, 3, 5, -9)):
        dx, dy = qx - px, qy - py
        L2 = dx * dx + dy * dy
        for x in range(-2, 8):
            for y in range(-11, 6):
                t = Fraction(0) if L2 == 0 else min(max(Fraction((x - px) * dx + (y - py) * dy, L2), 0), 1)
                d2 = (x - px - t * dx) ** 2 + (y - py - t * dy) ** 2
                assert LC.hit(px, py, qx, qy, x, y) == (d2 <= Fraction(1, 4)), (px, py, qx, qy, x, y)
                assert LC.hit(px, py, qx, qy, x, y, reach=2) == (d2 <= 1)


def test_reach_1_rule_of_the_changed_overlay_hit_is_the_existing_statement():
    """overlay_hit took a reach parameter: with the axes' reach the host function still paints tests/overlay_cases.py's pixels
    (and LC.hit(reach=2) is that rule)."""
    for seg in ((2, 3, 15, 3), (4, 1, 4, 11), (1, 1, 10, 10), (3, 0, 5, 12), (6, 6, 6, 6), (-5, -3, 30, 20), (16, 5, 2, 9), (17, 0, 0, 12)):
        mask = OC.hit_mask(13, 18, *seg)
        assert all(mask[y, x] == LC.hit(*seg, x, y, reach=2) for y in range(13) for x in range(18)), seg
    for h, w in ((33, 19), (64, 48)):
        for ci, (name, heads) in enumerate(OC.heads_cases(h, w).items()):
            frame = OC.frame_for(h, w, 100 + ci)
            got = host_planes(frame, OC.BGR, heads, OC.PACKED, 0, LC.SIMPLE)
            assert got[0].tobytes() == OC.annotate(frame, OC.BGR, *heads, OC.PACKED)[0].tobytes(), (h, w, name)


# ---- 5. the host function against the numpy statement ------------------------------------------------------------------------
def host_planes(frame, order, heads, fmt, matrix, display, extra=0, fill=0x5A, ex=True):
    h, w = frame.shape[:2]
    rects, valid, ypr = heads
    shapes = OC.plane_shapes(fmt, h, w)
    bufs = [np.full((rows, rb + extra), fill, np.uint8) for rows, rb in shapes]
    s = _lib.SurfaceC()
    for i, b in enumerate(bufs):
        s.plane[i], s.pitch[i] = b.ctypes.data, b.shape[1]
    s.format, s.matrix, s.on_device = fmt, matrix, 0
    rects, valid, ypr = _lib.overlay_heads(rects, valid, ypr)
    lib, P = _lib.load(), _lib._ptr
    args = (P(frame), h, w, order, P(rects), P(valid), P(ypr), len(rects), C.byref(s))
    rc = lib.whenet_annotate_host_ex(*args, display) if ex else lib.whenet_annotate_host(*args)
    assert rc == _lib.OK, lib.whenet_last_error(None)
    for b, (_, rb) in zip(bufs, shapes):
        assert (b[:, rb:] == fill).all(), "pitch padding written"
    return [b[:, :rb] for b, (_, rb) in zip(bufs, shapes)]


FRAME_H, FRAME_W = 97, 131


@pytest.fixture(scope="module")
def painted():
    """The numpy statement's packed picture of the head set, per channel order: computed once."""
    heads = LC.label_heads(FRAME_H, FRAME_W)
    frame = OC.frame_for(FRAME_H, FRAME_W, 31)
    return frame, heads, {order: LC.paint(frame, order, *heads) for order in (OC.BGR, OC.RGB)}


def test_the_head_set_is_what_it_says(painted):
    frame, (rects, valid, ypr), pictures = painted
    flags = [LC.labels(r, *a, valid=v)[2] for r, v, a in zip(rects, valid, ypr)]
    assert flags == [7, 7, 7, 1, 0, 3, 7, 7]
    assert rects[0][0] < 30 and rects[1][1] < 0 and FRAME_W - rects[2][1] <= 20
    bgr, rgb = pictures[OC.BGR], pictures[OC.RGB]
    assert (bgr.reshape(-1, 3) == LC.COLOUR_BGR).all(axis=1).sum() > 300                      # text was painted, in B, G, R
    assert np.array_equal((bgr.reshape(-1, 3) == LC.COLOUR_BGR).all(axis=1), (rgb.reshape(-1, 3) == LC.COLOUR_BGR[::-1]).all(axis=1))
    # paint order: the second overlapping head's rectangle (black) lies over the first one's yaw line
    simple = LC.paint(frame, OC.BGR, rects, valid, ypr, LC.SIMPLE)
    first = LC.paint(frame, OC.BGR, rects[6:7], None, ypr[6:7])
    text_of_first = (first.reshape(-1, 3) == LC.COLOUR_BGR).all(axis=1) & ~(frame.reshape(-1, 3) == LC.COLOUR_BGR).all(axis=1)
    covered = text_of_first & (bgr.reshape(-1, 3) == 0).all(axis=1)
    assert covered.sum() >= 2 and not np.array_equal(simple, bgr)


@pytest.mark.parametrize("fname,fmt", OC.FORMATS)
def test_host_function_equals_numpy_with_labels(painted, fname, fmt):
    frame, heads, pictures = painted
    for order in (OC.BGR, OC.RGB):
        for mi, (mname, matrix) in enumerate(OC.MATRICES):
            if fmt == OC.PACKED and mi > 0:
                continue
            got = host_planes(frame, order, heads, fmt, matrix, LC.FULL, extra=(0, 1, 5)[mi])
            want = OC.planes_of(pictures[order], order, fmt, matrix)
            for p, (g, wnt) in enumerate(zip(got, want)):
                assert g.shape == wnt.shape and g.tobytes() == wnt.tobytes(), (fname, mname, order, p)


def test_host_function_on_small_frames_and_on_the_seam_and_capacity_heads():
    for (h, w, heads) in ((48, 160, LC.seam_heads()), (48, 128, LC.capacity_heads(True)), (48, 128, LC.capacity_heads(False)),
                          (7, 5, (np.asarray([(6, -3, 7, 4)], np.int32), None, np.asarray([(1, 2, 3)], np.float32))),
                          (1, 1, (np.asarray([(0, 0, 1, 1)], np.int32), None, np.asarray([(1, 2, 3)], np.float32)))):
        frame = OC.frame_for(h, w, h + w)
        picture = LC.paint(frame, OC.BGR, *heads)
        for fmt in (OC.PACKED, OC.NV12):
            got = host_planes(frame, OC.BGR, heads, fmt, OC.BT709, LC.FULL)
            for g, wnt in zip(got, OC.planes_of(picture, OC.BGR, fmt, OC.BT709)):
                assert g.tobytes() == wnt.tobytes(), (h, w, fmt)


def test_simple_display_keeps_the_bytes_of_annotate_host(painted):
    frame, heads, _ = painted
    for fmt, matrix in ((OC.PACKED, 0), (OC.NV12, OC.BT709), (OC.I420, OC.JFIF)):
        for order in (OC.BGR, OC.RGB):
            old = host_planes(frame, order, heads, fmt, matrix, None, ex=False)
            new = host_planes(frame, order, heads, fmt, matrix, LC.SIMPLE)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(old, new))
            assert old[0].tobytes() == LC.annotate(frame, order, *heads, fmt, matrix, LC.SIMPLE)[0].tobytes()
    rects, valid, ypr = heads
    a = overlay.annotate_host(frame, rects, *ypr.T, valid=valid)
    assert np.array_equal(a, overlay.annotate_host(frame, rects, *ypr.T, valid=valid, display="simple"))
    assert not np.array_equal(a, overlay.annotate_host(frame, rects, *ypr.T, valid=valid, display="full"))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_a_bad_display_is_refused():
    frame = OC.frame_for(5, 7, 1)
    rects, ypr = np.asarray([(0, 0, 5, 7)], np.int32), np.zeros((1, 3), np.float32)
    out = np.zeros((5, 7, 3), np.uint8)
    s, _ = overlay.surface_of(out, 5, 7)
    lib, P = _lib.load(), _lib._ptr
    for bad in (2, -1, 7):
        assert lib.whenet_annotate_host_ex(P(frame), 5, 7, 1, P(rects), None, P(ypr), 1, C.byref(s), bad) == _lib.EINVAL
        assert b"display" in lib.whenet_last_error(None) and not out.any()
    assert lib.whenet_annotate_host_ex(P(frame), 5, 7, 1, P(rects), None, P(ypr), 1, C.byref(s), 1) == _lib.OK and out.any()
    assert lib.whenet_op_annotate_ex(None, P(frame), 5, 7, 1, P(rects), None, P(ypr), 1, C.byref(s), 1) == _lib.EINVAL       # no handle
    assert lib.whenet_frame_annotate_ex(None, 0, 0, C.byref(s), None, 1) == _lib.EINVAL
    for bad in ("Full", "labels", 1, None, True):
        with pytest.raises(ValueError, match="display"):
            overlay.annotate_host(frame, rects, [0.], [0.], [0.], display=bad)
        with pytest.raises(ValueError, match="display"):
            overlay.annotate(None, frame, rects, [0.], [0.], [0.], display=bad)           # refused before the handle is touched


class _Handle:
    """What FramePipeline needs of a handle, without a device: annotate calls are recorded."""

    def __init__(self):
        self.calls, self.next = [], 0

    def set_option(self, key, value):
        pass

    def _ticket(self, *a, **k):
        self.next += 1
        return self.next

    submit_frame = frame_begin = clip_begin = clip_begin_mixed = _ticket

    def frame_heads(self, ticket, rects):
        pass

    def clip_detect_heads(self, ticket, *a):
        return 4

    def frame_annotate(self, ticket, index, surface, stream=None, display=_lib.DISPLAY_SIMPLE):
        self.calls.append((ticket, index, stream, display))

    def collect(self, ticket, k):
        return np.zeros((k, 3), np.float32), None, None


def test_pipeline_passes_display_on_and_refuses_a_bad_one():
    m = type("M", (), {})()
    m._handle = _Handle()
    fp = FramePipeline(m, depth=2)
    frame, out = OC.frame_for(6, 8, 3), np.zeros((6, 8, 3), np.uint8)
    fp.submit(frame, np.asarray([(1, 1, 5, 6)], np.float32))
    with pytest.raises(ValueError, match="display"):
        fp.annotate(out, display="both")
    assert m._handle.calls == []
    fp.annotate(out, stream=5, display="full")
    fp.collect()
    fp.submit(frame, np.asarray([(1, 1, 5, 6)], np.float32))
    fp.annotate(out)
    fp.collect()
    assert m._handle.calls == [(1, 0, 5, _lib.DISPLAY_FULL), (2, 0, None, _lib.DISPLAY_SIMPLE)]
    fp._detector = type("D", (), {"anchors": np.zeros((6, 2), np.float32), "class_names": ["head"]})()
    fp.begin_clip([frame, frame])
    fp.detect_heads_clip(size=(32, 32), max_boxes=4)
    with pytest.raises(ValueError, match="display"):
        fp.annotate_clip([out, None], display=1)
    fp.annotate_clip([out, np.zeros_like(out)], display="full")
    assert m._handle.calls[2:] == [(3, 0, None, _lib.DISPLAY_FULL), (3, 1, None, _lib.DISPLAY_FULL)]
