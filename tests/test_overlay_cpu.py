"""The pose overlay without a GPU: the segments against the EXECUTED reference (utils.draw_axis under tests/refharness.py, committed
as tests/golden/reference_draw_axis.npz, and reference_draw_axis_lattice.npz for the exact-ratio table of
tests/overlay_lattice_cases.py, where one ulp of a sine moves a pixel), `whenet_annotate_host` against the numpy statement of tests/overlay_cases.py on the case
table, the BGR -> 4:2:0 coefficient rows against their expressions, executed Pillow and the round trip through the ingest's
conversion, and the plumbing: header, exports, every WHENET_EINVAL that needs no device, the ValueErrors of the Python layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import overlay_cases as OC
from tests import overlay_lattice_cases as LC
from tests import refharness
from whenet_hip import _lib, overlay
from whenet_hip.frames import FramePipeline
from whenet_hip.yuv import YUVFrame

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_draw_axis.npz")
GOLDEN_LATTICE = os.path.join(ROOT, "tests", "golden", "reference_draw_axis_lattice.npz")
HEADER = os.path.join(ROOT, "include", "whenet_hip.h")
MAT_NAME = {OC.BT601: "bt601", OC.BT709: "bt709", OC.JFIF: "jfif"}


# ---- 1. segments against executed reference code --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(GOLDEN))


def test_fixture_holds_the_case_set(recorded):
    rects, ypr = OC.reference_heads()
    assert np.array_equal(recorded["rects"], rects) and recorded["ypr"].tobytes() == ypr.tobytes()
    assert len(rects) >= OC.REFERENCE_HEADS + 4 * 9
    # what the reference passes to cv2.line besides the endpoints (utils.py:40-42): B, G, R colours and thickness 2
    assert (recorded["colours"] == np.array([(0, 0, 255), (0, 255, 0), (255, 0, 0)])).all() and (recorded["thickness"] == 2).all()


def test_segments_equal_the_recorded_cv2_line_calls(recorded):
    for i, (rect, a) in enumerate(zip(recorded["rects"], recorded["ypr"])):
        seg, flags = overlay.segments(rect, *a)
        assert flags == 3, i
        assert seg[:4].tolist() == [rect[1], rect[0], rect[3], rect[2]], i
        assert np.array_equal(seg[4:].reshape(3, 4), recorded["lines"][i]), (i, rect, a)
        assert seg.tolist() == OC.segments(rect, *a)[0], i           # (the numpy statement says the same)


def test_every_seeded_coordinate_is_clear_of_an_integer():
    rects, ypr = OC.reference_heads()
    worst, exact = 1.0, 0
    for i in range(OC.REFERENCE_HEADS):
        m = OC.integer_margin(rects[i], *ypr[i])
        if m is None:                                                 # size 0: every coordinate is tdx / tdy exactly
            a = OC.axis_arguments(rects[i], *ypr[i])
            c = OC.axis_coordinates(**a)
            assert c[0::2] == (a["tdx"],) * 3 and c[1::2] == (a["tdy"],) * 3, i
            exact += 1
            continue
        worst = min(worst, m)
        assert m >= 1e-6, (i, m)
    print(f"seeded heads: smallest distance of a rounded coordinate from an integer {worst:.3e}; {exact} heads of size 0 are exact")


@pytest.mark.skipif(not refharness.available(), reason="the reference tree is not present")
def test_live_reference_run_reproduces_the_fixture(recorded):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_overlay_fixture", os.path.join(ROOT, "tests", "golden", "make_overlay_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines, colours, thick = mod.run_reference(recorded["rects"], recorded["ypr"])      # every head: the seeded ones and the designed ones
    assert np.array_equal(lines, recorded["lines"]) and np.array_equal(colours, recorded["colours"])
    assert np.array_equal(thick, recorded["thickness"])


def test_segments_flags_and_range():
    seg, flags = overlay.segments((10, 20, 30, 40), float("nan"), 0, 0)
    assert flags == 1 and seg.tolist() == [20, 10, 40, 30] + [0] * 12
    assert overlay.segments((10, 20, 30, 40), 0, float("inf"), 0)[1] == 1
    with pytest.raises(ValueError, match="-4096..8192"):
        overlay.segments((0, 0, 10, 8193), 0, 0, 0)
    with pytest.raises(ValueError):
        overlay.segments((-4097, 0, 10, 10), 0, 0, 0)
    assert overlay.segments((-4096, -4096, 8192, 8192), 1, 2, 3)[1] == 3
    # size = (x1 - x0) // 2 floors
    assert overlay.segments((0, 10, 4, 7), 0, 0, 0)[0].tolist() == OC.segments((0, 10, 4, 7), 0, 0, 0)[0]


# ---- 1b. the exact-ratio table: where a last bit of a sine decides a pixel (tests/overlay_lattice_cases.py) -----------------------
@pytest.fixture(scope="module")
def lattice():
    return LC.tables()


def test_lattice_table_holds_the_sensitive_heads(lattice):
    count = lambda family: sum(int((T.sensitive & (T.family == family)).sum()) for T in lattice)
    heads = lambda family: sum(int((T.family == family).sum()) for T in lattice)
    print(f"sensitive: lattice {count(LC.LATTICE)} of {heads(LC.LATTICE)}, bin centres {count(LC.BIN)} of {heads(LC.BIN)}, "
          f"controls {count(LC.CONTROL)} of {heads(LC.CONTROL)}; per window {[int(T.sensitive.sum()) for T in lattice]}; "
          f"frames {[(T.h, T.w) for T in lattice]}")
    assert (heads(LC.LATTICE), heads(LC.BIN), heads(LC.CONTROL)) == (25350, 5760, 1812)
    assert count(LC.LATTICE) >= 2900 and count(LC.BIN) >= 90 and count(LC.CONTROL) == 0
    for T in lattice:                                             # every endpoint, moved or not, grown by the reach, is in the frame
        ends = np.concatenate([T.segments[None], T.perturbed]).reshape(-1, 8, 2)
        assert ends.min() >= 0 and ends[..., 0].max() + LC.REACH < T.w and ends[..., 1].max() + LC.REACH < T.h
        assert np.array_equal(T.sensitive, LC.sensitivity(T.rect, T.ypr))
        # one float32 step is far more than one ulp of a sine: the controls are the lattice's neighbours, not the lattice
        assert not T.sensitive[T.family == LC.CONTROL].any()


def test_every_lattice_perturbation_is_visible_in_the_picture(lattice):
    """Every sensitive head, painted alone on its window's frame: at least one of its moved segment sets gives another picture,
    so a kernel whose sine differs there by one ulp fails tests/test_overlay_gpu.py's byte comparison -- with one exception that
    the paint order makes, not the table: where the moved axis lies along an axis painted after it and is the shorter of the two
    (yaw -180, pitch 90, roll -60 on (0, 0, 8, 8): X ends at (1, 4) or (2, 4), Y at (0, 4)), no picture shows its end.  37 of the
    2,998 sensitive heads are of that kind (11, 9, 4, 7, 0, 6 per window); only a head's segments could tell them apart."""
    visible, hidden = 0, [0] * len(lattice)
    for T in lattice:
        frame = T.frame()
        for n, i in enumerate(np.flatnonzero(T.sensitive)):
            base = LC.paint_segments(frame, T.segments[i])
            if n % 50 == 0:                                          # the boxed raster is the whole-frame statement
                assert np.array_equal(base, OC.paint(frame, OC.BGR, [T.rect], None, [T.ypr[i]])), T.describe(i)
            moved = np.unique(T.perturbed[:, i][(T.perturbed[:, i] != T.segments[i]).any(axis=1)], axis=0)
            assert len(moved) >= 1
            shows = [not np.array_equal(LC.paint_segments(frame, m), base) for m in moved]
            covered = [LC.hidden_by_a_later_axis(T.segments[i], m) for m in moved]
            assert shows == [not c for c in covered], (T.describe(i), moved[:, 4:].tolist())      # hidden exactly where the rule says
            visible += any(shows)
            hidden[T.index] += not any(shows)
    print(f"sensitive heads with a visible perturbation: {visible}; hidden behind a later axis, per window: {hidden}")
    assert visible >= 2900 and sum(hidden) <= 40


def test_host_segments_equal_numpy_on_the_lattice_table(lattice):
    for T in lattice:
        for i in range(len(T.ypr)):
            seg, flags = overlay.segments(T.rect, *T.ypr[i])
            assert flags == 3 and seg.tolist() == T.segments[i].tolist(), T.describe(i)
            if T.sensitive[i] or i % 7 == 0:                          # (the vectorised statement is the scalar one)
                assert OC.segments(T.rect, *T.ypr[i])[0] == seg.tolist(), T.describe(i)


@pytest.fixture(scope="module")
def recorded_lattice():
    return dict(np.load(GOLDEN_LATTICE))


def _overlay_fixture_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_overlay_fixture", os.path.join(ROOT, "tests", "golden", "make_overlay_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_lattice_segments_equal_the_recorded_cv2_line_calls(lattice, recorded_lattice):
    index, lines = recorded_lattice["index"], recorded_lattice["lines"]
    assert lines.dtype == np.int16 and lines.shape == (len(index), 3, 4)
    want = np.concatenate([T.index * 65536 + T.recorded() for T in lattice])
    assert np.array_equal(index, want)                                # every sensitive head and every 7th other one, in table order
    assert len(index) >= sum(int(T.sensitive.sum()) for T in lattice) + 4000
    for code, line in zip(index, lines):
        T, i = lattice[code >> 16], code & 0xFFFF
        seg, _ = overlay.segments(T.rect, *T.ypr[i])
        assert np.array_equal(seg[4:].reshape(3, 4), line), T.describe(i)


@pytest.mark.skipif(not refharness.available(), reason="the reference tree is not present")
def test_live_reference_run_reproduces_the_lattice_fixture(recorded_lattice):
    index, lines = _overlay_fixture_module().run_reference_lattice()
    assert np.array_equal(index, recorded_lattice["index"]) and np.array_equal(lines, recorded_lattice["lines"])
    assert lines.dtype == recorded_lattice["lines"].dtype


# ---- 2. the host function against the numpy statement ----------------------------------------------------------------------
def host_planes(frame, order, heads, fmt, matrix, extra=0, fill=0x5A):
    """whenet_annotate_host into planes of pitch = row bytes + extra -> (the rows as tight arrays, the raw buffers)."""
    h, w = frame.shape[:2]
    rects, valid, ypr = heads
    shapes = OC.plane_shapes(fmt, h, w)
    bufs = [np.full((rows, rb + extra), fill, np.uint8) for rows, rb in shapes]
    s = _lib.SurfaceC()
    for i, b in enumerate(bufs):
        s.plane[i], s.pitch[i] = b.ctypes.data, b.shape[1]
    s.format, s.matrix, s.on_device = fmt, matrix, 0
    _lib.annotate_host(frame, rects, valid, ypr, s, bgr=order == OC.BGR)
    return [b[:, :rb] for b, (_, rb) in zip(bufs, shapes)], bufs


@pytest.mark.parametrize("h,w", OC.SIZES)
def test_host_function_equals_numpy_on_the_case_table(h, w):
    checked = 0
    for ci, (name, heads) in enumerate(OC.heads_cases(h, w).items()):
        frame = OC.frame_for(h, w, 100 + ci)
        order = (OC.BGR, OC.RGB)[ci & 1]
        painted = None
        for fi, (fname, fmt) in enumerate(OC.FORMATS):
            for mi, (mname, matrix) in enumerate(OC.MATRICES):
                if fmt == OC.PACKED and mi > 0:
                    continue
                if (h, w) == (96, 128) and name == "sixty_four" and mi != ci % 3 and fmt != OC.PACKED:
                    continue                                      # (the slowest numpy case: one matrix per format)
                extra = (0, 1, 5, 64)[(ci + fi + mi) & 3]
                got, bufs = host_planes(frame, order, heads, fmt, matrix, extra)
                if painted is None:
                    painted = OC.paint(frame, order, *heads)
                want = OC.planes_of(painted, order, fmt, matrix)
                for p, (g, wnt, b) in enumerate(zip(got, want, bufs)):
                    assert g.tobytes() == wnt.tobytes(), (name, fname, mname, order, p)
                    assert (b[:, g.shape[1]:] == 0x5A).all(), (name, fname, "pitch padding written")
                checked += 1
    assert checked >= 60


def test_both_channel_orders_paint_the_same_colours():
    h, w = 33, 19
    heads = OC.heads_cases(h, w)["mid_pose"]
    frame = OC.frame_for(h, w, 5)
    bgr = overlay.annotate_host(frame, heads[0], *heads[2].T, bgr=True)
    rgb = overlay.annotate_host(frame[..., ::-1], heads[0], *heads[2].T, bgr=False)
    assert np.array_equal(bgr, rgb[..., ::-1])
    assert (bgr.reshape(-1, 3) == (0, 0, 255)).all(axis=1).any()      # the X axis is red: B, G, R = 0, 0, 255
    for mname in MAT_NAME.values():                                   # and the planes do not depend on the order either
        a = overlay.annotate_host(frame, heads[0], *heads[2].T, format="i420", matrix=mname, bgr=True)
        b = overlay.annotate_host(frame[..., ::-1], heads[0], *heads[2].T, format="i420", matrix=mname, bgr=False)
        assert all(np.array_equal(p, q) for p, q in zip(a.planes, b.planes))


def test_no_heads_is_a_copy_and_the_source_is_untouched():
    frame = OC.frame_for(33, 19, 9)
    keep = frame.copy()
    none = (np.zeros((0, 4), np.int32), None, np.zeros((0, 3), np.float32))
    for got, want in zip(host_planes(frame, OC.RGB, none, OC.NV12, OC.JFIF)[0], OC.annotate(frame, OC.RGB, *none, OC.NV12, OC.JFIF)):
        assert got.tobytes() == want.tobytes()                    # no heads: a pure conversion
    assert np.array_equal(overlay.annotate_host(frame, np.zeros((0, 4), np.int32), [], [], []), frame)
    heads = OC.heads_cases(33, 19)["sixty_four"]
    overlay.annotate_host(frame, heads[0], *heads[2].T)
    assert np.array_equal(frame, keep)


def test_raster_rule_on_designed_segments():
    """The rule itself, on segments a window's axes cannot all express: horizontal, vertical, 45 degrees, steep, P = Q, endpoints
    outside and wholly outside -- the numpy mask against a brute-force statement in exact rationals."""
    from fractions import Fraction

    def brute(h, w, px, py, qx, qy):
        out = np.zeros((h, w), bool)
        dx, dy = qx - px, qy - py
        L2 = dx * dx + dy * dy
        for y in range(h):
            for x in range(w):
                if L2 == 0:
                    d2 = Fraction((x - px) ** 2 + (y - py) ** 2)
                else:
                    t = min(max(Fraction((x - px) * dx + (y - py) * dy, L2), 0), 1)
                    d2 = (x - px - t * dx) ** 2 + (y - py - t * dy) ** 2
                out[y, x] = d2 <= 1
        return out

    for seg in ((2, 3, 15, 3), (4, 1, 4, 11), (1, 1, 10, 10), (3, 0, 5, 12), (6, 6, 6, 6), (-5, -3, 30, 20), (-9, 4, -2, 8),
                (16, 5, 2, 9), (0, 0, 17, 12), (17, 0, 0, 12)):
        assert np.array_equal(OC.hit_mask(13, 18, *seg), brute(13, 18, *seg)), seg


# ---- 3. the coefficient rows ---------------------------------------------------------------------------------------------------
def test_coefficient_rows_equal_their_expressions_and_the_header():
    text = open(HEADER).read()
    m = re.search(r"#define WHENET_BGR2YUV_COEFFS ((?:.*\\\n)*.*)\n", text)
    rows = [tuple(int(v) for v in re.findall(r"-?\d+", r)) for r in re.findall(r"\{([^{}]+)\}", m.group(1))]
    assert len(rows) == 3
    for matrix in (OC.BT601, OC.BT709, OC.JFIF):
        assert rows[matrix] == OC.COEFFS[matrix] == OC.coeff_expressions(matrix)
    assert int(re.search(r"#define WHENET_SURF_PACKED (\d+)", text).group(1)) == _lib.SURF_PACKED == OC.PACKED


@pytest.fixture(scope="module")
def all_triples():
    """uint8 [8192, 8192, 3] R, G, B: every one of the 2^24 triples as a flat 2 x 2 block; block (by, bx) holds triple by * 4096 + bx."""
    idx = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    small = np.stack([(idx >> 16).astype(np.uint8), ((idx >> 8) & 255).astype(np.uint8), (idx & 255).astype(np.uint8)], axis=2)
    return small, np.ascontiguousarray(small.repeat(2, axis=0).repeat(2, axis=1))


def forward(frame_rgb, mname):
    return overlay.annotate_host(frame_rgb, np.zeros((0, 4), np.int32), [], [], [], format="i420", matrix=mname, bgr=False)


def test_jfif_row_against_executed_pillow_on_all_triples(all_triples):
    from PIL import Image
    small, big = all_triples
    out = forward(big, "jfif")
    ours = np.stack([out.planes[0][::2, ::2], out.planes[1], out.planes[2]], axis=2)
    assert np.array_equal(out.planes[0][::2, ::2], out.planes[0][1::2, 1::2])
    pil = np.asarray(Image.fromarray(small, "RGB").convert("YCbCr"))
    diff = np.abs(ours.astype(np.int16) - pil.astype(np.int16))
    print(f"JFIF forward against Pillow over 2^24 triples: max |delta| = {int(diff.max())}, equal {float((diff == 0).mean()):.1%}, "
          f"per channel max {[int(diff[..., c].max()) for c in range(3)]}")
    assert int(diff.max()) <= 1


# measured here over all 2^24 flat colours: the worst |level difference| of forward + whenet_yuv_to_bgr_host
ROUND_TRIP_WORST = {"bt601": 2, "bt709": 2, "jfif": 1}


@pytest.mark.parametrize("mname", ["bt601", "bt709", "jfif"])
def test_round_trip_through_the_ingest_conversion(all_triples, mname):
    small, big = all_triples
    back = forward(big, mname).to_bgr()[::2, ::2, ::-1]
    diff = np.abs(back.astype(np.int16) - small.astype(np.int16))
    print(f"round trip {mname}: worst |delta| = {int(diff.max())}, per channel {[int(diff[..., c].max()) for c in range(3)]}, "
          f"equal {float((diff == 0).all(axis=2).mean()):.1%}")
    assert int(diff.max()) == ROUND_TRIP_WORST[mname]


# ---- 4. plumbing ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_overlay_and_the_library_exports_it():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in ("whenet_overlay_segments", "whenet_annotate_host", "whenet_op_annotate", "whenet_frame_annotate"):
        assert re.search(r"WHENET_API int " + name + r"\(", text), name
        assert name in _lib.EXPORTS and getattr(lib, name)
    assert "#define WHENET_ABI_VERSION 6" in text and _lib.ABI_VERSION == 6
    assert "OpenCV has never run" in text                      # the raster rule says whose it is
    assert C.sizeof(_lib.SurfaceC) == 3 * C.sizeof(C.c_void_p) + 6 * C.sizeof(C.c_int)


def _surface(h, w, fmt=OC.PACKED, matrix=0):
    bufs = [np.zeros((rows, rb), np.uint8) for rows, rb in OC.plane_shapes(fmt, h, w)]
    s = _lib.SurfaceC()
    for i, b in enumerate(bufs):
        s.plane[i], s.pitch[i] = b.ctypes.data, b.shape[1]
    s.format, s.matrix, s.on_device = fmt, matrix, 0
    return s, bufs


SPOILS = [
    ("NULL", lambda s: s.plane.__setitem__(0, None), OC.PACKED),
    ("NULL", lambda s: s.plane.__setitem__(2, None), OC.I420),
    ("pitch", lambda s: s.pitch.__setitem__(0, 3 * 7 - 1), OC.PACKED),
    ("pitch", lambda s: s.pitch.__setitem__(1, 7), OC.NV12),
    ("format", lambda s: setattr(s, "format", 3), OC.PACKED),
    ("format", lambda s: setattr(s, "format", -1), OC.NV12),
    ("matrix", lambda s: setattr(s, "matrix", 3), OC.NV12),
    ("matrix", lambda s: setattr(s, "matrix", -1), OC.I420),
    ("host memory", lambda s: setattr(s, "on_device", 1), OC.PACKED),
]


@pytest.mark.parametrize("text,spoil,fmt", SPOILS)
def test_bad_surface_is_einval_and_the_next_call_succeeds(text, spoil, fmt):
    frame = OC.frame_for(5, 7, 1)
    heads = (np.asarray([(0, 0, 5, 7)], np.int32), None, np.zeros((1, 3), np.float32))
    s, bufs = _surface(5, 7, fmt)
    spoil(s)
    with pytest.raises(ValueError, match=text):
        _lib.annotate_host(frame, *heads, s)
    assert all((b == 0).all() for b in bufs)                   # refused before a byte is written
    s, bufs = _surface(5, 7, fmt)
    _lib.annotate_host(frame, *heads, s)
    assert any(b.any() for b in bufs)


def test_bad_arguments_are_einval():
    lib = _lib.load()
    frame = OC.frame_for(5, 7, 1)
    rects = np.asarray([(0, 0, 5, 7)], np.int32)
    ypr = np.zeros((1, 3), np.float32)
    s, _ = _surface(5, 7)
    P = _lib._ptr
    call = lib.whenet_annotate_host
    assert call(P(frame), 5, 7, 1, P(rects), None, P(ypr), 1, C.byref(s)) == _lib.OK
    assert call(None, 5, 7, 1, P(rects), None, P(ypr), 1, C.byref(s)) == _lib.EINVAL
    assert call(P(frame), 5, 7, 1, P(rects), None, P(ypr), 1, None) == _lib.EINVAL
    assert call(P(frame), 5, 7, 1, None, None, P(ypr), 1, C.byref(s)) == _lib.EINVAL
    assert call(P(frame), 5, 7, 1, P(rects), None, None, 1, C.byref(s)) == _lib.EINVAL
    assert call(P(frame), 5, 7, 2, P(rects), None, P(ypr), 1, C.byref(s)) == _lib.EINVAL           # channel order
    assert call(P(frame), 0, 7, 1, P(rects), None, P(ypr), 1, C.byref(s)) == _lib.EINVAL
    assert call(P(frame), 5, 8193, 1, P(rects), None, P(ypr), 1, C.byref(s)) == _lib.EINVAL
    assert call(P(frame), 5, 7, 1, P(rects), None, P(ypr), -1, C.byref(s)) == _lib.EINVAL
    assert call(P(frame), 5, 7, 1, P(rects), None, P(ypr), 257, C.byref(s)) == _lib.EINVAL
    far = np.asarray([(0, 0, 5, 9000)], np.int32)
    assert call(P(frame), 5, 7, 1, P(far), None, P(ypr), 1, C.byref(s)) == _lib.EINVAL               # a valid head out of range
    assert b"-4096..8192" in lib.whenet_last_error(None)
    zero = np.zeros(1, np.int32)
    assert call(P(frame), 5, 7, 1, P(far), P(zero), P(ypr), 1, C.byref(s)) == _lib.OK                # ... an invalid one is never read
    assert call(P(frame), 5, 7, 1, None, None, None, 0, C.byref(s)) == _lib.OK                       # no heads: nothing else needed
    seg = np.zeros(16, np.int32)
    assert lib.whenet_overlay_segments(None, 0, 0, 0, P(seg), None) == _lib.EINVAL
    assert lib.whenet_overlay_segments(P(rects), 0, 0, 0, None, None) == _lib.EINVAL
    assert lib.whenet_overlay_segments(P(rects), 0, 0, 0, P(seg), None) == _lib.OK
    # the entry points that need a handle refuse a NULL one
    assert lib.whenet_op_annotate(None, P(frame), 5, 7, 1, P(rects), None, P(ypr), 1, C.byref(s)) == _lib.EINVAL
    assert lib.whenet_frame_annotate(None, 0, 0, C.byref(s), None) == _lib.EINVAL


def test_python_destinations_are_checked_never_copied():
    frame = OC.frame_for(6, 8, 2)
    args = (frame, np.zeros((0, 4), np.int32), [], [], [])
    ro = np.zeros((6, 8, 3), np.uint8)
    ro.flags.writeable = False
    for bad in (ro, np.zeros((6, 8, 3), np.float32), np.zeros((3, 6, 8), np.uint8), np.zeros((6, 9, 3), np.uint8),
                np.zeros((6, 8, 6), np.uint8)[:, :, ::2], np.zeros((6, 8), np.uint8), [[0]], "surface"):
        with pytest.raises(ValueError):
            overlay.annotate_host(*args, out=bad)
    pitched = np.zeros((6, 40), np.uint8)
    view = np.lib.stride_tricks.as_strided(pitched, (6, 8, 3), (40, 3, 1))
    assert overlay.annotate_host(*args, out=view) is view and np.array_equal(view, frame) and not pitched[:, 24:].any()
    with pytest.raises(ValueError, match="unknown format"):
        overlay.annotate_host(*args, format="yuy2")
    with pytest.raises(ValueError, match="unknown matrix"):
        overlay.annotate_host(*args, format="nv12", matrix="bt2020")
    with pytest.raises(ValueError, match="one length"):
        overlay.annotate_host(frame, [(0, 0, 6, 8)], [1.0], [1.0, 2.0], [1.0])
    with pytest.raises(ValueError, match="1 windows"):
        overlay.annotate_host(frame, [(0, 0, 6, 8)], [1.0, 2.0], [1.0, 2.0], [1.0, 2.0])


def test_yuvframe_writable():
    y, uv = np.zeros((6, 8), np.uint8), np.zeros((3, 8), np.uint8)
    assert YUVFrame.nv12(y, uv).writable and YUVFrame.nv12(y, uv.reshape(3, 4, 2)).writable
    ro = np.zeros((3, 8), np.uint8)
    ro.flags.writeable = False
    assert not YUVFrame.nv12(y, ro).writable
    assert not YUVFrame.from_buffer(bytes(6 * 8 * 3 // 2), 6, 8, "i420").writable
    assert YUVFrame.from_buffer(bytearray(6 * 8 * 3 // 2), 6, 8, "i420").writable
    buf = np.zeros(16 * 9, np.uint8)
    f = YUVFrame.from_buffer(buf, 6, 8, "nv12", pitch=16)
    assert f.writable and f.pitches == (16, 16)
    overlay.annotate_host(np.full((6, 8, 3), 255, np.uint8), np.zeros((0, 4), np.int32), [], [], [], out=f)
    assert (buf.reshape(9, 16)[:6, :8] == 235).all() and not buf.reshape(9, 16)[:, 8:].any()
    with pytest.raises(ValueError, match="read-only"):
        overlay.annotate_host(np.zeros((6, 8, 3), np.uint8), np.zeros((0, 4), np.int32), [], [], [], out=YUVFrame.nv12(y, ro))
    with pytest.raises(ValueError, match="6 x 8"):
        overlay.annotate_host(np.zeros((4, 8, 3), np.uint8), np.zeros((0, 4), np.int32), [], [], [], out=YUVFrame.nv12(y, uv))


class _Handle:
    """What FramePipeline needs of a handle, without a device: tickets are handed out, annotate calls are recorded."""

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

    def frame_annotate(self, ticket, index, surface, stream=None):
        self.calls.append((ticket, index, surface.format, surface.on_device, surface.pitch[0], stream))

    def collect(self, ticket, k):
        return np.zeros((k, 3), np.float32), None, None


class _Model:
    def __init__(self):
        self._handle = _Handle()


def test_pipeline_annotate_checks_its_destination_before_the_library_sees_it():
    m = _Model()
    fp = FramePipeline(m, depth=2)
    frame = OC.frame_for(6, 8, 3)
    with pytest.raises(ValueError, match="no frame"):
        fp.annotate(np.zeros((6, 8, 3), np.uint8))
    fp.submit(frame, np.asarray([(1, 1, 5, 6)], np.float32))
    ro = np.zeros((6, 8, 3), np.uint8)
    ro.flags.writeable = False
    for bad in (ro, np.zeros((6, 8, 3), np.float32), np.zeros((3, 6, 8), np.uint8), np.zeros((8, 6, 3), np.uint8), None,
                YUVFrame.nv12(np.zeros((4, 8), np.uint8), np.zeros((2, 8), np.uint8))):
        with pytest.raises(ValueError):
            fp.annotate(bad)
    assert m._handle.calls == []
    out = np.zeros((6, 8, 3), np.uint8)
    fp.annotate(out, stream=5)
    assert m._handle.calls == [(1, 0, _lib.SURF_PACKED, 0, 24, 5)]
    with pytest.raises(ValueError, match="already"):
        fp.annotate(out)
    fp.collect()
    fp.begin(frame)
    fp.heads(np.zeros((0, 4), np.float32))
    fp.begin(frame)                                               # another frame begun since: `the frame submitted last` is ambiguous
    with pytest.raises(ValueError, match="begun since"):
        fp.annotate(out)
    fp.heads(np.zeros((0, 4), np.float32))
    fp.collect()
    fp.collect()
    # the resident form and a YUV destination
    fp.begin(frame)
    with pytest.raises(ValueError, match="no frame"):
        fp.annotate(out)                                          # its heads are not enqueued yet
    fp.heads(np.zeros((0, 4), np.float32))
    fp.annotate(YUVFrame.i420(np.zeros((6, 8), np.uint8), np.zeros((3, 4), np.uint8), np.zeros((3, 4), np.uint8), "bt709"))
    assert m._handle.calls[-1][:4] == (4, 0, _lib.YUV_I420, 0)
    with pytest.raises(ValueError, match="annotate_clip"):
        fp.annotate_clip([out])
    fp.collect()


def test_pipeline_annotate_clip_takes_one_destination_per_frame():
    m = _Model()
    fp = FramePipeline(m, depth=2)
    fp._detector = type("D", (), {"anchors": np.zeros((6, 2), np.float32), "class_names": ["head"]})()
    fp.begin_clip_mixed([OC.frame_for(6, 8, 1), OC.frame_for(4, 10, 2), OC.frame_for(6, 8, 3)])
    with pytest.raises(ValueError, match="no clip"):
        fp.annotate_clip([None] * 3)
    fp.detect_heads_clip(size=(32, 32), max_boxes=4)
    with pytest.raises(ValueError, match="annotate_clip"):
        fp.annotate(np.zeros((6, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="3 frames"):
        fp.annotate_clip([np.zeros((6, 8, 3), np.uint8)])
    with pytest.raises(ValueError, match=r"outs\[1\]"):
        fp.annotate_clip([np.zeros((6, 8, 3), np.uint8), np.zeros((6, 8, 3), np.uint8), None])
    assert m._handle.calls == []                                  # every destination is checked before the first is enqueued
    fp.annotate_clip([np.zeros((6, 8, 3), np.uint8), None, np.zeros((6, 8, 3), np.uint8)])
    assert [c[:2] for c in m._handle.calls] == [(1, 0), (1, 2)]
