"""The pose overlay on the GPU (csrc/overlay.hip; Engine::op_annotate / frame_annotate of csrc/engine_post.cpp;
FramePipeline.annotate / annotate_clip).  There is no tolerance anywhere: the kernels return the bytes of `whenet_annotate_host`,
which tests/test_overlay_cpu.py holds to the numpy statement -- also at the exact-ratio angles of tests/overlay_lattice_cases.py,
where a last bit of the device's sines would move a pixel; a device destination keeps every byte outside its rows; the collect
calls return what they return without an annotate."""
import json
import os

import numpy as np
import pytest
import torch

from tests import detector_cases as DC
from tests import overlay_cases as OC
from tests import overlay_lattice_cases as LC
from tests.test_clip_gpu import assert_same, kwargs
from tests.test_yuv_gpu import seeded_model
from whenet_hip import _lib, overlay
from whenet_hip.frames import FramePipeline
from whenet_hip.yuv import YUVFrame

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
GAP = 0xC3                 # what a device destination holds outside the bytes of its rows
FMT_NAME = {OC.PACKED: "bgr", OC.NV12: "nv12", OC.I420: "i420"}
MAT_NAME = {OC.BT601: "bt601", OC.BT709: "bt709", OC.JFIF: "jfif"}


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def model():
    m = seeded_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def kw():
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        return kwargs(json.load(f)["detect"], "tiny", score=0.02)       # a low threshold: the seeded detector then fires on small frames


@pytest.fixture(scope="module")
def frames():
    """Small BGR pictures cut from the committed sample frames: 97 x 131, 128 x 160 and 75 x 101."""
    f0, f1 = DC.sample_frame(0), DC.sample_frame(1)
    return dict(W=np.ascontiguousarray(f1[60:157, 200:331]), A=np.ascontiguousarray(f0[40:168, 180:340]),
                B=np.ascontiguousarray(f1[100:175, 300:401]))


def planes_of(out):
    """The rows of a host destination as tight arrays."""
    if isinstance(out, YUVFrame):
        return [np.ascontiguousarray(p) for p in out.planes]
    return [np.ascontiguousarray(out).reshape(out.shape[0], -1)]


def host_statement(frame, rects, ypr, fmt, matrix, valid=None, bgr=True):
    ypr = np.asarray(ypr, np.float32).reshape(-1, 3)
    out = overlay.annotate_host(frame, rects, ypr[:, 0], ypr[:, 1], ypr[:, 2], format=FMT_NAME[fmt], matrix=MAT_NAME[matrix], valid=valid,
                                bgr=bgr)
    return planes_of(out)


# ---- 5. the kernels alone are the host statement ---------------------------------------------------------------------------------
def op_equals_host(post, frame, order, heads, fmt, matrix, tag):
    rects, valid, ypr = heads
    h, w = frame.shape[:2]
    got = overlay.annotate(post, frame, rects, ypr[:, 0], ypr[:, 1], ypr[:, 2], format=FMT_NAME[fmt], matrix=MAT_NAME[matrix], valid=valid,
                           bgr=order == OC.BGR)
    want = host_statement(frame, rects, ypr, fmt, matrix, valid, bgr=order == OC.BGR)
    for p, (g, wnt) in enumerate(zip(planes_of(got), want)):
        assert g.shape == wnt.shape and g.tobytes() == wnt.tobytes(), (tag, h, w, FMT_NAME[fmt], MAT_NAME[matrix], order, p)


@pytest.mark.parametrize("h,w", OC.SIZES)
def test_op_annotate_equals_the_host_function_on_the_case_table(post, h, w):
    n = 0
    for ci, (name, heads) in enumerate(OC.heads_cases(h, w).items()):
        frame = OC.frame_for(h, w, 100 + ci)
        for fi, (_, fmt) in enumerate(OC.FORMATS):
            for order in (OC.BGR, OC.RGB):
                op_equals_host(post, frame, order, heads, fmt, (ci + fi + order) % 3, name)
                n += 1
    assert n >= 100


def test_op_annotate_on_tiles_heads_and_256_heads(post):
    spans = {"one_tile": 1, "four_tiles": 4}
    for i, (name, h, w, heads) in enumerate(OC.gpu_extra_cases()):
        frame = OC.frame_for(h, w, 7 + i)
        if name in spans:                                          # the cases are what their names say
            assert len(OC.tiles_touched(h, w, heads)) == spans[name], (name, OC.tiles_touched(h, w, heads))
        for fi, (_, fmt) in enumerate(OC.FORMATS):
            op_equals_host(post, frame, OC.BGR, heads, fmt, (i + fi) % 3, name)
    # the source frame's address is whatever the allocator gives; an odd width makes every row start unaligned
    h, w = 37, 131
    op_equals_host(post, OC.frame_for(h, w, 1), OC.RGB, OC.heads_cases(h, w)["sixty_four"], OC.NV12, OC.BT709, "odd_width")


def test_op_annotate_refuses_what_the_host_function_refuses(post):
    frame = OC.frame_for(5, 7, 1)
    out = np.zeros((5, 7, 3), np.uint8)
    with pytest.raises(ValueError, match="-4096..8192"):
        overlay.annotate(post, frame, [(0, 0, 5, 9000)], [0.], [0.], [0.], out=out)
    s, _ = overlay.surface_of(out, 5, 7)
    s.on_device = 1
    with pytest.raises(ValueError, match="host memory"):
        post.op_annotate(frame, np.zeros((0, 4), np.int32), None, np.zeros((0, 3), np.float32), s)
    t = torch.zeros((5, 7, 3), dtype=torch.uint8, device=DEV)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = t.data_ptr(), 21, _lib.SURF_PACKED, 0
    with pytest.raises(ValueError, match="device memory"):
        post.op_annotate(frame, np.zeros((0, 4), np.int32), None, np.zeros((0, 3), np.float32), s)
    assert not out.any() and not t.any().item()
    assert np.array_equal(overlay.annotate(post, frame, np.zeros((0, 4), np.int32), [], [], [], out=out), frame)      # the handle is usable


# ---- 5b. the exact-ratio table: the plan kernel's sines against the host's (tests/overlay_lattice_cases.py) ---------------------------
CALL_HEADS = 256           # the most heads a call takes


def lattice_differences(post, T, rows, batch, fmt=OC.PACKED, display="simple"):
    """The heads `rows` of window table T through op_annotate in calls of `batch` heads -> the first row of every call whose bytes
    are not those of annotate_host."""
    frame, bad = T.frame(), []
    got, want = overlay.new_output(T.h, T.w, FMT_NAME[fmt]), overlay.new_output(T.h, T.w, FMT_NAME[fmt])
    for at in range(0, len(rows), batch):
        r = rows[at:at + batch]
        args = (frame, T.rects[r], T.ypr[r, 0], T.ypr[r, 1], T.ypr[r, 2])
        overlay.annotate(post, *args, out=got, display=display)
        overlay.annotate_host(*args, out=want, display=display)
        if any(g.tobytes() != w.tobytes() for g, w in zip(planes_of(got), planes_of(want))):
            bad.append(int(r[0]))
    return bad


def explain(T, i, post):
    """A sensitive head whose picture differs: which one-ulp moves of a sine reproduce the device's picture, and by how many pixels."""
    got = overlay.annotate(post, T.frame(), T.rects[i:i + 1], *T.ypr[i:i + 1].T)
    moves = sorted({tuple(m) for m in T.perturbed[:, i].tolist() if np.array_equal(LC.paint_segments(T.frame(), m), got)})
    shift = [int(np.abs(np.asarray(m) - T.segments[i]).max()) for m in moves]
    return f"{T.describe(i)}; the device's picture is that of {[list(m[4:]) for m in moves]} (largest endpoint move {shift} px)"


@pytest.mark.parametrize("window", range(len(LC.WINDOWS)))
def test_every_sensitive_head_alone_equals_the_host_function(post, window):
    """One head per call, so nothing overpaints a moved endpoint and a failure names its head."""
    T = LC.table(window)
    rows = np.flatnonzero(T.sensitive)
    assert len(rows) >= 14 and T.h <= 352 and T.w <= 502
    bad = lattice_differences(post, T, rows, 1)
    assert not bad, (f"{len(bad)} of {len(rows)} sensitive heads differ between the kernels and whenet_annotate_host",
                     [explain(T, i, post) for i in bad[:8]])


@pytest.mark.parametrize("window", range(len(LC.WINDOWS)))
def test_the_whole_lattice_table_in_calls_of_256_heads(post, window):
    """Lattice, bin centres and controls, 256 co-centred heads per call: the draw kernel's list at its longest, both displays."""
    T = LC.table(window)
    rows = np.arange(len(T.ypr))
    for display in ("simple", "full"):
        bad = lattice_differences(post, T, rows, CALL_HEADS, display=display)
        assert not bad, (display, f"{len(bad)} calls differ; they begin at", [T.describe(i) for i in bad[:8]])


def test_the_largest_window_into_an_nv12_destination(post):
    T = max(LC.tables(), key=lambda t: t.h * t.w)
    assert T.rect == (100, 200, 300, 500)
    rows = np.flatnonzero(T.sensitive)
    bad = lattice_differences(post, T, rows, CALL_HEADS, fmt=OC.NV12)  # the 4:2:0 leg sees the same endpoints
    assert not bad, [T.describe(i) for i in bad[:8]]


# ---- 6. device destinations ---------------------------------------------------------------------------------------------------------
class DeviceSurface:
    """A destination in ONE device allocation filled with GAP: a guard band, then every plane at its pitch (plane 0 starts
    64 + base bytes in, the others wherever the odd gaps put them), then a guard band."""

    def __init__(self, h, w, fmt, matrix=OC.BT601, extra=0, base=0):
        self.shapes = OC.plane_shapes(fmt, h, w)
        self.pitches = [rb + extra for _, rb in self.shapes]
        self.offs, off = [], 64 + base
        for (rows, rb), p in zip(self.shapes, self.pitches):
            self.offs.append(off)
            off += rows * p + 33
        self.dev = torch.full((off + 64,), GAP, dtype=torch.uint8, device=DEV)
        assert self.dev.data_ptr() % 16 == 0
        views = [torch.as_strided(self.dev, (rows, rb), (p, 1), storage_offset=o) for (rows, rb), p, o in zip(self.shapes, self.pitches, self.offs)]
        if fmt == OC.PACKED:
            self.out = torch.as_strided(self.dev, (h, w, 3), (self.pitches[0], 3, 1), storage_offset=self.offs[0])
        elif fmt == OC.NV12:
            self.out = YUVFrame.nv12(views[0], views[1], matrix=MAT_NAME[matrix])
        else:
            self.out = YUVFrame.i420(*views, matrix=MAT_NAME[matrix])

    def check(self, want, tag=None):
        """The rows hold `want`; every other byte of the allocation still holds GAP."""
        host = self.dev.cpu().numpy()
        outside = np.ones(host.size, bool)
        for p, ((rows, rb), pitch, o, wnt) in enumerate(zip(self.shapes, self.pitches, self.offs, want)):
            got = np.lib.stride_tricks.as_strided(host[o:], (rows, rb), (pitch, 1))
            assert got.tobytes() == wnt.tobytes(), (tag, "plane", p)
            np.lib.stride_tricks.as_strided(outside[o:], (rows, rb), (pitch, 1))[...] = False
        assert (host[outside] == GAP).all(), (tag, "a byte outside the rows was written")


BOXES = {(33, 19): [(4, 3, 20, 15), (10, 2, 30, 12)], (34, 20): [(4, 3, 20, 15), (12, 6, 30, 18)]}


@pytest.mark.parametrize("fname,fmt", OC.FORMATS)
def test_device_destination_keeps_every_byte_outside_its_rows(model, fname, fmt):
    with FramePipeline(model, depth=1) as fp:
        for (h, w), boxes in BOXES.items():
            frame = OC.frame_for(h, w, h)
            for base in range(4):
                for ei, extra in enumerate((0, 1, 5, 64)):
                    matrix = (base + ei) % 3
                    s = DeviceSurface(h, w, fmt, matrix, extra, base)
                    fp.begin(frame)
                    fp.heads(np.asarray(boxes, np.float32))
                    fp.annotate(s.out)
                    rects, yaw, pitch, roll = fp.collect()
                    assert len(rects) == 2
                    s.check(host_statement(frame, rects, np.stack([yaw, pitch, roll], 1), fmt, matrix), (h, w, fname, base, extra))


# ---- 7. the pipeline ---------------------------------------------------------------------------------------------------------------
def ypr_of(res):
    return np.stack([res[1], res[2], res[3]], axis=1)


def test_every_frame_form_with_host_and_device_destinations(model, kw, frames):
    heads_painted = 0
    with FramePipeline(model, depth=1) as fp:
        for i, (key, frame) in enumerate(frames.items()):
            h, w = frame.shape[:2]
            boxes = np.asarray([(h // 4, w // 4, h // 2, w // 2), (h // 3, w // 2, h - 5, w - 7)], np.float32)
            forms = {
                "detect_heads": lambda: (fp.begin(frame), fp.detect_heads(**kw)),
                "heads": lambda: (fp.begin(frame), fp.heads(boxes)),
                "submit": lambda: fp.submit(frame, boxes),
                # heads([]) enqueues nothing, so it does not order the engine's stream behind the frame's upload on the copy stream:
                # Engine::frame_annotate itself waits for the slot's `copied` event in front of its kernels, for every form.  At
                # these sizes the upload has landed before the next Python call anyway, so this form checks the bytes, not the
                # ordering; the ordering holds by that wait (csrc/engine_post.cpp).
                "no_heads": lambda: (fp.begin(frame), fp.heads(np.zeros((0, 4), np.float32))),
            }
            for j, (form, enqueue) in enumerate(forms.items()):
                enqueue()
                plain = fp.collect()
                for d, (fname, fmt) in enumerate(OC.FORMATS):          # host, device, host: the one slot both ways
                    matrix = (i + j + d) % 3
                    want = host_statement(frame, plain[0], ypr_of(plain), fmt, matrix)
                    enqueue()
                    out = overlay.new_output(h, w, FMT_NAME[fmt], MAT_NAME[matrix])
                    fp.annotate(out)
                    assert_same(fp.collect(), plain)                   # collect returns what it returns without annotate
                    for p, (g, wnt) in enumerate(zip(planes_of(out), want)):
                        assert g.tobytes() == wnt.tobytes(), (key, form, fname, "host", p)
                    s = DeviceSurface(h, w, fmt, matrix, extra=(0, 5, 1)[d], base=d + 1)
                    enqueue()
                    fp.annotate(s.out)
                    assert_same(fp.collect(), plain)
                    s.check(want, (key, form, fname, "device"))
                heads_painted += len(plain[0])
    assert heads_painted >= 4 * len(frames)
    # two in flight: the annotate of frame i is enqueued while frame i - 1 is still uncollected
    with FramePipeline(model, depth=2) as fp:
        keys, outs, got = list(frames) * 2, [], []
        for i, key in enumerate(keys):
            frame = frames[key]
            fp.begin(frame)
            fp.detect_heads(**kw)
            outs.append(np.zeros_like(frame) if i % 2 else DeviceSurface(frame.shape[0], frame.shape[1], OC.NV12, OC.BT709, 5, 1))
            fp.annotate(outs[-1] if i % 2 else outs[-1].out)
            if i >= 1:
                got.append(fp.collect())
        got.append(fp.collect())
    for key, out, res in zip(keys, outs, got):
        if isinstance(out, DeviceSurface):
            out.check(host_statement(frames[key], res[0], ypr_of(res), OC.NV12, OC.BT709), key)
        else:
            assert out.tobytes() == host_statement(frames[key], res[0], ypr_of(res), OC.PACKED, 0)[0].tobytes()


def test_detections_without_a_window_paint_nothing(model, kw, frames):
    """collect(detections=True) shows the invalid heads; the annotated frame is that of the valid ones alone."""
    seen_invalid = 0
    with FramePipeline(model, depth=1) as fp:
        for key, frame in frames.items():
            fp.begin(frame)
            fp.detect_heads(**kw)
            out = np.zeros_like(frame)
            fp.annotate(out)
            res = fp.collect(detections=True)
            seen_invalid += int((res[7] == 0).sum())
            assert out.tobytes() == host_statement(frame, res[0], ypr_of(res), OC.PACKED, 0)[0].tobytes()
    print(f"detections without a window over the three pictures: {seen_invalid}")


def test_yuv_ingest_to_nv12_surface_is_the_documented_loop(model, kw, frames):
    """decoder planes -> begin_yuv(device) -> detect_heads -> annotate(NV12 surface) -> collect: the frame the overlay reads is
    the BGR frame the ingest built."""
    frame = frames["W"]
    h, w = frame.shape[:2]
    src = overlay.annotate_host(frame, np.zeros((0, 4), np.int32), [], [], [], format="nv12", matrix="bt709")     # a decoder's planes
    dev = YUVFrame.nv12(torch.from_numpy(np.ascontiguousarray(src.planes[0])).to(DEV), torch.from_numpy(np.ascontiguousarray(src.planes[1])).to(DEV),
                        matrix="bt709")
    with FramePipeline(model, depth=1) as fp:
        s = DeviceSurface(h, w, OC.NV12, OC.BT709, 61, 0)
        fp.begin_yuv(dev)
        fp.detect_heads(**kw)
        fp.annotate(s.out)
        res = fp.collect()
        s.check(host_statement(src.to_bgr(), res[0], ypr_of(res), OC.NV12, OC.BT709), "yuv loop")


def test_clips_with_annotate_clip(model, kw, frames):
    A = frames["A"]
    same = [A, np.ascontiguousarray(A[::-1]), np.ascontiguousarray(A[:, ::-1])]
    mixed = [frames["W"], frames["A"], frames["B"]]
    with FramePipeline(model, depth=1) as fp:
        for begin, clip, tag in ((fp.begin_clip, same, "clip"), (fp.begin_clip_mixed, mixed, "mixed")):
            for max_heads in (None, 1):                                # 1: every head but the first overflows and paints nothing
                begin(clip)
                fp.detect_heads_clip(max_heads=max_heads, **kw)
                plain = fp.collect_clip()
                if max_heads == 1:
                    assert plain[1][1] >= 1, "no overflow: the clip needs two heads"
                for device in (False, True, False):
                    outs = [DeviceSurface(f.shape[0], f.shape[1], (OC.NV12, OC.I420, OC.PACKED)[i], i, 5, i + 1) if device
                            else overlay.new_output(f.shape[0], f.shape[1], ("nv12", "i420", "bgr")[i], MAT_NAME[i]) for i, f in enumerate(clip)]
                    begin(clip)
                    fp.detect_heads_clip(max_heads=max_heads, **kw)
                    fp.annotate_clip([o.out if device else o for o in outs])
                    got = fp.collect_clip()
                    assert got[1] == plain[1]
                    for g, p in zip(got[0], plain[0]):
                        assert_same(g, p)
                    for i, (f, o, res) in enumerate(zip(clip, outs, got[0])):
                        want = host_statement(f, res[0], ypr_of(res), (OC.NV12, OC.I420, OC.PACKED)[i], i)
                        if device:
                            o.check(want, (tag, max_heads, i))
                        else:
                            for p, (g, wnt) in enumerate(zip(planes_of(o), want)):
                                assert g.tobytes() == wnt.tobytes(), (tag, max_heads, i, p)
        begin = fp.begin_clip                                          # a frame left out keeps its destination untouched
        begin(same)
        fp.detect_heads_clip(**kw)
        only = np.zeros_like(A)
        fp.annotate_clip([None, only, None])
        got = fp.collect_clip()
        assert only.tobytes() == host_statement(same[1], got[0][1][0], ypr_of(got[0][1]), OC.PACKED, 0)[0].tobytes()


def test_annotate_is_ordered_on_the_callers_stream(model, kw, frames):
    frame = frames["A"]
    h, w = frame.shape[:2]
    with FramePipeline(model, depth=1) as fp:
        s = DeviceSurface(h, w, OC.NV12, OC.BT601, 5, 2)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        fp.begin(frame)
        fp.detect_heads(**kw)
        with torch.cuda.stream(side):
            fp.annotate(s.out, stream=side.cuda_stream)
            copy = s.dev.clone()                                       # enqueued on the caller's stream behind annotate: no host wait between
        res = fp.collect()
        torch.cuda.synchronize()
        want = host_statement(frame, res[0], ypr_of(res), OC.NV12, OC.BT601)
        s.check(want, "surface")
        s.dev = copy
        s.check(want, "the copy enqueued behind annotate")


# ---- 8. refusals that need a handle -------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_is_enqueued_and_the_ticket_still_collects(model, frames):
    h = model._handle
    frame = frames["B"]
    fh, fw = frame.shape[:2]
    rects = _lib.frame_rects(fh, fw, np.asarray([(10, 10, 50, 60), (20, 40, 70, 90)], np.float32))
    t = h.frame_begin(frame)
    h.frame_heads(t, rects)
    plain = h.collect(t, 2, want_logits=True)

    out = np.zeros_like(frame)
    good, _ = overlay.surface_of(out, fh, fw)
    dev = DeviceSurface(fh, fw, OC.PACKED, 0, 5, 1)
    good_dev, _ = overlay.surface_of(dev.out, fh, fw)
    t = h.frame_begin(frame)
    with pytest.raises(ValueError, match="not enqueued"):
        h.frame_annotate(t, 0, good)                                   # before the heads
    h.frame_heads(t, rects)
    with pytest.raises(ValueError, match="unknown"):
        h.frame_annotate(t + 4 * 1000, 0, good)                        # an unknown ticket
    with pytest.raises(ValueError, match="frame index"):
        h.frame_annotate(t, 1, good)
    as_device = _lib.SurfaceC.from_buffer_copy(good)
    as_device.on_device = 1
    with pytest.raises(ValueError, match="not device memory"):
        h.frame_annotate(t, 0, as_device)                              # a host pointer passed as device memory
    as_host = _lib.SurfaceC.from_buffer_copy(good_dev)
    as_host.on_device = 0
    with pytest.raises(ValueError, match="is device memory"):
        h.frame_annotate(t, 0, as_host)                                # ... and the reverse
    need = fh * 3 * fw
    short = h.device_alloc(need - 1)                                   # (the library's own allocation: exactly that many bytes)
    h.h2d(short, np.full(need - 1, GAP, np.uint8))
    leaves = _lib.SurfaceC()
    leaves.plane[0], leaves.pitch[0], leaves.format, leaves.on_device = short, 3 * fw, _lib.SURF_PACKED, 1
    with pytest.raises(ValueError, match=f"needs {need} bytes .* its allocation has {need - 1}"):
        h.frame_annotate(t, 0, leaves)                                 # an extent that leaves its allocation
    for spoil in (lambda s: setattr(s, "format", 7), lambda s: s.pitch.__setitem__(0, 3 * fw - 1), lambda s: s.plane.__setitem__(0, None)):
        bad = _lib.SurfaceC.from_buffer_copy(good)
        spoil(bad)
        with pytest.raises(ValueError):
            h.frame_annotate(t, 0, bad)
    h.frame_annotate(t, 0, good_dev)
    with pytest.raises(ValueError, match="annotated already"):
        h.frame_annotate(t, 0, good)                                   # twice
    got = h.collect(t, 2, want_logits=True)
    for g, p in zip(got, plain):
        assert g.tobytes() == p.tobytes()
    torch.cuda.synchronize()
    back = np.zeros(need - 1, np.uint8)
    h.d2h(back, short)
    h.device_free(short)
    assert not out.any() and (back == GAP).all()                       # nothing was launched for a refused call
    dev.check(host_statement(frame, rects, got[0], OC.PACKED, 0), "the one accepted call")
    # tickets that hold no frame
    crops = np.zeros((1, 224, 224, 3), np.uint8)
    t = h.submit(crops)
    with pytest.raises(ValueError, match="holds no frame"):
        h.frame_annotate(t, 0, good)
    h.collect(t, 1)
    t = h.submit_frame(frame, np.zeros((0, 4), np.int32))
    with pytest.raises(ValueError, match="holds no frame"):
        h.frame_annotate(t, 0, good)
    h.collect(t, 0)
