"""Ingest from device memory on the GPU (csrc/ingest.hip, csrc/yuv.hip's plane kernel; Engine::*_device of csrc/engine_post.cpp;
FramePipeline.begin / begin_clip / begin_clip_mixed / begin_yuv / begin_clip_yuv on device arrays).  Device memory comes from torch
tensors.  Everything is bitwise, there is no tolerance: the packing kernel returns the bytes of np.ascontiguousarray, the plane
kernel those of the host function on the same pitched bytes, and a frame, a clip or a mixed clip begun from device memory returns
what the same submission begun from host memory returns.  Refused descriptors never reach a kernel."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import detector_cases as DC
from tests import yuv_cases as YC
from tests.test_clip_gpu import assert_same, hargs, kwargs
from tests.test_yuv_gpu import built, seeded_model
from whenet_hip import _lib
from whenet_hip.frames import FramePipeline
from whenet_hip.yuv import YUVFrame

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "tiny"
GAP = 0xC3                 # what lies in a device surface outside the bytes of its rows
SENTINEL = 0xA5            # what a byte of the ops' landing buffer holds that no thread wrote (csrc/engine_post.cpp GuardedOutput)
DEV = "cuda:0"


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
        return kwargs(json.load(f)["detect"], NAME)


# ---- device surfaces from host bytes ------------------------------------------------------------------------------------------------
def surface(rows2d, pitch, base=0):
    """A torch view [rows, row_bytes(, ...)] whose rows are `pitch` bytes apart and whose first byte lies `base` bytes into a fresh
    device allocation (torch's allocations are 512-byte aligned, so the address is `base` mod 4); everything around the rows is GAP.
    Returns (view [rows, row_bytes], host copy of the whole allocation)."""
    rows2d = np.ascontiguousarray(rows2d, np.uint8)
    rows, rb = rows2d.shape
    assert pitch >= rb
    host = np.full(base + (rows - 1) * pitch + rb, GAP, np.uint8)
    np.lib.stride_tricks.as_strided(host[base:], (rows, rb), (pitch, 1))[...] = rows2d
    dev = torch.from_numpy(host).to(DEV)
    assert dev.data_ptr() % 16 == 0
    view = torch.as_strided(dev, (rows, rb), (pitch, 1), storage_offset=base)
    assert view.data_ptr() % 4 == base % 4
    return view, host


def packed_surface(frame, pitch=None, base=0):
    """A uint8 [h,w,3] device tensor holding `frame` at a row pitch and a base offset."""
    h, w, _ = frame.shape
    pitch = 3 * w if pitch is None else pitch
    view, _ = surface(frame.reshape(h, 3 * w), pitch, base)
    t = torch.as_strided(view, (h, w, 3), (pitch, 3, 1), storage_offset=view.storage_offset())
    assert t.__cuda_array_interface__["data"][0] == view.data_ptr()
    return t


def device_yuv(b, matrix, bases=(0, 0, 0)):
    """The built case `b` (tests/yuv_cases.py) with its planes uploaded WITH their pitches and gap bytes, plane p at bases[p] mod 4."""
    views = [surface(v, p, base)[0] for v, p, base in zip(b["views"], b["pitches"], bases)]
    f = YUVFrame.nv12(views[0], views[1], matrix=matrix) if b["fmt"] == YC.NV12 else YUVFrame.i420(*views, matrix=matrix)
    assert f.on_device and (f.h, f.w) == (b["h"], b["w"])
    assert tuple(f.pitches[i] for i in range(len(views)) if f.planes[i].shape[0] > 1) == \
        tuple(b["pitches"][i] for i in range(len(views)) if f.planes[i].shape[0] > 1)
    return f


# ---- 1. the pack kernel is np.ascontiguousarray --------------------------------------------------------------------------------------
PACK_H, PACK_W = (1, 2, 3, 5), (1, 2, 3, 4, 5, 7, 8, 9, 17)


@pytest.fixture(scope="module")
def pool():
    """One device allocation of random bytes (and its host copy) that the packing tests cut their sources from."""
    host = np.random.default_rng(20261019).integers(0, 256, 1 << 14, dtype=np.uint8)
    dev = torch.from_numpy(host).to(DEV)
    assert dev.data_ptr() % 16 == 0
    return dev, host


def cut(pool, off, h, w, pitch):
    """(device view, expected tight host frame) of h rows of 3 w bytes, `pitch` apart, `off` bytes into the pool."""
    dev, host = pool
    assert off + (h - 1) * pitch + 3 * w <= host.size
    t = torch.as_strided(dev, (h, w, 3), (pitch, 3, 1), storage_offset=off)
    want = np.ascontiguousarray(np.lib.stride_tricks.as_strided(host[off:], (h, w, 3), (pitch, 3, 1)))
    return t, want


@pytest.mark.parametrize("extra", [0, 1, 5])
def test_pack_kernel_equals_ascontiguousarray(post, pool, extra):
    n = 0
    for h in PACK_H:
        for w in PACK_W:
            for base in range(4):
                t, want = cut(pool, 64 * n % 4096 + base, h, w, 3 * w + extra)
                n += 1
                assert t.data_ptr() % 4 == base
                got, = post.op_pack_device([t])
                assert got.dtype == np.uint8 and got.shape == (h, w, 3)
                assert got.tobytes() == want.tobytes(), (h, w, extra, base)
    # wider rows: every chunk kind in one row (full chunks, a short last one) at every source and destination alignment
    for w in (16, 21, 33, 100):
        for base in range(4):
            t, want = cut(pool, 1000 + base, 4, w, 3 * w + extra)
            assert post.op_pack_device([t])[0].tobytes() == want.tobytes(), (w, extra, base)


def test_packed_frames_do_not_touch_each_other(post, pool):
    shapes = ((3, 5), (2, 2), (5, 17), (1, 1), (10, 18), (33, 7))          # tests/test_yuv_gpu.py: output offsets 45, 57, 312, ...
    offsets = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in shapes])])
    assert offsets[1:4].tolist() == [45, 57, 312] and offsets[1] % 4 and offsets[2] % 4 and offsets[4] % 4
    frames, wants = [], []
    for i, (h, w) in enumerate(shapes):
        t, want = cut(pool, 2048 * (i % 4) + 7 * i + 1, h, w, 3 * w + (0, 1, 5)[i % 3])
        frames.append(t)
        wants.append(want)
    alone = [post.op_pack_device([t])[0] for t in frames]
    for a, want in zip(alone, wants):
        assert a.tobytes() == want.tobytes()
    for order in (list(range(len(frames))), list(range(len(frames)))[::-1]):
        got = post.op_pack_device([frames[i] for i in order])
        for g, i in zip(got, order):
            assert g.tobytes() == alone[i].tobytes(), (order, i)
    many = [frames[i % len(frames)] for i in range(16)]                   # sixteen frames
    for g, i in zip(post.op_pack_device(many), range(16)):
        assert g.tobytes() == alone[i % len(frames)].tobytes()
    one = cut(pool, 3, 5, 17, 60)                                          # [F,H,W,3] as one array: frames 4 x 60 + 9 bytes apart
    clip = torch.as_strided(pool[0], (3, 5, 17, 3), (249, 60, 3, 1), storage_offset=3)
    got = post.op_pack_device(clip)
    assert len(got) == 3 and got[0].tobytes() == one[1].tobytes()
    for f, g in enumerate(got):
        assert g.tobytes() == cut(pool, 3 + 249 * f, 5, 17, 60)[1].tobytes()


def test_a_byte_nobody_wrote_would_show(post, pool):
    """The landing buffer of the op is pre-filled: a source made of the sentinel's complement comes back without one sentinel byte."""
    frame = np.full((5, 17, 3), SENTINEL ^ 0xFF, np.uint8)
    for base in range(4):
        got, = post.op_pack_device([packed_surface(frame, 3 * 17 + 5, base)])
        assert got.tobytes() == frame.tobytes() and not (got == SENTINEL).any() and not (got == GAP).any()


# ---- 2. the plane kernel is the host function ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,matrix", YC.MATRICES)
@pytest.mark.parametrize("fname,fmt", YC.FORMATS)
def test_plane_kernel_equals_host_function_on_every_case(post, fname, fmt, mname, matrix):
    for i, case in enumerate(YC.CASES):
        b = YC.build(case, fmt)
        want = YC.frame_of(b, mname).to_bgr()
        small = b["h"] * b["w"] <= 400
        for r in (range(4) if small else (i % 4,)):                        # plane bases 0..3 mod 4, each plane its own
            frame = device_yuv(b, mname, (r, (r + 1) % 4, (r + 3) % 4))
            got, = post.op_yuv_to_bgr_device([frame])
            assert got.dtype == np.uint8 and got.shape == want.shape == (b["h"], b["w"], 3)
            assert got.tobytes() == want.tobytes(), (case[0], fname, mname, r)


def test_plane_launches_of_six_mixed_and_three_uniform_frames(post):
    shapes = ((3, 5), (2, 2), (5, 17), (1, 1), (10, 18), (33, 7))
    keep, frames, wants = [], [], []
    for i, (h, w) in enumerate(shapes):
        b = built(f"random_{h}x{w}", YC.FORMATS[i % 2][1])
        keep.append(b)
        frames.append(device_yuv(b, YC.MATRICES[i % 3][0], (i % 4, (i + 2) % 4, (i + 3) % 4)))
        wants.append(YC.frame_of(b, YC.MATRICES[i % 3][0]).to_bgr())
    alone = [post.op_yuv_to_bgr_device([f])[0] for f in frames]
    for a, want in zip(alone, wants):
        assert a.tobytes() == want.tobytes()
    for order in (list(range(6)), list(range(6))[::-1]):
        got = post.op_yuv_to_bgr_device([frames[i] for i in order])
        for g, i in zip(got, order):
            assert g.tobytes() == alone[i].tobytes(), (order, i)
    bs = [built(n, YC.I420) for n in ("random_5x17", "extremes_5x17", "random_5x17")]      # one size, format and matrix
    same = [device_yuv(b, "bt709", (1, 2, 3)) for b in bs]
    for g, b in zip(post.op_yuv_to_bgr_device(same), bs):
        assert g.tobytes() == YC.frame_of(b, "bt709").to_bgr().tobytes()
    pitched = built("random_pitched_64x130", YC.NV12)                      # a decoder's pitches, and sixteen frames
    many = [frames[i % 6] for i in range(15)] + [device_yuv(pitched, "bt601", (2, 2, 0))]
    got = post.op_yuv_to_bgr_device(many)
    for g, i in zip(got[:15], range(15)):
        assert g.tobytes() == alone[i % 6].tobytes()
    assert got[15].tobytes() == YC.frame_of(pitched, "bt601").to_bgr().tobytes()


# ---- 3. the resident frame is the same frame --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bgr_frames():
    """The sample-frame cuts tests/test_yuv_gpu.py uses, as BGR frames: 224 x 528, 225 x 547 and the 97 x 131 window."""
    f1 = DC.sample_frame(1)
    return dict(A=DC.sample_frame(0), B=f1, W=np.ascontiguousarray(f1[60:60 + 97, 200:200 + 131]))


@pytest.fixture(scope="module")
def yuv_frames():
    """name -> (host YUVFrame, device YUVFrame of the same bytes, planes at odd bases), as tests/test_yuv_gpu.py's pictures."""
    spec = dict(A=("sample0_224x528", YC.NV12, "bt601"), B=("sample1_225x547", YC.I420, "bt709"),
                A2=("sample0_224x528", YC.I420, "jfif"), W=("sample1_window_97x131", YC.NV12, "jfif"))
    out, keep = {}, []
    for i, (key, (name, fmt, matrix)) in enumerate(spec.items()):
        b = built(name, fmt)
        keep.append(b)
        out[key] = (YC.frame_of(b, matrix), device_yuv(b, matrix, (i % 4, (i + 1) % 4, (i + 2) % 4)))
    return out, keep


@pytest.mark.parametrize("bgr", [True, False])
def test_detector_input_of_a_device_frame_equals_that_of_its_host_copy(model, bgr_frames, bgr):
    t = packed_surface(bgr_frames["B"], 3 * 547 + 7, 3)
    with FramePipeline(model, depth=1, bgr=bgr) as fp:
        fp.begin(t)
        got = fp.detector_input((64, 96), as_uint8=True)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
        fp.begin(t.cpu().numpy())
        want = fp.detector_input((64, 96), as_uint8=True)
    assert got.shape == (64, 96, 3) and got.tobytes() == want.tobytes()
    assert len(np.unique(got)) > 16                                        # a picture, not a flat canvas


@pytest.mark.parametrize("key", ["A", "B"])
def test_detector_input_of_device_planes_equals_that_of_host_planes(model, yuv_frames, key):
    host, dev = yuv_frames[0][key]
    with FramePipeline(model, depth=1) as fp:
        fp.begin_yuv(dev)
        got = fp.detector_input((64, 96), as_uint8=True)
        fp.heads(np.zeros((0, 4), np.float32))
        fp.collect()
        fp.begin_yuv(host)
        want = fp.detector_input((64, 96), as_uint8=True)
    assert got.tobytes() == want.tobytes() and len(np.unique(got)) > 16


# ---- 4. submissions are bit for bit the host path ---------------------------------------------------------------------------------
def run_frame(fp, kw, begin, frame):
    begin(frame)
    fp.detect_heads(**kw)
    return fp.collect(detections=True)


def run_clip(fp, kw, begin, frames):
    begin(frames)
    fp.detect_heads_clip(**kw)
    return fp.collect_clip(detections=True)


def assert_same_clip(got, want):
    assert got[1] == want[1] and len(got[0]) == len(want[0])
    for g, w in zip(got[0], want[0]):
        assert_same(g, w)


def test_frame_submission_from_device_memory_equals_the_host_path(model, kw, bgr_frames, yuv_frames):
    dev = {k: packed_surface(f, 3 * f.shape[1] + (0, 1, 5)[i % 3], i + 1) for i, (k, f) in enumerate(bgr_frames.items())}
    with FramePipeline(model, depth=1) as fp:
        detections = 0
        for k in ("A", "B", "W"):
            want = run_frame(fp, kw, fp.begin, bgr_frames[k])              # host, device, host: the one slot both ways
            assert len(want) == 8
            assert_same(run_frame(fp, kw, fp.begin, dev[k]), want)
            assert_same(run_frame(fp, kw, fp.begin, bgr_frames[k]), want)
            detections += len(want[4])
        assert detections >= 1                                             # (the seeded detector does fire on these pictures)
        for k in ("A", "B", "W", "A2"):
            host, d = yuv_frames[0][k]
            want = run_frame(fp, kw, fp.begin_yuv, host)
            assert_same(run_frame(fp, kw, fp.begin_yuv, d), want)
            assert_same(run_frame(fp, kw, fp.begin_yuv, host), want)
    with FramePipeline(model, depth=2) as fp:                              # two in flight, sources alternating
        order = [("A", True), ("B", False), ("W", True), ("A", False), ("B", True)]
        got = []
        for i, (k, on_device) in enumerate(order):
            fp.begin(dev[k] if on_device else bgr_frames[k])
            fp.detect_heads(**kw)
            if i >= 1:
                got.append(fp.collect(detections=True))
        got.append(fp.collect(detections=True))
    with FramePipeline(model, depth=1) as fp:
        for g, (k, _) in zip(got, order):
            assert_same(g, run_frame(fp, kw, fp.begin, bgr_frames[k]))


def test_clip_submissions_from_device_memory_equal_the_host_path(model, kw, bgr_frames, yuv_frames):
    A = bgr_frames["A"]
    same_host = [A, np.ascontiguousarray(A[::-1]), A]
    same_dev = [packed_surface(f, 3 * 528 + (1, 0, 5)[i], i + 1) for i, f in enumerate(same_host)]
    stacked = torch.from_numpy(np.stack(same_host)).to(DEV)                # one [F,H,W,3] tensor
    mixed_host = [bgr_frames["W"], bgr_frames["A"], bgr_frames["B"]]      # 97 x 131 first: the frames behind it start unaligned
    assert (97 * 131 * 3) % 4 != 0
    mixed_dev = [packed_surface(f, 3 * f.shape[1] + (5, 1, 0)[i], 3 - i) for i, f in enumerate(mixed_host)]
    yuv_keys = ("W", "A", "B", "A2")
    yuv_host, yuv_dev = [yuv_frames[0][k][0] for k in yuv_keys], [yuv_frames[0][k][1] for k in yuv_keys]
    assert len({f.format for f in yuv_dev}) == 2 and len({f.matrix for f in yuv_dev}) == 3 and len({(f.h, f.w) for f in yuv_dev}) == 3
    with FramePipeline(model, depth=1) as fp:
        want = run_clip(fp, kw, fp.begin_clip, same_host)                  # host, device, host
        assert want[1][1] == 0 and len(want[0]) == 3
        assert_same_clip(run_clip(fp, kw, fp.begin_clip, same_dev), want)
        assert_same_clip(run_clip(fp, kw, fp.begin_clip, same_host), want)
        assert_same_clip(run_clip(fp, kw, fp.begin_clip, stacked), want)
        assert_same_clip(run_clip(fp, kw, fp.begin_clip_mixed, same_dev), want)      # one size through the mixed call: a clip_begin slot
        for host, dev in ((mixed_host, mixed_dev), (mixed_host[::-1], mixed_dev[::-1])):
            want = run_clip(fp, kw, fp.begin_clip_mixed, host)
            assert_same_clip(run_clip(fp, kw, fp.begin_clip_mixed, dev), want)
            assert_same_clip(run_clip(fp, kw, fp.begin_clip_mixed, host), want)
        want = run_clip(fp, kw, fp.begin_clip_yuv, yuv_host)               # mixed sizes, formats and matrices
        assert_same_clip(run_clip(fp, kw, fp.begin_clip_yuv, yuv_dev), want)
        assert_same_clip(run_clip(fp, kw, fp.begin_clip_yuv, yuv_host), want)
        pair_h, pair_d = [yuv_host[1], yuv_host[3]], [yuv_dev[1], yuv_dev[3]]      # one size: a clip_begin slot
        assert_same_clip(run_clip(fp, kw, fp.begin_clip_yuv, pair_d), run_clip(fp, kw, fp.begin_clip_yuv, pair_h))
    # through the handle, in every array (argmax and logits too)
    h = model._handle
    for begin_h, begin_d, F in ((lambda: h.clip_begin_mixed(mixed_host), lambda: h.clip_begin_device(mixed_dev), 3),
                                (lambda: h.clip_begin(np.stack(same_host)), lambda: h.clip_begin_device(same_dev), 3),
                                (lambda: h.clip_begin_yuv(yuv_host), lambda: h.clip_begin_yuv_device(yuv_dev), 4)):
        t = begin_h()
        want = h.collect_clip(t, F, h.clip_detect_heads(t, *hargs(kw)), want_logits=True)
        t = begin_d()
        got = h.collect_clip(t, F, h.clip_detect_heads(t, *hargs(kw)), want_logits=True)
        for g, w in zip(got, want):
            assert (g.tobytes() == w.tobytes()) if isinstance(w, np.ndarray) else g == w


# ---- 5. stream order ----------------------------------------------------------------------------------------------------------------
def test_begin_is_ordered_on_the_callers_stream(model, kw, bgr_frames):
    frame = bgr_frames["A"]
    with FramePipeline(model, depth=1) as fp:
        want = run_frame(fp, kw, fp.begin, frame)
        assert len(want[4]) >= 1
        pinned = torch.from_numpy(frame).pin_memory()
        t = torch.zeros(frame.shape, dtype=torch.uint8, device=DEV)
        a = torch.ones((4096, 4096), device=DEV)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(6):                                             # a few milliseconds of unrelated work ahead of the copy
                a = (a @ a) * 1e-4
            t.copy_(pinned, non_blocking=True)                             # the frame arrives on the side stream ...
            fp.begin(t, stream=s.cuda_stream)                              # ... the ingest must see it ...
            t.zero_()                                                      # ... and this must not reach the tensor before the ingest has read it
        fp.detect_heads(**kw)
        got = fp.collect(detections=True)
        torch.cuda.synchronize()
        assert not t.any().item()
    assert_same(got, want)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_descriptors_are_einval_before_anything_is_enqueued(model, kw, bgr_frames, yuv_frames):
    h = model._handle
    lib, tk = _lib.load(), C.c_int(-1)
    frame = bgr_frames["W"]
    fh, fw = frame.shape[:2]
    good = packed_surface(frame, 3 * fw + 1, 1)
    gf = _lib.device_frame(good)
    ydev = yuv_frames[0]["W"][1]
    with FramePipeline(model, depth=1) as fp:
        want = run_frame(fp, kw, fp.begin, frame)

        def still_works():
            assert_same(run_frame(fp, kw, fp.begin, good), want)

        for _ in range(_lib.MAX_INFLIGHT + 1):                             # (a refusal that took a slot would use them up)
            # a host pointer handed to the device entry points
            host_frame = _lib.DeviceFrame(frame.ctypes.data, 3 * fw, fh, fw, frame)
            for call in (lambda: h.frame_begin_device(host_frame), lambda: h.clip_begin_device([gf, host_frame]),
                         lambda: h.op_pack_device([gf, host_frame])):
                with pytest.raises(ValueError, match="not device memory"):
                    call()
            hy = yuv_frames[0]["W"][0].descriptor()
            for call in (lambda: h.frame_begin_yuv_device(hy), lambda: h.clip_begin_yuv_device([ydev, hy]),
                         lambda: h.op_yuv_to_bgr_device([ydev, hy])):
                with pytest.raises(ValueError, match="frame [01]: plane 0 is not device memory"):
                    call()
            # a pitch below the row bytes
            with pytest.raises(ValueError, match=r"frame 1: pitch \d+ is below its row"):
                h.clip_begin_device([gf, _lib.DeviceFrame(gf.ptr, 3 * fw - 1, fh, fw)])
            d = ydev.descriptor()
            d.pitch[1] = 2 * ((fw + 1) // 2) - 1
            with pytest.raises(ValueError, match="frame 0: pitch"):
                h.frame_begin_yuv_device(d)
            # 17 frames (the Python layer refuses them itself: straight to the C entry points)
            with pytest.raises(ValueError, match="1..16"):
                h.clip_begin_device([gf] * 17)
            ptrs, pitch, ah, aw = _lib._device_args([gf] * 17)
            for n in (0, 17):
                assert lib.whenet_clip_begin_device(h._h, ptrs, _lib._ptr(pitch), n, _lib._ptr(ah), _lib._ptr(aw), _lib.BGR, None,
                                                    C.byref(tk)) == _lib.EINVAL
                assert "1..16" in lib.whenet_last_error(h._h).decode()
                arr = (_lib.YuvFrameC * 17)(*[ydev.descriptor()] * 17)
                assert lib.whenet_clip_begin_yuv_device(h._h, arr, n, None, C.byref(tk)) == _lib.EINVAL
            # sides and NULLs
            for bad, text in ((_lib.DeviceFrame(gf.ptr, 3 * 8193, 1, 8193), "sides must be 1..8192"), (_lib.DeviceFrame(0, 3, 1, 1), "NULL")):
                with pytest.raises(ValueError, match=text):
                    h.frame_begin_device(bad)
            assert lib.whenet_frame_begin_device(h._h, gf.ptr, gf.pitch, fh, fw, 2, None, C.byref(tk)) == _lib.EINVAL      # channel order
        still_works()
        assert fp.in_flight == 0


def test_a_descriptor_that_leaves_its_allocation_is_refused(model):
    """1,100 bytes of a 1,000-byte allocation: the overrun would stay inside the allocation's page, so even a wrong check cannot fault."""
    h = model._handle
    p = h.device_alloc(1000)
    try:
        host = (np.arange(1000) * 7 & 255).astype(np.uint8)
        h.h2d(p, host)
        for _ in range(_lib.MAX_INFLIGHT + 1):                             # (a refusal that took a slot would use them up)
            y = _lib.YuvFrameC()                                           # Y plane: 11 rows of 100 bytes at pitch 100 = 1,100 bytes
            y.plane[0], y.plane[1], y.pitch[0], y.pitch[1] = p, p, 100, 100
            y.format, y.matrix, y.h, y.w = _lib.YUV_NV12, _lib.YUV_BT601, 11, 100
            for call in (lambda: h.frame_begin_yuv_device(y), lambda: h.clip_begin_yuv_device([y]), lambda: h.op_yuv_to_bgr_device([y])):
                with pytest.raises(ValueError, match="frame 0: plane 0 needs 1100 bytes .* its allocation has 1000"):
                    call()
        for f, text in ((_lib.DeviceFrame(p, 100, 11, 33), "needs 1099 bytes .* its allocation has 1000"),      # 10 x 100 + 99
                        (_lib.DeviceFrame(p + 100, 100, 10, 33), "needs 999 bytes .* its allocation has 900"),  # from inside the allocation
                        (_lib.DeviceFrame(p + 999, 3, 1, 1), "needs 3 bytes .* its allocation has 1")):
            for call in (h.frame_begin_device, lambda f: h.op_pack_device([f]), lambda f: h.clip_begin_device([f, f])):
                with pytest.raises(ValueError, match="frame 0 " + text):
                    call(f)
        # what fits is taken: the whole allocation, and its last bytes
        got, = h.op_pack_device([_lib.DeviceFrame(p + 1, 111, 9, 37)])     # 8 x 111 + 111 = 999 bytes from byte 1
        assert got.tobytes() == host[1:1000].tobytes()
        got, = h.op_pack_device([_lib.DeviceFrame(p + 997, 3, 1, 1)])
        assert got.tobytes() == host[997:].tobytes()
        t = h.frame_begin_device(_lib.DeviceFrame(p, 100, 10, 33))
        h.frame_heads(t, np.zeros((0, 4), np.int32))
        h.collect(t, 0)
    finally:
        h.device_free(p)


def test_more_sizes_than_the_letterbox_cache_is_refused_and_takes_no_slot(kw, bgr_frames, yuv_frames):
    dev = [packed_surface(bgr_frames[k]) for k in ("W", "A", "B")]
    ydev = [yuv_frames[0][k][1] for k in ("W", "A", "B")]
    m = seeded_model()
    try:
        h = m._handle
        h.set_option("letterbox_cache", 2)
        with FramePipeline(m, depth=1) as fp:
            for _ in range(_lib.MAX_INFLIGHT + 1):                        # (a leak would use up the slots)
                for call in (lambda: fp.begin_clip_mixed(dev), lambda: h.clip_begin_device(dev), lambda: fp.begin_clip_yuv(ydev),
                             lambda: h.clip_begin_yuv_device(ydev)):
                    with pytest.raises(ValueError, match="letterbox_cache"):
                        call()
            assert fp.in_flight == 0
            tickets = [h.frame_begin_device(dev[0]) for _ in range(_lib.MAX_INFLIGHT)]      # every slot is still there
            for t in tickets:
                h.frame_heads(t, np.zeros((0, 4), np.int32))
                h.collect(t, 0)
            want = run_clip(fp, kw, fp.begin_clip_mixed, [bgr_frames["W"], bgr_frames["A"]])      # two sizes fit
            assert_same_clip(run_clip(fp, kw, fp.begin_clip_mixed, dev[:2]), want)
            run_clip(fp, kw, fp.begin_clip, [dev[1], dev[1], dev[1]])      # three frames of ONE size need no entry each
    finally:
        m.close()


def test_wrong_ticket_kinds_fail_as_for_host_tickets(model, kw, bgr_frames):
    h = model._handle
    args = hargs(kw)[:5]
    dev = packed_surface(bgr_frames["A"], 3 * 528 + 1, 2)
    tk = h.frame_begin_device(dev)
    with pytest.raises(ValueError, match="holds a single frame"):
        h.clip_detect_heads(tk, *args, 20)
    cap = h.frame_detect_heads(tk, *args, 20)
    with pytest.raises(ValueError, match="was not submitted by clip_detect_heads"):
        h.collect_clip(tk, 1, cap)
    with pytest.raises(ValueError, match="collect_detect returns it"):
        h.collect(tk, cap)
    res = h.collect_detect(tk, cap)
    tk = h.frame_begin(bgr_frames["A"])
    cap = h.frame_detect_heads(tk, *args, 20)
    for g, w in zip(res, h.collect_detect(tk, cap)):
        assert (g is None and w is None) or g.tobytes() == w.tobytes()
    tk = h.clip_begin_device([packed_surface(bgr_frames["W"]), dev])
    for call in (lambda: h.frame_detect_heads(tk, *args, 20), lambda: h.frame_detect(tk, *args, 20), lambda: h.frame_letterbox(tk, (64, 96)),
                 lambda: h.frame_heads(tk, np.array([[10, 10, 50, 50]], np.int32))):
        with pytest.raises(ValueError, match="holds a clip"):
            call()
    k = h.clip_detect_heads(tk, *args, 20)
    with pytest.raises(ValueError, match="collect_clip returns it"):
        h.collect(tk, 3)
    res = h.collect_clip(tk, 2, k)
    assert res[0][1] == len(h_detections(model, kw, bgr_frames["A"]))
    with FramePipeline(model, depth=1) as fp:                              # no slot leaked: every one is taken in turn
        for _ in range(_lib.MAX_INFLIGHT + 1):
            run_frame(fp, kw, fp.begin, dev)


def h_detections(model, kw, frame):
    with FramePipeline(model, depth=1) as fp:
        return run_frame(fp, kw, fp.begin, frame)[4]
