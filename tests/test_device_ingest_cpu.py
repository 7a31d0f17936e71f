"""Ingest from device memory, the parts that need no GPU: the six entry points are exported and declared in a header that is still
C, `__cuda_array_interface__` is parsed into the descriptors the C side gets (pointer, pitch, h, w) and everything the kernels
could not read as it lies is refused -- never copied --, and a `YUVFrame` knows where its planes are."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from whenet_hip import _lib
from whenet_hip.frames import FramePipeline
from whenet_hip.yuv import YUVFrame

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("whenet_frame_begin_device", "whenet_clip_begin_device", "whenet_frame_begin_yuv_device", "whenet_clip_begin_yuv_device",
           "whenet_op_pack_device", "whenet_op_yuv_to_bgr_device")


class Fake:
    """What a torch-ROCm tensor or a CuPy array shows of itself: the dict, nothing else."""

    def __init__(self, ptr, shape, strides=None, typestr="|u1", readonly=False, **extra):
        self.cai = dict(shape=tuple(shape), typestr=typestr, data=(ptr, readonly), version=3, **extra)
        if strides is not None or "strides" in extra:
            self.cai["strides"] = strides

    @property
    def __cuda_array_interface__(self):
        return self.cai


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_six_symbols_are_exported_and_bound():
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.EXPORTS
        assert getattr(lib, s).restype is C.c_int
    assert _lib.ABI_VERSION == 6
    with open(os.path.join(ROOT, "include", "whenet_hip.h")) as f:
        text = f.read()
    assert "#define WHENET_ABI_VERSION 6" in text
    for s in SYMBOLS:
        assert text.count(s + "(") == 1, s


def test_header_with_the_device_entry_points_is_valid_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "use_device_ingest.c"
    src.write_text(
        '#include "whenet_hip.h"\n'
        "int probe(whenet_t* h, const uint8_t* d_frame, void* stream, uint8_t* host) {\n"
        "    int ticket = 0; const int pitch = 4096, fh = 720, fw = 1280;\n"
        "    const uint8_t* frames[1]; uint8_t* out[1]; whenet_yuv_frame_t y;\n"
        "    frames[0] = d_frame; out[0] = host;\n"
        "    y.plane[0] = d_frame; y.plane[1] = d_frame + 4096 * 720; y.plane[2] = 0; y.pitch[0] = y.pitch[1] = 4096; y.pitch[2] = 0;\n"
        "    y.format = WHENET_YUV_NV12; y.matrix = WHENET_YUV_BT709; y.h = fh; y.w = fw;\n"
        "    if (whenet_frame_begin_device(h, d_frame, pitch, fh, fw, WHENET_BGR, stream, &ticket) != WHENET_OK) return -1;\n"
        "    if (whenet_clip_begin_device(h, frames, &pitch, 1, &fh, &fw, WHENET_RGB, stream, &ticket) != WHENET_OK) return -1;\n"
        "    if (whenet_frame_begin_yuv_device(h, &y, stream, &ticket) != WHENET_OK) return -1;\n"
        "    if (whenet_clip_begin_yuv_device(h, &y, 1, 0, &ticket) != WHENET_OK) return -1;\n"
        "    if (whenet_op_pack_device(h, frames, &pitch, 1, &fh, &fw, stream, out) != WHENET_OK) return -1;\n"
        "    return whenet_op_yuv_to_bgr_device(h, &y, 1, stream, out);\n"
        "}\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{os.path.join(ROOT, 'include')}", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_null_handle_and_null_ticket_are_einval():
    lib = _lib.load()
    t = C.c_int(0)
    assert lib.whenet_frame_begin_device(None, 1, 3, 1, 1, _lib.BGR, None, C.byref(t)) == _lib.EINVAL
    assert lib.whenet_frame_begin_yuv_device(None, None, None, C.byref(t)) == _lib.EINVAL
    assert lib.whenet_op_pack_device(None, None, None, 1, None, None, None, None) == _lib.EINVAL
    assert lib.whenet_op_yuv_to_bgr_device(None, None, 1, None, None) == _lib.EINVAL


# ---- __cuda_array_interface__ -> descriptor ---------------------------------------------------------------------------------------
def test_frame_descriptor_pointer_pitch_h_w():
    f = _lib.device_frame(Fake(0x7F0000001003, (5, 7, 3)))                 # no strides: C order
    assert (f.ptr, f.pitch, f.h, f.w) == (0x7F0000001003, 21, 5, 7)
    f = _lib.device_frame(Fake(0x1000, (5, 7, 3), strides=None))
    assert (f.pitch, f.h, f.w) == (21, 5, 7)
    f = _lib.device_frame(Fake(0x1001, (5, 7, 3), strides=(26, 3, 1)))     # a row pitch
    assert (f.ptr, f.pitch, f.h, f.w) == (0x1001, 26, 5, 7)
    f = _lib.device_frame(Fake(0x1000, (1, 7, 3), strides=(4096, 3, 1)))   # one row: its pitch is its row
    assert (f.pitch, f.h, f.w) == (21, 1, 7)
    f = _lib.device_frame(Fake(0x1000, (4, 1, 3), strides=(64, 99, 1)))    # one pixel per row: no pixel stride to hold
    assert (f.pitch, f.h, f.w) == (64, 4, 1)
    owner = Fake(0x2000, (2, 2, 3))
    assert _lib.device_frame(owner).owner is owner                         # the array stays alive with its descriptor
    assert _lib.device_frame(f) is f                                       # a descriptor passes through


def test_readonly_flag_is_accepted():
    f = _lib.device_frame(Fake(0x1000, (5, 7, 3), readonly=True))
    assert (f.ptr, f.pitch) == (0x1000, 21)
    y = Fake(0x1000, (4, 6), readonly=True)
    uv = Fake(0x2000, (2, 6), readonly=True)
    assert YUVFrame.nv12(y, uv).on_device


def test_clip_descriptors_from_one_array_and_from_a_list():
    items = _lib.device_frames(Fake(0x100, (3, 5, 7, 3), strides=(200, 32, 3, 1)))
    assert [(f.ptr, f.pitch, f.h, f.w) for f in items] == [(0x100, 32, 5, 7), (0x100 + 200, 32, 5, 7), (0x100 + 400, 32, 5, 7)]
    items = _lib.device_frames([Fake(0x100, (5, 7, 3)), Fake(0x900, (2, 2, 3), strides=(8, 3, 1))])
    assert [(f.ptr, f.pitch, f.h, f.w) for f in items] == [(0x100, 21, 5, 7), (0x900, 8, 2, 2)]
    ptrs, pitch, fh, fw = _lib._device_args(items)
    assert list(ptrs) == [0x100, 0x900] and pitch.tolist() == [21, 8] and fh.tolist() == [5, 2] and fw.tolist() == [7, 2]
    assert pitch.dtype == fh.dtype == fw.dtype == np.int32
    with pytest.raises(ValueError, match="one size"):
        _lib.device_frames([Fake(0x100, (5, 7, 3)), Fake(0x900, (2, 2, 3))], one_size=True)
    for n in (0, 17):
        with pytest.raises(ValueError, match="1..16"):
            _lib.device_frames([Fake(0x100, (5, 7, 3))] * n)
    with pytest.raises(ValueError, match="1..16"):
        _lib.device_frames(Fake(0x100, (17, 5, 7, 3)))


@pytest.mark.parametrize("fake,text", [
    (Fake(0x1000, (5, 7, 3), typestr="<f4"), "uint8"),
    (Fake(0x1000, (5, 7, 3), typestr="|i1"), "uint8"),
    (Fake(0x1000, (5, 7, 3), typestr="<u2"), "uint8"),
    (Fake(0x1000, (5, 7, 3), strides=(21, 1, 7)), "inner strides"),        # a CHW tensor permuted to HWC
    (Fake(0x1000, (5, 7, 3), strides=(28, 4, 1)), "inner strides"),        # the first three channels of BGRA
    (Fake(0x1000, (5, 7, 3), strides=(42, 6, 2)), "inner strides"),
    (Fake(0x1000, (5, 7, 3), strides=(21, 3, -1)), "negative"),
    (Fake(0x1000, (5, 7, 3), strides=(20, 3, 1)), "below its row"),        # overlapping rows
    (Fake(0x1000, (5, 7, 3), strides=(0, 3, 1)), "below its row"),         # a broadcast row
    (Fake(0x1000, (5, 7), strides=(7, 1)), r"\[H,W,3\]"),
    (Fake(0x1000, (2, 5, 7, 3)), r"\[H,W,3\]"),
    (Fake(0x1000, (5, 7, 4)), r"\[H,W,3\]"),
    (Fake(0x1000, (5, 7, 3), strides=(21, 3)), "do not fit"),
    (Fake(0, (5, 7, 3)), "NULL"),
    (Fake(0x1000, (0, 7, 3)), "sides must be 1..8192"),
    (Fake(0x1000, (5, 8193, 3)), "sides must be 1..8192"),
])
def test_frames_the_kernel_could_not_read_as_they_lie_are_refused(fake, text):
    with pytest.raises(ValueError, match=text):
        _lib.device_frame(fake)


def test_mixed_host_and_device_lists_are_refused():
    host = np.zeros((5, 7, 3), np.uint8)
    dev = Fake(0x1000, (5, 7, 3))
    for frames in ([dev, host], [host, dev], [host, dev, host]):
        with pytest.raises(ValueError, match="not mixed"):
            _lib.device_frames(frames)
        assert _lib.any_on_device(frames)
    assert not _lib.any_on_device([host, host]) and not _lib.any_on_device(np.zeros((2, 5, 7, 3), np.uint8))
    assert _lib.any_on_device(Fake(0x1000, (2, 5, 7, 3))) and _lib.any_on_device([dev])


class _Model:
    """A model whose handle records what the pipeline asks of it (no GPU): begin calls must route by residency."""

    class _H:
        def __init__(self):
            self.calls = []

        def set_option(self, *a):
            pass

        def __getattr__(self, name):
            def call(*a, **kw):
                self.calls.append((name, a, kw))
                return len(self.calls)
            return call

    def __init__(self):
        self._handle = self._H()


def test_pipeline_routes_by_residency_and_passes_the_stream():
    m = _Model()
    fp = FramePipeline(m, depth=4, bgr=False)
    dev, host = Fake(0x1000, (5, 7, 3), strides=(32, 3, 1)), np.zeros((5, 7, 3), np.uint8)
    fp.begin(dev, stream=1234)
    name, a, kw = m._handle.calls[-1]
    assert name == "frame_begin_device" and (a[0].ptr, a[0].pitch, a[0].h, a[0].w) == (0x1000, 32, 5, 7) and kw == dict(bgr=False, stream=1234)
    assert fp._begun[1:] == (5, 7)
    fp._begun = None
    fp.begin(host)
    assert m._handle.calls[-1][0] == "frame_begin"                          # numpy callers see no change
    fp._begun = None
    fp.begin_clip(Fake(0x100, (2, 5, 7, 3)), stream=None)
    name, a, kw = m._handle.calls[-1]
    assert name == "clip_begin_device" and len(a[0]) == 2 and fp._begun_clip[1] == 2
    fp._begun_clip = None
    with pytest.raises(ValueError, match="one size"):
        fp.begin_clip([dev, Fake(0x2000, (2, 2, 3))])
    fp.begin_clip_mixed([dev, Fake(0x2000, (2, 2, 3))], stream=7)
    name, a, kw = m._handle.calls[-1]
    assert name == "clip_begin_device" and [(f.h, f.w) for f in a[0]] == [(5, 7), (2, 2)] and kw["stream"] == 7
    fp._begun_clip = None
    n = len(m._handle.calls)
    for call in (fp.begin_clip, fp.begin_clip_mixed):
        with pytest.raises(ValueError, match="not mixed"):
            call([dev, host])
    with pytest.raises(ValueError, match="inner strides"):
        fp.begin(Fake(0x1000, (5, 7, 3), strides=(21, 1, 7)))
    assert len(m._handle.calls) == n and fp._begun is None and fp._begun_clip is None      # nothing reached the handle
    fp.begin_clip_mixed([host, host[:2]])
    assert m._handle.calls[-1][0] == "clip_begin_mixed"
    fp._begun_clip = None
    # YUV frames
    yd = YUVFrame.nv12(Fake(0x1000, (4, 6), strides=(8, 1)), Fake(0x2000, (2, 6), strides=(8, 1)))
    yh = YUVFrame.nv12(np.zeros((4, 6), np.uint8), np.zeros((2, 6), np.uint8))
    fp.begin_yuv(yd, stream=9)
    assert m._handle.calls[-1][0] == "frame_begin_yuv_device" and m._handle.calls[-1][2] == dict(stream=9)
    fp._begun = None
    fp.begin_yuv(yh)
    assert m._handle.calls[-1][0] == "frame_begin_yuv"
    fp._begun = None
    fp.begin_clip_yuv([yd, yd], stream=9)
    assert m._handle.calls[-1][0] == "clip_begin_yuv_device"
    fp._begun_clip = None
    fp.begin_clip_yuv([yh, yh])
    assert m._handle.calls[-1][0] == "clip_begin_yuv"
    fp._begun_clip = None
    with pytest.raises(ValueError, match="not mixed"):
        fp.begin_clip_yuv([yd, yh])
    fp._pending.clear()


def test_stream_argument():
    assert _lib._stream(None) is None and _lib._stream(0) is None
    assert _lib._stream(0x7F00DEAD0000).value == 0x7F00DEAD0000
    for bad in ("0", 1.5, object()):
        with pytest.raises(ValueError, match="stream"):
            _lib._stream(bad)


# ---- YUVFrame -----------------------------------------------------------------------------------------------------------------------
def test_yuv_frame_on_device_and_its_descriptor():
    y, uv = Fake(0x10000, (5, 7), strides=(16, 1)), Fake(0x20002, (3, 4, 2), strides=(24, 2, 1))      # interleaved [ch, cw, 2]
    f = YUVFrame.nv12(y, uv, matrix="bt709")
    assert f.on_device and (f.h, f.w) == (5, 7) and f.pitches == (16, 24)
    d = f.descriptor()
    assert (d.plane[0], d.plane[1], d.plane[2]) == (0x10000, 0x20002, None)
    assert (d.pitch[0], d.pitch[1], d.format, d.matrix, d.h, d.w) == (16, 24, _lib.YUV_NV12, _lib.YUV_BT709, 5, 7)
    g = YUVFrame.i420(Fake(0x1001, (5, 7)), Fake(0x2003, (3, 4), strides=(9, 1)), Fake(0x3005, (3, 4)), matrix="jfif")
    assert g.on_device and g.pitches == (7, 9, 4)
    d = g.descriptor()
    assert (d.plane[0], d.plane[1], d.plane[2]) == (0x1001, 0x2003, 0x3005)
    host = YUVFrame.nv12(np.zeros((5, 7), np.uint8), np.zeros((3, 8), np.uint8))
    assert host.on_device is False and host.to_bgr().shape == (5, 7, 3)
    # a decoder's single allocation in device memory
    h, w, pitch = 7, 13, 32
    surf = Fake(0x40000, (pitch * h + 4 * pitch,))
    f = YUVFrame.from_buffer(surf, h, w, "nv12", pitch=pitch)
    assert f.on_device and [p.ptr for p in f.planes] == [0x40000, 0x40000 + pitch * h] and f.pitches == (pitch, pitch)
    f = YUVFrame.from_buffer(surf, h, w, "i420", pitch=pitch)
    assert [p.ptr for p in f.planes] == [0x40000, 0x40000 + pitch * h, 0x40000 + pitch * h + 16 * 4] and f.pitches == (32, 16, 16)
    with pytest.raises(ValueError, match="the frame needs"):
        YUVFrame.from_buffer(Fake(0x40000, (100,)), h, w, "nv12", pitch=pitch)
    with pytest.raises(ValueError, match="contiguous"):
        YUVFrame.from_buffer(Fake(0x40000, (400,), strides=(2,)), h, w, "nv12", pitch=pitch)


def test_planes_of_differing_residency_and_bad_device_planes_are_refused():
    yd, uvd = Fake(0x1000, (4, 6)), Fake(0x2000, (2, 6))
    yh, uvh = np.zeros((4, 6), np.uint8), np.zeros((2, 6), np.uint8)
    for planes in ((yd, uvh), (yh, uvd)):
        with pytest.raises(ValueError, match="all in device memory or all in host memory"):
            YUVFrame.nv12(*planes)
    with pytest.raises(ValueError, match="all in device memory or all in host memory"):
        YUVFrame.i420(yd, Fake(0x2000, (2, 3)), np.zeros((2, 3), np.uint8))
    for planes, text in (((Fake(0x1000, (4, 6), typestr="<f4"), uvd), "uint8"), ((yd, Fake(0x2000, (2, 5))), r"\[2,6\]"),
                         ((Fake(0x1000, (4, 6), strides=(12, 2)), uvd), "contiguous"), ((Fake(0x1000, (4, 6), strides=(5, 1)), uvd), "below its row"),
                         ((Fake(0x1000, (4, 6, 1)), uvd), r"\[h,w\]"), ((yd, Fake(0, (2, 6))), "NULL")):
        with pytest.raises(ValueError, match=text):
            YUVFrame.nv12(*planes)


def test_to_bgr_of_a_device_frame_names_the_device_call():
    f = YUVFrame.nv12(Fake(0x1000, (4, 6)), Fake(0x2000, (2, 6)))
    with pytest.raises(ValueError, match="Handle.op_yuv_to_bgr_device"):
        f.to_bgr()
