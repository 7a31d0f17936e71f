"""The pose overlay: the annotated frame of the reference's video loop, produced by the library.

demo_video.py:26-29 draws, for every head, `cv2.rectangle` of its window and `draw_axis` (utils.py:13-43) from the window's centre,
and demo_video.py:60 writes the frame out.  Here the same picture is painted by two kernels (`csrc/overlay.hip`) from what the
forward leaves in device memory, into a host array or into a pitched BGR / NV12 / I420 surface in device memory, by the integer
statement of include/whenet_hip.h (POSE OVERLAY): `segments()` are the reference's endpoints exactly; the raster of a segment --
every pixel within distance 1 of it -- is the project's own rule, not OpenCV's.

    fp.begin_yuv(frame, stream=s); fp.detect_heads(); fp.annotate(nv12_surface, stream=s); rects, yaw, pitch, roll = fp.collect()

`annotate()` / `annotate_host()` below are the stage alone, on host arrays: the kernels, and the same arithmetic on the host inside
the library (no GPU).  A destination is never copied to make it fit: a writable uint8 [H,W,3] numpy array, a uint8 [H,W,3] device
array with inner strides (3, 1), or a `whenet_hip.yuv.YUVFrame` whose planes are writable -- or a ValueError.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .yuv import FORMATS, YUVFrame, _code

PACKED_NAMES = ("bgr", "rgb", "packed")        # the frame's own channel order: `format` names the layout, not a colour conversion


def segments(rect, yaw: float, pitch: float, roll: float):
    """Window (y0, x0, y1, x1) + angles in degrees -> (int32 [16], flags): `x0, y0, x1, y1` of the rectangle, then the start and
    the end of the X (red), Y (green) and Z (blue) axis as (x, y) pairs -- the arguments of the reference's three `cv2.line`
    calls for `draw_axis(frame, yaw, pitch, roll, tdx=(x0+x1)/2, tdy=(y0+y1)/2, size=(x1-x0)//2)`.  flags: 1 rectangle | 2 axes
    (angles that are not finite: the rectangle only)."""
    return _lib.overlay_segments(rect, yaw, pitch, roll)


def labels(rect, yaw: float, pitch: float, roll: float):
    """Window (y0, x0, y1, x1) + angles in degrees -> (texts, origins int32 [3,2], flags): the three lines `--display full` writes
    next to a head -- 'yaw: 10.0', 'pitch: -5.0', 'roll: 2.0', the numbers as the reference's `"{}".format(np.round(a))` prints
    them -- and the (x, y) each starts at, the arguments of the reference's three `cv2.putText` calls.  flags: 1 rectangle | 2 axes |
    4 labels; a head without the 4 (angles not finite, or a rounded angle beyond +-9999) has empty texts."""
    return _lib.overlay_labels(rect, yaw, pitch, roll)


def glyph(ch: str):
    """The strokes of a character of the labels' font (the project's own: include/whenet_hip.h, WHENET_OVERLAY_FONT) as int32
    [n,4] rows of x0, y0, x1, y1 relative to the character's baseline-left origin, y growing downward."""
    return _lib.overlay_glyph(ch)


def surface_of(out, h: int, w: int, what: str = "out"):
    """A destination of an h x w frame -> (`_lib.SurfaceC`, the object that keeps its memory alive).  ValueError for anything that
    would need a copy or a conversion: a read-only array, another shape or dtype, CHW, pixels that are not packed."""
    s = _lib.SurfaceC()
    if isinstance(out, YUVFrame):
        if out.needs_ext:
            raise ValueError(f"{what}: a 16-bit, 4:4:4 or BT.2020 frame as a destination is not built: destinations are packed "
                             "BGR / RGB, or 8-bit NV12 / I420 under BT.601, BT.709 or JFIF")
        if out.format not in (_lib.YUV_NV12, _lib.YUV_I420):
            raise ValueError(f"{what}: a packed 4:2:2 frame (YUYV / UYVY) as a destination is not built: destinations are packed "
                             "BGR / RGB, NV12 or I420")
        if (out.h, out.w) != (h, w):
            raise ValueError(f"{what}: the surface is {out.h} x {out.w}, the frame {h} x {w}")
        if not out.writable:
            raise ValueError(f"{what}: the planes of the YUVFrame are read-only")
        for i, (a, p) in enumerate(zip(out.planes, out.pitches)):
            s.plane[i] = a.ptr if out.on_device else a.ctypes.data
            s.pitch[i] = p
        s.format, s.matrix, s.on_device = out.format, out.matrix, int(out.on_device)
        return s, out
    if isinstance(out, np.ndarray):
        if out.dtype != np.uint8 or out.ndim != 3 or out.shape != (h, w, 3):
            raise ValueError(f"{what} must be uint8 [{h},{w},3], got {out.dtype} {out.shape}")
        if not out.flags.writeable:
            raise ValueError(f"{what} is a read-only array")
        if out.strides[2] != 1 or (w > 1 and out.strides[1] != 3) or (h > 1 and out.strides[0] < 3 * w):
            raise ValueError(f"{what}: the pixels of a row must be packed (inner strides (3, 1), got {out.strides}); it is never copied")
        s.plane[0], s.pitch[0] = out.ctypes.data, int(out.strides[0]) if h > 1 else 3 * w
        s.format, s.matrix, s.on_device = _lib.SURF_PACKED, 0, 0
        return s, out
    if _lib.is_device_array(out) or isinstance(out, _lib.DeviceFrame):
        if not isinstance(out, (_lib.DeviceFrame, _lib.DeviceView)) and bool(out.__cuda_array_interface__.get("data", (0, True))[1]):
            raise ValueError(f"{what} is a read-only device array")
        f = _lib.device_frame(out, what)
        if (f.h, f.w) != (h, w):
            raise ValueError(f"{what} is {f.h} x {f.w}, the frame {h} x {w}")
        s.plane[0], s.pitch[0] = f.ptr, f.pitch
        s.format, s.matrix, s.on_device = _lib.SURF_PACKED, 0, 1
        return s, out
    raise ValueError(f"{what} must be a writable uint8 [H,W,3] numpy array, a uint8 [H,W,3] device array or a whenet_hip.yuv.YUVFrame, "
                     f"got {type(out).__name__}")


def new_output(h: int, w: int, format="bgr", matrix="bt601"):
    """A fresh host destination: a uint8 [h,w,3] array for 'bgr' / 'rgb' / 'packed' (the frame's channel order), a tight
    `YUVFrame` for 'nv12' / 'i420'."""
    if isinstance(format, str) and format.lower() in PACKED_NAMES:
        return np.empty((h, w, 3), np.uint8)
    # (the planar formats only: a packed 4:2:2 destination is not built, its names are unknown formats here as they were)
    fmt = _code({k: v for k, v in FORMATS.items() if v in (_lib.YUV_NV12, _lib.YUV_I420)}, format, "format")
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y = np.empty((h, w), np.uint8)
    if fmt == _lib.YUV_NV12:
        return YUVFrame.nv12(y, np.empty((ch, 2 * cw), np.uint8), matrix)
    return YUVFrame.i420(y, np.empty((ch, cw), np.uint8), np.empty((ch, cw), np.uint8), matrix)


def _frame_u8(frame) -> np.ndarray:
    frame = np.asarray(frame)
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise ValueError(f"frame must be uint8 [H,W,3], got {frame.dtype} {frame.shape}")
    return np.ascontiguousarray(frame)


def _ypr(yaw, pitch, roll) -> np.ndarray:
    cols = [np.asarray(v, np.float32).reshape(-1) for v in (yaw, pitch, roll)]
    if len({c.shape[0] for c in cols}) != 1:
        raise ValueError("yaw, pitch and roll must have one length")
    return np.stack(cols, axis=1) if cols[0].shape[0] else np.zeros((0, 3), np.float32)


def annotate(model, frame, rects, yaw, pitch, roll, out=None, format="bgr", matrix="bt601", valid=None, bgr: bool = True,
             display: str = "simple"):
    """The stage alone, on the device: `frame` uint8 [H,W,3] (BGR unless `bgr=False`) with the k heads `rects` int32 [k,4]
    (y0, x0, y1, x1 as `collect()` returns them) and their angles painted in -> `out` (a host destination; `out=None` allocates one
    of `format` / `matrix`), which is returned.  `model` is a `whenet.WHENet` or a `_lib.Handle` (a postproc handle will do).
    `display="full"` adds the three labels of every head (`labels()`), as demo_video.py's `--display full` does."""
    code = _lib.display_code(display)
    frame = _frame_u8(frame)
    if out is None:
        out = new_output(frame.shape[0], frame.shape[1], format, matrix)
    surface, _ = surface_of(out, frame.shape[0], frame.shape[1])
    handle = getattr(model, "_handle", model)
    handle.op_annotate(frame, rects, valid, _ypr(yaw, pitch, roll), surface, bgr=bgr, display=code)
    return out


def annotate_host(frame, rects, yaw, pitch, roll, out=None, format="bgr", matrix="bt601", valid=None, bgr: bool = True,
                  display: str = "simple"):
    """`annotate()` as pure host arithmetic inside the library (no GPU): the statement the kernels are held to, byte for byte."""
    code = _lib.display_code(display)
    frame = _frame_u8(frame)
    if out is None:
        out = new_output(frame.shape[0], frame.shape[1], format, matrix)
    surface, _ = surface_of(out, frame.shape[0], frame.shape[1])
    _lib.annotate_host(frame, rects, valid, _ypr(yaw, pitch, roll), surface, bgr=bgr, display=code)
    return out
