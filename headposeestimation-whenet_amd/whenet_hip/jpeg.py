"""The JPEG encoder: a frame in, a baseline JPEG stream out, produced by the library.

demo_video.py:46-47, :60 store the annotated frame as Motion-JPEG through `cv2.VideoWriter`.  Here the stream is written by the
kernels of `csrc/jpeg.hip` from a 4:2:0 JFIF surface -- what the pose overlay leaves in device memory -- or from packed pixels, by
the integer statement of include/whenet_hip.h (JPEG ENCODER): baseline sequential DCT, 4:2:0, the standard's Annex K tables scaled
the IJG way, one restart interval per MCU row.

    data = jpeg.encode(frame, quality=95, handle=model)        # bytes: any JPEG decoder opens them
    with MJPGWriter("out.avi", 30, (w, h)) as out: out.write(data)

`encode()` runs the kernels, `encode_host()` the same arithmetic on the host inside the library (no GPU): the two return the same
bytes.  A frame is a uint8 [H,W,3] array (B, G, R order unless bgr=False) or a `whenet_hip.yuv.YUVFrame` in host memory whose
matrix is 'jfif'; it is never copied to make it fit.  What is pinned: Pillow (libjpeg-turbo) decodes every stream of the test
table, and its quality and size stay next to Pillow's own encoder at the same tables (docs/experiments.md section 29).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .yuv import YUVFrame

DEFAULT_QUALITY = _lib.JPEG_DEFAULT_QUALITY
HEADER_BYTES = _lib.JPEG_HEADER_BYTES
CapacityError = _lib.CapacityError


def header(h: int, w: int, quality: int = DEFAULT_QUALITY) -> bytes:
    """The 629 bytes SOI..SOS of the stream of an h x w frame: they depend on (h, w, quality) only."""
    return _lib.jpeg_header(h, w, quality)[0]


def quantisers(quality: int = DEFAULT_QUALITY) -> np.ndarray:
    """int32 [2,64]: the luminance and the chrominance quantiser at `quality`, natural order."""
    return _lib.jpeg_header(16, 16, quality)[1]


def bound(h: int, w: int) -> int:
    """A capacity no stream of an h x w frame exceeds (`whenet_jpeg_bound`)."""
    return _lib.jpeg_bound(h, w)


def source_of(frame, what: str = "frame"):
    """A source frame -> (`_lib.SurfaceC`, h, w, the object that keeps its memory alive).  ValueError for anything that would need a
    copy: another dtype or shape, pixels that are not packed, planes in device memory."""
    s = _lib.SurfaceC()
    if isinstance(frame, YUVFrame):
        if frame.on_device:
            raise ValueError(f"{what}: the planes are in device memory: Handle.jpeg_encode_device encodes those")
        for i, (a, p) in enumerate(zip(frame.planes, frame.pitches)):
            s.plane[i], s.pitch[i] = a.ctypes.data, p
        s.format, s.matrix, s.on_device = frame.format, frame.matrix, 0
        return s, frame.h, frame.w, frame
    a = np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{what} must be uint8 [H,W,3] or a whenet_hip.yuv.YUVFrame, got {a.dtype} {a.shape}")
    h, w = int(a.shape[0]), int(a.shape[1])
    if a.strides[2] != 1 or (w > 1 and a.strides[1] != 3) or (h > 1 and a.strides[0] < 3 * w):
        raise ValueError(f"{what}: the pixels of a row must be packed (inner strides (3, 1), got {a.strides}); it is never copied")
    s.plane[0], s.pitch[0] = a.ctypes.data, int(a.strides[0]) if h > 1 else 3 * w
    s.format, s.matrix, s.on_device = _lib.SURF_PACKED, 0, 0
    return s, h, w, a


def _finish(rc: int, size: int, out: np.ndarray) -> bytes:
    if rc == _lib.EOVERFLOW:
        raise CapacityError(size, f"the JPEG stream has {size} bytes, the capacity is {out.size}")
    return out[:size].tobytes()


def _handle_of(handle):
    return getattr(handle, "_handle", handle)      # a WHENet model or a _lib.Handle


def encode(frame, quality: int = DEFAULT_QUALITY, handle=None, bgr: bool = True, capacity=None) -> bytes:
    """The stream of `frame`, written by the kernels (`whenet_op_jpeg_encode`).  `handle`: a `WHENet` model or a `_lib.Handle`; None
    opens a postproc handle on device 0 for the call.  `capacity` (default: `bound(h, w)`) below the stream's length raises
    `CapacityError` with the needed size."""
    s, h, w, _keep = source_of(frame)
    out = np.empty(bound(h, w) if capacity is None else int(capacity), np.uint8)
    if handle is None:
        with _lib.Handle.postproc(0) as own:
            rc, size = own.op_jpeg_encode(s, h, w, bgr, quality, out)
    else:
        rc, size = _handle_of(handle).op_jpeg_encode(s, h, w, bgr, quality, out)
    return _finish(rc, size, out)


def encode_host(frame, quality: int = DEFAULT_QUALITY, bgr: bool = True, capacity=None) -> bytes:
    """The same stream by pure host arithmetic inside the library (`whenet_jpeg_encode_host`, no GPU): the statement the kernels are
    held to."""
    s, h, w, _keep = source_of(frame)
    out = np.empty(bound(h, w) if capacity is None else int(capacity), np.uint8)
    rc, size = _lib.jpeg_encode_host(s, h, w, bgr, quality, out)
    return _finish(rc, size, out)
