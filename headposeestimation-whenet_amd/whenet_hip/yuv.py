"""YUV frames as video decoders and cameras deliver them -- 4:2:0 planes (NV12, I420) and packed 4:2:2 (YUYV alias YUY2, UYVY: the
raw formats of V4L2 / UVC cameras and capture cards) -- for `FramePipeline.begin_yuv` / `begin_clip_yuv`.

A `YUVFrame` describes the planes where they are: nothing is copied or converted here.  The planes are uploaded as they are (1.5
bytes per pixel for 4:2:0, 2 for packed 4:2:2) and the packed BGR frame is built on the device (`csrc/yuv.hip`) by the integer conversion stated in
include/whenet_hip.h; `to_bgr()` runs the same arithmetic on the host inside the library.

    frame = YUVFrame.from_buffer(decoder_buffer, 1080, 1920, "nv12", pitch=2048, matrix="bt709")
    fp.begin_yuv(frame); fp.detect_heads(); rects, yaw, pitch, roll = fp.collect()

The planes may also lie in DEVICE memory -- a hardware decoder's surface, torch-ROCm tensors, CuPy arrays: anything that exposes
`__cuda_array_interface__` is taken as a plane (all planes of a frame on the device, or all on the host; `on_device` tells which).
`begin_yuv` then converts them where they are (no host copy, no PCIe), ordered on the caller's stream:

    surface = torch.empty(2048 * 1620, dtype=torch.uint8, device="cuda")          # filled by the decoder
    frame = YUVFrame.from_buffer(surface, 1080, 1920, "nv12", pitch=2048, matrix="bt709")
    fp.begin_yuv(frame, stream=torch.cuda.current_stream().cuda_stream)

What a decoder makes of 10-bit video, and 4:4:4 surfaces (include/whenet_hip_yuv_ext.h, `csrc/yuvx.hip`): a frame is a LAYOUT (the
four above, or planar 4:4:4) times a sample CONTAINER -- 8 bits, or 16 bits little endian with a `shift` (the sample at 16 bits is
`(word << shift) & 0xFFFF`: 0 for P010 / P016 and a hardware decoder's 16-bit surfaces, 6 for yuv420p10le / I010, 4 for the 12-bit
LSB-aligned forms) -- and a fourth matrix, "bt2020" (non-constant luminance, video range):

    frame = YUVFrame.p010(y16, uv16, matrix="bt2020")                       # uint16 planes, or uint8 views with an even row
    frame = YUVFrame.from_buffer(buf, 1080, 1920, "yuv420p10le", matrix="bt2020")
    frame = YUVFrame.i444(y, u, v)                                          # uint8 or uint16 planes

`begin_yuv` / `begin_clip_yuv` take such frames as they take the others (a clip may mix them).  The constructors `nv12`, `i420`,
`yuyv`, `uyvy` keep the three matrices they had; and so do `from_buffer` with their names and the plain
constructor; an 8-bit frame under BT.2020 is `YUVFrame(planes, "nv12", "bt2020", h, w, container=8)`: naming the container
opens the extended tables.  Not built: Y210 / Y216 / v210, NV16 / NV24, big-endian samples, HDR transfer functions (PQ /
HLG), full-range BT.709 / BT.2020, 10-bit destinations of `annotate`.
"""
from __future__ import annotations

import numpy as np

from . import _lib

FORMATS = {"nv12": _lib.YUV_NV12, "i420": _lib.YUV_I420, "yuyv": _lib.YUV_YUYV, "yuy2": _lib.YUV_YUYV, "uyvy": _lib.YUV_UYVY}
PACKED = (_lib.YUV_YUYV, _lib.YUV_UYVY)        # one plane of h rows of 4 * ((w + 1) // 2) bytes
_NAMES = {_lib.YUV_NV12: "NV12", _lib.YUV_I420: "I420", _lib.YUV_YUYV: "YUYV", _lib.YUV_UYVY: "UYVY"}
MATRICES = {"bt601": _lib.YUV_BT601, "bt709": _lib.YUV_BT709, "jfif": _lib.YUV_JFIF}
# {yoff, CY, CVR, CUG, CVG, CUB} per matrix: WHENET_YUV_COEFFS of include/whenet_hip.h (tests/test_yuv_cpu.py holds both to the text)
COEFFS = {"bt601": (16, 1220542, 1673527, 409993, 852492, 2116026),
          "bt709": (16, 1220945, 1879825, 223578, 558767, 2215014),
          "jfif": (0, 1048576, 1470104, 360853, 748826, 1858077)}
MAX_SIDE = _lib.MAX_FRAME_SIDE
# ---- include/whenet_hip_yuv_ext.h: layouts, containers, the fourth matrix ----
I444 = _lib.YUVX_I444
LAYOUTS = dict(FORMATS, i444=I444)
_NAMES_EXT = dict(_NAMES)
_NAMES_EXT[I444] = "I444"
MATRICES_EXT = dict(MATRICES, bt2020=_lib.YUV_BT2020)
COEFFS_EXT = dict(COEFFS, bt2020=(16, 1220945, 1760217, 196426, 682019, 2245811))      # WHENET_YUVX_COEFFS: a fourth row
# names of `from_buffer` -> (layout, container bits, shift)
FORMATS_EXT = {"p010": (_lib.YUV_NV12, 16, 0), "p012": (_lib.YUV_NV12, 16, 0), "p016": (_lib.YUV_NV12, 16, 0),
               "i010": (_lib.YUV_I420, 16, 6), "yuv420p10le": (_lib.YUV_I420, 16, 6), "yuv420p12le": (_lib.YUV_I420, 16, 4),
               "yuv420p16le": (_lib.YUV_I420, 16, 0),
               "i444": (I444, 8, 0), "yuv444p": (I444, 8, 0), "yuv444p16": (I444, 16, 0), "yuv444p16le": (I444, 16, 0),
               "yuv444p10le": (I444, 16, 6), "yuv444p12le": (I444, 16, 4)}


def _code(table: dict, value, what: str) -> int:
    if isinstance(value, str):
        if value.lower() not in table:
            raise ValueError(f"unknown {what} {value!r}: one of {sorted(table)}")
        return table[value.lower()]
    if value not in table.values():
        raise ValueError(f"unknown {what} {value!r}: one of {sorted(table)}")
    return int(value)


def _plane(a, rows: int, row_bytes: int, name: str, wide: bool = False) -> np.ndarray:
    """A plane as a uint8 array of `rows` rows of `row_bytes` contiguous bytes (an interleaved plane may be [rows, cw, 2]); the row
    stride is the pitch.  Nothing is copied: a plane whose bytes within a row are not contiguous is refused."""
    a = np.asarray(a)
    if wide and a.dtype == np.dtype("<u2"):         # 16-bit samples: the same rows as bytes
        if a.ndim == 3 and a.shape[2] == 2 and a.strides[1:] == (4, 2):
            a = np.lib.stride_tricks.as_strided(a, (a.shape[0], a.shape[1] * 2), (a.strides[0], 2), writeable=False)
        if a.ndim != 2 or (a.shape[1] > 1 and a.strides[1] != 2):
            raise ValueError(f"{name} plane: the samples of a row must be contiguous (shape {a.shape}, strides {a.strides})")
        a = np.lib.stride_tricks.as_strided(a, (a.shape[0], a.shape[1]), (a.strides[0], 2), writeable=False).view(np.uint8)
    if a.dtype != np.uint8:
        raise ValueError(f"{name} plane must be {'uint16 (or uint8 bytes)' if wide else 'uint8'}, got {a.dtype}")
    if a.ndim == 3 and a.shape[2] == 2 and a.strides[1:] == (2, 1):
        a = np.lib.stride_tricks.as_strided(a, (a.shape[0], a.shape[1] * 2), (a.strides[0], 1), writeable=False)
    if a.ndim != 2 or a.shape != (rows, row_bytes):
        raise ValueError(f"{name} plane must be uint8 [{rows},{row_bytes}], got shape {a.shape}")
    if row_bytes > 1 and a.strides[1] != 1:
        raise ValueError(f"{name} plane: the bytes of a row must be contiguous (strides {a.strides})")
    if rows > 1 and a.strides[0] < row_bytes:
        raise ValueError(f"{name} plane: row stride {a.strides[0]} is below its row of {row_bytes} bytes")
    return a


def _device_bytes(a, what: str, wide: bool) -> "_lib.DeviceView":
    """`_lib.device_view`, which takes uint8; for a 16-bit frame also a `<u2` device array, as the same rows of bytes."""
    cai = getattr(a, "__cuda_array_interface__", None)
    if not (wide and isinstance(cai, dict) and cai.get("typestr") in ("<u2", "=u2") and "shape" in cai and "data" in cai):
        return _lib.device_view(a, what)
    shape = tuple(int(v) for v in cai["shape"])
    strides = cai.get("strides")
    if strides is None:
        strides, acc = [], 2
        for n in reversed(shape):
            strides.append(acc)
            acc *= n
        strides = tuple(reversed(strides))
    strides = tuple(int(v) for v in strides)
    if len(shape) < 1 or len(strides) != len(shape) or any(v < 0 for v in strides) or (shape[-1] > 1 and strides[-1] != 2):
        raise ValueError(f"{what}: the samples of a row must be contiguous (shape {shape}, strides {strides})")
    ptr = cai["data"][0]
    if not ptr and all(shape):
        raise ValueError(f"{what}: NULL device pointer")
    return _lib.DeviceView(int(ptr or 0), shape[:-1] + (shape[-1] * 2,), strides[:-1] + (1,), a)


def _device_plane(a, rows: int, row_bytes: int, name: str, wide: bool = False) -> "_lib.DeviceView":
    """`_plane` for a plane in device memory: the same shapes and stride rules, read from `__cuda_array_interface__`."""
    v = _device_bytes(a, f"{name} plane", wide)
    shape, strides = v.shape, v.strides
    if len(shape) == 3 and shape[2] == 2 and strides[1:] == (2, 1):
        shape, strides = (shape[0], shape[1] * 2), (strides[0], 1)
    if len(shape) == 3 and shape[2] == 4 and strides[1:] == (4, 1):      # (an interleaved plane of 16-bit samples as [ch, cw, 2])
        shape, strides = (shape[0], shape[1] * 4), (strides[0], 1)
    if len(shape) != 2 or shape != (rows, row_bytes):
        raise ValueError(f"{name} plane must be uint8 [{rows},{row_bytes}], got shape {v.shape}")
    if row_bytes > 1 and strides[1] != 1:
        raise ValueError(f"{name} plane: the bytes of a row must be contiguous (strides {strides})")
    if rows > 1 and strides[0] < row_bytes:
        raise ValueError(f"{name} plane: row stride {strides[0]} is below its row of {row_bytes} bytes")
    return _lib.DeviceView(v.ptr, shape, strides, v.owner)


def _array_writable(a) -> bool:
    """Whether a plane's memory may be written: numpy's `writeable` flag, or the read-only flag of `__cuda_array_interface__` (of
    the owner, for a `_lib.DeviceView`: a view carries no flag of its own)."""
    if isinstance(a, _lib.DeviceView):
        if a.owner is None:
            return True
        a = a.owner
    if _lib.is_device_array(a):
        data = a.__cuda_array_interface__.get("data", (0, True))
        return not bool(data[1])
    return bool(np.asarray(a).flags.writeable)


class YUVFrame:
    """The planes of one frame of h x w luma samples: `planes` (2 arrays for NV12: Y, interleaved UV; 3 for I420: Y, U, V; 1 for the
    packed 4:2:2 formats YUYV / UYVY), their byte `pitches`, `format`, `matrix` (codes of include/whenet_hip.h), `h`, `w`.  The
    chroma planes of a 4:2:0 frame have (h + 1) // 2 rows of (w + 1) // 2 samples.  A packed frame is one plane of h rows of
    4 * ((w + 1) // 2) bytes (Y0 U Y1 V, or U Y0 V Y1, per pixel pair; every row has its own chroma); for even w it may be handed
    in as [h, w, 2]."""

    def __init__(self, planes, format, matrix, h: int, w: int, _writable=None, container=None, shift: int = 0):
        # without `container` the constructor takes what it always took: the four formats and three matrices of whenet_yuv_frame_t;
        # with it (8 or 16) also planar 4:4:4 and BT.2020 (include/whenet_hip_yuv_ext.h)
        ext = container is not None
        self.format = _code(LAYOUTS if ext else FORMATS, format, "format")
        self.matrix = _code(MATRICES_EXT if ext else MATRICES, matrix, "matrix")
        self.container, self.shift = int(container) if ext else 8, int(shift)
        if self.container not in (8, 16):
            raise ValueError(f"unknown container {container!r}: 8 or 16 bits per stored sample")
        if not 0 <= self.shift <= 8 or (self.shift and self.container == 8):
            raise ValueError(f"shift {self.shift} with a container of {self.container} bits: 0..8 for 16-bit samples, 0 for 8-bit ones")
        if self.format in PACKED and self.container != 8:
            raise ValueError(f"{_NAMES_EXT[self.format]} has an 8-bit container (Y210 / Y216 are not built)")
        wide, bs = self.container == 16, self.container // 8
        self.h, self.w = int(h), int(w)
        if not (1 <= self.h <= MAX_SIDE and 1 <= self.w <= MAX_SIDE):
            raise ValueError(f"frame is {self.h} x {self.w}: sides must be 1..{MAX_SIDE}")
        ch, cw = (self.h + 1) // 2, (self.w + 1) // 2
        if self.format in PACKED:
            shapes = [(self.h, 4 * cw, _NAMES_EXT[self.format])]
        elif self.format == _lib.YUV_NV12:
            shapes = [(self.h, self.w * bs, "Y"), (ch, 2 * cw * bs, "UV")]
        elif self.format == I444:
            shapes = [(self.h, self.w * bs, "Y"), (self.h, self.w * bs, "U"), (self.h, self.w * bs, "V")]
        else:
            shapes = [(self.h, self.w * bs, "Y"), (ch, cw * bs, "U"), (ch, cw * bs, "V")]
        planes = list(planes)
        if len(planes) != len(shapes):
            raise ValueError(f"{_NAMES_EXT[self.format]} has {len(shapes)} plane{'s' if len(shapes) > 1 else ''}, got {len(planes)}")
        on_device = [_lib.is_device_array(a) for a in planes]
        if any(on_device) and not all(on_device):
            raise ValueError("the planes of a frame are all in device memory or all in host memory, got " +
                             ", ".join(f"{n}: {'device' if d else 'host'}" for (_, _, n), d in zip(shapes, on_device)))
        self.on_device = all(on_device)       # the planes are device memory (`_lib.DeviceView`s), not numpy arrays
        # whether the memory behind every plane may be written (a destination of `FramePipeline.annotate`): asked of the arrays as
        # they were handed in -- the views kept in `planes` are read-only whatever their memory is
        self.writable = bool(_writable) if _writable is not None else all(_array_writable(a) for a in planes)
        if self.on_device:
            self.planes = tuple(_device_plane(a, r, b, n, wide) for a, (r, b, n) in zip(planes, shapes))
        else:
            self.planes = tuple(_plane(a, r, b, n, wide) for a, (r, b, n) in zip(planes, shapes))
        # a plane of one row has no row stride of its own: its pitch is its row
        self.pitches = tuple(int(a.strides[0]) if a.shape[0] > 1 else int(a.shape[1]) for a in self.planes)
        if wide:
            for (_, _, n), a, p in zip(shapes, self.planes, self.pitches):
                if (a.ptr if self.on_device else a.ctypes.data) & 1 or p & 1:
                    raise ValueError(f"{n} plane: 16-bit samples lie at an even address with an even pitch (pitch {p})")

    @property
    def needs_ext(self) -> bool:
        """Whether whenet_yuv_frame_t cannot describe this frame: a 16-bit container, planar 4:4:4 or BT.2020 (then the calls of
        include/whenet_hip_yuv_ext.h take it, and `descriptor()` is their struct)."""
        return self.container != 8 or self.format == I444 or self.matrix == _lib.YUV_BT2020

    @classmethod
    def nv12(cls, y, uv, matrix="bt601") -> "YUVFrame":
        """Y uint8 [h,w] and the interleaved chroma plane uint8 [ch, 2 cw] (or [ch, cw, 2]: U, V)."""
        h, w = cls._luma_size(y)
        return cls((y, uv), _lib.YUV_NV12, matrix, h, w)

    @classmethod
    def i420(cls, y, u, v, matrix="bt601") -> "YUVFrame":
        """Y uint8 [h,w], U and V uint8 [ch,cw]."""
        h, w = cls._luma_size(y)
        return cls((y, u, v), _lib.YUV_I420, matrix, h, w)

    @classmethod
    def p010(cls, y, uv, matrix="bt709") -> "YUVFrame":
        """P010 (and P012): Y uint16 [h,w] and the interleaved chroma plane uint16 [ch, 2 cw] (or [ch, cw, 2]), the sample in the
        HIGH bits of every word; or the same planes as uint8 bytes [h, 2 w] / [ch, 4 cw].  The low bits are used as they are."""
        h, w = cls._luma_size(y, 16)
        return cls((y, uv), _lib.YUV_NV12, matrix, h, w, container=16, shift=0)

    p016 = p010      # one layout: all 16 bits are the sample

    @classmethod
    def i010(cls, y, u, v, depth=10, matrix="bt709") -> "YUVFrame":
        """I010 / yuv420p10le (depth=10), yuv420p12le (12) or 16-bit planes (16): Y uint16 [h,w], U and V uint16 [ch,cw], the
        sample in the LOW `depth` bits of every word (bits above them are masked off); or the planes as uint8 bytes."""
        if depth not in range(8, 17):
            raise ValueError(f"depth {depth!r}: 8..16 bits in a 16-bit word")
        h, w = cls._luma_size(y, 16)
        return cls((y, u, v), _lib.YUV_I420, matrix, h, w, container=16, shift=16 - int(depth))

    @classmethod
    def i444(cls, y, u, v, matrix="bt601", shift=0) -> "YUVFrame":
        """Planar 4:4:4: Y, U, V all [h,w], uint8 (I444, a decoder's YUV444 surface) or uint16 (its 16-bit twin, `shift` as for
        every 16-bit container: 0 for MSB-aligned samples, 6 for yuv444p10le)."""
        first = y.__cuda_array_interface__["typestr"] if _lib.is_device_array(y) else np.asarray(y).dtype.str
        bits = 16 if first in ("<u2", "=u2") else 8
        h, w = cls._luma_size(y, bits)
        return cls((y, u, v), I444, matrix, h, w, container=bits, shift=shift)

    @classmethod
    def yuyv(cls, buf, matrix="bt601", w=None) -> "YUVFrame":
        """The one plane of a YUYV (YUY2) frame: uint8 [h, 4 cw] (bytes Y0 U Y1 V per pixel pair), or [h, w, 2] for even w.  The
        width is 2 cw unless `w` says that the last pair's second pixel is not part of the frame (w = 2 cw - 1)."""
        return cls._packed(buf, _lib.YUV_YUYV, matrix, w)

    @classmethod
    def uyvy(cls, buf, matrix="bt601", w=None) -> "YUVFrame":
        """The one plane of a UYVY frame: as `yuyv`, bytes U Y0 V Y1 per pixel pair."""
        return cls._packed(buf, _lib.YUV_UYVY, matrix, w)

    @classmethod
    def _packed(cls, buf, fmt, matrix, w):
        shape = tuple(buf.__cuda_array_interface__["shape"]) if _lib.is_device_array(buf) else np.asarray(buf).shape
        if len(shape) == 3 and shape[2] == 2 and shape[1] % 2 == 0:
            full = int(shape[1])
        elif len(shape) == 2 and shape[1] % 4 == 0 and shape[1] > 0:
            full = int(shape[1]) // 2
        else:
            raise ValueError(f"{_NAMES[fmt]} plane must be uint8 [h, 4 cw] or [h, w, 2] with even w, got shape {shape}")
        w = full if w is None else int(w)
        if w not in (full, full - 1):
            raise ValueError(f"a {_NAMES[fmt]} plane of {2 * full} bytes per row holds a frame {full - 1} or {full} wide, got w = {w}")
        return cls((buf,), fmt, matrix, int(shape[0]), w)

    @staticmethod
    def _luma_size(y, bits=8):
        dev = _lib.is_device_array(y)
        shape = tuple(y.__cuda_array_interface__["shape"]) if dev else np.asarray(y).shape
        if len(shape) != 2:
            raise ValueError(f"Y plane must be uint{bits} [h,w], got shape {shape}")
        h, w = int(shape[0]), int(shape[1])
        if bits == 16 and (y.__cuda_array_interface__["typestr"] if dev else np.asarray(y).dtype.str) in ("|u1", "<u1", "=u1"):
            if w % 2:
                raise ValueError(f"Y plane: a row of 16-bit samples handed in as bytes is even, got {w} bytes")
            w //= 2
        return h, w

    @classmethod
    def from_buffer(cls, buf, h: int, w: int, format="nv12", pitch=None, matrix="bt601") -> "YUVFrame":
        """A decoder's single allocation: h rows of luma at `pitch` bytes, then the chroma rows.  NV12: (h + 1) // 2 interleaved
        rows at the same pitch.  I420: the U rows and then the V rows at (pitch + 1) // 2 bytes.  YUYV (YUY2) / UYVY: h rows of
        4 * ((w + 1) // 2) bytes at `pitch` and nothing else.  Without `pitch` the planes are
        tight: every row is followed by the next.  `buf` is anything with
        the buffer interface (bytes, a memoryview, a uint8 array), or a contiguous uint8 DEVICE array (the decoder's surface in
        device memory: the frame is then `on_device`); it is not copied."""
        if isinstance(format, str) and format.lower() in FORMATS_EXT:
            return cls._from_buffer_ext(buf, int(h), int(w), format.lower(), pitch, matrix)
        fmt = _code(FORMATS, format, "format")
        h, w = int(h), int(w)
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"frame is {h} x {w}: sides must be 1..{MAX_SIDE}")
        dev = None
        writable = _array_writable(buf) if _lib.is_device_array(buf) or isinstance(buf, np.ndarray) else not memoryview(buf).readonly
        if _lib.is_device_array(buf):
            dev = _lib.device_view(buf, "buffer")
            size, acc = int(np.prod(dev.shape, dtype=np.int64)), 1
            for n, st in zip(reversed(dev.shape), reversed(dev.strides)):
                if n > 1 and st != acc:
                    raise ValueError("buffer must be contiguous")
                acc *= n
        else:
            a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
            if a.dtype != np.uint8:
                raise ValueError(f"buffer must hold uint8, got {a.dtype}")
            a = a.reshape(-1) if a.flags.c_contiguous else None
            if a is None:
                raise ValueError("buffer must be contiguous")
            size = a.size
        ch, cw = (h + 1) // 2, (w + 1) // 2

        def view(off, rows, row_bytes, p):
            if dev is not None:
                return _lib.DeviceView(dev.ptr + off, (rows, row_bytes), (p, 1), dev.owner)
            return np.lib.stride_tricks.as_strided(a[off:], (rows, row_bytes), (p, 1), writeable=False)

        if fmt in PACKED:
            row = 4 * cw
            pitch = row if pitch is None else int(pitch)
            if pitch < row:
                raise ValueError(f"pitch {pitch} is below a row of the {h} x {w} frame ({row} bytes)")
            need = pitch * (h - 1) + row
            if size < need:
                raise ValueError(f"buffer holds {size} bytes, the frame needs {need} in format {_NAMES[fmt]} ({h} rows of {row} bytes, "
                                 f"2 per pixel, at pitch {pitch})")
            return cls([view(0, h, row, pitch)], fmt, matrix, h, w, _writable=writable)
        crow = 2 * cw if fmt == _lib.YUV_NV12 else cw
        if pitch is None:               # tight: every plane's pitch is its row
            pitch, cpitch = w, crow
        else:
            pitch = int(pitch)
            cpitch = pitch if fmt == _lib.YUV_NV12 else (pitch + 1) // 2
        if pitch < w or cpitch < crow:
            raise ValueError(f"pitch {pitch} is below a row of the {h} x {w} frame")
        nchroma = 1 if fmt == _lib.YUV_NV12 else 2
        need = pitch * h + (nchroma * ch - 1) * cpitch + crow      # (the last row ends with its last sample)
        if size < need:
            raise ValueError(f"buffer holds {size} bytes, the frame needs {need}")
        planes = [view(0, h, w, pitch)]
        for i in range(nchroma):
            planes.append(view(pitch * h + i * cpitch * ch, ch, crow, cpitch))
        return cls(planes, fmt, matrix, h, w, _writable=writable)

    @classmethod
    def _from_buffer_ext(cls, buf, h, w, name, pitch, matrix):
        """`from_buffer` for the names of FORMATS_EXT.  `pitch` is in BYTES: the luma rows' and, NV12-like, the interleaved rows';
        I420-like chroma rows lie at the even pitch 2 * ceil(pitch / 4) (8-bit: (pitch + 1) // 2); every 4:4:4 plane at `pitch`."""
        layout, bits, shift = FORMATS_EXT[name]
        bs = bits // 8
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"frame is {h} x {w}: sides must be 1..{MAX_SIDE}")
        writable = _array_writable(buf) if _lib.is_device_array(buf) or isinstance(buf, np.ndarray) else not memoryview(buf).readonly
        dev = a = None
        if _lib.is_device_array(buf):
            dev = _device_bytes(buf, "buffer", bits == 16)
            size, acc = int(np.prod(dev.shape, dtype=np.int64)), 1
            for n, st in zip(reversed(dev.shape), reversed(dev.strides)):
                if n > 1 and st != acc:
                    raise ValueError("buffer must be contiguous")
                acc *= n
        else:
            a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
            if not a.flags.c_contiguous:
                raise ValueError("buffer must be contiguous")
            if a.dtype == np.dtype("<u2") and bits == 16:
                a = a.reshape(-1).view(np.uint8)
            if a.dtype != np.uint8:
                raise ValueError(f"buffer must hold uint8{' or uint16' if bits == 16 else ''}, got {a.dtype}")
            a = a.reshape(-1)
            size = a.size
        ch, cw = (h + 1) // 2, (w + 1) // 2
        row = w * bs
        if layout == I444:
            crow, crows, nchroma = row, h, 2
        elif layout == _lib.YUV_NV12:
            crow, crows, nchroma = 2 * cw * bs, ch, 1
        else:
            crow, crows, nchroma = cw * bs, ch, 2
        if pitch is None:
            pitch, cpitch = row, crow
        else:
            pitch = int(pitch)
            cpitch = pitch if layout != _lib.YUV_I420 else ((pitch + 1) // 2 if bs == 1 else 2 * ((pitch + 3) // 4))
        if pitch < row or cpitch < crow:
            raise ValueError(f"pitch {pitch} is below a row of the {h} x {w} frame ({row} bytes)")
        if bs == 2 and pitch % 2:
            raise ValueError(f"pitch {pitch}: the rows of 16-bit samples lie an even number of bytes apart")
        need = pitch * h + (nchroma * crows - 1) * cpitch + crow
        if size < need:
            raise ValueError(f"buffer holds {size} bytes, the frame needs {need} in format {name}")

        def view(off, rows, row_bytes, p):
            if dev is not None:
                return _lib.DeviceView(dev.ptr + off, (rows, row_bytes), (p, 1), dev.owner)
            return np.lib.stride_tricks.as_strided(a[off:], (rows, row_bytes), (p, 1), writeable=False)

        planes = [view(0, h, row, pitch)] + [view(pitch * h + i * cpitch * crows, crows, crow, cpitch) for i in range(nchroma)]
        return cls(planes, layout, matrix, h, w, _writable=writable, container=bits, shift=shift)

    def descriptor_ext(self) -> "_lib.YuvxFrameC":
        """The whenet_yuvx_frame_t of this frame, whatever its format (it points into the planes: keep the frame alive)."""
        d = _lib.YuvxFrameC()
        for i, (a, p) in enumerate(zip(self.planes, self.pitches)):
            d.plane[i] = a.ptr if self.on_device else a.ctypes.data
            d.pitch[i] = p
        d.layout, d.container, d.shift, d.matrix, d.h, d.w = self.format, self.container, self.shift, self.matrix, self.h, self.w
        return d

    def descriptor(self):
        """The whenet_yuv_frame_t of this frame (it points into the planes: keep the frame alive while it is used); the
        whenet_yuvx_frame_t (`descriptor_ext()`) of a frame that `needs_ext`."""
        if self.needs_ext:
            return self.descriptor_ext()
        d = _lib.YuvFrameC()
        for i, (a, p) in enumerate(zip(self.planes, self.pitches)):
            d.plane[i] = a.ptr if self.on_device else a.ctypes.data
            d.pitch[i] = p
        d.format, d.matrix, d.h, d.w = self.format, self.matrix, self.h, self.w
        return d

    def to_bgr(self) -> np.ndarray:
        """uint8 [h,w,3] in B, G, R order: the frame `begin_yuv` builds on the device, computed on the host inside the library."""
        if self.on_device:
            raise ValueError("to_bgr() runs on the host and this frame's planes are in device memory: Handle.op_yuv_to_bgr_device([frame]) "
                             "converts them on the device")
        if self.needs_ext:
            return _lib.yuvx_to_bgr_host(self.descriptor_ext())
        return _lib.yuv_to_bgr_host(self.descriptor())
