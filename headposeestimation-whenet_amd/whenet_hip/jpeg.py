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


def header(h: int, w: int, quality: int = DEFAULT_QUALITY, sampling: str = "4:2:0") -> bytes:
    """The 629 bytes SOI..SOS of the stream of an h x w frame with the standard tables: they depend on (h, w, quality, sampling)
    only.  (An optimize=True stream carries its own, shorter, DHT segments.)"""
    return _lib.jpeg_header(h, w, quality, sampling)[0]


def quantisers(quality: int = DEFAULT_QUALITY) -> np.ndarray:
    """int32 [2,64]: the luminance and the chrominance quantiser at `quality`, natural order."""
    return _lib.jpeg_header(16, 16, quality)[1]


def bound(h: int, w: int, sampling: str = "4:2:0") -> int:
    """A capacity no stream of an h x w frame exceeds (`whenet_jpeg_bound_ex`); it does not depend on `optimize`."""
    return _lib.jpeg_bound(h, w, sampling)


def optimal_table(freq):
    """(bits uint8 [16], vals uint8 [n]): the Huffman table T.81 K.2 gives the symbol frequencies uint32 [256], ties broken as libjpeg
    breaks them (`whenet_jpeg_optimal_table`): what optimize=True builds from a frame's histograms."""
    return _lib.jpeg_optimal_table(freq)


def source_of(frame, what: str = "frame"):
    """A source frame -> (`_lib.SurfaceC`, h, w, the object that keeps its memory alive).  ValueError for anything that would need a
    copy: another dtype or shape, pixels that are not packed, planes in device memory."""
    s = _lib.SurfaceC()
    if isinstance(frame, YUVFrame):
        if frame.needs_ext:
            raise ValueError(f"{what}: a 16-bit, 4:4:4 or BT.2020 frame as an encoder source is not built")
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


def encode(frame, quality: int = DEFAULT_QUALITY, handle=None, bgr: bool = True, capacity=None, sampling: str = "4:2:0",
           optimize: bool = False, hist=None) -> bytes:
    """The stream of `frame`, written by the kernels (`whenet_op_jpeg_encode_ex`).  `handle`: a `WHENet` model or a `_lib.Handle`; None
    opens a postproc handle on device 0 for the call.  `capacity` (default: `bound(h, w, sampling)`) below the stream's length raises
    `CapacityError` with the needed size.  `sampling`: "4:2:0" (the default), "4:2:2" or "4:4:4" -- the last two take packed pixels
    only (a YUVFrame carries 4:2:0 chroma).  optimize=True: Huffman tables built on the device from the frame's own symbols -- the
    same pixels in a smaller stream; `hist`: a uint32 [4,256] array that receives the device histograms then."""
    s, h, w, _keep = source_of(frame)
    out = np.empty(bound(h, w, sampling) if capacity is None else int(capacity), np.uint8)
    if handle is None:
        with _lib.Handle.postproc(0) as own:
            rc, size = own.op_jpeg_encode(s, h, w, bgr, quality, out, sampling, optimize, hist)
    else:
        rc, size = _handle_of(handle).op_jpeg_encode(s, h, w, bgr, quality, out, sampling, optimize, hist)
    return _finish(rc, size, out)


def encode_host(frame, quality: int = DEFAULT_QUALITY, bgr: bool = True, capacity=None, sampling: str = "4:2:0", optimize: bool = False,
                hist=None) -> bytes:
    """The same stream by pure host arithmetic inside the library (`whenet_jpeg_encode_host_ex`, no GPU): the statement the kernels
    are held to."""
    s, h, w, _keep = source_of(frame)
    out = np.empty(bound(h, w, sampling) if capacity is None else int(capacity), np.uint8)
    rc, size = _lib.jpeg_encode_host(s, h, w, bgr, quality, out, sampling, optimize, hist)
    return _finish(rc, size, out)


# ---- the decoder: JPEG bytes in, a frame out (csrc/jpeg_dec.hip, include/whenet_hip.h JPEG DECODER) ----
class DecodeError(ValueError):
    """Damaged entropy data (status WHENET_EFORMAT): `interval` is the first bad restart interval -- for a progressive stream the
    first bad flat (scan, interval) item, or the item count where the progression is incomplete --, `frame` the fully defined frame
    the decoder still produced (damaged intervals end in zero coefficients)."""

    def __init__(self, interval: int, frame: np.ndarray):
        super().__init__(f"the JPEG stream is damaged from restart interval {interval} on")
        self.interval = int(interval)
        self.frame = frame


def add_default_tables(data) -> bytes:
    """The stream completed by the Huffman tables a UVC camera's or an AVI writer's MJPG frame leaves out
    (`whenet_jpeg_add_default_tables`): for each of the slots DC 0, AC 0, DC 1, AC 1 that no DHT in front of the first SOS defines,
    T.81's Annex K table (what libjpeg's std_huff_tables installs there), all in one DHT segment directly in front of that SOS, at
    most 420 bytes more.  A stream that defines all four comes back byte for byte, and so does anything whose header cannot be
    followed to an SOS: this never raises for a stream, the decoder gives its own reason.  Ids 2 and 3 are never filled."""
    return _lib.jpeg_add_default_tables(data)


def _completed(data, default_tables: bool):
    return _lib.jpeg_add_default_tables(data) if default_tables else data


def _parse(data, progressive, layouts):
    """the header of a stream by the parser the flags select (layouts: the ..._accept call)"""
    if layouts:
        return _lib.jpeg_parse_scans_accept(data, _lib.jpeg_accept_bits(progressive, True))[0]
    return _lib.jpeg_parse_scans(data)[0] if progressive else _lib.jpeg_parse(data)


def _auto_form(data, i, entropy, seg_bytes, decide: bool):
    """(entropy argument, seg_bytes argument) of the op calls; decide: "auto" is resolved here by the library's rule"""
    form, seg = _lib.JPEG_ENTROPY[entropy], 128 if seg_bytes is None else int(seg_bytes)
    if form == 2 and decide:
        form = 1 if (int(_lib._stream_array(data).size) - i.data_offset) // max(i.intervals, 1) >= _lib.JPEG_SEG_AUTO_BYTES else 0
    return (-1 if form == 2 else form), seg


def info(data, progressive: bool = False, default_tables: bool = False, layouts: bool = False) -> dict:
    """The header SOI..SOS of a stream (`whenet_jpeg_parse`): h, w, components, sampling (hs, vs), restart_interval, intervals,
    data_offset, the quantisers uint8 [4,64] in natural order and the table ids.  ValueError with the reason for anything but a
    baseline stream the decoder accepts (progressive, arithmetic, 12 bit, 4 components, several scans, ...).
    progressive=True (`whenet_jpeg_parse_scans`): a progressive (SOF2) stream is accepted too, and "scans" lists every scan as a
    dict: components, ss, se, ah, al, dc_ids, ac_ids, tables, ri, intervals, level, first_item, data_offset, data_bytes.
    default_tables=True: the header of `add_default_tables(data)` (offsets are that stream's).
    layouts=True (`whenet_jpeg_parse_scans_accept`): the samplings 4:4:0 (1, 2), 4:1:1 (4, 1) and 4:1:0 (4, 2) and a single-scan SOF1
    stream are accepted too; "scans" is listed as with progressive=True (a sequential stream: its one scan)."""
    data = _completed(data, default_tables)
    scans = None
    if progressive or layouts:
        i, recs = _lib.jpeg_parse_scans_accept(data, _lib.jpeg_accept_bits(progressive, True)) if layouts else _lib.jpeg_parse_scans(data)
        scans = [{"components": tuple(r.comp[:r.ns]), "ss": r.ss, "se": r.se, "ah": r.ah, "al": r.al, "dc_ids": tuple(r.dc[:r.ns]),
                  "ac_ids": tuple(r.ac[:r.ns]), "tables": r.tables, "ri": r.ri, "intervals": r.intervals, "level": r.level,
                  "first_item": r.first_item, "data_offset": r.data_offset, "data_bytes": r.data_bytes} for r in recs]
    else:
        i = _lib.jpeg_parse(data)
    out = {"h": i.h, "w": i.w, "components": i.components, "sampling": (i.hs, i.vs), "restart_interval": i.restart_interval,
           "intervals": i.intervals, "data_offset": i.data_offset, "quantisers": np.ctypeslib.as_array(i.q).copy(),
           "quantiser_ids": tuple(i.qt[:i.components]), "dc_ids": tuple(i.dc[:i.components]), "ac_ids": tuple(i.ac[:i.components])}
    if scans is not None:
        out["scans"] = scans
    return out


def orientation(data) -> int:
    """The EXIF orientation of a stream, 1..8 (`whenet_jpeg_orientation`): tag 0x0112 in IFD0 of the first Exif APP1 in front of SOS,
    either byte order, type SHORT or LONG.  1 for a stream without the tag and for any broken EXIF structure: it never raises."""
    return _lib.jpeg_orientation(data)


def oriented_shape(h: int, w: int, value: int):
    """(rows, columns) of the oriented frame of an h x w stream: the sides swap for the values 5..8."""
    return (w, h) if value >= 5 else (h, w)


def packed_surface(frame: np.ndarray) -> "_lib.SurfaceC":
    """A uint8 [H,W,3] host array whose rows' pixels are packed (any row stride) as a destination surface."""
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0] = frame.ctypes.data, int(frame.strides[0]) if frame.shape[0] > 1 else 3 * frame.shape[1]
    s.format, s.matrix, s.on_device = _lib.SURF_PACKED, 0, 0
    return s


def _result(frame: np.ndarray, status: np.ndarray, strict: bool):
    if strict and status[0] != _lib.OK:
        raise DecodeError(int(status[1]), frame)
    return frame


def _run_decode(handle, data, frame, bgr, entropy, seg_bytes, rule, progressive, orient):
    """(status, statistics) of `whenet_op_jpeg_decode_oriented` into `frame`; handle None: a postproc handle on device 0 for the call"""
    if handle is None:
        with _lib.Handle.postproc(0) as own:
            return own.op_jpeg_decode_oriented(data, packed_surface(frame), bgr, entropy, seg_bytes, rule, progressive, orient)[:2]
    return _handle_of(handle).op_jpeg_decode_oriented(data, packed_surface(frame), bgr, entropy, seg_bytes, rule, progressive, orient)[:2]


def decode(data, handle=None, bgr: bool = True, strict: bool = True, entropy: str = "auto", seg_bytes=None, stats: bool = False,
           rule: str = "own", progressive: bool = False, orient: bool = False, default_tables: bool = False, layouts: bool = False):
    """uint8 [H,W,3] (B, G, R order unless bgr=False): the frame of a baseline JPEG stream, decoded by the kernels
    (`whenet_op_jpeg_decode`).  `handle`: a `WHENet` model or a `_lib.Handle`; None opens a postproc handle on device 0 for the call.
    Damaged data raises `DecodeError` (strict=False: returns the defined frame).  `entropy`: the form of the entropy stage --
    "interval" (one restart interval per lane: a stream without restart markers is one lane, correct and slow), "segmented" (every
    interval by many lanes, `seg_bytes` of the data each: a power of two in 4..4096, None = 128) or "auto" (the handle's options
    "jpeg_entropy" / "jpeg_seg_bytes": by default segmented from 4096 bytes per interval on).  The frame is the same, bit for bit.
    stats=True: (frame, the statistics int64 [8] of `whenet_op_jpeg_decode_ex`); with "auto" the form is then chosen here by the
    same rule.  `rule`: "own" (the project's inverse DCT, nearest chroma, JFIF row: the default) or "libjpeg" (the bytes of a
    libjpeg-turbo decode with its defaults: what `cv2.imread` and Pillow give; `whenet_op_jpeg_decode_rule`).  "own" goes through
    the calls that read the handle's option "jpeg_rule", whose default it is.  progressive=True also accepts a progressive (SOF2)
    stream (`whenet_op_jpeg_decode_progressive`; `DecodeError.interval` is then the flat (scan, interval) item, and stats are items,
    levels, scans, scan-kernel launches); `entropy` and `seg_bytes` apply where the stream is baseline and are ignored otherwise.
    orient=True (`whenet_op_jpeg_decode_oriented`): the stream's EXIF orientation (`orientation(data)`) is applied by the frame kernel
    itself, as `cv2.imread` applies it: the frame is `decode_host(data, orient=True, ...)`, its sides swapped for the values 5..8.
    orient=False is an upright decode on every handle: every path here goes through that call with `orient` stated, so the handle's
    option "jpeg_orient" (which the plain C calls read) never turns a frame this function sized upright.
    default_tables=True: `add_default_tables(data)` is decoded in its place (an MJPG frame without DHT; refused otherwise).
    layouts=True (`whenet_op_jpeg_decode_accept`): 4:4:0, 4:1:1 and 4:1:0 streams and single-scan SOF1 streams are accepted too
    (include/whenet_hip.h, JPEG DECODER, LAYOUTS); the frame is `decode_host(data, layouts=True, ...)` in either entropy form.
    With False, the default, the call is what it was and refuses them on every handle: the header is parsed here first, without the
    bit, so the handle's option "jpeg_layouts" (which the plain C calls read) does not reach this function."""
    data = _completed(data, default_tables)
    if entropy not in _lib.JPEG_ENTROPY:
        raise ValueError("entropy must be 'auto', 'interval' or 'segmented'")
    _lib.jpeg_rule_code(rule)
    if layouts:
        i = _parse(data, progressive, True)
        frame = np.empty((oriented_shape(i.h, i.w, orientation(data)) if orient else (i.h, i.w)) + (3,), np.uint8)
        form, seg = _auto_form(data, i, entropy, seg_bytes, stats or seg_bytes is not None)
        accept = _lib.jpeg_accept_bits(progressive, True)
        def run(h):
            return h.op_jpeg_decode_accept(data, packed_surface(frame), bgr, form, seg, rule, accept, bool(orient))[:2]
        if handle is None:
            with _lib.Handle.postproc(0) as own:
                status, st = run(own)
        else:
            status, st = run(_handle_of(handle))
        out = _result(frame, status, strict)
        return (out, st) if stats else out
    if orient:
        i = _lib.jpeg_parse_scans(data)[0] if progressive else _lib.jpeg_parse(data)
        frame = np.empty(oriented_shape(i.h, i.w, orientation(data)) + (3,), np.uint8)
        form, seg = _lib.JPEG_ENTROPY[entropy], 128 if seg_bytes is None else int(seg_bytes)
        if form == 2 and seg_bytes is not None:
            form = 1 if (int(_lib._stream_array(data).size) - i.data_offset) // max(i.intervals, 1) >= _lib.JPEG_SEG_AUTO_BYTES else 0
        status, st = _run_decode(handle, data, frame, bgr, -1 if form == 2 else form, seg, rule, bool(progressive), True)
        out = _result(frame, status, strict)
        return (out, st) if stats else out
    if progressive:
        i, scans = _lib.jpeg_parse_scans(data)
        if scans[0].progressive:      # a SOF2 stream
            frame = np.empty((i.h, i.w, 3), np.uint8)
            status, st = _run_decode(handle, data, frame, bgr, -1, 128, rule, True, False)      # (what whenet_op_jpeg_decode_progressive runs)
            out = _result(frame, status, strict)
            return (out, st) if stats else out
    i = _lib.jpeg_parse(data)
    frame = np.empty((i.h, i.w, 3), np.uint8)
    form, seg = _lib.JPEG_ENTROPY[entropy], 128 if seg_bytes is None else int(seg_bytes)
    if form == 2 and (stats or seg_bytes is not None):
        form = 1 if (int(_lib._stream_array(data).size) - i.data_offset) // max(i.intervals, 1) >= _lib.JPEG_SEG_AUTO_BYTES else 0

    # (rule "own" and SOF2 are left to the handle's options "jpeg_rule" / "jpeg_progressive", as whenet_op_jpeg_decode[_ex] leave them)
    status, st = _run_decode(handle, data, frame, bgr, -1 if form == 2 else form, seg, None if rule == "own" else rule, None, False)
    out = _result(frame, status, strict)
    return (out, st) if stats else out


def decode_clip(datas, bgr: bool = True, entropy=None, seg_bytes=None, handle=None, strict: bool = True, rule: str = "own",
                progressive: bool = False, orient: bool = False, default_tables: bool = False, layouts: bool = False):
    """(frames, statuses) of 1..16 baseline JPEG streams decoded as ONE clip by the kernels (`whenet_op_jpeg_decode_clip`): a list of
    uint8 [H_f,W_f,3] frames and the status words int32 [F,2].  Frame f is `decode(datas[f])`, bit for bit.  `entropy`: None or
    "auto" (the handle's options, stream by stream), "interval" or "segmented" (`seg_bytes`: None = 128).  A stream the decoder does
    not accept is a ValueError that names the frame; a damaged one raises `DecodeError` with the frame's index in its text
    (strict=False: its defined frame and status are returned with the others).  `rule`: "own" or "libjpeg", as `decode`.
    progressive=True (`whenet_op_jpeg_decode_clip_progressive`): progressive (SOF2) streams are accepted too, alone or next to
    baseline ones -- a folder of stills as one clip.  Frame f is then `decode_host(datas[f], rule=rule, progressive=True)` with its
    status; the scan kernel is launched once per level for all progressive frames together, and `entropy` / `seg_bytes` apply to
    the baseline frames.  The handle's option "jpeg_progressive" is not read by clips: only this argument accepts SOF2.
    orient=True (`whenet_op_jpeg_decode_clip_oriented`): every frame by its own EXIF orientation -- frame f is
    `decode_host(datas[f], orient=True, ...)` --, upright and turned frames in one clip, at most one launch more than without.
    default_tables=True: every stream is completed by `add_default_tables` first.
    layouts=True (`whenet_op_jpeg_decode_clip_accept`): the streams `decode(..., layouts=True)` accepts may be frames of the clip;
    frame f is `decode_host(datas[f], layouts=True, ...)`.  Clips do not read the handle's option "jpeg_layouts"."""
    _lib.jpeg_rule_code(rule)
    if entropy is not None and entropy not in _lib.JPEG_ENTROPY:
        raise ValueError("entropy must be None, 'auto', 'interval' or 'segmented'")
    datas = [_completed(d, default_tables) for d in datas]
    if not 1 <= len(datas) <= _lib.MAX_CLIP_FRAMES:
        raise ValueError(f"a clip holds 1..{_lib.MAX_CLIP_FRAMES} frames, got {len(datas)}")
    frames = []
    for f, d in enumerate(datas):
        try:
            i = _parse(d, progressive, layouts)
        except ValueError as e:
            raise ValueError(f"decode_clip: frame {f}: {e}") from None
        frames.append(np.empty((oriented_shape(i.h, i.w, orientation(d)) if orient else (i.h, i.w)) + (3,), np.uint8))
    form = -1 if entropy in (None, "auto") else _lib.JPEG_ENTROPY[entropy]
    seg = 128 if seg_bytes is None else int(seg_bytes)
    surfaces = [packed_surface(fr) for fr in frames]
    def run(h):
        if layouts:
            return h.op_jpeg_decode_clip_accept(datas, surfaces, bgr, form, seg, rule, _lib.jpeg_accept_bits(progressive, True), bool(orient))[0]
        if orient:
            return h.op_jpeg_decode_clip_oriented(datas, surfaces, bgr, form, seg, rule, bool(progressive), True)[0]
        if progressive:
            return h.op_jpeg_decode_clip_progressive(datas, surfaces, bgr, form, seg, rule)
        if rule != "own":
            return h.op_jpeg_decode_clip_rule(datas, surfaces, bgr, form, seg, rule)
        return h.op_jpeg_decode_clip(datas, surfaces, bgr, form, seg)

    if handle is None:
        with _lib.Handle.postproc(0) as own:
            status = run(own)
    else:
        status = run(_handle_of(handle))
    if strict:
        for f in range(len(frames)):
            if status[f, 0] != _lib.OK:
                e = DecodeError(int(status[f, 1]), frames[f])
                e.args = (f"frame {f}: {e.args[0]}",)
                e.index = f
                raise e
    return frames, status


def decode_host(data, bgr: bool = True, strict: bool = True, rule: str = "own", progressive: bool = False, orient: bool = False,
                default_tables: bool = False, layouts: bool = False) -> np.ndarray:
    """The same frame by pure host arithmetic inside the library (`whenet_jpeg_decode_host`, no GPU): the statement the kernels are
    held to.  `rule`: "own" or "libjpeg", as `decode` (`whenet_jpeg_decode_rule_host`).  progressive=True: a progressive (SOF2)
    stream is accepted too (`whenet_jpeg_decode_progressive_host`).  orient=True (`whenet_jpeg_decode_oriented_host`): the EXIF
    orientation applied to that frame -- with u the upright frame and t = u.transpose(1, 0, 2): 1 u, 2 u[:, ::-1], 3 u[::-1, ::-1],
    4 u[::-1], 5 t, 6 t[:, ::-1], 7 t[::-1, ::-1], 8 t[::-1].  default_tables=True: `add_default_tables(data)` is decoded in its place.
    layouts=True (`whenet_jpeg_decode_accept_host`): 4:4:0, 4:1:1, 4:1:0 and single-scan SOF1 streams are accepted too."""
    data = _completed(data, default_tables)
    _lib.jpeg_rule_code(rule)
    if layouts:
        i = _parse(data, progressive, True)
        frame = np.empty((oriented_shape(i.h, i.w, orientation(data)) if orient else (i.h, i.w)) + (3,), np.uint8)
        status = _lib.jpeg_decode_accept_host(data, packed_surface(frame), bgr, rule, _lib.jpeg_accept_bits(progressive, True), orient)[0]
        return _result(frame, status, strict)
    if orient:
        i = _lib.jpeg_parse_scans(data)[0] if progressive else _lib.jpeg_parse(data)
        frame = np.empty(oriented_shape(i.h, i.w, orientation(data)) + (3,), np.uint8)
        return _result(frame, _lib.jpeg_decode_oriented_host(data, packed_surface(frame), bgr, rule, progressive), strict)
    if progressive:
        i = _lib.jpeg_parse_scans(data)[0]
        frame = np.empty((i.h, i.w, 3), np.uint8)
        return _result(frame, _lib.jpeg_decode_progressive_host(data, packed_surface(frame), bgr, rule), strict)
    i = _lib.jpeg_parse(data)
    frame = np.empty((i.h, i.w, 3), np.uint8)
    if rule != "own":
        return _result(frame, _lib.jpeg_decode_rule_host(data, packed_surface(frame), bgr, rule), strict)
    return _result(frame, _lib.jpeg_decode_host(data, packed_surface(frame), bgr), strict)


def decode_segmented_host(data, seg_bytes: int = 128, window: int = _lib.JPEG_SEG_WINDOW, bgr: bool = True, strict: bool = True,
                          stats: bool = False, rule: str = "own", layouts: bool = False):
    """`decode_host` with the entropy stage run as the host emulation of the segmented form (`whenet_jpeg_decode_segmented_host`):
    segments of `seg_bytes`, sync windows of `window` segments, lanes in a plain loop.  The same frame, bit for bit.
    stats=True: (frame, status int32 [2], statistics int64 [8]) and damaged data does not raise.  `rule`: as `decode_host`.
    layouts=True (`whenet_jpeg_decode_segmented_accept_host`): as `decode_host`."""
    _lib.jpeg_rule_code(rule)
    i = _parse(data, False, layouts)
    frame = np.empty((i.h, i.w, 3), np.uint8)
    if layouts:
        status, st = _lib.jpeg_decode_segmented_accept_host(data, packed_surface(frame), bgr, seg_bytes, window, rule, _lib.JPEG_ACCEPT_LAYOUTS)
    elif rule != "own":
        status, st = _lib.jpeg_decode_segmented_rule_host(data, packed_surface(frame), bgr, seg_bytes, window, rule)
    else:
        status, st = _lib.jpeg_decode_segmented_host(data, packed_surface(frame), bgr, seg_bytes, window)
    if stats:
        return frame, status, st
    return _result(frame, status, strict)


def decode_segmented_planes_host(data, seg_bytes: int = 128, window: int = _lib.JPEG_SEG_WINDOW, layouts: bool = False):
    """`decode_planes_host` by the segmented form's host emulation: (planes, status int32 [2], statistics int64 [8]).  layouts=True
    (`whenet_jpeg_decode_segmented_accept_planes_host`): as `decode_host`."""
    i = _parse(data, False, layouts)
    shapes = [(i.h, i.w)] + [((i.h + i.vs - 1) // i.vs, (i.w + i.hs - 1) // i.hs)] * (i.components - 1)
    planes = [np.empty(s, np.uint8) for s in shapes]
    if layouts:
        status, st = _lib.jpeg_decode_segmented_accept_planes_host(data, planes, seg_bytes, window, "own", _lib.JPEG_ACCEPT_LAYOUTS)
        return planes, status, st
    status, st = _lib.jpeg_decode_segmented_planes_host(data, planes, seg_bytes, window)
    return planes, status, st


def decode_planes_host(data, progressive: bool = False, rule: str = "own", default_tables: bool = False, layouts: bool = False):
    """(the component planes [Y] or [Y, Cb, Cr] as uint8 arrays -- luma h x w, chroma ceil(h / vs) x ceil(w / hs) -- and the status
    int32 [2]) by the host statement: what the tests compare.  progressive=True: a progressive stream is accepted too, and `rule`
    chooses the inverse DCT (`whenet_jpeg_decode_progressive_planes_host`).  default_tables=True: `add_default_tables(data)` is
    decoded in its place.  layouts=True (`whenet_jpeg_decode_accept_planes_host`): as `decode_host`; `rule` applies either way."""
    data = _completed(data, default_tables)
    _lib.jpeg_rule_code(rule)
    if layouts:
        i = _parse(data, progressive, True)
        shapes = [(i.h, i.w)] + [((i.h + i.vs - 1) // i.vs, (i.w + i.hs - 1) // i.hs)] * (i.components - 1)
        planes = [np.empty(s, np.uint8) for s in shapes]
        return planes, _lib.jpeg_decode_accept_planes_host(data, planes, rule, _lib.jpeg_accept_bits(progressive, True))
    i = _lib.jpeg_parse_scans(data)[0] if progressive else _lib.jpeg_parse(data)
    if rule != "own" and not progressive:
        raise ValueError("decode_planes_host: the planes of rule 'libjpeg' come from the progressive=True call (which takes baseline streams too)")
    shapes = [(i.h, i.w)] + [((i.h + i.vs - 1) // i.vs, (i.w + i.hs - 1) // i.hs)] * (i.components - 1)
    planes = [np.empty(s, np.uint8) for s in shapes]
    if progressive:
        return planes, _lib.jpeg_decode_progressive_planes_host(data, planes, rule)
    status = _lib.jpeg_decode_planes_host(data, planes)
    return planes, status
