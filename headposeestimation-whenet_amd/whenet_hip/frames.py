"""Per-frame driver for video callers: all heads of a frame in ONE submission, overlapped with the
caller's next detection.

The reference's video loop (/root/reference/demo_video.py:49-63) runs, per frame, YOLO on the host
and then `process_detection` once per head, sequentially: bbox margins (13-19), numpy slice (21),
cv2.cvtColor (22), cv2.resize to 224x224 (23) and a batch-1 `get_angle` (27).  Here

  * the margin arithmetic runs once per frame inside the library (`whenet_frame_rects`);
  * the frame crosses PCIe once (pinned staging copy + async H2D) and every head is cropped /
    BGR->RGB-swapped / resized by one kernel straight into the forward's input (`csrc/frame.hip`,
    bit-exact with OpenCV's generic fixed-point INTER_LINEAR as restated in the oracle);
  * the k heads go through the network as ONE batch;
  * `submit()` returns as soon as the work is enqueued, so the caller can run the detector on the
    next frame while this one is on the GPU; `collect()` returns results in submission order;
  * a caller that also wants the DETECTOR's input from the GPU uses the resident form: `begin(frame)`
    uploads the frame once, `detector_input()` returns the `image_data` of YOLO.detect
    (yolo_postprocess.py:186-196: Pillow-BICUBIC letterbox and /255, `csrc/letterbox.hip`, bit-exact),
    `heads(bboxes)` enqueues what `submit()` enqueues without copying the frame again;
  * with a detector attached to the model's handle (`whenet_hip.detector.YOLO(handle=model, ...)`), `detect()` between
    `begin` and `heads` runs YOLO.detect itself on that device copy -- letterbox, Darknet body, box selection -- and
    returns the boxes: a frame goes in, head boxes and head poses come out, with one library;
  * `detect_heads()` takes the place of `detect()` + `heads()`: the boxes stay on the device, a kernel turns them into windows and
    crop plans (`csrc/headplan.hip`), and the call returns as soon as everything is enqueued -- `begin; detect_heads; collect`
    is one submission per frame, so with `depth` > 1 the next frame is begun and detected while this one is on the GPU;
  * a caller that has the next frames in hand (a video file, a rig of identical cameras) sends a CLIP: `begin_clip(frames)`,
    `detect_heads_clip()`, `collect_clip()` put F frames of one size through letterbox, detector, selection, head plans, crops
    and pose as one submission.  The heads that have a window are compacted on the device, so the forward runs over
    `max_heads` rows, not over F x max_boxes; every frame's result is bit for bit what `begin; detect_heads; collect` returns;
  * frames of DIFFERENT sizes (a rig of different cameras, several files behind one handle) travel as a clip too:
    `begin_clip_mixed(frames)` in the place of `begin_clip`, the other two calls and the contract unchanged;
  * a caller fed by a video decoder hands over its 4:2:0 planes or a camera's packed 4:2:2 frame (`whenet_hip.yuv.YUVFrame`: NV12, I420, YUYV or UYVY) with `begin_yuv(frame)`
    / `begin_clip_yuv(frames)`: half the bytes cross PCIe and the BGR frame is built on the device (`csrc/yuv.hip`); everything
    that follows is what `begin(frame.to_bgr())` / `begin_clip...` would have been followed by, bit for bit.

  * a frame that is ALREADY in device memory -- a hardware decoder's surface, a torch-ROCm tensor, a CuPy array: anything that
    exposes `__cuda_array_interface__` -- goes to the same calls: `begin(tensor, stream=...)`, `begin_clip`, `begin_clip_mixed`,
    and `begin_yuv` / `begin_clip_yuv` with a `YUVFrame` whose planes are device arrays.  One kernel (`csrc/ingest.hip`,
    `csrc/yuv.hip`) reads it where it is, with its row pitch, ordered on the caller's stream: no host copy, no PCIe, no host
    wait, and the same results bit for bit.  A device frame is never copied to make it fit: uint8 [H,W,3] with inner strides
    (3, 1) or a ValueError.  10-bit and 4:4:4 surfaces (P010 / P016, yuv420p10le,
    I444; `whenet_hip.yuv`) go through the same two calls.  Not built: BGRA / 4-channel, float or CHW tensors, memory of another GPU.

Only numpy and the C ABI are used (no torch, no cv2); there is no CPU fallback.
"""
from __future__ import annotations

from collections import deque
from typing import Deque, Tuple

import numpy as np

from . import _lib

MAX_INFLIGHT = 4          # WHENET_MAX_INFLIGHT
_CLIP = "clip"            # in the place of a pending entry's rects: the entry is (ticket, _CLIP, (frames, slots per frame))


def clip_slots(size, anchors, num_classes: int, max_boxes: int) -> int:
    """K of a clip: the detection slots per frame = num_classes x max_boxes, max_boxes cut to the number of boxes the detector's maps
    hold for the input `size` (3 per cell, one map per three anchors, the coarsest 32 x smaller than the input)."""
    if int(max_boxes) < 1:
        raise ValueError("max_boxes must be >= 1")
    layers = len(np.asarray(anchors).reshape(-1, 2)) // 3
    held = sum(((int(size[0]) // 32) << l) * ((int(size[1]) // 32) << l) * 3 for l in range(layers))
    return int(num_classes) * min(int(max_boxes), max(held, 1))


def scatter_clip(counts, boxes, scores, classes, rects, valid, row, ypr, detections: bool = False):
    """The per-frame results of a clip from its slot arrays ([F,K,...] as `Handle.collect_clip` returns them): for frame f a tuple
    shaped like `collect()` -- (rects [k,4], yaw, pitch, roll) of the heads among its first counts[f] slots that have a window
    (valid) AND a forward row (row >= 0) -- and with `detections` also (boxes [n,4], scores [n], classes [n], valid [n]) of all
    n = counts[f] detections."""
    out = []
    for f, n in enumerate(np.asarray(counts).tolist()):
        keep = (valid[f, :n] != 0) & (row[f, :n] >= 0)
        y = ypr[f, :n][keep]
        res = (np.ascontiguousarray(rects[f, :n][keep]), y[:, 0].copy(), y[:, 1].copy(), y[:, 2].copy())
        if detections:
            res += (boxes[f, :n].copy(), scores[f, :n].copy(), classes[f, :n].copy(), valid[f, :n].copy())
        out.append(res)
    return out


class JpegFrame:
    """The JPEG stream of one annotated frame (`FramePipeline.annotate_jpeg`): `width`, `height`; `tobytes()` after the frame's
    collect call.  It owns the memory the library writes into."""

    def __init__(self, width: int, height: int, capacity: int):
        if capacity < 0:
            raise ValueError(f"capacity must not be negative, got {capacity}")
        self.width, self.height = width, height
        self._out = np.empty(capacity, np.uint8)
        self._result = np.zeros(2, np.int64)       # the stream's length; the status (an int32 in the first half)
        self._done = False

    @property
    def ready(self) -> bool:
        return self._done

    def tobytes(self) -> bytes:
        if not self._done:
            raise ValueError("JpegFrame.tobytes(): the frame is not collected yet (collect() / collect_clip() first)")
        size, status = int(self._result[0]), int(self._result[1:].view(np.int32)[0])
        if status == _lib.EOVERFLOW:
            raise _lib.CapacityError(size, f"the JPEG stream has {size} bytes, the capacity is {self._out.size}")
        return self._out[:size].tobytes()


class JpegStatus:
    """What the decoder says about the stream of one `FramePipeline.begin_jpeg` frame, after the frame's collect call: `ok`, and
    `interval` = the first damaged restart interval (-1: none).  A damaged stream still gives a fully defined frame.  It owns the
    memory the library writes into."""

    def __init__(self):
        self._status = np.zeros(2, np.int32)
        self._done = False
        self._orientation = 1

    @property
    def orientation(self) -> int:
        """The EXIF orientation that was applied to the frame, 1..8 (1 where the decode was not an oriented one)."""
        return self._orientation

    @property
    def ready(self) -> bool:
        return self._done

    def _read(self, i: int) -> int:
        if not self._done:
            raise ValueError("JpegStatus: the frame is not collected yet (collect() first)")
        return int(self._status[i])

    @property
    def ok(self) -> bool:
        return self._read(0) == _lib.OK

    @property
    def interval(self) -> int:
        return self._read(1)


class FramePipeline:
    """`with FramePipeline(model) as fp:` ... `fp.submit(frame_bgr, bboxes)` ... `fp.collect()`.

    `model` is a `whenet.WHENet`; `bboxes` is what `YOLO.detect` returns first: float32 [k,4] rows
    (y_min, x_min, y_max, x_max) in frame pixels.  `collect()` returns
    `(rects, yaw, pitch, roll)`: rects int32 [k,4] = the enlarged windows (y0, x0, y1, x1) that
    demo_video.py:25,29 also needs for drawing, and three float32 (k,) arrays as `get_angle`
    returns them."""

    def __init__(self, model, depth: int = 2, bgr: bool = True):
        if not 1 <= depth <= MAX_INFLIGHT:
            raise ValueError(f"depth must be 1..{MAX_INFLIGHT}")
        self._h = model._handle
        # `depth` frames in flight = `depth` engines behind the handle (own streams / arena / graphs):
        # frame i+1's staging, crop and forward overlap frame i's on the GPU
        self._h.set_option("inflight", min(depth, 4))
        self._depth = depth
        self._bgr = bool(bgr)
        self._pending: Deque[Tuple[int, object, int]] = deque()      # (ticket, rects, 0) or, from detect_heads, (ticket, None, capacity)
        self._detector = None
        self._begun = None         # (ticket, frame_h, frame_w) of the frame begun last, until its heads are enqueued
        self._begun_clip = None    # (ticket, frames) of the clip begun last, until detect_heads_clip
        self._last_sizes = None    # (h, w) of every frame of the submission begun last: what annotate() checks its destination against
        self._annotated = None     # the ticket annotated last

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._begun is not None:            # a frame without heads: released as a frame with none
            self.heads(np.zeros((0, 4), np.float32))
        if self._begun_clip is not None:       # a clip without heads: released the same way
            ticket = self._begun_clip[0]
            self._begun_clip = None
            self._h.frame_heads(ticket, np.zeros((0, 4), np.int32))
            self._pending.append((ticket, np.zeros((0, 4), np.int32), 0))
        while self._pending:
            if self._pending[0][1] is _CLIP:
                self.collect_clip()
            else:
                self.collect()

    @property
    def in_flight(self) -> int:
        return len(self._pending)

    def submit(self, frame: np.ndarray, bboxes) -> None:
        """Enqueue one frame; raises ValueError if `depth` frames are already in flight
        (collect one first) or if a box degenerates to an empty window (cv2.resize would raise)."""
        if len(self._pending) >= self._depth:
            raise ValueError(f"{self._depth} frames already in flight: collect() first")
        frame = np.asarray(frame)
        if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
            raise ValueError(f"frame must be uint8 [H,W,3], got {frame.dtype} {frame.shape}")
        rects = _lib.frame_rects(frame.shape[0], frame.shape[1], bboxes)
        ticket = self._h.submit_frame(frame, rects, bgr=self._bgr)
        self._last_sizes = [frame.shape[:2]]
        self._pending.append((ticket, rects, 0))

    def begin(self, frame: np.ndarray, stream=None) -> None:
        """Resident form, step 1: upload the frame (it crosses PCIe once).  The frame holds one of the `depth`
        places from here until its `collect()`; `heads()` must follow before the next `begin()` / `submit()`.

        A uint8 [H,W,3] DEVICE array (inner strides (3, 1), the row stride is the pitch) is read where it is, ordered on `stream`:
        an integer stream handle, `None` = the default stream, which is where torch enqueues unless told otherwise:

            fp.begin(tensor, stream=torch.cuda.current_stream().cuda_stream)

        What was enqueued on `stream` before the call is seen; what is enqueued on it afterwards may overwrite the tensor; any
        other writer (the host, another stream) waits until `collect()` has returned.  `stream` is ignored for host frames."""
        if self._begun is not None:
            raise ValueError("the frame begun last has no heads yet: heads() first")
        if self._begun_clip is not None:
            raise ValueError("the clip begun last has no heads yet: detect_heads_clip() first")
        if len(self._pending) >= self._depth:
            raise ValueError(f"{self._depth} frames already in flight: collect() first")
        if _lib.is_device_array(frame) or isinstance(frame, _lib.DeviceFrame):
            f = _lib.device_frame(frame)
            ticket = self._h.frame_begin_device(f, bgr=self._bgr, stream=stream)
            self._begun = (ticket, f.h, f.w)
            self._last_sizes = [(f.h, f.w)]
            return
        frame = np.asarray(frame)
        if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
            raise ValueError(f"frame must be uint8 [H,W,3], got {frame.dtype} {frame.shape}")
        ticket = self._h.frame_begin(frame, bgr=self._bgr)
        self._begun = (ticket, frame.shape[0], frame.shape[1])
        self._last_sizes = [frame.shape[:2]]

    def begin_clip(self, frames, stream=None) -> None:
        """A clip, step 1: upload F frames (1..16) of ONE size, a uint8 [F,H,W,3] array or a list of uint8 [H,W,3] frames (stacked
        here), with one copy.  The clip holds one of the `depth` places until its `collect_clip()`; `detect_heads_clip()` must
        follow before the next `begin()` / `begin_clip()` / `submit()`.  Frames in device memory (one [F,H,W,3] device array or a
        list of [H,W,3] device arrays, all of them) are read where they are, ordered on `stream` as in `begin()`."""
        if self._begun is not None:
            raise ValueError("the frame begun last has no heads yet: heads() first")
        if self._begun_clip is not None:
            raise ValueError("the clip begun last has no heads yet: detect_heads_clip() first")
        if len(self._pending) >= self._depth:
            raise ValueError(f"{self._depth} frames already in flight: collect() first")
        if _lib.any_on_device(frames):
            items = _lib.device_frames(frames, one_size=True)
            self._begun_clip = (self._h.clip_begin_device(items, bgr=self._bgr, stream=stream), len(items))
            self._last_sizes = [(f.h, f.w) for f in items]
            return
        frames = _lib.clip_u8(frames)
        ticket = self._h.clip_begin(frames, bgr=self._bgr)
        self._begun_clip = (ticket, frames.shape[0])
        self._last_sizes = [frames.shape[1:3]] * frames.shape[0]

    def begin_clip_mixed(self, frames, stream=None) -> None:
        """A clip of frames of DIFFERENT sizes (several cameras, several files), step 1: upload a list of 1..16 uint8 [H_i,W_i,3]
        frames, packed back to back, with one copy.  From here on it is a clip like `begin_clip()`'s: `detect_heads_clip()` and
        `collect_clip()` follow, and frame f returns what `begin(); detect_heads(); collect()` return for it alone.  A list of
        device arrays (all of them) is packed by one kernel on the device, ordered on `stream` as in `begin()`."""
        if self._begun is not None:
            raise ValueError("the frame begun last has no heads yet: heads() first")
        if self._begun_clip is not None:
            raise ValueError("the clip begun last has no heads yet: detect_heads_clip() first")
        if len(self._pending) >= self._depth:
            raise ValueError(f"{self._depth} frames already in flight: collect() first")
        if _lib.any_on_device(frames):
            items = _lib.device_frames(frames)
            self._begun_clip = (self._h.clip_begin_device(items, bgr=self._bgr, stream=stream), len(items))
            self._last_sizes = [(f.h, f.w) for f in items]
            return
        frames = _lib.mixed_u8(frames)
        ticket = self._h.clip_begin_mixed(frames, bgr=self._bgr)
        self._begun_clip = (ticket, len(frames))
        self._last_sizes = [f.shape[:2] for f in frames]

    def _check_can_begin(self) -> None:
        if self._begun is not None:
            raise ValueError("the frame begun last has no heads yet: heads() first")
        if self._begun_clip is not None:
            raise ValueError("the clip begun last has no heads yet: detect_heads_clip() first")
        if len(self._pending) >= self._depth:
            raise ValueError(f"{self._depth} frames already in flight: collect() first")

    def begin_yuv(self, frame, stream=None) -> None:
        """`begin()` from a decoder's planes (a `whenet_hip.yuv.YUVFrame`): the planes are uploaded as they are, 1.5 bytes per pixel,
        and the BGR frame is built on the device.  Everything that follows -- `detector_input`, `detect`, `heads`, `detect_heads`,
        `collect` -- is what it is after `begin(frame.to_bgr())` on a pipeline made with `bgr=True`.  A frame whose planes are in
        device memory (`frame.on_device`) is converted where it is, ordered on `stream` as in `begin()`."""
        from .yuv import YUVFrame
        self._check_can_begin()
        if not isinstance(frame, YUVFrame):
            raise ValueError(f"begin_yuv takes a whenet_hip.yuv.YUVFrame, got {type(frame).__name__}")
        if frame.needs_ext:                 # a 16-bit container, 4:4:4 or BT.2020: the calls of include/whenet_hip_yuv_ext.h
            ticket = self._h.frame_begin_yuvx_device(frame, stream=stream) if frame.on_device else self._h.frame_begin_yuvx(frame)
        else:
            ticket = self._h.frame_begin_yuv_device(frame, stream=stream) if frame.on_device else self._h.frame_begin_yuv(frame)
        self._begun = (ticket, frame.h, frame.w)
        self._last_sizes = [(frame.h, frame.w)]

    def begin_jpeg(self, data, rule=None, progressive=None, orient=None, default_tables: bool = False, layouts: bool = False) -> "JpegStatus":
        """`begin()` from the bytes of a baseline JPEG stream (a still, or one frame of an MJPG file: `whenet_hip.mjpeg.MJPGReader`):
        what stands for `cv2.imread` / `cap.read()`.  Only the compressed bytes cross the link; the frame is decoded on the device
        (`whenet_hip.jpeg`, csrc/jpeg_dec.hip) in the pipeline's channel order, and everything that follows is what it is after
        `begin(jpeg.decode_host(data, bgr=...))`.  A stream the decoder does not accept (progressive unless turned on, arithmetic, 12 bit, ...) is a
        ValueError with the reason and takes no place.  Returns a `JpegStatus`, valid after the frame's `collect()`: damaged entropy
        data does not raise, it yields a defined frame and `ok == False`.  The entropy stage's form follows the handle's options
        "jpeg_entropy" (0: an interval per lane, 1: segmented, 2: auto, the default) and "jpeg_seg_bytes"; the frame is the same.
        The decode rule follows the handle's option "jpeg_rule" (0: the project's own, the default; 1: libjpeg's bytes, what
        `cv2.imread` gives) unless `rule` says "own" or "libjpeg" for this frame; the frame is then what
        `jpeg.decode_host(data, rule=...)` makes.  `progressive`: True also accepts a progressive (SOF2) stream -- the frame is then
        `jpeg.decode_host(data, progressive=True, rule=...)`, and `JpegStatus.interval` is the flat (scan, interval) item; None
        (the default) follows the handle's option "jpeg_progressive" (0: refused, the default).  `orient`: True applies the
        stream's EXIF orientation as `cv2.imread` does -- the frame is `jpeg.decode_host(data, orient=True, ...)`, turned by the
        kernel that writes it, and everything that follows (boxes included) is in the upright picture's coordinates; None (the
        default) follows the handle's option "jpeg_orient" (0: the tag is ignored, the default).  `JpegStatus.orientation` is
        the value applied.  default_tables=True: the stream is completed by `jpeg.add_default_tables` first -- the MJPG frame of a
        UVC camera or of an AVI whose writer left the DHT segment out, which is refused otherwise.  layouts=True
        (`whenet_frame_begin_jpeg_accept`): 4:4:0, 4:1:1 and 4:1:0 streams and single-scan SOF1 streams are accepted too -- the
        frame is `jpeg.decode_host(data, layouts=True, ...)`; a `progressive` of None counts as False then (the call states its
        accept bits), `orient` keeps its meaning.  False, the default, is the call as it was and refuses these streams on EVERY handle: the header is
        parsed here first, without the bit, so the handle's option "jpeg_layouts" (which the plain C calls read) does not reach
        this method; say layouts=True."""
        self._check_can_begin()
        if default_tables:
            data = _lib.jpeg_add_default_tables(data)
        _lib.jpeg_rule_code(rule)
        if layouts:
            accept = _lib.jpeg_accept_bits(bool(progressive), True)
            info = _lib.jpeg_parse_scans_accept(data, accept)[0]
            st = JpegStatus()
            ticket, st._orientation = self._h.frame_begin_jpeg_accept(data, st._status, bgr=self._bgr, rule=rule, accept=accept, orient=orient)
            if self._jpeg is None:
                self._jpeg = {}
            self._jpeg.setdefault(ticket, []).append(st)
            h, w = (info.w, info.h) if st._orientation >= 5 else (info.h, info.w)
            self._begun = (ticket, h, w)
            self._last_sizes = [(h, w)]
            return st
        info = _lib.jpeg_parse(data) if progressive is False else _lib.jpeg_parse_scans(data)[0]
        st = JpegStatus()
        # (always the call that carries `orient`: False must switch the turn off on a handle whose option is on; and as in
        # Handle.frame_begin_jpeg a progressive of False leaves SOF2 to the handle's option)
        ticket, st._orientation = self._h.frame_begin_jpeg_oriented(data, st._status, bgr=self._bgr, rule=rule,
                                                                    progressive=progressive or None, orient=orient)
        if self._jpeg is None:
            self._jpeg = {}
        self._jpeg.setdefault(ticket, []).append(st)
        h, w = (info.w, info.h) if st._orientation >= 5 else (info.h, info.w)
        self._begun = (ticket, h, w)
        self._last_sizes = [(h, w)]
        return st

    def begin_clip_jpeg(self, datas, rule=None, progressive: bool = False, orient: bool = False, default_tables: bool = False,
                        layouts: bool = False) -> list:
        """A clip from the bytes of 1..16 baseline JPEG streams (consecutive frames of an MJPG file: `MJPGReader.clips(16)`), each
        with its own size, sampling, tables and DRI: one upload of the compressed bytes, every decoder stage in one launch for all
        frames.  Frame f is what `begin_jpeg(datas[f])` makes; frames of one size make a clip as `begin_clip()` makes it, frames of
        different sizes one as `begin_clip_mixed()` makes it (at most option "letterbox_cache" of them).  `detect_heads_clip()` and
        `collect_clip()` follow.  One stream the decoder does not accept is a ValueError that names the frame, and the clip takes no
        place.  Returns a `JpegStatus` per frame, valid after `collect_clip()`: a damaged stream does not raise, it yields its own
        defined frame and `ok == False` and leaves the other frames untouched.  `rule`: as `begin_jpeg`, one rule for the clip.
        progressive=True: progressive (SOF2) streams are accepted too, alone or mixed with baseline ones (a folder of stills:
        `demo.py` walks Sample/*.jpeg) -- frame f is then what `begin_jpeg(datas[f], progressive=True)` makes, and
        `JpegStatus.interval` of a progressive frame is its flat (scan, interval) item.  Clips do not read the handle's option
        "jpeg_progressive": only this argument accepts SOF2.  orient=True: every frame by its own EXIF orientation, as
        `begin_jpeg(datas[f], orient=True)`; a clip is one-size by the sizes of the turned frames.  Clips do not read the option
        "jpeg_orient" either.  default_tables=True: every stream is completed by `jpeg.add_default_tables` first.  layouts=True
        (`whenet_clip_begin_jpeg_accept`): the streams `begin_jpeg(..., layouts=True)` accepts may be frames of the clip."""
        self._check_can_begin()
        _lib.jpeg_rule_code(rule)
        datas = [_lib.jpeg_add_default_tables(d) for d in datas] if default_tables else list(datas)
        if not 1 <= len(datas) <= _lib.MAX_CLIP_FRAMES:
            raise ValueError(f"a clip holds 1..{_lib.MAX_CLIP_FRAMES} frames, got {len(datas)}")
        infos = []
        for i, d in enumerate(datas):
            try:
                if layouts:
                    infos.append(_lib.jpeg_parse_scans_accept(d, _lib.jpeg_accept_bits(progressive, True))[0])
                else:
                    infos.append(_lib.jpeg_parse_scans(d)[0] if progressive else _lib.jpeg_parse(d))
            except ValueError as e:
                raise ValueError(f"begin_clip_jpeg: frame {i}: {e}") from None
        block = np.zeros((len(datas), 2), np.int32)      # (one array for the library to write; every JpegStatus is a row of it)
        applied = np.ones(len(datas), np.int32)
        if layouts:
            ticket, applied = self._h.clip_begin_jpeg_accept(datas, block, bgr=self._bgr, rule=rule,
                                                             accept=_lib.jpeg_accept_bits(progressive, True), orient=bool(orient))
        elif orient:
            ticket, applied = self._h.clip_begin_jpeg_oriented(datas, block, bgr=self._bgr, rule=rule, progressive=progressive, orient=True)
        else:
            ticket = self._h.clip_begin_jpeg(datas, block, bgr=self._bgr, rule=rule, progressive=progressive)
        sts = []
        for f in range(len(datas)):
            st = JpegStatus()
            st._status = block[f]
            st._orientation = int(applied[f])
            sts.append(st)
        if self._jpeg is None:
            self._jpeg = {}
        self._jpeg.setdefault(ticket, []).extend(sts)
        self._begun_clip = (ticket, len(datas))
        self._last_sizes = [(i.w, i.h) if o >= 5 else (i.h, i.w) for i, o in zip(infos, applied)]
        return sts

    def begin_clip_yuv(self, frames, stream=None) -> None:
        """A clip from the planes of 1..16 `YUVFrame`s, each with its own format and matrix: frames of one size make a clip as
        `begin_clip()` makes it, frames of different sizes one as `begin_clip_mixed()` makes it (at most option "letterbox_cache"
        of them).  `detect_heads_clip()` and `collect_clip()` follow.  The frames' planes are all in device memory (converted
        where they are, ordered on `stream` as in `begin()`) or all in host memory."""
        from .yuv import YUVFrame
        self._check_can_begin()
        frames = list(frames)
        if not 1 <= len(frames) <= _lib.MAX_CLIP_FRAMES:
            raise ValueError(f"a clip holds 1..{_lib.MAX_CLIP_FRAMES} frames, got {len(frames)}")
        for i, f in enumerate(frames):
            if not isinstance(f, YUVFrame):
                raise ValueError(f"begin_clip_yuv: frame {i} must be a whenet_hip.yuv.YUVFrame, got {type(f).__name__}")
        if len({f.on_device for f in frames}) > 1:
            raise ValueError("begin_clip_yuv: a clip's frames are all in device memory or all in host memory, not mixed: frames " +
                             str([i for i, f in enumerate(frames) if not f.on_device]) + " are host frames")
        if any(f.needs_ext for f in frames):      # (the extended calls take the old formats too: a clip may mix them)
            ticket = self._h.clip_begin_yuvx_device(frames, stream=stream) if frames[0].on_device else self._h.clip_begin_yuvx(frames)
        else:
            ticket = self._h.clip_begin_yuv_device(frames, stream=stream) if frames[0].on_device else self._h.clip_begin_yuv(frames)
        self._begun_clip = (ticket, len(frames))
        self._last_sizes = [(f.h, f.w) for f in frames]

    def _begun_frame(self, what: str):
        """The frame begun last, for the calls that work on ONE frame."""
        if self._begun is None:
            if self._begun_clip is not None:
                raise ValueError(f"{what}: a clip was begun last, not a frame: detect_heads_clip() enqueues it")
            raise ValueError("no frame begun (or its heads are already enqueued): begin() first")
        return self._begun

    def detect_heads_clip(self, size=(416, 416), score=.3, iou=.45, max_boxes=20, anchors=None, num_classes=1, max_heads=None) -> None:
        """A clip, step 2: `detect_heads()` of every frame of the clip begun last as ONE submission; returns as soon as the work is
        enqueued.  Per frame there are K = num_classes x max_boxes detection slots, F x K <= 1024.  The heads that have a window are
        numbered in (frame, detection) order and the first `max_heads` of them (1..256, default min(F x K, 256)) are the rows of one
        forward; `collect_clip()` reports how many rows were used and how many heads overflowed."""
        from .yolo import check_model_image_size
        if self._begun_clip is None:
            if self._begun is not None:
                raise ValueError("detect_heads_clip: a single frame was begun last, not a clip: detect_heads() enqueues it")
            raise ValueError("no clip begun (or its heads are already enqueued): begin_clip() first")
        check_model_image_size(size)
        _lib.check_max_heads(max_heads)
        anchors, num_classes = self._anchors(anchors, num_classes)
        ticket, F = self._begun_clip
        K = clip_slots(size, anchors, num_classes, max_boxes)
        if F * K > _lib.MAX_CLIP_SLOTS:
            raise ValueError(f"detect_heads_clip: frames x classes x max_boxes = {F} x {K} must be 1..{_lib.MAX_CLIP_SLOTS}")
        k = self._h.clip_detect_heads(ticket, anchors, num_classes, size, score, iou, max_boxes, max_heads)
        self._begun_clip = None
        self._pending.append((ticket, _CLIP, (F, k)))

    def collect_clip(self, detections: bool = False):
        """Oldest submission, a clip -> (frames, (rows_used, overflow)): `frames` is a list of F tuples shaped like `collect()` /
        `collect(detections=True)`, one per frame of the clip, in which the heads are those with a window inside the frame AND a row
        of the forward; `rows_used` = rows of the forward that held a head, `overflow` = heads with a window that got no row
        (max_heads too small).  On a submission that is not a clip: ValueError, and it stays in flight."""
        if not self._pending:
            raise ValueError("nothing in flight")
        ticket, kind, fk = self._pending[0]
        if kind is not _CLIP:
            raise ValueError("collect_clip: the oldest submission in flight is not a clip: collect() returns it")
        res = self._h.collect_clip(ticket, fk[0], fk[1])
        self._pending.popleft()
        self._finish_jpeg(ticket)
        counts, boxes, scores, classes, rects, valid, row, ypr, _, _, used, over = res
        return scatter_clip(counts, boxes, scores, classes, rects, valid, row, ypr, detections), (used, over)

    def detector_input(self, size=(416, 416), as_uint8: bool = False) -> np.ndarray:
        """Resident form, step 2 (any number of times): float32 [1, h, w, 3], the `image_data` YOLO.detect feeds to
        sess.run, cut from the frame begun last; `size` = (h, w) as `model_image_size`, multiples of 32."""
        from .yolo import check_model_image_size
        self._begun_frame("detector_input")
        check_model_image_size(size)
        u8, f32 = self._h.frame_letterbox(self._begun[0], size, want_u8=as_uint8, want_f32=not as_uint8)
        return u8 if as_uint8 else f32[None]

    def detect(self, size=(416, 416), score=.3, iou=.45, max_boxes=20, anchors=None, num_classes=1):
        """Resident form, step 2 with a detector loaded on the model's handle: YOLO.detect (yolo_postprocess.py:180-205) of
        the frame begun last, on the device -> (boxes [k,4] y_min, x_min, y_max, x_max, scores [k], classes [k]).  `anchors`
        and `num_classes` default to those of the `whenet_hip.detector.YOLO` that loaded the detector on this handle (or the
        one given to `attach_detector`)."""
        from .yolo import check_model_image_size
        self._begun_frame("detect")
        check_model_image_size(size)
        anchors, num_classes = self._anchors(anchors, num_classes)
        return self._h.frame_detect(self._begun[0], anchors, num_classes, size, score, iou, max_boxes)

    def _anchors(self, anchors, num_classes):
        if anchors is None:
            det = self._detector if self._detector is not None else getattr(self._h, "detector", None)
            if det is None:
                raise ValueError("detect: no whenet_hip.detector.YOLO was built on this model's handle: pass anchors= and num_classes=")
            anchors, num_classes = det.anchors, len(det.class_names)
        return anchors, num_classes

    def detect_heads(self, size=(416, 416), score=.3, iou=.45, max_boxes=20, anchors=None, num_classes=1) -> None:
        """Resident form, steps 2 and 3 as ONE submission: `detect()` and `heads()` of the frame begun last without the host in
        between.  Returns as soon as the work is enqueued; `collect()` returns the heads that have a window inside the frame,
        `collect(detections=True)` the detector's boxes as well.  num_classes x max_boxes <= 64: every slot is a crop of the forward
        (few heads in a large `max_boxes` pay for the padding; `detect()` + `heads()` run the forward at the head count)."""
        from .yolo import check_model_image_size
        self._begun_frame("detect_heads")
        check_model_image_size(size)
        anchors, num_classes = self._anchors(anchors, num_classes)
        ticket = self._begun[0]
        cap = self._h.frame_detect_heads(ticket, anchors, num_classes, size, score, iou, max_boxes)
        self._begun = None
        self._pending.append((ticket, None, cap))

    def attach_detector(self, yolo) -> None:
        """Use this `whenet_hip.detector.YOLO`'s anchors and class count in `detect()` (the default is the one built last with
        `handle=model`)."""
        self._detector = yolo

    def heads(self, bboxes) -> None:
        """Resident form, step 3: the detector's boxes of the frame begun last (an empty list is fine) -> margins,
        crops, one batched forward, exactly as `submit()`; `collect()` returns them in order with the submitted frames."""
        if self._begun is None and self._begun_clip is not None:
            raise ValueError("heads: a clip was begun last, not a frame: detect_heads_clip() enqueues it")
        if self._begun is None:
            raise ValueError("no frame begun: begin() first")
        ticket, fh, fw = self._begun
        rects = _lib.frame_rects(fh, fw, bboxes)
        self._h.frame_heads(ticket, rects)
        self._begun = None
        self._pending.append((ticket, rects, 0))

    def collect(self, detections: bool = False):
        """Oldest submitted frame -> (rects [k,4] int32, yaw, pitch, roll float32 (k,)).  A `detect_heads()` frame: the k heads
        whose window lies inside the frame; with `detections=True` also (boxes [n,4], scores [n], classes [n], valid [n]) of ALL n
        detections (valid 0: a window that is empty or leaves the frame -- `heads()` raises for such a box).  `detections=True` on
        a frame submitted any other way raises ValueError and leaves it in flight."""
        if not self._pending:
            raise ValueError("nothing in flight")
        ticket, rects, cap = self._pending[0]
        if rects is _CLIP:
            raise ValueError("collect: the oldest submission in flight is a clip: collect_clip() returns it")
        if rects is None:
            boxes, scores, classes, rects, valid, ypr, _, _ = self._h.collect_detect(ticket, cap)
            self._pending.popleft()
            self._finish_jpeg(ticket)
            keep = valid != 0
            res = (np.ascontiguousarray(rects[keep]), ypr[keep, 0].copy(), ypr[keep, 1].copy(), ypr[keep, 2].copy())
            return res + (boxes, scores, classes, valid) if detections else res
        if detections:
            raise ValueError("collect(detections=True): the oldest frame in flight was not submitted by detect_heads()")
        self._pending.popleft()
        k = rects.shape[0]
        ypr, _, _ = self._h.collect(ticket, k)
        self._finish_jpeg(ticket)
        return rects, ypr[:, 0].copy(), ypr[:, 1].copy(), ypr[:, 2].copy()

    def annotate(self, out, stream=None, display: str = "simple") -> None:
        """The annotated frame of the frame submitted last -- every head's window as a rectangle and its pose as three axes
        (demo_video.py:26-29, utils.py:13-43; `whenet_hip.overlay`) -- enqueued behind its forward; returns without waiting.  Call
        it once, after `submit()`, `heads()` or `detect_heads()`, before the next `begin()` and before that frame's `collect()`.
        `out`: a writable uint8 [H,W,3] numpy array (complete when the frame's `collect()` returns), a uint8 [H,W,3] device array
        with inner strides (3, 1), or a `YUVFrame` (NV12 / I420 with its matrix) whose planes are writable host or device arrays.
        The caller keeps a destination alive until that `collect()`: nothing here holds a reference.  A device destination is
        written in place: with `stream` (an integer stream handle) the kernel waits for what was enqueued on it before the call
        and work enqueued on it afterwards sees the annotated surface; without it the surface is complete when `collect()`
        returns.  Anything else -- a read-only array, another shape, CHW, float -- is a ValueError, never a silent copy.  The
        values `collect()` returns are unchanged.  `display="full"` adds the three text lines of demo_video.py's `--display full`
        to every head ('yaw: 10.0', 'pitch: -5.0', 'roll: 2.0' at the window's corner; `whenet_hip.overlay.labels`); the default
        paints exactly what it painted before."""
        from .overlay import surface_of
        extra = {"display": _lib.DISPLAY_FULL} if _lib.display_code(display) == _lib.DISPLAY_FULL else {}
        if not self._pending or self._pending[-1][1] is _CLIP:
            raise ValueError("annotate: no frame with its heads enqueued (submit(), heads() or detect_heads() first; a clip takes "
                             "annotate_clip())")
        if self._begun is not None or self._begun_clip is not None:
            raise ValueError("annotate: another frame or clip was begun since: annotate() follows the heads of the frame it paints, "
                             "before the next begin()")
        ticket = self._pending[-1][0]
        if self._annotated == ticket:
            raise ValueError("annotate: the frame submitted last is annotated already")
        (h, w), = self._last_sizes
        surface, _ = surface_of(out, int(h), int(w))
        self._h.frame_annotate(ticket, 0, surface, stream=stream, **extra)
        self._annotated = ticket

    def annotate_clip(self, outs, stream=None, display: str = "simple") -> None:
        """`annotate()` for the clip submitted last (after `detect_heads_clip()`, before its `collect_clip()`): `outs` holds one
        destination per frame of the clip, each as in `annotate()`; `None` leaves a frame out; `display` as in `annotate()`."""
        from .overlay import surface_of
        extra = {"display": _lib.DISPLAY_FULL} if _lib.display_code(display) == _lib.DISPLAY_FULL else {}
        if not self._pending or self._pending[-1][1] is not _CLIP:
            raise ValueError("annotate_clip: no clip with its heads enqueued (detect_heads_clip() first)")
        if self._begun is not None or self._begun_clip is not None:
            raise ValueError("annotate_clip: another frame or clip was begun since: annotate_clip() follows detect_heads_clip(), "
                             "before the next begin")
        ticket = self._pending[-1][0]
        if self._annotated == ticket:
            raise ValueError("annotate_clip: the clip submitted last is annotated already")
        sizes = self._last_sizes
        outs = list(outs)
        if len(outs) != len(sizes):
            raise ValueError(f"annotate_clip: the clip has {len(sizes)} frames, got {len(outs)} destinations")
        surfaces = [None if o is None else surface_of(o, int(h), int(w), f"outs[{i}]")[0] for i, (o, (h, w)) in enumerate(zip(outs, sizes))]
        for i, surface in enumerate(surfaces):      # (every destination is checked before the first is enqueued)
            if surface is not None:
                self._h.frame_annotate(ticket, i, surface, stream=stream, **extra)
        self._annotated = ticket                   # (after the last call: a clip the library refused part-way can be annotated again,
                                                   #  the library itself refuses the frames that are done)

    _jpeg = None                   # ticket -> the JpegFrames of annotate_jpeg / annotate_clip_jpeg, until its collect call

    def _finish_jpeg(self, ticket) -> None:
        for f in (self._jpeg.pop(ticket, ()) if self._jpeg else ()):
            f._done = True

    def _jpeg_frame(self, ticket, index, h, w, quality, display, capacity, sampling="4:2:0", optimize=False) -> "JpegFrame":
        from . import jpeg
        f = JpegFrame(int(w), int(h), jpeg.bound(int(h), int(w), sampling) if capacity is None else int(capacity))
        self._h.frame_annotate_jpeg(ticket, index, _lib.display_code(display), quality, f._out, f._result, sampling, optimize)
        if self._jpeg is None:
            self._jpeg = {}
        self._jpeg.setdefault(ticket, []).append(f)
        return f

    def annotate_jpeg(self, quality: int = 95, display: str = "simple", capacity=None, sampling: str = "4:2:0",
                      optimize: bool = False) -> "JpegFrame":
        """`annotate()` with the annotated frame compressed where it lies: the overlay goes into an I420 JFIF surface in device memory
        that the library owns, the JPEG encoder (`whenet_hip.jpeg`, csrc/jpeg.hip) runs behind it, and only the stream's bytes come
        back (demo_video.py:60, `out.write(frame)` into an MJPG writer).  Returns at once; the `JpegFrame`'s `tobytes()` is valid
        after the frame's `collect()` and raises before it.  `capacity` (default: `whenet_hip.jpeg.bound(h, w)`) is the room for the
        stream: one that does not fit raises `whenet_hip.jpeg.CapacityError`, naming the needed size, at `tobytes()`.  Call order as
        `annotate()`: it is the frame's one annotate call.  The values `collect()` returns are unchanged.  `sampling` "4:2:2" /
        "4:4:4": the overlay goes into a packed surface in the pipeline's channel order instead (an I420 surface cannot carry the
        chroma of one-pixel axes and text strokes), and the stream is `jpeg.encode_host(overlay.annotate_host(frame, ...),
        sampling=...)`'s.  optimize=True: Huffman tables of the frame's own symbols, built on the device; still enqueue-only."""
        if not self._pending or self._pending[-1][1] is _CLIP:
            raise ValueError("annotate_jpeg: no frame with its heads enqueued (submit(), heads() or detect_heads() first; a clip takes "
                             "annotate_clip_jpeg())")
        if self._begun is not None or self._begun_clip is not None:
            raise ValueError("annotate_jpeg: another frame or clip was begun since: annotate_jpeg() follows the heads of the frame it "
                             "paints, before the next begin()")
        ticket = self._pending[-1][0]
        if self._annotated == ticket:
            raise ValueError("annotate_jpeg: the frame submitted last is annotated already")
        (h, w), = self._last_sizes
        f = self._jpeg_frame(ticket, 0, h, w, quality, display, capacity, sampling, optimize)
        self._annotated = ticket
        return f

    def annotate_clip_jpeg(self, quality: int = 95, display: str = "simple", capacity=None, sampling: str = "4:2:0", optimize: bool = False):
        """`annotate_jpeg()` for every frame of the clip submitted last (after `detect_heads_clip()`, before its `collect_clip()`):
        a list of one `JpegFrame` per frame, valid after `collect_clip()`."""
        if not self._pending or self._pending[-1][1] is not _CLIP:
            raise ValueError("annotate_clip_jpeg: no clip with its heads enqueued (detect_heads_clip() first)")
        if self._begun is not None or self._begun_clip is not None:
            raise ValueError("annotate_clip_jpeg: another frame or clip was begun since: it follows detect_heads_clip(), before the "
                             "next begin")
        ticket = self._pending[-1][0]
        if self._annotated == ticket:
            raise ValueError("annotate_clip_jpeg: the clip submitted last is annotated already")
        out = [self._jpeg_frame(ticket, i, h, w, quality, display, capacity, sampling, optimize) for i, (h, w) in enumerate(self._last_sizes)]
        self._annotated = ticket
        return out

    def process(self, frame: np.ndarray, bboxes):
        """Synchronous form: one frame in, its heads' angles out."""
        self.submit(frame, bboxes)
        while len(self._pending) > 1:
            self.collect()
        return self.collect()


def crop_heads(model, frame: np.ndarray, bboxes, bgr: bool = True):
    """The crops `process_detection` would have handed to `get_angle`, made on the device:
    returns (rects int32 [k,4], crops uint8 [k,224,224,3] RGB)."""
    frame = np.asarray(frame)
    rects = _lib.frame_rects(frame.shape[0], frame.shape[1], bboxes)
    if rects.shape[0] == 0:
        return rects, np.zeros((0, 224, 224, 3), np.uint8)
    return rects, model._handle.op_crop_resize(frame, rects, bgr=bgr)
