"""Drop-ins for the reference's detector PRE- and POST-processing, on the GPU.

`letterbox` returns the `image_data` that `YOLO.detect` feeds to `sess.run` (yolo_postprocess.py:186-196): the
Pillow-BICUBIC `letterbox_image` of yolo_v3/utils.py:23-34 and the float32 `/ 255.`, bit for bit.

`yolo_eval` keeps the name, argument order and defaults of /root/reference/yolo_v3/model.py:193-199; the
reference builds TensorFlow graph ops from symbolic tensors and runs them in `sess.run`
(yolo_postprocess.py:102-104, 198-204), here the arguments are the numpy output maps of the detector
(`sess.run(yolo_model.output)`) and the result is numpy: boxes [k,4] (y_min, x_min, y_max, x_max), scores
[k], classes [k] -- what `YOLO.detect` returns (yolo_postprocess.py:205).  The detector network between the two runs on
the device as well (whenet_hip/detector.py: `YOLO`, csrc/dconv.hip); there is no CPU fallback.
"""
from __future__ import annotations

import threading
from typing import Dict, Optional

import numpy as np

from . import _lib

_default_handles: Dict[int, _lib.Handle] = {}
_lock = threading.Lock()


def _handle(device: int) -> _lib.Handle:
    """One network-less handle per device (whenet_create_postproc: a device context, a stream and the scratch of
    the two post-processing launches -- no weights are synthesised or uploaded), created on first use."""
    with _lock:
        h = _default_handles.get(device)
        if h is None:
            h = _default_handles[device] = _lib.Handle.postproc(device)
        return h


def yolo_eval(yolo_outputs, anchors, num_classes, image_shape, max_boxes=20, score_threshold=.6, iou_threshold=.5,
              handle: Optional[_lib.Handle] = None, device: int = 0):
    """Evaluate YOLO model on given input and return filtered boxes (model.py:193-232).  `handle`: any whenet_hip
    handle (e.g. the WHENet model's) to run on; else a post-processing handle of `device` (handles are not
    thread-safe: callers that run this from several threads pass their own)."""
    h = handle if handle is not None else _handle(device)
    return h.yolo_eval(yolo_outputs, np.asarray(anchors, np.float32), int(num_classes), image_shape,
                       max_boxes=max_boxes, score_threshold=score_threshold, iou_threshold=iou_threshold)


def letterbox(handle_or_model, frame, size=(416, 416), bgr=True, as_uint8=False):
    """The detector input of one frame: float32 [1, h, w, 3], exactly the `image_data` of yolo_postprocess.py:191-196
    (`as_uint8=True`: the uint8 canvas [h, w, 3] that `letterbox_image` returns instead).  `handle_or_model`: a whenet_hip
    handle, a `whenet.WHENet`, or None for the post-processing handle of device 0.  `frame` uint8 [H, W, 3], BGR as cv2
    delivers it unless `bgr=False`; `size` = (h, w) as the reference's `model_image_size`, multiples of 32 as
    YOLO.detect asserts (yolo_postprocess.py:184-185)."""
    h = handle_or_model if handle_or_model is not None else _handle(0)
    h = getattr(h, "_handle", h)
    check_model_image_size(size)
    u8, f32 = h.op_letterbox(frame, size, bgr=bgr, want_u8=as_uint8, want_f32=not as_uint8)
    return u8 if as_uint8 else f32[None]


def check_model_image_size(size) -> None:
    if len(size) != 2 or int(size[0]) < 32 or int(size[1]) < 32 or size[0] % 32 != 0 or size[1] % 32 != 0:
        raise ValueError(f"Multiples of 32 required, got model_image_size {tuple(size)}")
