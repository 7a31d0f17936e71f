"""Drop-in for the reference's detector class (`yolo_v3/yolo_postprocess.py:26-205`) on the GPU, without TensorFlow.

`YOLO(**kwargs)` takes the reference's keyword names and defaults; `detect(image)` returns `(boxes, scores, classes)` as numpy,
as yolo_postprocess.py:205 does: boxes float32 [k,4] (y_min, x_min, y_max, x_max) in image pixels.  Letterbox
(csrc/letterbox.hip), the Darknet body (csrc/dconv.hip) and the box selection (csrc/yolo.hip) run as one chain on the device
(`whenet_op_detect`).

The body's arithmetic is chosen by keyword-only `dtype`:
  * `'f16'` (default): binary16 storage of weights and activations, f32 accumulation -- the fast form.  Its boxes lie up to a few
    pixels (tiny body) or tens of pixels (full body, random weights) from a float64 evaluation's, so the integer crop windows
    `process_detection` derives from them can differ from the reference's.
  * `'f32'`: float32 from the image to the maps on the f32 matrix instructions, nothing rounded to binary16 -- the parity-grade
    form.  Its boxes lie within hundredths of a pixel of the float64 evaluation's and give the same crop windows, so the pose
    parity of `WHENet(dtype='f32' | 'f32s')` carries over to the whole frame path.

Differences a caller sees:
  * `model_path` is a packed WHNPACK1 detector snapshot (a path, bytes, or a dict of arrays: whenet_hip/detector_weights.py).
    A Keras `.h5` is NOT read: the reference's `head_detect.h5` is not part of its tree and the package has no HDF5 reader for
    the detector; a `.h5` path raises ValueError saying so.
  * `anchors_path` / `classes_path` are read as the reference reads them; an array of anchors / a list of names is accepted too.
    The defaults name `yolo_anchors.txt` / `head_classes.txt` beside this module, as the reference's `data_file()` does.
  * `gpu_num` is accepted and ignored; keyword-only `handle=` (any whenet_hip handle, e.g. `WHENet(...)._handle`) or `device=`,
    and `dtype=` (above).  A handle that already holds a detector keeps that detector's dtype: another one is a ValueError from
    the library.
There is no CPU fallback: without a gfx950 device construction raises WhenetError (ENODEV).
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib
from . import detector_weights as DW
from .yolo import check_model_image_size


def data_file(filename):
    """Prepend the path to the data subdirectory to filename (yolo_postprocess.py:22-24)."""
    return os.path.join(os.path.dirname(__file__), "data", filename)


H5_MESSAGE = ("a Keras .h5 of the detector is not read by this package: pack its arrays with whenet_hip.detector_weights "
              "(dconvNNN/kernel, dbnNNN/..., dconvNNN/bias) and pass the packed snapshot as model_path")


class YOLO(object):
    _defaults = {
        "model_path": data_file("head_detect.h5"),
        "anchors_path": data_file("yolo_anchors.txt"),
        "classes_path": data_file("head_classes.txt"),
        "score": 0.3,
        "iou": 0.45,
        "model_image_size": (416, 416),
        "gpu_num": 1,
    }

    @classmethod
    def get_defaults(cls, n):
        if n in cls._defaults:
            return cls._defaults[n]
        else:
            return "Unrecognized attribute name '" + n + "'"

    def __init__(self, *, handle=None, device: int = 0, dtype: str = "f16", **kwargs):
        if dtype not in _lib.DETECTOR_DTYPES:
            raise ValueError(f"YOLO(dtype=...) must be one of {sorted(_lib.DETECTOR_DTYPES)}, got {dtype!r}")
        self.dtype = dtype
        unknown = set(kwargs) - set(self._defaults)
        if unknown:
            raise TypeError(f"YOLO() got unexpected keyword arguments {sorted(unknown)}")
        self.__dict__.update(self._defaults)
        self.__dict__.update(kwargs)
        size = self.model_image_size
        if size is None or tuple(size) == (None, None):
            raise ValueError("model_image_size=(None, None) is not supported: give (h, w), multiples of 32")
        check_model_image_size(size)
        self.model_image_size = (int(size[0]), int(size[1]))
        snapshot = self._snapshot(self.model_path)
        self.class_names = self._get_class()
        self.anchors = self._get_anchors()
        if len(self.anchors) not in (6, 9):
            raise ValueError(f"{len(self.anchors)} anchors: yolo_body needs 9, tiny_yolo_body 6")
        kind, out_filters = DW.kind_of(DW.parse(snapshot)) if not isinstance(self.model_path, dict) else DW.kind_of(self.model_path)
        if (kind == DW.TINY) != (len(self.anchors) == 6) or out_filters != 3 * (len(self.class_names) + 5):
            raise ValueError("Mismatch between model and given anchor and class sizes")
        self._own = handle is None
        self._handle = _lib.Handle.postproc(device) if handle is None else getattr(handle, "_handle", handle)
        self._handle.detector_load(snapshot, dtype)
        self._handle.detector = self               # FramePipeline.detect finds the anchors and the class count here

    @staticmethod
    def _snapshot(model_path) -> bytes:
        if isinstance(model_path, dict):
            return DW.pack(model_path)
        if isinstance(model_path, (bytes, bytearray, memoryview)):
            return bytes(model_path)
        path = os.path.expanduser(os.fspath(model_path))
        if path.endswith(".h5"):
            raise ValueError(f"{path}: {H5_MESSAGE}")
        with open(path, "rb") as f:
            return f.read()

    def _get_class(self):
        if not isinstance(self.classes_path, (str, os.PathLike)):
            return [str(c) for c in self.classes_path]
        with open(os.path.expanduser(self.classes_path)) as f:
            return [c.strip() for c in f.readlines()]

    def _get_anchors(self):
        if not isinstance(self.anchors_path, (str, os.PathLike)):
            return np.array(self.anchors_path, dtype=float).reshape(-1, 2)
        with open(os.path.expanduser(self.anchors_path)) as f:
            anchors = f.readline()
        return np.array([float(x) for x in anchors.split(",")]).reshape(-1, 2)

    def detect(self, image, max_boxes: int = 20):
        """`image`: a PIL image (RGB) or a uint8 RGB array [H,W,3] -> (out_boxes, out_scores, out_classes)."""
        frame = np.asarray(image.convert("RGB") if hasattr(image, "convert") else image)
        return self._handle.op_detect(frame, self.anchors, len(self.class_names), self.model_image_size, self.score, self.iou,
                                      max_boxes, bgr=False)

    def close_session(self):
        if self._handle is not None and getattr(self._handle, "detector", None) is self:
            self._handle.detector = None
        if self._own and self._handle is not None:
            self._handle.close()
        self._handle = None
