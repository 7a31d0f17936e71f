"""Executes the reference's own detector bodies (`yolo_body` / `tiny_yolo_body`, yolo_v3/model.py:20-122) without Keras.

`keras` and `tensorflow` are not installed where this project is built, and the detector's Keras layers are third party: what
the REFERENCE contributes is the wiring -- which layer feeds which, the padding sides, the routes `darknet.layers[152]` and
`[92]`, the order of upsample and concatenate.  This module puts eager stand-ins for `keras.layers`, `keras.models`,
`keras.regularizers`, `keras.backend` and `tensorflow` into `sys.modules`, imports the reference's model.py fresh and calls its
functions: every layer computes its output in float64 (torch.nn.functional on the CPU) the moment the reference's code calls it.

  * Conv2D, BatchNormalization (epsilon 1e-3, Keras' default), LeakyReLU, ZeroPadding2D, UpSampling2D (nearest), Concatenate,
    Add, MaxPooling2D ('same' pads bottom / right with -inf), Input;
  * `Model` records the layers in creation order with the InputLayer as index 0, so that `darknet.layers[152].output` resolves
    as Keras resolves it for these chain-shaped graphs;
  * weights come from a `whenet_hip.detector_weights` dict: the k-th Conv2D created reads `dconv{k:03d}`, the k-th
    BatchNormalization `dbn{k:03d}`.

`run(kind, weights, image, anchors_per_scale, num_classes)` returns the output maps, the recorded convolution / pool list
(what tests compare the engine's layer table with) and per-row statistics.  Needs /root/reference (`available()`).
"""
from __future__ import annotations

import contextlib
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REFERENCE = os.environ.get("WHENET_REFERENCE", "/root/reference")


def available() -> bool:
    return os.path.exists(os.path.join(REFERENCE, "yolo_v3", "model.py"))


class _Ctx:
    weights = None
    layers = None          # creation order, InputLayer first
    rows = None            # convolutions and pools in creation order
    n_conv = 0
    n_bn = 0


_ctx = _Ctx()


class Tensor:
    """An evaluated Keras tensor: NHWC float64 value + the row (convolution / pool) whose output chain it belongs to."""

    def __init__(self, value, row=None):
        self.value = value
        self.row = row


class Layer:
    def __init__(self):
        _ctx.layers.append(self)
        self.output = None

    def __call__(self, x):
        self.output = self.call(x)
        return self.output


class InputLayer(Layer):
    pass


def Input(shape=None, tensor=None, **kw):
    layer = InputLayer()
    layer.output = Tensor(tensor)
    return layer.output


def _nchw(v):
    return torch.from_numpy(np.ascontiguousarray(v)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


class Conv2D(Layer):
    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", use_bias=True, kernel_regularizer=None, **kw):
        super().__init__()
        self.filters = int(filters)
        self.k = int(kernel_size[0] if isinstance(kernel_size, (tuple, list)) else kernel_size)
        self.stride = int(strides[0] if isinstance(strides, (tuple, list)) else strides)
        self.padding, self.use_bias = padding, bool(use_bias)
        self.index = _ctx.n_conv
        _ctx.n_conv += 1

    def call(self, x):
        kernel = np.asarray(_ctx.weights[f"dconv{self.index:03d}/kernel"], np.float64)
        assert kernel.shape == (self.k, self.k, x.value.shape[3], self.filters), (self.index, kernel.shape, x.value.shape)
        w = torch.from_numpy(kernel).permute(3, 2, 0, 1).contiguous()
        pad = (self.k // 2) if self.padding == "same" else 0
        assert self.padding in ("same", "valid") and (self.padding == "valid" or self.stride == 1)
        y = F.conv2d(_nchw(x.value), w, None, stride=self.stride, padding=pad)
        if self.use_bias:
            y = y + torch.from_numpy(np.asarray(_ctx.weights[f"dconv{self.index:03d}/bias"], np.float64)).view(1, -1, 1, 1)
        row = {"op": 0, "k": self.k, "stride": self.stride, "cin": int(x.value.shape[3]), "cout": self.filters, "bn": 0, "leaky": 0,
               "bias": int(self.use_bias), "padded_top_left": int(getattr(x, "padded", None) == ((1, 0), (1, 0)))}
        _ctx.rows.append(row)
        return Tensor(_nhwc(y), row)


class BatchNormalization(Layer):
    def __init__(self, epsilon=1e-3, **kw):
        super().__init__()
        self.epsilon = epsilon
        self.index = _ctx.n_bn
        _ctx.n_bn += 1

    def call(self, x):
        g, b, m, v = (np.asarray(_ctx.weights[f"dbn{self.index:03d}/{leaf}"], np.float64)
                      for leaf in ("gamma", "beta", "moving_mean", "moving_variance"))
        x.row["bn"] = 1
        return Tensor((x.value - m) / np.sqrt(v + self.epsilon) * g + b, x.row)


class LeakyReLU(Layer):
    def __init__(self, alpha=0.3, **kw):
        super().__init__()
        self.alpha = alpha

    def call(self, x):
        assert self.alpha == 0.1
        x.row["leaky"] = 1
        return Tensor(np.where(x.value < 0, x.value * self.alpha, x.value), x.row)


class ZeroPadding2D(Layer):
    def __init__(self, padding=(1, 1), **kw):
        super().__init__()
        self.padding = tuple(tuple(p) for p in padding)

    def call(self, x):
        (t, b), (l, r) = self.padding
        out = Tensor(np.pad(x.value, ((0, 0), (t, b), (l, r), (0, 0))), x.row)
        out.padded = self.padding
        return out


class UpSampling2D(Layer):
    def __init__(self, size=(2, 2), **kw):
        super().__init__()
        self.size = int(size[0] if isinstance(size, (tuple, list)) else size)

    def call(self, x):
        return Tensor(np.repeat(np.repeat(x.value, self.size, axis=1), self.size, axis=2), x.row)


class Concatenate(Layer):
    def __init__(self, axis=-1, **kw):
        super().__init__()

    def call(self, xs):
        return Tensor(np.concatenate([t.value for t in xs], axis=-1))


class Add(Layer):
    def call(self, xs):
        a, b = xs
        return Tensor(a.value + b.value, b.row)


class MaxPooling2D(Layer):
    def __init__(self, pool_size=(2, 2), strides=None, padding="valid", **kw):
        super().__init__()
        self.pool = int(pool_size[0])
        self.stride = int((strides or pool_size)[0])
        self.padding = padding

    def call(self, x):
        assert self.pool == 2 and self.padding == "same"
        n, h, w, c = x.value.shape
        ph = (-(-h // self.stride) - 1) * self.stride + 2 - h          # TensorFlow 'same': the surplus goes bottom / right
        pw = (-(-w // self.stride) - 1) * self.stride + 2 - w
        v = np.pad(x.value, ((0, 0), (0, max(ph, 0)), (0, max(pw, 0)), (0, 0)), constant_values=-np.inf)
        y = F.max_pool2d(_nchw(v), 2, self.stride)
        row = {"op": 1, "k": 2, "stride": self.stride, "cin": c, "cout": c, "bn": 0, "leaky": 0, "bias": 0, "padded_top_left": 0}
        _ctx.rows.append(row)
        return Tensor(_nhwc(y), row)


class Model:
    def __init__(self, inputs, outputs):
        self.layers = list(_ctx.layers)            # creation order, InputLayer = 0
        self.inputs = inputs
        self.outputs = outputs if isinstance(outputs, (list, tuple)) else [outputs]
        self.output = outputs


@contextlib.contextmanager
def _stand_ins():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    layers = mod("keras.layers", Conv2D=Conv2D, Add=Add, ZeroPadding2D=ZeroPadding2D, UpSampling2D=UpSampling2D,
                 Concatenate=Concatenate, MaxPooling2D=MaxPooling2D, Input=Input, BatchNormalization=BatchNormalization,
                 LeakyReLU=LeakyReLU)
    mods = {
        "keras": mod("keras", layers=layers), "keras.layers": layers,
        "keras.layers.advanced_activations": mod("keras.layers.advanced_activations", LeakyReLU=LeakyReLU),
        "keras.layers.normalization": mod("keras.layers.normalization", BatchNormalization=BatchNormalization),
        "keras.models": mod("keras.models", Model=Model),
        "keras.regularizers": mod("keras.regularizers", l2=lambda *a, **k: None),
        "keras.backend": mod("keras.backend"),
        "tensorflow": mod("tensorflow"),
    }
    mods["keras"].backend = mods["keras.backend"]
    names = list(mods) + ["yolo_v3", "yolo_v3.model", "yolo_v3.utils"]
    saved = {n: sys.modules.get(n) for n in names}
    for n in names:
        sys.modules.pop(n, None)
    sys.modules.update(mods)
    sys.path.insert(0, REFERENCE)
    try:
        yield importlib.import_module("yolo_v3.model")
    finally:
        sys.path.remove(REFERENCE)
        for n in names:
            sys.modules.pop(n, None)
            if saved[n] is not None:
                sys.modules[n] = saved[n]


def run(kind: int, weights, image: np.ndarray, anchors_per_scale: int = 3, num_classes: int = 1):
    """image float [n,H,W,3] -> {"maps": [float64 NHWC, coarsest first], "rows": [...], "stats": [(rms, max|x|) per row],
    "routes": channels of darknet.layers[152] / [92] (full body)}."""
    _ctx.weights, _ctx.layers, _ctx.rows, _ctx.n_conv, _ctx.n_bn = weights, [], [], 0, 0
    with _stand_ins() as model_py, torch.no_grad():
        inputs = Input(tensor=np.asarray(image, np.float64))
        fn = model_py.tiny_yolo_body if kind == 1 else model_py.yolo_body
        model = fn(inputs, anchors_per_scale, num_classes)
        layers = list(_ctx.layers)
    out = {"maps": [t.value for t in model.outputs], "rows": [dict(r) for r in _ctx.rows]}
    # a row's output is the last tensor of its chain (conv -> BN -> Leaky -> Add): walk the layers once more
    final = {}
    for layer in layers:
        t = layer.output
        if t is not None and getattr(t, "row", None) is not None and not isinstance(layer, (ZeroPadding2D, UpSampling2D)):
            final[id(t.row)] = t.value
    out["stats"] = [(float(np.sqrt(np.mean(final[id(r)] ** 2))), float(np.abs(final[id(r)]).max())) for r in _ctx.rows]
    if kind == 0:
        out["routes"] = [(type(layers[i]).__name__, int(layers[i].output.value.shape[3])) for i in (152, 92)]
    _ctx.weights = _ctx.layers = _ctx.rows = None
    return out
