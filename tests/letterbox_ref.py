"""Numpy restatement of what the reference's detector pre-processing computes (test side only):

  * `letterbox_image` (yolo_v3/utils.py:23-34): geometry in Python floats, Pillow's 8-bit BICUBIC
    resample, paste centred on a grey (128) canvas;
  * `np.array(..., 'float32') / 255.` (yolo_v3/yolo_postprocess.py:191-195).

Pillow's 8-bit resample (src/libImaging/Resample.c) is integer arithmetic on tables it computes in
double: `precompute_coeffs` (per output pixel a window [xmin, xmin + n) and n normalised cubic weights,
a = -0.5), `normalize_coeffs_8bpc` (22 fractional bits, rounded half away from zero), a horizontal pass
and then a vertical pass, each `(2^21 + sum p * k) >> 22` clipped to 0..255 and stored as 8 bits in
between.  tests/golden/make_letterbox_fixture.py executes the reference itself; this file supplies whole
expected arrays where the fixture holds only a hash, and the integer tables the library must reproduce.
"""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
MAX_FRAME_SIDE = 8192         # documented limits of the library (include/whenet_hip.h)
MAX_BOX_SIDE = 4096


def geometry(ih: int, iw: int, box_h: int, box_w: int):
    """utils.py:25-33 -> (nw, nh, x0, y0)."""
    w, h = box_w, box_h
    scale = min(w / iw, h / ih)
    nw = int(iw * scale)
    nh = int(ih * scale)
    return nw, nh, (w - nw) // 2, (h - nh) // 2


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def axis_tables(in_size: int, out_size: int):
    """precompute_coeffs + normalize_coeffs_8bpc for one axis: (ksize, bounds int32 [out, 2] = (xmin, n),
    coeffs int32 [out, ksize], zero beyond n)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5))
        n = xmax - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        bounds[xx] = (xmin, n)
        for x, v in enumerate(k):
            coeffs[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return ksize, bounds, coeffs


def _resample_axis1(img: np.ndarray, bounds: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
    """One pass along axis 1 of uint8 [a, in, c] -> uint8 [a, out, c]."""
    out = np.empty((img.shape[0], bounds.shape[0], img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for xx in range(bounds.shape[0]):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.tensordot(src[:, xmin:xmin + n, :], coeffs[xx, :n].astype(np.int64), axes=([1], [0]))
        out[:, xx, :] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out


def resize_bicubic_u8(img: np.ndarray, nh: int, nw: int) -> np.ndarray:
    """Image.resize((nw, nh), Image.BICUBIC) on an 8-bit 3-channel image: horizontal pass, then vertical.
    (Pillow skips a pass whose size does not change; such a pass is the identity in this arithmetic.)"""
    if nh <= 0 or nw <= 0:
        raise ValueError("height and width must be > 0")
    ih, iw = img.shape[:2]
    _, bx, cx = axis_tables(iw, nw)
    _, by, cy = axis_tables(ih, nh)
    tmp = _resample_axis1(img, bx, cx)
    return _resample_axis1(tmp.transpose(1, 0, 2), by, cy).transpose(1, 0, 2)


def letterbox_u8(frame_rgb: np.ndarray, box_h: int, box_w: int) -> np.ndarray:
    """np.array(letterbox_image(Image.fromarray(frame_rgb), (box_w, box_h))): uint8 [box_h, box_w, 3]."""
    ih, iw = frame_rgb.shape[:2]
    nw, nh, x0, y0 = geometry(ih, iw, box_h, box_w)
    small = resize_bicubic_u8(frame_rgb, nh, nw)
    canvas = np.full((box_h, box_w, 3), 128, np.uint8)
    canvas[y0:y0 + nh, x0:x0 + nw] = small
    return canvas


def image_data(canvas_u8: np.ndarray) -> np.ndarray:
    """yolo_postprocess.py:191-196: float32 [1, h, w, 3]."""
    x = np.array(canvas_u8, dtype="float32")
    x /= 255.
    return np.expand_dims(x, 0)
