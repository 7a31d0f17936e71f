"""Table-driven restatement of the detector body (test side only): driven by the rows of `whenet_detector_spec`, never by the
reference's code (tests/detector_harness.py executes that).  Three arithmetic modes:

  "f64"     float64 throughout: the oracle;
  "f32"     float32 throughout (folded weights rounded to float32);
  "f16emu"  what binary16 STORAGE costs, computed on the CPU: float32 arithmetic, folded weights and the input image rounded to
            binary16, every row's output rounded to binary16 (after the residual add); output convolutions stay float32.

Convolutions go through torch.nn.functional on the CPU.  `layer()` is one row alone, as whenet_op_dconv computes it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3


def fold(rows, weights):
    """Per row: (kernel HWIO float64 with the BatchNorm scale folded in, bias float64) or None for a pool."""
    out, ci, bi = [], 0, 0
    for r in rows:
        if r["op"] != 0:
            out.append(None)
            continue
        k = np.asarray(weights[f"dconv{ci:03d}/kernel"], np.float64)
        if r["bn"]:
            g, b, m, v = (np.asarray(weights[f"dbn{bi:03d}/{leaf}"], np.float64) for leaf in ("gamma", "beta", "moving_mean", "moving_variance"))
            s = g / np.sqrt(v + BN_EPS)
            out.append((k * s, b - m * s))
            bi += 1
        else:
            out.append((k, np.asarray(weights[f"dconv{ci:03d}/bias"], np.float64)))
        ci += 1
    return out


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).permute(0, 3, 1, 2)


def conv(x, kernel, bias, stride, leaky, x2=None, skip=None, dtype=np.float64):
    """x NHWC (with x2: the half-resolution source, upsampled by 2 and concatenated in FRONT of x2), kernel HWIO, stride 2 pads
    top / left only.  Returns NHWC in `dtype` (no storage rounding)."""
    with torch.no_grad():
        xt = _t(x, dtype)
        if x2 is not None:
            xt = torch.cat([xt.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), _t(x2, dtype)], dim=1)
        k = kernel.shape[0]
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(kernel, dtype))).permute(3, 2, 0, 1).contiguous()
        if stride == 2:
            xt = F.pad(xt, (1, 0, 1, 0))
            y = F.conv2d(xt, w, None, stride=2)
        else:
            y = F.conv2d(xt, w, None, padding=k // 2)
        y = y + torch.from_numpy(np.asarray(bias, dtype)).view(1, -1, 1, 1)
        if leaky:
            y = torch.where(y < 0, y * torch.tensor(0.1, dtype=y.dtype), y)
        if skip is not None:
            y = y + _t(skip, dtype)
        return y.permute(0, 2, 3, 1).contiguous().numpy()


def pool(x, stride):
    """MaxPooling2D(2, strides=stride, 'same'): the surplus row / column is bottom / right and never wins."""
    n, h, w, c = x.shape
    ho, wo = (-(-h // stride), -(-w // stride))
    v = np.pad(x, ((0, 0), (0, (ho - 1) * stride + 2 - h), (0, (wo - 1) * stride + 2 - w), (0, 0)), constant_values=-np.inf)
    return np.max(np.stack([v[:, dy:dy + (ho - 1) * stride + 1:stride, dx:dx + (wo - 1) * stride + 1:stride] for dy in (0, 1) for dx in (0, 1)]), axis=0)


def r16(a):
    return np.asarray(a).astype(np.float16).astype(np.float32)


def forward(rows, weights, image, mode="f64", want_stats=False):
    """image float [n,H,W,3] -> output maps (coarsest first); with want_stats also [(rms, max|x|)] per row."""
    dtype = np.float64 if mode == "f64" else np.float32
    folded = fold(rows, weights)
    x0 = np.asarray(image, dtype)
    if mode == "f16emu":
        x0 = r16(x0)
    acts, maps, stats = [], [], []
    for r, fw in zip(rows, folded):
        src = x0 if r["src0"] < 0 else acts[r["src0"]]
        if r["op"] == 1:
            y = pool(src, r["stride"])
        else:
            kernel, bias = fw
            if mode == "f16emu":
                kernel = r16(kernel)
            y = conv(src, kernel, bias, r["stride"], r["leaky"], x2=acts[r["src1"]] if r["src1"] >= 0 else None,
                     skip=acts[r["skip"]] if r["skip"] >= 0 else None, dtype=dtype)
            if mode == "f16emu" and not r["is_output"]:
                y = r16(y)
        acts.append(y)
        if r["is_output"]:
            maps.append(y)
        stats.append((float(np.sqrt(np.mean(np.square(y, dtype=np.float64)))), float(np.abs(y).max())))
    return (maps, stats) if want_stats else maps
