"""Weights of the detector body (csrc/detector.cpp): tensor names and shapes, a seeded synthetic snapshot, and the packer.

The reference's detector loads a Keras HDF5 (`yolo_model.load_weights`, yolo_postprocess.py:66-79) whose file,
`head_detect.h5`, is not part of the reference tree.  As for WHENet itself, the snapshot format here is the flat WHNPACK1
container (whenet_hip/weights.py) with the Keras-native arrays under canonical names:

    dconvNNN/kernel   Keras HWIO [k, k, Cin, Cout]           every convolution, NNN from 000 in layer-creation order
    dbnNNN/gamma, beta, moving_mean, moving_variance [Cout]   every BatchNormalization, counted on their own from 000
    dconvNNN/bias     [Cout]                                  the output convolutions (no BatchNorm, linear)

The list comes from the engine's own layer table (`whenet_detector_spec`), so it cannot drift from what the library loads.
"""
from __future__ import annotations

import io
import struct
from typing import Dict, List, Tuple

import numpy as np

from . import _lib
from .weights import MAGIC, unpack

FULL, TINY = 0, 1


def tensors(kind: int, anchors_per_scale: int = 3, num_classes: int = 1) -> List[Tuple[str, Tuple[int, ...]]]:
    """[(name, shape)] of the snapshot of one body, in layer-creation order."""
    out: List[Tuple[str, Tuple[int, ...]]] = []
    ci = bi = 0
    for row in _lib.detector_spec(kind, anchors_per_scale, num_classes):
        if row["op"] != 0:
            continue
        out.append((f"dconv{ci:03d}/kernel", (row["k"], row["k"], row["cin"], row["cout"])))
        if row["bn"]:
            out += [(f"dbn{bi:03d}/{leaf}", (row["cout"],)) for leaf in ("gamma", "beta", "moving_mean", "moving_variance")]
            bi += 1
        else:
            out.append((f"dconv{ci:03d}/bias", (row["cout"],)))
        ci += 1
    return out


def synthetic(kind: int, seed: int, anchors_per_scale: int = 3, num_classes: int = 1) -> Dict[str, np.ndarray]:
    """Seeded random weights of one body: He-normal kernels (gain 2 / (1 + 0.1^2) for the LeakyReLU that follows, so a layer
    keeps its input's second moment), BatchNorm statistics near identity, and the convolution that closes a residual block
    scaled by 0.2 (gamma) so that the 23 blocks of the full body do not grow.  The kernels are 12 % (full) / 20 % (tiny) larger
    than that: on the smallest input the deep maps are 1 x 1 and eight of a 3 x 3 kernel's nine taps read padding.  The output convolutions are
    LeCun-normal with a small bias.  Every layer's rms stays within [0.1, 10] on the sample frames
    (tests/golden/make_detector_fixture.py checks it)."""
    rng = np.random.RandomState(seed)
    rows = [r for r in _lib.detector_spec(kind, anchors_per_scale, num_classes) if r["op"] == 0]
    w: Dict[str, np.ndarray] = {}
    bi = 0
    for ci, row in enumerate(rows):
        k, cin, cout = row["k"], row["cin"], row["cout"]
        fan_in = k * k * cin
        if row["bn"]:
            std = np.sqrt(2.0 / 1.01 / fan_in) * (1.2 if kind == TINY else 1.12)
            w[f"dconv{ci:03d}/kernel"] = rng.normal(0.0, std, (k, k, cin, cout)).astype(np.float32)
            gamma = rng.uniform(0.9, 1.1, cout)
            if row["skip"] >= 0:
                gamma *= 0.2
            w[f"dbn{bi:03d}/gamma"] = gamma.astype(np.float32)
            w[f"dbn{bi:03d}/beta"] = rng.normal(0.0, 0.05, cout).astype(np.float32)
            w[f"dbn{bi:03d}/moving_mean"] = rng.normal(0.0, 0.05, cout).astype(np.float32)
            w[f"dbn{bi:03d}/moving_variance"] = rng.uniform(0.9, 1.1, cout).astype(np.float32)
            bi += 1
        else:
            w[f"dconv{ci:03d}/kernel"] = rng.normal(0.0, np.sqrt(1.0 / fan_in), (k, k, cin, cout)).astype(np.float32)
            w[f"dconv{ci:03d}/bias"] = rng.normal(0.0, 0.1, cout).astype(np.float32)
    return w


def pack_named(names: List[Tuple[str, Tuple[int, ...]]], weights: Dict[str, np.ndarray]) -> bytes:
    """weights.py's WHNPACK1 writer for an arbitrary (name, shape) list."""
    table, payload = io.BytesIO(), io.BytesIO()
    for name, shape in names:
        if name not in weights:
            raise ValueError(f"missing tensor {name}")
        a = np.ascontiguousarray(weights[name], dtype="<f4")
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {a.shape} != expected {tuple(shape)}")
        off = payload.tell()
        pad = (-off) % 64
        payload.write(b"\0" * pad)
        off += pad
        raw = a.tobytes()
        payload.write(raw)
        nb = name.encode()
        table.write(struct.pack("<H", len(nb)) + nb + struct.pack("<BB", 0, a.ndim) + struct.pack(f"<{a.ndim}I", *a.shape) +
                    struct.pack("<QQ", off, len(raw)))
    tb = table.getvalue()
    data_off = 24 + len(tb)
    data_off += (-data_off) % 64
    blob = MAGIC + struct.pack("<IIQ", 1, len(names), data_off) + tb
    return blob + b"\0" * (data_off - len(blob)) + payload.getvalue()


def kind_of(weights: Dict[str, np.ndarray]) -> Tuple[int, int]:
    """(kind, A * (5 + C)) of a dict of detector arrays: 75 kernels = yolo_body, 13 = tiny_yolo_body."""
    n = sum(1 for k in weights if k.startswith("dconv") and k.endswith("/kernel"))
    if n not in (75, 13):
        raise ValueError(f"not a detector snapshot: {n} dconvNNN/kernel tensors (yolo_body has 75, tiny_yolo_body 13)")
    return (FULL if n == 75 else TINY), int(np.shape(weights[f"dconv{n - 1:03d}/kernel"])[3])


def pack(weights: Dict[str, np.ndarray]) -> bytes:
    kind, out_filters = kind_of(weights)
    return pack_named(tensors(kind, 1, out_filters - 5), weights)      # (the table depends on A * (5 + C) alone)


def parse(blob: bytes) -> Dict[str, np.ndarray]:
    return unpack(blob)


def save(path: str, weights: Dict[str, np.ndarray]) -> None:
    with open(path, "wb") as f:
        f.write(pack(weights))


def load(path: str) -> Dict[str, np.ndarray]:
    with open(path, "rb") as f:
        return unpack(f.read())
