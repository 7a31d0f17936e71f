"""Non-finite values: the one table of cases that tests/test_nonfinite_gpu.py (isolation of a poisoned crop from its batch, what
the poisoned crop itself returns, the decode) and the CPU rows of tests/test_oracle.py / tests/test_detector_cpu.py share.

Every batch-invariance test of the suite runs on finite data, which cannot see a term that crosses from one crop into another
with weight zero: 0 * x = 0 and the bits agree.  With x = Inf or NaN the same term is NaN.  So one crop (or detector image) of a
batch is poisoned here, and every OTHER crop's output must stay, byte for byte, what the clean batch gave.

The snapshot is the seeded one (whenet_hip.weights.synthetic(1234)): its He-normal kernels have no zeros.  The probe snapshots of
tests/probe_cases.py are sparse integers whose zero project weights would hide a leak; they are not used.
"""
from __future__ import annotations

import numpy as np

KINDS = ("nan_all", "nan_corner", "nan_centre", "pinf_one", "ninf_one", "huge")
# the kinds after which nothing of the poisoned crop may come back finite ("never a silently wrong number"); `huge` (finite in
# float32, Inf once stored as binary16) is held to isolation only: what an f32 handle returns for it depends on the weights
POISON_SELF = ("nan_all", "nan_corner", "nan_centre", "pinf_one", "ninf_one")
HUGE = np.float32(3e38)


def poison(x_j: np.ndarray, kind: str) -> np.ndarray:
    """A copy of one crop or image [h, w, c] float32 with the kind's elements set."""
    assert x_j.ndim == 3 and x_j.dtype == np.float32, (x_j.shape, x_j.dtype)
    h, w, c = x_j.shape
    out = x_j.copy()
    centre = (h // 2, w // 2, c // 2)
    if kind == "nan_all":
        out[...] = np.nan
    elif kind == "nan_corner":
        out[0, 0, 0] = np.nan
    elif kind == "nan_centre":
        out[centre] = np.nan
    elif kind == "pinf_one":
        out[centre] = np.inf
    elif kind == "ninf_one":
        out[centre] = -np.inf
    elif kind == "huge":
        out[centre] = HUGE
    else:
        raise ValueError(kind)
    return out


def poisoned(x: np.ndarray, js, kind: str) -> np.ndarray:
    """A copy of the batch x [n, h, w, c] with crops `js` (an index or several) poisoned."""
    out = x.copy()
    for j in np.atleast_1d(js):
        out[j] = poison(x[j], kind)
    return out


def group_slots(n: int):
    """The crops to poison in a batch that front7.hip / head7.hip cut into groups of 2 (up to 16 crops) or 4: every slot of a
    group, the first crop of the next group, and the last two crops -- the last one is what a tail group copies into its idle
    slots."""
    return sorted({j for j in (0, 1, 3, 4, n - 2, n - 1) if 0 <= j < n})


def block_operands(index: int, n: int, salt: int = 0) -> np.ndarray:
    """Seeded normals in block `index`'s input shape, as tests/test_static_shapes_gpu.py draws them for op_block."""
    from whenet_hip import spec
    b = spec.blocks()[index - 1]
    return np.random.default_rng(200 + index + 1000 * salt).standard_normal((n, b.h_in, b.h_in, b.cin)).astype(np.float32)


def head_operands(n: int, salt: int = 0) -> np.ndarray:
    return np.random.default_rng(217 + 1000 * salt).standard_normal((n, 7, 7, 320)).astype(np.float32)


# ---- the decode: logit rows [252] = yaw 120 | pitch 66 | roll 66 -----------------------------------------------------------------
N_YAW, N_PITCH = 120, 66
HEADS = ((0, N_YAW), (N_YAW, N_YAW + N_PITCH), (N_YAW + N_PITCH, N_YAW + 2 * N_PITCH))


def decode_rows():
    """(name, logits [252] float32, argmax literal [3], angle is NaN [3]) -- np.argmax's rule: NaN counts as the maximum and the
    first NaN wins; a row without NaN gives the first index of its maximum (0 for a row of -inf).  The angle of a head is NaN
    wherever the float64 softmax is: a NaN anywhere, +inf anywhere (inf - inf), or -inf throughout."""
    normal = np.random.default_rng(77).standard_normal(252).astype(np.float32)
    rows = []

    def row(name, fill, argmax, nan_angle=(True, True, True)):
        lg = normal.copy()
        fill(lg)
        rows.append((name, lg, np.array(argmax, np.int32), np.array(nan_angle)))

    def all_of(v):
        def fill(lg):
            lg[:] = v
        return fill

    def at(v, *bins, heads=(0, 1, 2)):
        def fill(lg):
            for k in heads:
                for b in bins:
                    lg[HEADS[k][0] + b] = v
        return fill

    row("all_nan", all_of(np.nan), (0, 0, 0))
    row("nan_at_37", at(np.nan, 37), (37, 37, 37))
    yaw_only = [int(np.argmax(normal[lo:hi])) for lo, hi in HEADS]
    row("nan_at_90_and_12_yaw", at(np.nan, 90, 12, heads=(0,)), (12, yaw_only[1], yaw_only[2]), (True, False, False))
    row("all_ninf", all_of(-np.inf), (0, 0, 0))
    row("all_pinf", all_of(np.inf), (0, 0, 0))
    row("pinf_at_5", at(np.inf, 5), (5, 5, 5))
    return rows


def decode_logits():
    rows = decode_rows()
    return (np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]), [r[0] for r in rows])


# ---- the detector ---------------------------------------------------------------------------------------------------------------
DCONV_CASES = ("k3s1_5x7_n3", "k3s2_6x4_n3", "first_3to16", "cat_n2_6x10")
DPOOL_CASES = ("pool_s2_6x4", "pool_s1_13x13")
DCONV_KINDS = ("nan_corner", "pinf_one")
DCONV_FOOTPRINT_KINDS = ("nan_corner", "nan_centre")


def dconv_sources(c):
    """The sources of a convolution case that can be poisoned: "x" always, and "x2" where the case reads two -- for cat_n2_6x10,
    x2 is the route source (full resolution) and x the half-resolution one."""
    return ("x2", "x") if c["cin2"] else ("x",)


def nan_footprint(c, which: str, element) -> np.ndarray:
    """The output positions [ho, wo] whose receptive field holds input element (y, x) of source `which`: the halo is substituted
    zeros, not multiplied ones, so exactly these are NaN (in every output channel: no weight of the random operands is zero)."""
    h, w, k, s = c["h"], c["w"], c["k"], c["stride"]
    ho, wo = ((h - 2) // 2 + 1, (w - 2) // 2 + 1) if s == 2 else (h, w)
    ey, ex = element
    ys, xs = ((2 * ey, 2 * ey + 1), (2 * ex, 2 * ex + 1)) if (c["cin2"] and which == "x") else ((ey,), (ex,))     # (upsampled by 2)
    pad = 1 if s == 2 else k // 2                      # stride 2 pads top / left by one; stride 1 is 'same'
    mask = np.zeros((ho, wo), bool)
    for oy in range(ho):
        for ox in range(wo):
            for iy in ys:
                for ix in xs:
                    if 0 <= iy - (oy * s - pad) < k and 0 <= ix - (ox * s - pad) < k:
                        mask[oy, ox] = True
    return mask
