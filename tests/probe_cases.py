"""Exact probe snapshots of the pose network: builders, plain numpy, no GPU (tests/test_probe_cpu.py checks every claim made here,
tests/test_probe_gpu.py runs the kernels on them).

The idea: small-integer weights, BatchNorm that folds to the identity (GAMMA, VAR below) and inputs that are 0 or 18..24 keep every value of an
MBConv block on integers for which Swish is exact in float32 (z <= -104 -> 0, 0 -> 0, 18 <= z <= 2048 -> z) and every
squeeze-excite gate on a saturated sigmoid (argument >= 24 -> 1, <= -104 -> 0).  Small integers are exact in binary16, in float32
and in the f32s hi/lo split, and every partial sum of them is exact in any order: ONE expected tensor holds for every dtype, every
kernel form and every batch position, bit for bit.  This tests structure (indexing, completeness of sums, wiring between crops and
channels, tile seams, padding), not rounding points.

Families (each a full weights dict with the names and shapes of spec.tensors(); W.pack takes it unchanged):
  routing        every 1x1 kernel one weight of 1 per output channel (a channel map that differs per layer), every depthwise kernel
                 one tap of 1 per channel (the tap walks with the channel), every gate forced to 1 (se_expand kernel 0, bias 32).
  dense_expand   expand kernels dense (1 or 2; the non-positive class -8), depthwise the centre tap, project routing.
  dense_dw       every tap of every channel non-zero (1 or 2; the non-positive class -8), expand and project routing.
  dense_project  project kernels dense signed (+-1, +-2), signed project_bn/beta, expand routing, depthwise the centre tap.
  Every family but routing: one output channel in eight of the expand stage (c % 8 == 3) and of the depthwise stage (c % 8 == 5)
  has all-non-positive weights scaled by 8 (pre-activation 0 or <= -144 -> output exactly 0), and squeeze-excite weights whose
  gates are exactly 0 or 1 as a function of the crop's own channel means (_design_se).

Inputs: crop i of (family, block) is a function of i alone (its generator is seeded with the crop index): a batch of n is the first
n of one sequence, no two crops are equal and the batch has no period.
  "lines" (routing, dense_dw): every channel carries impulses along a wrapped diagonal -- every row and every column of the image,
      so every tile edge and every halo edge of every tile plan -- or along every third row of it (the channel's sum then differs by
      3x between crops: the gates' thresholds sit in that gap).
  "sparse" (dense_expand, dense_project): 1 or 3 impulses per channel (as the bound sum |w||x| < 2048 allows), dealt over a
      permutation of the pixels so that no pixel holds more than its share; stride-2 blocks: over the pixels the centre tap reads.
  Both: the four corners of the image are set.

The heads stage (pooling + Dense + softmax + decode) and the whole forward have families of their own, HEAD_FAMILIES and the forward
snapshot: see the comment above them at the end of this module.
"""
from __future__ import annotations

import functools
from typing import Dict, Optional

import numpy as np

from whenet_hip import spec

FAMILIES = ("routing", "dense_expand", "dense_dw", "dense_project")
FAM_ID = {f: i for i, f in enumerate(FAMILIES)}
LINES = ("routing", "dense_dw")
BLOCKS = spec.blocks()
N_MAX = 17                       # the largest batch of the GPU tests; the gates are designed on these crops
N_CHAIN = 5                      # crops of the chained runs
# BatchNorm that folds to the identity: gamma = the float32 just above sqrt(1e-3), var = float32(gamma^2 - 1e-3) = 1.28e-10, mean 0.  In double,
# gamma / sqrt(var + 1e-3) = 1 + 4.4e-16 (var is so small against 1e-3 that its float32 rounding moves the sum by 3e-17 of it).
# The obvious choice, gamma 1 and var float32(0.999), folds to 1 - 6.4e-9: w -> w in float32 and in binary16, but the f32s weight
# images are split from the DOUBLE product (snapshot.cpp pack_pw_split: hi = f16(w'), lo = f16(w' - hi), 22 bits of it), so their
# lo halves would be -6.4e-9 w, not zero -- measured on the MI355X: with those weights every expand output that is a power of two
# >= 32 came back one float32 ulp low on the f32s handle (31.999998 for 32), f32 and f16 exact.  With this fold lo is 0.
GAMMA = np.nextafter(np.float32(np.sqrt(1e-3)), np.float32(1))          # (the float32 just above sqrt(1e-3): var > 0)
VAR = np.float32(float(GAMMA) ** 2 - 1e-3)
EXPAND_NEG, DW_NEG = 3, 5        # c % 8 of the non-positive classes
SE_BIAS_ON, SE_BIAS_OFF, SE_L = 32.0, -128.0, 64.0
HEAD = 17                        # "block" index of the head conv in inputs()


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _hi(i: int, ch: np.ndarray) -> np.ndarray:
    """1 = channel ch of crop i carries the full pattern, 0 = a third of it (or nothing, where a pixel's budget is tight).  Crops 0
    (mod 3) are high in the channels with ch % 3 != 1, crops 2 (mod 3) in those with ch % 3 != 0: two different patterns, neither
    constant over the channels, and every channel is high in one of them.  Crops 1 (mod 3) are low in every channel, so that the
    sums behind a DENSE kernel, which add all channels up, differ by 2x between the crops of a batch as well."""
    return np.where(i % 3 == 1, 0, np.where(i % 3 == 0, ch % 3 != 1, ch % 3 != 0)).astype(np.int64)


def _shape(index: int):
    if index == HEAD:
        return 7, 320, 1
    b = BLOCKS[index - 1]
    return b.h_in, b.cin, b.s


def sparse_budget(family: str) -> int:
    """Impulses a pixel may hold (over all channels) so that sum |w||x| stays below 2048.
    dense_expand: q * 24 * 8 in the non-positive expand channels, and 8 x the expand output (q * 24 * 1..2) in the non-positive
    depthwise channels: q = 6.  dense_project: six expanded channels per input channel, q * 6 * 24 * |p| with |p| = 2 for one
    entry in eight: q = 8.  (test_probe_cpu.py asserts the bound itself on every block.)"""
    return 6 if family == "dense_expand" else 8


def _one_input(family: str, index: int, i: int) -> np.ndarray:
    H, C, s = _shape(index)
    rng = np.random.default_rng([FAM_ID[family], index, i, 1])
    x = np.zeros((H, H, C), np.float32)
    ch = np.arange(C)
    hi = _hi(i, ch)
    if family in LINES and index != HEAD:
        for c in range(C):
            shift = int(rng.integers(H))
            rows = np.arange(H) if hi[c] else np.arange(int(rng.integers(3)), H, 3)
            cols = (rows + shift) % H if c % 2 == 0 else (shift - rows) % H
            x[rows, cols, c] = rng.integers(18, 25, size=len(rows))
    else:
        if s == 2:      # the pixels the centre tap of the stride-2 depthwise conv reads (odd rows and columns)
            pix = np.stack(np.meshgrid(np.arange(1, H, 2), np.arange(1, H, 2), indexing="ij"), -1).reshape(-1, 2)
        else:
            pix = np.stack(np.meshgrid(np.arange(H), np.arange(H), indexing="ij"), -1).reshape(-1, 2)
        pix = pix[rng.permutation(len(pix))]
        room = (sparse_budget(family) - 1) * len(pix)          # (one more per pixel for the corners)
        full = C - C // 3                          # (the high channels of a crop, at most)
        top = 3 if C + 2 * full <= room else (2 if C + full <= room else 1)
        mult = max(1, min(8, room // (4 * 3 * C))) if top == 3 else 1
        count = np.where(hi == 1, top, 1 if top > 1 else 0) * mult
        assert count.sum() <= room
        t = int(rng.integers(len(pix)))
        for c in range(C):
            p = pix[(t + np.arange(count[c])) % len(pix)]
            # (low channels 18..19, high channels 22..24: with 2 impulses against 1 the sums still differ by more than 2x)
            x[p[:, 0], p[:, 1], c] = rng.integers(22, 25, size=count[c]) if hi[c] else rng.integers(18, 20, size=count[c])
            t += int(count[c])
    for j, (r, c) in enumerate(((0, 0), (0, H - 1), (H - 1, 0), (H - 1, H - 1))):
        x[r, c, (i + j) % C] = 18 + (i + j) % 7
    return x


@functools.lru_cache(maxsize=None)
def _inputs_cached(family: str, index: int, n: int) -> np.ndarray:
    a = np.stack([_one_input(family, index, i) for i in range(n)])
    a.setflags(write=False)
    return a


def inputs(family: str, index: int, n: int) -> np.ndarray:
    """float32 [n, H, H, cin] of block `index` (HEAD: [n, 7, 7, 320]): values 0 or 18..24; the first n crops of the family's sequence."""
    return _inputs_cached(family, index, N_MAX)[:n] if n <= N_MAX else _inputs_cached(family, index, n)


def chain_inputs(family: str, n: int = N_CHAIN, first: int = 100) -> np.ndarray:
    """The input of the chained runs (op_block_range from block 1), crops first, first + 1, ... of the sequence.  routing: the lines pattern
    (so that impulses survive four stride-2 stages); the other families: 8 or 24 impulses per channel, no two on one pixel (a dense
    project kernel spreads every impulse over all output channels: the next block's sums must stay below 2048)."""
    if family == "routing":
        return np.stack([_one_input("routing", 1, first + i) for i in range(n)])
    H, C = 112, 32
    x = np.zeros((n, H, H, C), np.float32)
    for j in range(n):
        i = first + j
        rng = np.random.default_rng([FAM_ID[family], 0, i, 2])
        pix = rng.permutation(H * H - 2)[:24 * C] + 1                # (neither the first nor the last pixel)
        x[j, 0, 0, i % C] = 18 + i % 7
        x[j, H - 1, H - 1, (i + 3) % C] = 18 + (i + 3) % 7
        t = 0
        for c in range(C):
            cnt = 24 if _hi(i, np.array(c)) else 8
            p = pix[t:t + cnt]
            x[j, p // H, p % H, c] = rng.integers(18, 25, size=cnt)
            t += cnt
    return x


# ------------------------------------------------------------------------------------------------------------------------------
# the integer reference (float32 arithmetic on integers below 2^24 is exact; the squeeze-excite path in float64)
# ------------------------------------------------------------------------------------------------------------------------------
def in_exact_set(z: np.ndarray) -> np.ndarray:
    return (z <= -104) | (z == 0) | ((z >= 18) & (z <= 2048))


def swish_exact(z: np.ndarray) -> np.ndarray:
    """Swish on the exact set: z for 18 <= z <= 2048, 0 for z = 0 and z <= -104."""
    return np.where(z >= 18, z, 0).astype(z.dtype)


def _depthwise(x: np.ndarray, k3: np.ndarray, s: int, h_out: int, pad: int, bound: bool = False) -> np.ndarray:
    n, H, _, C = x.shape
    k = k3.shape[0]
    xp = np.zeros((n, H + k + 1, H + k + 1, C), x.dtype)
    xp[:, pad:pad + H, pad:pad + H] = x
    y = np.zeros((n, h_out, h_out, C), x.dtype)
    span = (h_out - 1) * s + 1
    for ky in range(k):
        for kx in range(k):
            wt = k3[ky, kx]
            if not wt.any():
                continue
            y += xp[:, ky:ky + span:s, kx:kx + span:s] * (np.abs(wt) if bound else wt)
    return y


def ref_block(x: np.ndarray, w: Dict[str, np.ndarray], index: int, mut: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """MBConv block `index` on integer input x, in the order of oracle.whenet_oracle.block, with BatchNorm as the identity plus beta.
    Returns the pre-activations (`expand_pre`, `dw_pre`), the tensors the GPU test compares (`expand`, `dw`, `gate`, `out`), the
    squeeze-excite internals (`sum`, `a`, `arg`) and the bound sum |w||x| + |bias| + |skip| per stage (`bound`).
    `mut`: one mutation of the arithmetic (test_probe_cpu.py's restatement of what a broken kernel would compute):
      {"squeeze_drop_last": 1}   the squeeze sum misses the last pixel
      {"mean_scale": 0.5}        1/(H W) halved
      {"gate_from": d}           crop i takes the gate of crop (i + d) % n
      {"halo_shift": (y0, y1)}   the output rows y0..y1-1 (one tile) see their top halo row shifted by one input row
      {"halo_neighbour": (y0, y1)}  ... see the previous crop's last input row as their top halo row"""
    mut = mut or {}
    b = BLOCKS[index - 1]
    p = f"b{index}"
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    r: Dict[str, np.ndarray] = {}
    bound = 0.0
    e = x
    if b.has_expand:
        we = w[f"{p}/expand/kernel"][0, 0]
        be = w[f"{p}/expand_bn/beta"]
        r["expand_pre"] = x @ we + be
        bound = max(bound, float((np.abs(x) @ np.abs(we) + np.abs(be)).max()))
        e = r["expand"] = swish_exact(r["expand_pre"])
    k3 = w[f"{p}/dw/kernel"][:, :, :, 0]
    bd = w[f"{p}/dw_bn/beta"]
    pad = spec.same_pad(b.h_in, b.k, b.s)[1]
    r["dw_pre"] = _depthwise(e, k3, b.s, b.h_out, pad) + bd
    for key in ("halo_shift", "halo_neighbour"):
        if key in mut:
            y0, y1 = mut[key]
            row = y0 * b.s - pad                      # the tile's top halo row (an input row)
            assert 1 <= row < b.h_in
            em = e.copy()
            em[:, row] = e[:, row - 1] if key == "halo_shift" else np.roll(e, 1, axis=0)[:, b.h_in - 1]
            r["dw_pre"] = r["dw_pre"].copy()
            r["dw_pre"][:, y0:y1] = (_depthwise(em, k3, b.s, b.h_out, pad) + bd)[:, y0:y1]
    bound = max(bound, float((_depthwise(np.abs(e), k3, b.s, b.h_out, pad, bound=True) + np.abs(bd)).max()))
    d = r["dw"] = swish_exact(r["dw_pre"])
    dsum = d.astype(np.float64)
    if mut.get("squeeze_drop_last"):
        dsum = dsum.copy()
        dsum[:, -1, -1, :] = 0
    S = r["sum"] = dsum.sum(axis=(1, 2))
    mean = S / (b.h_out * b.h_out) * mut.get("mean_scale", 1.0)
    w1 = w[f"{p}/se_reduce/kernel"][0, 0].astype(np.float64)
    r["se_products"] = float((np.abs(S)[:, :, None] * np.abs(w1)[None]).max())
    a = r["a"] = mean @ w1 + w[f"{p}/se_reduce/bias"].astype(np.float64)
    with np.errstate(over="ignore"):
        red = a / (1 + np.exp(-a))
    arg = r["arg"] = red @ w[f"{p}/se_expand/kernel"][0, 0].astype(np.float64) + w[f"{p}/se_expand/bias"].astype(np.float64)
    g = (arg >= 0).astype(np.float32)
    if "gate_from" in mut:
        g = np.roll(g, -mut["gate_from"], axis=0)
    r["gate"] = g
    wp = w[f"{p}/project/kernel"][0, 0]
    bp = w[f"{p}/project_bn/beta"]
    out = (d * g[:, None, None, :]) @ wp + bp
    bnd = (d * g[:, None, None, :]) @ np.abs(wp) + np.abs(bp)
    if b.has_skip:
        out = out + x
        bnd = bnd + np.abs(x)
    bound = max(bound, float(bnd.max()))
    r["out"] = out
    r["bound"] = np.float64(bound)
    return r


def ref_head(x: np.ndarray, w: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Head conv (exact integers), the pooled sum S (feat = S / 49) and the logits' features: logit j = S[:, head_feature(j)] / 49."""
    x = np.asarray(x, np.float32)
    pre = x @ w["head/conv/kernel"][0, 0] + w["head/bn/beta"]
    conv = swish_exact(pre)
    S = conv.astype(np.float64).sum(axis=(1, 2))
    bound = float((np.abs(x) @ np.abs(w["head/conv/kernel"][0, 0])).max())
    return {"pre": pre, "conv": conv, "S": S, "logits": S[:, head_feature(np.arange(spec.N_LOGITS))] / 49.0, "bound": np.float64(bound)}


def head_feature(j):
    return (j * 5 + 3) % spec.FEAT


# ------------------------------------------------------------------------------------------------------------------------------
# snapshots
# ------------------------------------------------------------------------------------------------------------------------------
def expand_map(index: int, c: np.ndarray, cin: int) -> np.ndarray:
    return (11 * c + index + 1) % cin          # (11 divides no channel count of the network: every k is read)


def project_map(index: int, o: np.ndarray, cexp: int, skip_neg: bool) -> np.ndarray:
    c = (13 * o + index) % cexp
    if skip_neg:
        while True:
            bad = (c % 8 == EXPAND_NEG) | (c % 8 == DW_NEG)
            if not bad.any():
                break
            c = np.where(bad, (c + 1) % cexp, c)
    return c


def dw_tap(index: int, c: np.ndarray, k: int) -> np.ndarray:
    return (c + index) % (k * k)


def _routing_1x1(src: np.ndarray, cin: int, cout: int, value: np.ndarray) -> np.ndarray:
    m = np.zeros((cin, cout), np.float32)
    m[src, np.arange(cout)] = value
    return m


def _design_se(S: np.ndarray, last: np.ndarray, hw: int, R: int, cexp: int):
    """Squeeze-excite weights whose gates are exactly 0 or 1 as a function of the crop's own channel sums S [crops, cexp].
    Reduce output j reads ONE channel c_j with an integer weight w (a power of two) and bias -w T / hw: a_j = w (S - T) / hw.
    se_expand: 64 on r_{c % R}, bias -128: argument -128 + 64 swish(a), >= 190 for a >= 5 and <= -128 for a <= 0.
    T = 0.75 v, where v is the smallest sum of the crops that are ON and the largest sum of the crops that are OFF is <= 0.55 v:
    with the mean halved every ON crop at v falls below T.  Where a crop has a non-zero LAST pixel in a channel, j = 0 takes the
    fine threshold T = S - last / 2 instead: the squeeze sum without its last pixel falls below it.
    `last` [crops, cexp]: the depthwise output at the last pixel."""
    w1 = np.zeros((cexp, R), np.float32)
    b1 = np.zeros(R, np.float32)
    limit = 2.0 ** 24

    def fits(c, w, T):
        a = w * (S[:, c] - T) / hw
        # (|bias| <= 1024 and a >= 5 or <= -2: were a kernel to keep the bias AND the mean in binary16, a would move by 0.5 + 0.7,
        # and 64 swish(3.8) - 128 = 110 is still beyond 24 + 16; a <= 900: 64 a stays a binary16 number)
        return (w * S[:, c].max() < limit and w <= 32768 and abs(w * T / hw) <= 1024 and ((a >= 5) | (a <= -2)).all()
                and (a >= 5).any() and (a <= -2).any() and a.max() <= 900)

    done = set()
    for c in range(cexp):                      # j = 0: the fine threshold
        i = int(np.argmax(last[:, c]))
        v = last[i, c]
        if v <= 0:
            continue
        T = S[i, c] - v / 2
        w = max(1.0, 2.0 ** np.ceil(np.log2(10 * hw / v)))
        if T > S[i, c] / 2 and fits(c, w, T):
            w1[c, 0], b1[0] = w, -w * T / hw
            done.add(0)
            break
    for j in range(R):
        if j in done:
            continue
        for c in list(range(j, cexp, R)) + list(range(cexp)):
            u = np.unique(S[:, c])
            best = None
            for k in range(1, len(u)):
                if u[k] > 0 and u[k - 1] <= 0.55 * u[k]:
                    on = int((S[:, c] >= u[k]).sum())
                    score = abs(on - len(S) / 2)
                    if best is None or score < best[0]:
                        best = (score, u[k])
            if best is None:
                continue
            v = best[1]
            T = 0.75 * v
            w = max(1.0, 2.0 ** np.ceil(np.log2(20 * hw / v)))
            if fits(c, w, T):
                w1[c, j], b1[j] = w, -w * T / hw
                done.add(j)
                break
        assert j in done, f"no channel with a usable gap for reduce output {j}"
    w2 = np.zeros((R, cexp), np.float32)
    w2[np.arange(cexp) % R, np.arange(cexp)] = SE_L
    return w1, b1, w2, np.full(cexp, SE_BIAS_OFF, np.float32)


def _bn(w: dict, prefix: str, c: int, beta=None) -> None:
    w[f"{prefix}/gamma"] = np.full(c, GAMMA, np.float32)
    w[f"{prefix}/beta"] = np.zeros(c, np.float32) if beta is None else np.asarray(beta, np.float32)
    w[f"{prefix}/mean"] = np.zeros(c, np.float32)
    w[f"{prefix}/var"] = np.full(c, VAR, np.float32)


@functools.lru_cache(maxsize=None)
def snapshot(family: str) -> Dict[str, np.ndarray]:
    """The full weights dict of a family (see the module docstring)."""
    assert family in FAMILIES
    routing = family == "routing"
    rng = np.random.default_rng([FAM_ID[family], 77])
    w: Dict[str, np.ndarray] = {"stem/conv/kernel": np.zeros((3, 3, 3, spec.STEM_C), np.float32)}
    _bn(w, "stem/bn", spec.STEM_C)
    chain = chain_inputs(family)
    for b in BLOCKS:
        p, L = f"b{b.index}", b.index
        ce = np.arange(b.cexp)
        e_neg = (ce % 8 == EXPAND_NEG) & (not routing) & b.has_expand
        d_neg = (ce % 8 == DW_NEG) & (not routing)
        if b.has_expand:
            if family == "dense_expand":
                m = (1 + (rng.integers(8, size=(b.cin, b.cexp)) == 0)).astype(np.float32)
                m[:, e_neg] = -8
            else:
                m = _routing_1x1(expand_map(L, ce, b.cin), b.cin, b.cexp, np.where(e_neg, -8, 1))
            w[f"{p}/expand/kernel"] = m.reshape(1, 1, b.cin, b.cexp)
            _bn(w, f"{p}/expand_bn", b.cexp)
        kk = b.k * b.k
        taps = np.zeros((kk, b.cexp), np.float32)
        if family == "dense_dw":
            taps[:] = 1 + (rng.integers(4, size=(kk, b.cexp)) == 0)
            taps[:, d_neg] = -8
        else:
            t = dw_tap(L, ce, b.k) if routing else np.full(b.cexp, (b.k // 2) * b.k + b.k // 2)
            taps[t, ce] = np.where(d_neg, -8, 1)
        w[f"{p}/dw/kernel"] = taps.reshape(b.k, b.k, b.cexp, 1)
        _bn(w, f"{p}/dw_bn", b.cexp)
        R = b.se_reduced
        # project
        beta = np.zeros(b.cout, np.float32)
        if family == "dense_project":
            mag = (1 + (rng.integers(8, size=(b.cexp, b.cout)) == 0)).astype(np.float32)
            if L == 1:
                # block 1 feeds block 2's Swish in the chained runs (op_block_range(1, 2), option fold12): a column is all 1..2 (output
                # 0 or >= 18) or all -6..-7 (output 0 or <= -108), beta 0.  Three columns in four are negative: block 2's dense
                # project then sums 24 positive expanded channels, not 96.  Block 2's non-positive expand channels (c % 8 == 3)
                # read columns 4 and 12 only (expand_map): positive ones, so -8 never meets a negative input.
                neg_col = np.arange(b.cout) % 4 != 0
                pk = np.where(neg_col[None, :], -5 - mag, mag)
            else:
                pk = mag * np.where(rng.integers(2, size=(b.cexp, b.cout)) == 0, -1, 1)
                beta = rng.integers(-3, 4, size=b.cout).astype(np.float32)
        else:
            pk = _routing_1x1(project_map(L, np.arange(b.cout), b.cexp, not routing), b.cexp, b.cout, np.ones(b.cout))
        w[f"{p}/project/kernel"] = pk.astype(np.float32).reshape(1, 1, b.cexp, b.cout)
        _bn(w, f"{p}/project_bn", b.cout, beta)
        # squeeze-excite: forced to 1 (routing), or designed on the sums of the probe crops (and of the chained crops: blocks 1, 2)
        w[f"{p}/se_reduce/kernel"] = np.zeros((1, 1, b.cexp, R), np.float32)
        w[f"{p}/se_reduce/bias"] = np.zeros(R, np.float32)
        w[f"{p}/se_expand/kernel"] = np.zeros((1, 1, R, b.cexp), np.float32)
        w[f"{p}/se_expand/bias"] = np.full(b.cexp, SE_BIAS_ON, np.float32)
        if not routing:
            xs = [inputs(family, L, N_MAX)]
            if L <= 2 and family == "dense_project":
                xs.append(chain)
            S, last = [], []
            for x in xs:
                for lo in range(0, len(x), 6):
                    r = ref_block(x[lo:lo + 6], w, L)
                    S.append(r["sum"])
                    last.append(r["dw"][:, -1, -1, :])
            w1, b1, w2, b2 = _design_se(np.concatenate(S), np.concatenate(last), b.h_out * b.h_out, R, b.cexp)
            w[f"{p}/se_reduce/kernel"] = w1.reshape(1, 1, b.cexp, R)
            w[f"{p}/se_reduce/bias"] = b1
            w[f"{p}/se_expand/kernel"] = w2.reshape(1, 1, R, b.cexp)
            w[f"{p}/se_expand/bias"] = b2
            if L == 1 and family == "dense_project":
                chain = ref_block(chain, w, 1)["out"]
    co = np.arange(spec.FEAT)
    if family == "dense_expand":
        m = (1 + (rng.integers(8, size=(320, spec.FEAT)) == 0)).astype(np.float32)
        m[:, co % 8 == EXPAND_NEG] = -8
    else:
        m = _routing_1x1((11 * co + 17) % 320, 320, spec.FEAT, np.where((co % 8 == EXPAND_NEG) & (not routing), -8, 1))
    w["head/conv/kernel"] = m.reshape(1, 1, 320, spec.FEAT)
    _bn(w, "head/bn", spec.FEAT)
    lo = 0
    for name, nb in (("yaw", spec.N_YAW), ("pitch", spec.N_PITCH), ("roll", spec.N_ROLL)):
        w[f"{name}/kernel"] = _routing_1x1(head_feature(lo + np.arange(nb)), spec.FEAT, nb, np.ones(nb))
        w[f"{name}/bias"] = np.zeros(nb, np.float32)
        lo += nb
    for a in w.values():
        a.setflags(write=False)
    return w


def gate_margin(arg: np.ndarray) -> float:
    """How far the arguments of the final sigmoid lie beyond 24 (gates of 1) and -104 (gates of 0): the smaller of the two."""
    on, off = arg[arg >= 0], arg[arg < 0]
    return float(min((on - 24).min() if on.size else np.inf, (-104 - off).min() if off.size else np.inf))


@functools.lru_cache(maxsize=None)
def _expected_cached(family: str, index: int) -> Dict[str, np.ndarray]:
    w = snapshot(family)
    x = inputs(family, index, N_MAX)
    parts = [ref_block(x[lo:lo + 6], w, index) for lo in range(0, N_MAX, 6)]
    keep = ("expand", "dw", "gate", "out")
    r = {k: np.concatenate([q[k] for q in parts]).astype(np.float32) for k in keep if k in parts[0]}
    # what test_probe_cpu.py asserts over all N_MAX crops
    r["bound"] = max(float(q["bound"]) for q in parts)
    r["exact"] = all(in_exact_set(q[k]).all() for q in parts for k in ("expand_pre", "dw_pre") if k in q)
    r["se_limit"] = max(max(float(q["se_products"]), float(np.abs(q["sum"]).max())) for q in parts)
    r["margin"] = min(gate_margin(q["arg"]) for q in parts)
    r["a_min"] = min(float(np.abs(q["a"]).min()) for q in parts)
    return r


def expected(family: str, index: int, n: int) -> Dict[str, np.ndarray]:
    """The ONE expected tensor of each stage (`expand`, `dw`, `gate`, `out`) for the first n crops of inputs(family, index, .)."""
    assert n <= N_MAX
    return {k: v[:n] for k, v in _expected_cached(family, index).items() if isinstance(v, np.ndarray)}


def stats(family: str, index: int) -> dict:
    """Over all N_MAX crops: `bound` (max sum |w||x| + |bias| + |skip|), `exact` (every pre-activation in the exact set), `se_limit`
    (largest squeeze sum and se_reduce product), `margin` (of the gate arguments), `a_min` (smallest |se_reduce output|)."""
    return {k: v for k, v in _expected_cached(family, index).items() if not isinstance(v, np.ndarray)}


def expected_chain(family: str, first: int, last: int, n: int = N_CHAIN) -> np.ndarray:
    x = chain_inputs(family, n)
    w = snapshot(family)
    for index in range(first, last + 1):
        x = ref_block(x, w, index)["out"]
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _routing_range_cached(first: int, last: int) -> np.ndarray:
    w = snapshot("routing")
    x = np.asarray(inputs("routing", first, N_MAX))
    for index in range(first, last + 1):
        r = ref_block(x, w, index)
        assert r["bound"] < 2048 and all(in_exact_set(r[k]).all() for k in ("expand_pre", "dw_pre") if k in r), (index, r["bound"])
        x = r["out"]
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def expected_routing_range(first: int, last: int, n: int) -> np.ndarray:
    """Blocks first..last of the routing snapshot chained on inputs("routing", first, n): the routing snapshot alone stays on the
    exact set through a chain (a dense block's output -- signed, or hundreds in every channel -- does not feed a Swish exactly)."""
    assert n <= N_MAX
    return _routing_range_cached(first, last)[:n]


def tile_rows(plan: dict, b) -> list:
    """[(y0, y1)] output-row ranges of a plan's tiles."""
    return [(t * plan["TH"], min((t + 1) * plan["TH"], b.h_out)) for t in range(plan["tiles_y"])]


def tile_cols(plan: dict, b) -> list:
    tw = b.h_out // plan["tiles_x"]
    return [(t * tw, (t + 1) * tw) for t in range(plan["tiles_x"])]


# ------------------------------------------------------------------------------------------------------------------------------
# the hardware premise: Swish of every argument of the exact set, through block 16's expand conv (7 x 7, 192 -> 1152 channels)
# ------------------------------------------------------------------------------------------------------------------------------
PREMISE_BLOCK = 16


def premise_snapshot() -> Dict[str, np.ndarray]:
    """The routing snapshot with block 16's expand conv as a sweep: output channels 0..575 read input channel c % 96 with weight 1,
    channels 576..1151 read input channel 96 + c % 96 with weight -1; the depthwise conv is the centre tap."""
    w = dict(snapshot("routing"))
    b = BLOCKS[PREMISE_BLOCK - 1]
    c = np.arange(b.cexp)
    pos = c < b.cexp // 2
    m = _routing_1x1(np.where(pos, c % 96, 96 + c % 96), b.cin, b.cexp, np.where(pos, 1, -1))
    w[f"b{PREMISE_BLOCK}/expand/kernel"] = m.reshape(1, 1, b.cin, b.cexp)
    taps = np.zeros((b.k * b.k, b.cexp), np.float32)
    taps[(b.k // 2) * b.k + b.k // 2] = 1
    w[f"b{PREMISE_BLOCK}/dw/kernel"] = taps.reshape(b.k, b.k, b.cexp, 1)
    return w


def premise_input() -> np.ndarray:
    """[1, 7, 7, 192]: channels 0..95 sweep 18..2048 over the pixels (then 0), channels 96..191 sweep 104..2048 (then 0): with the
    weights above the expand pre-activations are every integer of 18..2048 and of -2048..-104, and 0."""
    b = BLOCKS[PREMISE_BLOCK - 1]
    t = np.arange(49)[:, None] * 96 + np.arange(96)[None, :]
    lo = np.where(18 + t <= 2048, 18 + t, 0)
    hi = np.where(104 + t <= 2048, 104 + t, 0)
    return np.concatenate([lo, hi], axis=1).reshape(1, b.h_in, b.h_in, b.cin).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# the heads stage (pooling + Dense + softmax + decode: head.hip's two kernels) and the whole forward
#
# The arithmetic: float32(49 m) * (float32(1) / float32(49)) == m for every integer m of 0..4096 (test_probe_cpu.py) -- a head-conv
# output that is the SAME integer m at all 49 positions pools to exactly m in every pooling expression of the library (the sum 49 m
# is exact in any order, the one product rounds back to m).  With integer features and small-integer Dense weights and biases every
# partial sum of the Dense layer is an integer below 2^24: the logits are ONE bit pattern for the single-workgroup kernel, for the
# three instantiations of the four-workgroup kernel (whatever the split of the 1280-long contraction over workgroups and waves) and
# for all three dtypes.
#
# Families (the routing snapshot with another head conv and other Dense layers; FAMILIES and its four snapshots do not change):
#   dense_heads   head conv: feature co reads input channel (7 co + 5) % 320 with a positive integer weight (HEAD_GAIN: features 0 or
#                 18..2040); Dense kernels dense +-1, +-2; biases non-zero integers.  Expected logits: an exact integer array.
#   decode        feature 5 j + 3 reads input channel (3 j + 1) % 320 with weight 1 and logit j reads that feature alone with weight
#                 DECODE_GAIN = 5 (bias 0): logit j of crop i is 5 x (channel (3 j + 1) % 320 of crop i), an injective function of ONE
#                 input channel -- 252 distinct channels (head_feature() of the four old families collides at j and j + 64).  The
#                 crops are designed rows (DECODE_ROWS), not random ones.  Levels: 0 and 90, 95 .. 120: a row of 18s and 19s has a
#                 spread of 5, a one-hot row stands 120 above the rest (exp(-120) is 0 in float32).
#   forward       the routing snapshot with a routing stem (stem output co reads ONE tap of ONE input channel with weight 1), fed a
#                 float32 image of 0 or 18..24 through forward_f32, the real-valued entry point (no byte LUT; eager; stem and block
#                 1's depthwise conv as two kernels).  The routing Dense makes logit j = float32(S) * float32(1/49) with S the exact
#                 pooled sum of feature head_feature(j): ONE rounding.
# The uint8 forward (LUT, stemdw.hip, graph replay and lanes) cannot be made exact -- the LUT's values are not integers -- and stays
# with test_stem_fused_with_block_1_depthwise_is_bitwise_the_two_kernels and test_graph_replay_equals_eager.
# ------------------------------------------------------------------------------------------------------------------------------
HEAD_FAMILIES = ("dense_heads", "decode")
HEAD_GAIN = (1, 2, 3, 5, 8, 13, 40, 85)          # head conv weight of feature co: HEAD_GAIN[co % 8] (85 * 24 = 2040 <= 2048)
DECODE_GAIN = 5
HEADS = (("yaw", 0, spec.N_YAW), ("pitch", spec.N_YAW, spec.N_PITCH), ("roll", spec.N_YAW + spec.N_PITCH, spec.N_ROLL))
INV49 = np.float32(1) / np.float32(49)
# name -> (bins set to the row's maximum on the 120-bin head, on a 66-bin head).  Every other bin is lower.
DECODE_MAXIMA = {"max_first": ((0,), (0,)), "max_last": ((119,), (65,)), "max_63": ((63,), (63,)), "max_64": ((64,), (64,)),
                 "tie_63_64": ((63, 64), (63, 64)),          # across the lane 63 / lane 0 boundary (a lane's second element)
                 "tie_1_65": ((1, 65), (1, 65)),             # both in lane 1
                 # a lane's first element against a later lane's second one; on 66 bins (second elements: bins 64 and 65 only)
                 # against an EARLIER lane's second one, which a reduction ordered by lane alone would prefer
                 "tie_5_100": ((5, 100), (5, 64))}
DECODE_ROWS = ("equal", "max_first", "max_last", "max_63", "max_64", "tie_63_64", "tie_1_65", "tie_5_100", "one_hot", "narrow", "wide")


def head_const_inputs(family: str, n: int) -> np.ndarray:
    """float32 [n, 7, 7, 320], every channel constant over the 49 positions, values 0 or 18..24; crop i is a function of i alone.
    dense_heads: a quarter of the channels 0, the others random.  decode: the designed rows (decode_row) behind the logits'
    channels, random values in the 68 channels no logit reads."""
    assert family in HEAD_FAMILIES
    x = np.zeros((n, 7, 7, 320), np.float32)
    for i in range(n):
        rng = np.random.default_rng([10 + HEAD_FAMILIES.index(family), i, 3])
        v = np.where(rng.integers(4, size=320) == 0, 0, rng.integers(18, 25, size=320))
        if family == "decode":
            v[decode_channel(np.arange(spec.N_LOGITS))] = np.concatenate([decode_row(i, h) for h in range(3)])
        x[i] = v
    return x


def decode_channel(j):
    return (3 * j + 1) % 320


def decode_feature(j):
    return 5 * j + 3


def decode_kind(i: int, head: int) -> str:
    """Crop i puts a different kind of row on each head; every kind meets every head within 11 consecutive crops."""
    return DECODE_ROWS[(i + (0, 4, 7)[head]) % len(DECODE_ROWS)]


def decode_row(i: int, head: int) -> np.ndarray:
    """The input values (0 or 18..24; the logits are DECODE_GAIN x these) behind the bins of `head` (0 yaw, 1 pitch, 2 roll) of crop i."""
    nb = HEADS[head][2]
    kind = decode_kind(i, head)
    rng = np.random.default_rng([20, i, head])
    if kind == "equal":
        return np.full(nb, 18 + i % 7)
    if kind == "one_hot":
        v = np.zeros(nb, np.int64)
        v[int(rng.integers(nb))] = 24
        return v
    if kind == "narrow":                 # logits 90 or 95: half of the bins share the maximum, the others weigh e^-5 each
        return rng.integers(18, 20, size=nb)
    if kind == "wide":                   # logits 90, 95 .. 120, the maximum several times
        return rng.integers(18, 25, size=nb)
    v = rng.integers(18, 24, size=nb)    # below the maximum: 18..23
    v[list(DECODE_MAXIMA[kind][0 if nb == spec.N_YAW else 1])] = 24
    return v


@functools.lru_cache(maxsize=None)
def head_snapshot(family: str) -> Dict[str, np.ndarray]:
    """The weights dict of a heads family (see the comment above): the routing snapshot with its own head conv and Dense layers."""
    assert family in HEAD_FAMILIES
    w = dict(snapshot("routing"))
    co = np.arange(spec.FEAT)
    j = np.arange(spec.N_LOGITS)
    rng = np.random.default_rng([30, HEAD_FAMILIES.index(family)])
    if family == "dense_heads":
        conv = _routing_1x1((7 * co + 5) % 320, 320, spec.FEAT, np.asarray(HEAD_GAIN)[co % 8])
        dense = (rng.integers(1, 3, size=(spec.FEAT, spec.N_LOGITS)) * np.where(rng.integers(2, size=(spec.FEAT, spec.N_LOGITS)) == 0, -1, 1))
        bias = rng.integers(1, 8, size=spec.N_LOGITS) * np.where(rng.integers(2, size=spec.N_LOGITS) == 0, -1, 1)
    else:
        src = co % 320
        src[decode_feature(j)] = decode_channel(j)
        conv = _routing_1x1(src, 320, spec.FEAT, np.ones(spec.FEAT))
        dense = np.zeros((spec.FEAT, spec.N_LOGITS))
        dense[decode_feature(j), j] = DECODE_GAIN
        bias = np.zeros(spec.N_LOGITS)
    w["head/conv/kernel"] = conv.astype(np.float32).reshape(1, 1, 320, spec.FEAT)
    for name, lo, nb in HEADS:
        w[f"{name}/kernel"] = np.ascontiguousarray(dense[:, lo:lo + nb]).astype(np.float32)
        w[f"{name}/bias"] = bias[lo:lo + nb].astype(np.float32)
    for a in w.values():
        a.setflags(write=False)
    return w


def dense_matrix(w: Dict[str, np.ndarray]):
    """The three Dense layers as one [1280, 252] kernel and one [252] bias (float64)."""
    return (np.concatenate([w[f"{name}/kernel"] for name, _, _ in HEADS], axis=1).astype(np.float64),
            np.concatenate([w[f"{name}/bias"] for name, _, _ in HEADS]).astype(np.float64))


def decode_f64(logits: np.ndarray):
    """The float64 decode of the oracle's arithmetic (utils.softmax + the expectation over the bin indices, x 3 - 180 / - 99),
    restated: test_probe_cpu.py holds it to oracle.whenet_oracle.decode.  Returns ypr [n, 3]."""
    lg = np.asarray(logits, np.float64)
    out = []
    for h, (_, lo, nb) in enumerate(HEADS):
        z = lg[:, lo:lo + nb] - lg[:, lo:lo + nb].max(axis=1, keepdims=True)
        a = np.exp(z)
        out.append((a / a.sum(axis=1, keepdims=True) * np.arange(nb)).sum(axis=1) * 3 - (180 if h == 0 else 99))
    return np.stack(out, axis=1)


def argmax_first(logits: np.ndarray) -> np.ndarray:
    return np.stack([np.argmax(logits[:, lo:lo + nb], axis=1) for _, lo, nb in HEADS], axis=1).astype(np.int32)


def ref_heads(x: np.ndarray, w: Dict[str, np.ndarray], mut: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """Head conv, pooling, Dense, argmax and decode on an input that is constant over the 49 positions, in exact integers (float64).
    `feat` [n, 1280] and `logits` [n, 252] are integers; `argmax` is np.argmax per head (first index among equals), `ypr` the
    float64 decode.  `bound`: the largest sum |feat||W| + |bias| (every partial sum of the contraction is an integer below it).
    `mut`: one mutation (what a broken kernel would compute):
      {"drop_slice": (c0, c1)}   the contraction misses features c0..c1-1
      {"drop_partial": q}        the partial vector of workgroup q (features 320 q .. 320 q + 319) is not added
      {"bias_per_workgroup": 1}  every one of the four workgroups adds the bias
      {"argmax_last": 1}         the last index among equals
      {"argmax_first_64": 1}     the argmax looks at bins 0..63 of each head only (a lane's first element)
      {"logits_from": d}         crop i decodes the logits of crop (i + d) % n
      {"pitch_from": 119}        the pitch head starts at logit 119 instead of 120"""
    mut = mut or {}
    x = np.asarray(x, np.float64)
    assert (x == x[:, :1, :1, :]).all(), "the input must be constant over the 49 positions"
    pre = x[:, 0, 0, :] @ w["head/conv/kernel"][0, 0].astype(np.float64) + w["head/bn/beta"].astype(np.float64)
    assert in_exact_set(pre).all()
    feat = swish_exact(pre)
    D, bias = dense_matrix(w)
    f = feat
    if "drop_slice" in mut:
        f = feat.copy()
        f[:, mut["drop_slice"][0]:mut["drop_slice"][1]] = 0
    if "drop_partial" in mut:
        f = feat.copy()
        f[:, 320 * mut["drop_partial"]:320 * mut["drop_partial"] + 320] = 0
    logits = f @ D + bias * (4 if mut.get("bias_per_workgroup") else 1)
    seen = np.roll(logits, -mut["logits_from"], axis=0) if "logits_from" in mut else logits
    heads = [(name, mut.get("pitch_from", lo) if name == "pitch" else lo, nb) for name, lo, nb in HEADS]
    am = []
    for _, lo, nb in heads:
        row = seen[:, lo:lo + nb]
        if mut.get("argmax_first_64"):
            row = row[:, :64]
        am.append(row.shape[1] - 1 - np.argmax(row[:, ::-1], axis=1) if mut.get("argmax_last") else np.argmax(row, axis=1))
    shifted = np.concatenate([seen[:, lo:lo + nb] for _, lo, nb in heads], axis=1)
    return {"feat": feat, "logits": logits, "argmax": np.stack(am, axis=1).astype(np.int32), "ypr": decode_f64(shifted),
            "bound": np.float64((np.abs(feat) @ np.abs(D) + 4 * np.abs(bias)).max())}


@functools.lru_cache(maxsize=None)
def _expected_heads_cached(family: str, n: int):
    r = ref_heads(head_const_inputs(family, n), head_snapshot(family))
    out = {"feat": r["feat"].astype(np.float32), "logits": r["logits"].astype(np.float32), "argmax": r["argmax"], "ypr": r["ypr"]}
    assert np.array_equal(out["feat"], r["feat"]) and np.array_equal(out["logits"], r["logits"])
    for a in out.values():
        a.setflags(write=False)
    return out


def expected_heads(family: str, n: int) -> Dict[str, np.ndarray]:
    """`feat`, `logits` (float32 images of exact integers), `argmax` (int32) and `ypr` (float64) for head_const_inputs(family, n)."""
    big = _expected_heads_cached(family, N_MAX if n <= N_MAX else n)
    return {k: v[:n] for k, v in big.items()}


# ---- the whole forward ---------------------------------------------------------------------------------------------------------
def stem_tap(co):
    """Stem output co of the forward snapshot reads tap (ky, kx) of input channel ci: all 27 (tap, channel) pairs occur."""
    t = (5 * np.asarray(co) + 2) % 27
    return t // 9, (t // 3) % 3, t % 3


@functools.lru_cache(maxsize=None)
def forward_snapshot() -> Dict[str, np.ndarray]:
    w = dict(snapshot("routing"))
    k = np.zeros((3, 3, 3, spec.STEM_C), np.float32)
    co = np.arange(spec.STEM_C)
    k[stem_tap(co) + (co,)] = 1
    k.setflags(write=False)
    w["stem/conv/kernel"] = k
    return w


def forward_images(n: int, first: int = 0) -> np.ndarray:
    """float32 [n, 224, 224, 3], values 0 or 18..24 on the lines pattern: every channel carries TWO wrapped diagonals whose shifts
    differ in parity (a stride-2 tap (ky, kx) sees the pixels with row = ky and column = kx modulo 2 only: one diagonal reaches the
    taps with kx - ky even, the other one the rest; with a single diagonal half of the stem's channels would be zero), along every row
    or, in the crop's low channels (_hi), along every third row."""
    x = np.zeros((n, 224, 224, 3), np.float32)
    for j in range(n):
        i = first + j
        rng = np.random.default_rng([40, i])
        for c in range(3):
            shift = int(rng.integers(112)) * 2
            for d in range(2):
                rows = np.arange(224) if _hi(i, np.array(c)) else np.arange(int(rng.integers(3)), 224, 3)
                cols = (rows + shift + d + 2 * int(rng.integers(8))) % 224 if (c + d) % 2 == 0 else (shift + d + 2 * int(rng.integers(8)) - rows) % 224
                x[j, rows, cols, c] = rng.integers(18, 25, size=len(rows))
        for t, (r, c) in enumerate(((0, 0), (0, 223), (223, 0), (223, 223))):
            x[j, r, c, (i + t) % 3] = 18 + (i + t) % 7
    return x


def ref_stem(x: np.ndarray, w: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The stem on an integer image: Conv2D 3 x 3, stride 2, 'SAME' as the oracle pads the even 224 input (nothing before, one row
    and column of zeros after), BatchNorm as the identity plus beta, Swish on the exact set."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    out_size, before, after = spec.same_pad(spec.IMG, 3, 2)
    assert (out_size, before, after) == (112, 0, 1)
    xp = np.zeros((n, spec.IMG + 1, spec.IMG + 1, 3), np.float32)
    xp[:, :spec.IMG, :spec.IMG] = x
    k = w["stem/conv/kernel"]
    pre = np.zeros((n, 112, 112, spec.STEM_C), np.float32) + w["stem/bn/beta"]
    bound = np.zeros((n, 112, 112, spec.STEM_C), np.float32) + np.abs(w["stem/bn/beta"])
    for ky in range(3):
        for kx in range(3):
            patch = xp[:, ky:ky + 223:2, kx:kx + 223:2]
            pre += patch @ k[ky, kx]
            bound += np.abs(patch) @ np.abs(k[ky, kx])
    return {"pre": pre, "out": swish_exact(pre), "bound": np.float64(bound.max())}


@functools.lru_cache(maxsize=None)
def _expected_forward_cached(n: int, first: int):
    w = forward_snapshot()
    S, stats = [], {"bound": 0.0, "exact": True}
    for lo in range(0, n, 3):          # (three crops at a time: the 112 x 112 x 96 tensors of block 2)
        r = ref_stem(forward_images(min(3, n - lo), first + lo), w)
        stats["bound"] = max(stats["bound"], float(r["bound"]))
        stats["exact"] = stats["exact"] and bool(in_exact_set(r["pre"]).all())
        x = r["out"]
        for index in range(1, 17):
            b = ref_block(x, w, index)
            stats["bound"] = max(stats["bound"], float(b["bound"]))
            stats["exact"] = stats["exact"] and all(bool(in_exact_set(b[k]).all()) for k in ("expand_pre", "dw_pre") if k in b)
            stats["exact"] = stats["exact"] and bool((b["gate"] == 1).all())
            x = b["out"]
        h = ref_head(x, w)
        stats["bound"] = max(stats["bound"], float(h["bound"]))
        stats["exact"] = stats["exact"] and bool(in_exact_set(h["pre"]).all()) and float(h["conv"].max()) <= 2048
        S.append(h["S"])
    S = np.concatenate(S)
    S.setflags(write=False)
    return S, stats


def expected_forward(n: int, first: int = 0) -> Dict[str, np.ndarray]:
    """forward_snapshot() on forward_images(n, first): `S` [n, 1280] the exact pooled sums (float64 integers), `logits` [n, 252] =
    float32(S[head_feature(j)]) * float32(1/49) (one rounding: the routing Dense multiplies by 1 and adds zeros), `argmax`, `ypr`
    (float64 decode of those logits), and the chain's `bound` / `exact` (test_probe_cpu.py asserts them)."""
    S, stats = _expected_forward_cached(N_MAX if (first == 0 and n <= N_MAX) else n, first)
    S = S[:n]
    assert S.max() < 2 ** 24
    logits = S[:, head_feature(np.arange(spec.N_LOGITS))].astype(np.float32) * INV49
    return {"S": S, "logits": logits, "argmax": argmax_first(logits), "ypr": decode_f64(logits), **stats}


def head_pooled_inputs(family: str, n: int) -> np.ndarray:
    """Head inputs of the routing and dense_expand snapshots that are constant over the 49 positions (their features pool to
    integers).  routing: the crops of head_const_inputs("dense_heads", .).  dense_expand: ten non-zero channels per crop, which walk
    with the crop (10 x 24 x 8 = 1920 in the non-positive class: below 2048)."""
    assert family in ("routing", "dense_expand")
    x = head_const_inputs("dense_heads", n).copy()
    if family == "dense_expand":
        for i in range(n):
            keep = (7 * i + 32 * np.arange(10)) % 320
            v = np.zeros(320, np.float32)
            v[keep] = np.where(x[i, 0, 0, keep] == 0, 18 + i % 7, x[i, 0, 0, keep])
            x[i] = v
    return x
