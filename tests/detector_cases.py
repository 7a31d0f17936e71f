"""The single-layer cases of the detector kernels (tests/test_detector_gpu.py) and their operands: the smallest shapes at which
each part of csrc/dconv.hip can still go wrong.  Shared with tests/golden/make_detector_fixture.py, which measures on the CPU
the float32-vs-float64 deviation `e32` that the random-operand tolerance is built from.

A convolution case: (name, dict(n, h, w, cin, cout, k, stride, cin2, skip, f32_out)).  With cin2 > 0 the first source is the
HALF-resolution tensor [n, h/2, w/2, cin] and the second [n, h, w, cin2] (upsample + concatenate read); h, w are the
convolution's input size.
"""
from __future__ import annotations

import numpy as np

from tests import detector_ref as R


def _c(n, h, w, cin, cout, k, stride=1, cin2=0, skip=False, f32_out=False):
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, k=k, stride=stride, cin2=cin2, skip=skip, f32_out=f32_out)


CONV_CASES = [
    # k3 s1: 1x1 (every tap but the centre is padding), odd and ragged tiles, more than one pixel tile
    ("k3s1_1x1", _c(1, 1, 1, 32, 64, 3)),
    ("k3s1_2x3", _c(1, 2, 3, 32, 64, 3)),
    ("k3s1_5x7", _c(1, 5, 7, 32, 64, 3)),
    ("k3s1_13x13", _c(1, 13, 13, 32, 64, 3)),
    ("k3s1_5x7_n3", _c(3, 5, 7, 32, 64, 3)),                 # a flattened M must not read a neighbour image's rows as halo
    # first layer (Cin = 3 through the image stage), full and tiny
    ("first_3to32", _c(1, 8, 8, 3, 32, 3)),
    ("first_3to16", _c(2, 8, 8, 3, 16, 3)),
    # k3 s2: top / left padding only
    ("k3s2_2x2", _c(1, 2, 2, 32, 64, 3, 2)),
    ("k3s2_6x4", _c(1, 6, 4, 32, 64, 3, 2)),
    ("k3s2_26x26", _c(1, 26, 26, 32, 64, 3, 2)),
    ("k3s2_6x4_n3", _c(3, 6, 4, 32, 64, 3, 2)),
    # k1: shallow, deep K (split-K), the float32 output store with Cout not a multiple of 16
    ("k1_64to32", _c(1, 5, 7, 64, 32, 1)),
    ("k1_1024to512", _c(1, 2, 2, 1024, 512, 1)),
    ("k1_out18", _c(1, 5, 7, 64, 18, 1, f32_out=True)),
    ("k1_out255", _c(1, 5, 7, 64, 255, 1, f32_out=True)),
    ("k1_out18_deep", _c(1, 2, 2, 1024, 18, 1, f32_out=True)),
    # 3x3 with K = 4,608 (split-K order)
    ("k3_512to1024", _c(1, 2, 2, 512, 1024, 3)),
    # residual add
    ("k3s1_skip", _c(1, 5, 7, 32, 64, 3, skip=True)),
    ("k3_skip_deep", _c(1, 2, 2, 512, 1024, 3, skip=True)),
    # two-source read: upsampled (y >> 1, x >> 1) + route
    ("cat_256up_512_k1", _c(1, 4, 4, 256, 256, 1, cin2=512)),
    ("cat_128up_256_k3", _c(1, 4, 4, 128, 256, 3, cin2=256)),
    ("cat_n2_6x10", _c(2, 6, 10, 16, 32, 3, cin2=32)),
]
POOL_CASES = [("pool_s2_2x2", (1, 2, 2, 16, 2)), ("pool_s2_6x4", (2, 6, 4, 16, 2)), ("pool_s2_5x3", (1, 5, 3, 8, 2)),
              ("pool_s1_1x1", (1, 1, 1, 16, 1)), ("pool_s1_2x2", (1, 2, 2, 16, 1)), ("pool_s1_13x13", (2, 13, 13, 24, 1))]


def shapes(c):
    """(x, x2 or None, kernel, out) shapes of a case."""
    h, w = c["h"], c["w"]
    ho, wo = ((h - 2) // 2 + 1, (w - 2) // 2 + 1) if c["stride"] == 2 else (h, w)
    x = (c["n"], h // 2, w // 2, c["cin"]) if c["cin2"] else (c["n"], h, w, c["cin"])
    x2 = (c["n"], h, w, c["cin2"]) if c["cin2"] else None
    return x, x2, (c["k"], c["k"], c["cin"] + c["cin2"], c["cout"]), (c["n"], ho, wo, c["cout"])


def _idx(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.int64) for s in shape], indexing="ij")


def integer_operands(c):
    """Asymmetric small integers, sparse enough that sum |w| |x| + |bias| + |skip| < 2048 over every receptive field (asserted
    by the test): every partial sum, in whatever order it is taken, is then exact in binary16 and float32."""
    xs, x2s, ks, os_ = shapes(c)
    K = ks[0] * ks[1] * ks[2]
    m = max(1, -(-4 * K // 1200))                           # keep one value in m

    def image(shape, salt):
        n, y, x, ch = _idx(shape)
        h = n * 997 + y * 131 + x * 71 + ch * 37 + salt
        return np.where(h % m == 0, (h // m + y + 2 * x) % 5 - 2, 0).astype(np.float64)

    ky, kx, ci, co = _idx(ks)
    kernel = ((3 * (ky * ks[1] + kx) + 5 * ci + 7 * co) % 5 - 2).astype(np.float64)
    bias = (np.arange(ks[3]) % 7 - 3).astype(np.float64)
    skip = None
    if c["skip"]:
        n, y, x, ch = _idx(os_)
        skip = ((n + 3 * y + 5 * x + 7 * ch) % 9 - 4).astype(np.float64)
    return image(xs, 0), (image(x2s, 5) if x2s else None), kernel, bias, skip


def integer_expected(c, x, x2, kernel, bias, skip, leaky):
    """The kernel's arithmetic on exact operands: acc + bias exact; ONE float32 multiply by float32(0.1) for negative values;
    float32 add of the skip; one rounding to binary16 (none for the float32 output store).  Also returns the magnitude bound."""
    acc = R.conv(x, kernel, bias, c["stride"], False, x2=x2, dtype=np.float64)
    bound = R.conv(np.abs(x), np.abs(kernel), np.abs(bias), c["stride"], False, x2=None if x2 is None else np.abs(x2), dtype=np.float64)
    y = acc.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), acc)
    if leaky:
        y = np.where(y < 0, y * np.float32(0.1), y).astype(np.float32)
    if skip is not None:
        y = (y + skip.astype(np.float32)).astype(np.float32)
        bound = bound + np.abs(skip)
    return (y if c["f32_out"] else y.astype(np.float16).astype(np.float32)), float(bound.max())


def random_operands(c, seed):
    """Normal operands pre-rounded to binary16 (bias: float32), He-scaled so that outputs are of order one."""
    rng = np.random.RandomState(seed)
    xs, x2s, ks, os_ = shapes(c)
    h16 = lambda a: a.astype(np.float16).astype(np.float64)
    x = h16(rng.normal(0, 1, xs))
    x2 = h16(rng.normal(0, 1, x2s)) if x2s else None
    kernel = h16(rng.normal(0, np.sqrt(2.0 / (ks[0] * ks[1] * ks[2])), ks))
    bias = rng.normal(0, 0.3, ks[3]).astype(np.float32).astype(np.float64)
    skip = h16(rng.normal(0, 1, os_)) if c["skip"] else None
    return x, x2, kernel, bias, skip


def case_seed(name: str) -> int:
    return 1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100000


# ---- whole-body fixture inputs -------------------------------------------------------------------------------------------
KINDS = (("full", 0), ("tiny", 1))
SEEDS = {"full": 77, "tiny": 78}                  # whenet_hip.detector_weights.synthetic(kind, seed)
SIZES = ((32, 32), (64, 96))
ANCHORS = {"full": [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326],
           "tiny": [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]}


def sample_frame(i: int = 0) -> np.ndarray:
    """BGR uint8 frame of tests/golden/sample_frames.npz."""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_frames.npz")) as z:
        return np.ascontiguousarray(z[f"frame{i}"])


def fixture_image(h: int, w: int, frame: int = 0) -> np.ndarray:
    """image_data of YOLO.detect for a sample frame, float32 [1,h,w,3], through the numpy restatement of the letterbox."""
    from tests import letterbox_ref as LB
    return LB.image_data(LB.letterbox_u8(np.ascontiguousarray(sample_frame(frame)[:, :, ::-1]), h, w))
