"""The references of tests/test_nonfinite_gpu.py, pinned on the CPU: what numpy's argmax and the float64 decode give for rows of
NaN / Inf logits (the device decode is held to exactly this), the poison table, the NaN footprint of the float64 convolution,
and the drop-in class's decision between "the caller's own NaN" and "binary16's range" on a stand-in handle."""
import warnings

import numpy as np
import pytest

from oracle import whenet_oracle as O
from tests import detector_cases as DC
from tests import detector_ref as R
from tests import nonfinite_cases as NF
from whenet_hip import _lib


def test_poison_table():
    x = np.random.default_rng(0).standard_normal((6, 4, 5)).astype(np.float32)
    for kind in NF.KINDS:
        p = NF.poison(x, kind)
        assert p is not x and p.dtype == np.float32 and p.shape == x.shape
        changed = p.view(np.uint32) != x.view(np.uint32)
        if kind == "nan_all":
            assert np.isnan(p).all()
            continue
        where = (0, 0, 0) if kind == "nan_corner" else (3, 2, 2)
        assert changed.sum() == 1 and changed[where]
        v = p[where]
        with np.errstate(over="ignore"):
            huge16 = np.isinf(np.float16(v))
        assert {"nan_corner": np.isnan(v), "nan_centre": np.isnan(v), "pinf_one": v == np.inf, "ninf_one": v == -np.inf,
                "huge": np.isfinite(v) and huge16}[kind]
    b = np.stack([x, x + 1, x + 2])
    pb = NF.poisoned(b, [0, 2], "nan_centre")
    assert np.isnan(pb[0]).sum() == 1 and np.isnan(pb[2]).sum() == 1 and np.array_equal(pb[1], b[1]) and np.isfinite(b).all()
    assert NF.group_slots(5) == [0, 1, 3, 4] and NF.group_slots(17) == [0, 1, 3, 4, 15, 16] and NF.group_slots(1) == [0]


def test_argmax_and_decode_of_nan_and_inf_rows():
    """np.argmax: NaN counts as the maximum and the first NaN wins; a row of -inf or +inf gives 0.  The float64 decode is NaN for
    each of these rows -- a NaN anywhere, inf - inf, or 0 / 0 after exp(-inf - -inf)."""
    lg, literal, nan_angle, names = NF.decode_logits()
    assert names == ["all_nan", "nan_at_37", "nan_at_90_and_12_yaw", "all_ninf", "all_pinf", "pinf_at_5"]
    assert np.array_equal(O.argmax_bins(lg), literal), (O.argmax_bins(lg).tolist(), literal.tolist())
    assert literal[:2].tolist() == [[0, 0, 0], [37, 37, 37]] and literal[2, 0] == 12 and literal[3:].tolist() == [[0] * 3, [0] * 3, [5] * 3]
    with np.errstate(invalid="ignore"):
        for dtype in (np.float64, np.float32):
            ypr = np.stack(O.decode(lg.astype(dtype)), axis=1)
            assert np.array_equal(np.isnan(ypr), nan_angle), (dtype, ypr.tolist())
    assert nan_angle[2].tolist() == [True, False, False] and nan_angle[[0, 1, 3, 4, 5]].all()
    assert (np.abs(ypr[2, 1:]) <= 180).all()


@pytest.mark.parametrize("name", NF.DCONV_CASES)
def test_nan_footprint_of_the_float64_convolution(name):
    """detector_ref.R.conv on operands with ONE NaN element: NaN exactly where the receptive field holds it, in every channel, in
    the poisoned image only -- the mask the device kernel is compared with."""
    c = dict(DC.CONV_CASES)[name]
    x, x2, kernel, bias, _ = DC.random_operands(c, DC.case_seed(name))
    assert (kernel != 0).all()
    x, x2 = x.astype(np.float32), None if x2 is None else x2.astype(np.float32)
    j = c["n"] - 1
    for which in NF.dconv_sources(c):
        src = x if which == "x" else x2
        for kind, element in (("nan_corner", (0, 0)), ("nan_centre", (src.shape[1] // 2, src.shape[2] // 2))):
            px, px2 = (NF.poisoned(x, j, kind), x2) if which == "x" else (x, NF.poisoned(x2, j, kind))
            mask = np.isnan(R.conv(px, kernel, bias, c["stride"], True, x2=px2, dtype=np.float64))
            want = np.zeros(mask.shape, bool)
            want[j] = NF.nan_footprint(c, which, element)[:, :, None]
            assert np.array_equal(mask, want), (name, which, kind)
            assert want[j].any() and not want[j].all()


# ---- the drop-in class on a stand-in handle ---------------------------------------------------------------------------------------
class FakeHandle:
    """forward / forward_f32 of a handle whose f32s kernels answer `range_bad` crops with NaN and whose exact-float32 kernels
    answer `f32_bad` crops with NaN; a crop whose real-valued input is not finite is NaN under both."""

    def __init__(self, range_bad=(), f32_bad=()):
        self.range_bad, self.f32_bad, self.split_pw, self.calls, self.sets = set(range_bad), set(f32_bad), 1, 0, []

    def set_option(self, key, value):
        assert key == "split_pw"
        self.split_pw = value
        self.sets.append(value)

    def _run(self, n, dirty):
        self.calls += 1
        ypr = np.full((n, 3), 1.0 if self.split_pw else 2.0, np.float32)
        for i in range(n):
            if dirty[i] or i in self.f32_bad or (self.split_pw and i in self.range_bad):
                ypr[i] = np.nan
        return ypr, np.zeros((n, 3), np.int32), np.zeros((n, 252), np.float32)

    def forward(self, u8, want_logits=True):
        return self._run(len(u8), [False] * len(u8))

    def forward_f32(self, x, want_logits=True):
        return self._run(len(x), [not np.isfinite(x[i]).all() for i in range(len(x))])

    def close(self):
        pass


def model_on(handle):
    import whenet
    m = whenet.WHENet.__new__(whenet.WHENet)
    m._handle, m._dtype, m.last_logits, m.last_argmax = handle, _lib.F32S, None, None
    return m


def real_batch(n=4, nan=()):
    x = np.full((n, 224, 224, 3), 0.5, np.float32)
    for i in nan:
        x[i, 7, 7, 1] = np.nan
    return x


def caught(fn):
    with warnings.catch_warnings(record=True) as record:
        warnings.simplefilter("always")
        out = fn()
    return out, [str(w.message) for w in record]


def test_class_returns_the_callers_own_nan_without_a_switch():
    h = FakeHandle()
    m = model_on(h)
    (ypr, _, _), said = caught(lambda: m._forward_f32(real_batch(nan=[1, 3])))
    assert said == [] and h.calls == 1 and h.sets == [] and m._dtype == _lib.F32S
    assert np.isnan(ypr[[1, 3]]).all() and (ypr[[0, 2]] == 1.0).all()


def test_class_leaves_binary16_range_on_bytes_and_on_finite_real_input():
    for call in (lambda m: m._forward(np.zeros((4, 224, 224, 3), np.uint8)), lambda m: m._forward_f32(real_batch()),
                 lambda m: m._forward_f32(real_batch(nan=[0]))):              # (crop 0 the caller's NaN, crop 2 the range's)
        h = FakeHandle(range_bad=[2])
        m = model_on(h)
        (ypr, _, _), said = caught(lambda: call(m))
        assert len(said) == 1 and "binary16" in said[0] and h.calls == 2 and h.sets == [0] and m._dtype == _lib.F32
        assert (ypr[[1, 2, 3]] == 2.0).all()
        (_, _, _), said = caught(lambda: call(m))
        assert said == [] and h.calls == 3


def test_class_stays_f32s_where_exact_f32_is_nan_too():
    for call in (lambda m: m._forward(np.zeros((4, 224, 224, 3), np.uint8)), lambda m: m._forward_f32(real_batch())):
        h = FakeHandle(range_bad=[2], f32_bad=[2])
        m = model_on(h)
        (ypr, _, _), said = caught(lambda: call(m))
        assert len(said) == 1 and "binary16" not in said[0] and h.calls == 2 and h.sets == [0, 1] and m._dtype == _lib.F32S
        assert np.isnan(ypr[2]).all() and (ypr[[0, 1, 3]] == 1.0).all()                 # (the f32s run's values)


def test_other_dtypes_never_look():
    h = FakeHandle(f32_bad=[0])
    m = model_on(h)
    m._dtype = _lib.F32
    (ypr, _, _), said = caught(lambda: m._forward(np.zeros((2, 224, 224, 3), np.uint8)))
    assert said == [] and h.calls == 1 and h.sets == [] and np.isnan(ypr[0]).all()
