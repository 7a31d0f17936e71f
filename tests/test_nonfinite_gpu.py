"""Non-finite values on the GPU (pytest -m gpu), all three dtypes: a poisoned crop (NaN, +-Inf, or 3e38 -- Inf once stored as
binary16) must not reach its neighbours in the batch, and must itself come back as NaN, never as a finite number.

The batch-invariance tests of the suite run on finite data, and finite data cannot see a term that crosses from one crop (or one
detector image) into another with weight zero: 0 * x = 0.  With x = Inf or NaN it is NaN.  The kernels that put several crops
into one workgroup are where such a term can hide: front7.hip / head7.hip (groups of 2 or 4 crops, a tail group filled with
copies of the last crop), the split-K forms of pw.hip (32 B2 rows spanning up to three crops), mb7.hip, the matrix-core excite of
se_fuse = 3, and dconv.hip (M flattened over the images of a clip).

The pattern of every isolation test: run the clean batch and keep its outputs; run ANOTHER input of the same shape, so that rows
a launch fails to write differ from what is expected (tests/test_probe_gpu.py::scrub_block gives the reason); run the batch with
crop j poisoned; every output row of every crop != j is, byte for byte (tobytes), the clean run's.  No tolerance anywhere, but the
one of the dconv footprint test, which is tests/test_detector_gpu.py::test_conv_random_against_float64's (binary16 storage) and
tests/test_detector_f32_gpu.py::test_conv_against_float64's (float32 storage), with the committed e32.

The decode rows reach the single-workgroup kernel's argmax through op_decode; the split kernel's copy of the same lines (one
device function serves both) sees rows of NaN through op_head and forward_f32 under split_heads = 1: a NaN feature makes every
logit of the crop NaN, so a partly-NaN row cannot be produced by a Dense layer with finite weights."""
import functools

import numpy as np
import pytest

from oracle import whenet_oracle as O
from tests import detector_cases as DC
from tests import detector_f32_cases as FC
from tests import detector_ref as R
from tests import nonfinite_cases as NF
from tests.test_probe_gpu import SETTINGS, applies, options
from whenet_hip import _lib, synth, weights as W

pytestmark = pytest.mark.gpu
DTYPES = {"f32": _lib.F32, "f16": _lib.F16, "f32s": _lib.F32S}
NAMES = list(DTYPES)
HEAD_MATRIX = [{"split_heads": s, "head_fuse": f} for s in (0, 1) for f in (0, 1)]
SETTINGS_7_12 = [{}, {"se_fuse": 0}, {"se_fuse": 2}, {"se_fuse": 3}, {"front_impl": 0}, {"front_impl": 2}, {"pw_staged": 0}]
N_FORWARD = 65                  # two chains of 33 and 32 crops; every static row of the project GEMMs' tables live
N_TILES = {**{i: 21 for i in range(7, 12)}, **{i: 55 for i in range(12, 17)}}         # (tests/test_static_shapes_gpu.py)


def sid(setting):
    return "-".join(f"{k}{v}" for k, v in setting.items()) or "default"


@pytest.fixture(scope="module")
def handles(weights):
    """get(dtype name) -> the handle of the seeded snapshot in that dtype, created on first use."""
    blob = W.pack(weights)
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _lib.Handle(blob, device=0, dtype=DTYPES[name])
        return cache[name]

    yield get
    for h in cache.values():
        h.close()


@functools.lru_cache(maxsize=None)
def block_x(index, n, salt=0):
    x = NF.block_operands(index, n, salt)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def head_x(n, salt=0):
    x = NF.head_operands(n, salt)
    x.setflags(write=False)
    return x


def others_same(got, want, js, tag):
    """Every row of every crop not in `js` is bitwise the clean run's; the message names the crops that differ."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype and got.itemsize == 4, (tag, got.shape, want.shape)
    keep = np.ones(len(got), bool)
    keep[np.atleast_1d(js)] = False
    g, w = got[keep], want[keep]
    if g.tobytes() == w.tobytes():
        return
    diff = (g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1)
    crops = np.flatnonzero(keep)[diff.any(axis=1)]
    nan = np.isnan(g.reshape(len(g), -1)[diff]).sum() if g.dtype == np.float32 else 0
    raise AssertionError(f"{tag}: poisoned crop(s) {np.atleast_1d(js).tolist()} changed crop(s) {crops.tolist()}: "
                         f"{int(diff.sum())} elements differ, {int(nan)} of them NaN")


def all_nan(a, tag):
    bad = ~np.isnan(a)
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {a.size} elements are not NaN, first {np.asarray(a)[bad][:5].tolist()}"


def wrote_gate(r):
    return not np.isnan(r["gate"]).all()           # (NaN throughout where no launch writes the gate: tests/test_probe_gpu.py)


class BlockRun:
    """op_block of one (handle, block, batch, setting): the clean outputs once, then poisoned runs, each behind a run on another
    input of the same shape."""

    def __init__(self, h, index, n, setting, tag):
        self.h, self.index, self.n, self.setting, self.tag = h, index, n, setting, f"{tag} block {index} n={n} {setting}"
        self.x, self.other = block_x(index, n), block_x(index, n, 1)
        with options(h, setting):
            self.clean = h.op_block(index, self.x)
        for key in ("dw", "out"):
            assert np.isfinite(self.clean[key]).all(), (self.tag, key)

    def poisoned(self, j, kind):
        with options(self.h, self.setting):
            r = self.h.op_block(self.index, self.other)
            assert r["dw"].tobytes() != self.clean["dw"].tobytes() and r["out"].tobytes() != self.clean["out"].tobytes()
            r = self.h.op_block(self.index, NF.poisoned(self.x, j, kind))
        tag = f"{self.tag} crop {j} {kind}"
        others_same(r["dw"], self.clean["dw"], j, tag + " dw")
        others_same(r["out"], self.clean["out"], j, tag + " out")
        assert wrote_gate(r) == wrote_gate(self.clean), tag
        if wrote_gate(self.clean):
            others_same(r["gate"], self.clean["gate"], j, tag + " gate")
        return r


# ---- blocks 7-16: groups of 2 and 4 crops, three crops per project workgroup ------------------------------------------------------
@pytest.mark.parametrize("index", range(7, 17))
@pytest.mark.parametrize("name", NAMES)
def test_blocks_7_to_16_keep_a_poisoned_crop_to_itself(handles, name, index):
    """n = 5 (front7 / head7 form pairs; a project workgroup holds three crops at HW = 49) and n = 17 (groups of four and a tail
    group of one); j: each slot of a group, the first crop of the next group, the crop the tail group replicates."""
    for n in (5, 17):
        run = BlockRun(handles(name), index, n, {}, name)
        for j in NF.group_slots(n):
            for kind in ("nan_centre", "pinf_one", "huge"):
                run.poisoned(j, kind)


@pytest.mark.parametrize("index", range(7, 17))
@pytest.mark.parametrize("name", NAMES)
def test_blocks_7_to_16_larger_row_tiles(handles, name, index):
    """The smallest batches at which the split-K GEMMs take 2 x 2 tiles: 21 crops on blocks 7-11, 55 on the 7 x 7 maps (64 rows
    spanning three crops)."""
    n = N_TILES[index]
    run = BlockRun(handles(name), index, n, {}, name)
    for j in (0, n // 2, n - 1):
        run.poisoned(j, "nan_centre")


# ---- blocks 1-6: one crop per front workgroup, 128 GEMM rows spanning two crops ---------------------------------------------------
@pytest.mark.parametrize("index", range(1, 7))
@pytest.mark.parametrize("name", NAMES)
def test_blocks_1_to_6_keep_a_poisoned_crop_to_itself(handles, name, index):
    """op_block_range(i, i): the block output only (op_block would copy the expanded 112 x 112 tensor back on every call)."""
    h, n = handles(name), 3
    x, other = block_x(index, n), block_x(index, n, 1)
    clean = h.op_block_range(index, index, x)
    assert np.isfinite(clean).all()
    for j in range(n):
        for kind in ("nan_corner", "huge"):
            assert h.op_block_range(index, index, other).tobytes() != clean.tobytes()
            got = h.op_block_range(index, index, NF.poisoned(x, j, kind))
            others_same(got, clean, j, f"{name} block {index} n={n} crop {j} {kind} out")


# ---- the options that change the kernel form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [s for s in SETTINGS if applies(s, "f32") and applies(s, "f16")], ids=sid)
@pytest.mark.parametrize("index", range(13, 17))
@pytest.mark.parametrize("name", NAMES)
def test_blocks_13_to_16_under_every_option(handles, name, index, setting):
    run = BlockRun(handles(name), index, 17, setting, name)
    for j in (1, 16):
        run.poisoned(j, "nan_centre")


@pytest.mark.parametrize("index", range(13, 17))
def test_blocks_13_to_16_with_the_exact_f32_kernels_of_an_f32s_handle(handles, index):
    """SETTINGS' split_pw = 0: the one setting that applies to a single dtype."""
    assert [s for s in SETTINGS if not applies(s, "f32") or not applies(s, "f16")] == [{"split_pw": 0}]
    run = BlockRun(handles("f32s"), index, 17, {"split_pw": 0}, "f32s")
    for j in (1, 16):
        run.poisoned(j, "nan_centre")


@pytest.mark.parametrize("setting", SETTINGS_7_12, ids=sid)
@pytest.mark.parametrize("index", range(7, 13))
@pytest.mark.parametrize("name", NAMES)
def test_blocks_7_to_12_under_the_options(handles, name, index, setting):
    run = BlockRun(handles(name), index, 17, setting, name)
    for j in (1, 16):
        run.poisoned(j, "nan_centre")


# ---- the poisoned crop itself: never a silently wrong number ----------------------------------------------------------------------
@pytest.mark.parametrize("index", range(1, 17))
@pytest.mark.parametrize("name", NAMES)
def test_block_output_of_a_poisoned_crop_is_nan(handles, name, index):
    """The squeeze-excite gate multiplies the whole crop: one NaN or Inf element of the input (the Swish of -inf is NaN, and so is
    inf - inf in the depthwise sums) makes every element of out[j] NaN; with the crop NaN throughout, dw[j] as well."""
    n, j = (3, 1) if index <= 6 else (5, 3)
    run = BlockRun(handles(name), index, n, {}, name)
    for kind in NF.POISON_SELF:
        r = run.poisoned(j, kind)
        all_nan(r["out"][j], f"{name} block {index} {kind} out[{j}]")
        if kind == "nan_all":
            all_nan(r["dw"][j], f"{name} block {index} {kind} dw[{j}]")


# ---- the head -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", HEAD_MATRIX, ids=sid)
@pytest.mark.parametrize("name", NAMES)
def test_head_keeps_a_poisoned_crop_to_itself(handles, name, setting):
    """op_head at n = 5 and 17 under split_heads 0 / 1 x head_fuse 0 / 1: pooled features, logits, angles and argmax of the other
    crops are bitwise the clean run's.  A NaN element gives the crop NaN logits, and the argmax np.argmax gives for them: 0."""
    h = handles(name)
    for n in (5, 17):
        x, other = head_x(n), head_x(n, 1)
        with options(h, setting):
            clean = h.op_head(x)
            assert all(np.isfinite(clean[k]).all() for k in ("feat", "logits", "ypr"))
            for j in NF.group_slots(n):
                for kind in ("nan_centre", "pinf_one", "huge"):
                    assert h.op_head(other)["logits"].tobytes() != clean["logits"].tobytes()
                    r = h.op_head(NF.poisoned(x, j, kind))
                    for key in ("feat", "logits", "ypr", "argmax"):
                        others_same(r[key], clean[key], j, f"{name} head n={n} {setting} crop {j} {kind} {key}")
                    if kind == "nan_centre":
                        all_nan(r["logits"][j], f"{name} head n={n} {setting} logits[{j}]")
                        all_nan(r["ypr"][j], f"{name} head n={n} {setting} ypr[{j}]")
                        assert r["argmax"][j].tolist() == O.argmax_bins(r["logits"][j:j + 1])[0].tolist() == [0, 0, 0]


# ---- the whole forward ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def images():
    """(65 normalised scene crops, 65 others): float32 [65, 224, 224, 3], 39 MB each, drawn once and never written to."""
    a = O.normalise(synth.scene_crops(N_FORWARD, seed=51)).astype(np.float32)
    b = O.normalise(synth.scene_crops(N_FORWARD, seed=52)).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def check_forward(h, x, other, clean, js, kind, tag):
    assert h.forward_f32(other)[2].tobytes() != clean[2].tobytes()
    got = h.forward_f32(NF.poisoned(x, js, kind))
    for g, c, key in zip(got, clean, ("ypr", "argmax", "logits")):
        others_same(g, c, js, f"{tag} crops {js} {kind} {key}")
    if kind in NF.POISON_SELF:
        for j in np.atleast_1d(js):
            all_nan(got[0][j], f"{tag} {kind} ypr[{j}]")
            all_nan(got[2][j], f"{tag} {kind} logits[{j}]")
            assert got[1][j].tolist() == O.argmax_bins(got[2][j:j + 1])[0].tolist() == [0, 0, 0], (tag, kind, j, got[1][j])


@pytest.mark.parametrize("lanes", [2, 1])
@pytest.mark.parametrize("name", NAMES)
def test_forward_keeps_poisoned_crops_to_themselves(handles, images, name, lanes):
    """forward_f32 at 65 crops under the default options (two chains of 33 and 32 crops) and as one chain (lanes = 1): the last
    crop of the first chain, the first of the second, both ends; each alone, then all four together."""
    h = handles(name)
    x, other = images
    h.set_option("lanes", lanes)
    try:
        clean = h.forward_f32(x)
        assert np.isfinite(clean[0]).all() and np.isfinite(clean[2]).all()
        for kind in ("nan_all", "huge"):
            for js in (0, 32, 33, 64, [0, 32, 33, 64]):
                check_forward(h, x, other, clean, js, kind, f"{name} forward n={N_FORWARD} lanes={lanes}")
    finally:
        h.set_option("lanes", 2)


@pytest.mark.parametrize("name", NAMES)
def test_forward_of_a_poisoned_crop_is_nan(handles, images, name):
    """Every kind of NaN / Inf on one crop of five: its angles and logits are NaN, its argmax np.argmax's of the returned logits.
    (An f16 handle's stem clamps real-valued input to binary16's range with fmaxf / fminf, which answer NaN with the other
    operand: before stem.hip kept the clamp to finite values, one NaN pixel went in as -65504 and the crop came back with the
    angles -180, -99, 96; an infinite pixel as +-65504.)"""
    h = handles(name)
    x, other = images[0][:5], images[1][:5]
    clean = h.forward_f32(x)
    for kind in NF.POISON_SELF:
        check_forward(h, x, other, clean, 3, kind, f"{name} forward n=5")


# ---- the decode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split_heads", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_decode_rows_with_nan_and_inf(handles, name, split_heads):
    """op_decode on the rows of nonfinite_cases.decode_rows: argmax is np.argmax's and the table's literal; the angle is NaN where
    the float64 decode is NaN, and within the existing 2e-4 degrees of it where it is finite."""
    h = handles(name)
    lg, literal, nan_angle, names = NF.decode_logits()
    with np.errstate(invalid="ignore"):
        want = np.stack(O.decode(lg.astype(np.float64)), axis=1)
    assert np.array_equal(np.isnan(want), nan_angle) and np.array_equal(O.argmax_bins(lg), literal)
    with options(h, {"split_heads": split_heads}):
        h.op_decode(np.ascontiguousarray(np.nan_to_num(lg[::-1], nan=1.0, posinf=2.0, neginf=-2.0)))
        ypr, am = h.op_decode(lg)
    for i, row in enumerate(names):
        assert am[i].tolist() == literal[i].tolist(), (name, row, am[i].tolist(), literal[i].tolist())
    assert np.array_equal(np.isnan(ypr), nan_angle), (name, ypr.tolist())
    assert (np.abs(ypr.astype(np.float64) - want)[~nan_angle] < 2e-4).all(), (name, ypr.tolist(), want.tolist())


# ---- the detector -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def post():
    hs = {}
    for dd in (0, 1):
        hs[dd] = _lib.Handle.postproc(0)
        hs[dd].set_option("detector_dtype", dd)
    yield hs
    for h in hs.values():
        h.close()


@functools.lru_cache(maxsize=None)
def conv_operands(name, salt=0):
    c = FC.CASES[name]
    x, x2, kernel, bias, skip = DC.random_operands(c, DC.case_seed(name) + 7919 * salt)
    assert skip is None and not c["f32_out"]
    return c, x.astype(np.float32), None if x2 is None else x2.astype(np.float32), kernel, bias


def run_conv(h, c, x, x2, kernel, bias):
    return h.op_dconv(x, kernel, bias, stride=c["stride"], leaky=True, x2=x2, f32_out=False)


def poison_source(x, x2, which, j, kind):
    return (NF.poisoned(x, j, kind), x2) if which == "x" else (x, NF.poisoned(x2, j, kind))


@pytest.mark.parametrize("name", NF.DCONV_CASES)
@pytest.mark.parametrize("detector_dtype", [0, 1])
def test_dconv_keeps_a_poisoned_image_to_itself(post, detector_dtype, name):
    """dconv.hip flattens M over the images of a clip: each image poisoned in turn (for the two-source case the route source, then
    the half-resolution one), the other images' outputs are bitwise the clean run's."""
    h = post[detector_dtype]
    c, x, x2, kernel, bias = conv_operands(name)
    _, ox, ox2, _, _ = conv_operands(name, 1)
    clean = run_conv(h, c, x, x2, kernel, bias)
    assert np.isfinite(clean).all()
    for which in NF.dconv_sources(c):
        for j in range(c["n"]):
            for kind in NF.DCONV_KINDS:
                assert run_conv(h, c, ox, ox2, kernel, bias).tobytes() != clean.tobytes()
                got = run_conv(h, c, *poison_source(x, x2, which, j, kind), kernel, bias)
                others_same(got, clean, j, f"dconv {name} detector_dtype={detector_dtype} source {which} image {j} {kind}")
                assert not np.isfinite(got[j]).all()


@pytest.mark.parametrize("name", NF.DCONV_CASES)
@pytest.mark.parametrize("detector_dtype", [0, 1])
def test_dconv_nan_has_the_exact_footprint_of_float64(post, detector_dtype, name):
    """The halo is substituted zeros, not multiplied ones: one NaN element makes NaN exactly the outputs whose receptive field holds
    it -- the NaN mask of tests/detector_ref.R.conv in float64 on the same operands; the finite elements agree with it within
    2^-10 |ref| + 4 e32 (binary16 storage: test_conv_random_against_float64) or 2^-23 |ref| + 4 e32 (float32 storage:
    test_conv_against_float64), e32 the committed figure of the case."""
    h = post[detector_dtype]
    c, x, x2, kernel, bias = conv_operands(name)
    _, ox, ox2, _, _ = conv_operands(name, 1)
    e32 = FC.load_meta()[0]["e32"][name]
    ulp = 2.0 ** -23 if detector_dtype else 2.0 ** -10
    for which in NF.dconv_sources(c):
        for kind in NF.DCONV_FOOTPRINT_KINDS:
            j = c["n"] - 1
            px, px2 = poison_source(x, x2, which, j, kind)
            ref = R.conv(px, kernel, bias, c["stride"], True, x2=px2, dtype=np.float64)
            mask = np.isnan(ref)
            assert mask[j].any() and not mask[j].all() and not np.delete(mask, j, axis=0).any()
            run_conv(h, c, ox, ox2, kernel, bias)
            got = run_conv(h, c, px, px2, kernel, bias).astype(np.float64)
            tag = f"dconv {name} detector_dtype={detector_dtype} source {which} {kind}"
            assert np.array_equal(np.isnan(got), mask), (tag, np.argwhere(np.isnan(got) != mask)[:8].tolist())
            excess = (np.abs(got - ref) - (ulp * np.abs(ref) + 4 * e32))[~mask]
            assert excess.max() <= 0, (tag, float(excess.max()))


@pytest.mark.parametrize("name", NF.DPOOL_CASES)
@pytest.mark.parametrize("detector_dtype", [0, 1])
def test_dpool_keeps_a_poisoned_image_to_itself(post, detector_dtype, name):
    """Isolation only: what a max of NaN returns is not defined by the reference."""
    h = post[detector_dtype]
    n, hh, ww, ch, stride = dict(DC.POOL_CASES)[name]
    rng = np.random.RandomState(DC.case_seed(name))
    x = rng.normal(0, 2, (n, hh, ww, ch)).astype(np.float16).astype(np.float32)
    other = rng.normal(0, 2, (n, hh, ww, ch)).astype(np.float16).astype(np.float32)
    clean = h.op_dpool(x, stride)
    assert np.array_equal(clean, R.pool(x, stride))
    for j in range(n):
        for kind in NF.DCONV_KINDS:
            assert h.op_dpool(other, stride).tobytes() != clean.tobytes()
            got = h.op_dpool(NF.poisoned(x, j, kind), stride)
            others_same(got, clean, j, f"dpool {name} detector_dtype={detector_dtype} image {j} {kind}")
