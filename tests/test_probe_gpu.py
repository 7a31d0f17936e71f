"""Exact probe snapshots on the GPU (pytest -m gpu): every kernel form of the pose network, in all three dtypes, held to BITWISE
equality with the integer reference of tests/probe_cases.py (tests/test_probe_cpu.py checks that reference against the float64
oracle, and that the probes can see the errors they are for).  Structure, not rounding points: the tolerance tests of
tests/test_gpu_parity.py, tests/test_f32s.py and tests/test_mb7.py keep doing that.

Every comparison is np.array_equal over every element, except the pooled features and logits of the head on inputs that do not
pool to integers (a counted bound: test_head) and the angles of the decode (2e-4 degrees of the float64 decode).

The heads stage (pooling + Dense + softmax + decode) runs through op_head, which launches what the forward launches: under
split_heads 0 / 1 x head_fuse 0 / 1 the single-workgroup kernel and the three instantiations of the four-workgroup kernel
(test_dense_heads, test_decode_rows, test_ticket_counters).  The whole forward, stem to angles, runs through forward_f32
(test_forward_probe).  The uint8 forward (byte LUT, stemdw.hip, graph replay, lanes) cannot be made exact -- the LUT's values are
not integers: it stays with test_stem_fused_with_block_1_depthwise_is_bitwise_the_two_kernels and test_graph_replay_equals_eager."""
import numpy as np
import pytest

from tests import probe_cases as P
from whenet_hip import _lib, weights as W

pytestmark = pytest.mark.gpu
DTYPES = {"f32": _lib.F32, "f16": _lib.F16, "f32s": _lib.F32S}
DEFAULTS = {"fuse_front": 1, "front_impl": 1, "se_fuse": 1, "front7": 1, "mb7": 0, "pw_impl": 0, "pw_staged": 1, "split_pw": 1,
            "act_layout": 1, "xcd_map": 7, "f2s_mask": -1, "fold12": 1, "head_fuse": 1, "concurrent": 0, "split_heads": 1}
F2S_ALL = (1 << 17) - 1
# every value Engine::set_option accepts for each option that chooses a kernel form of ONE block, one option at a time against the
# default, and the pairs.  act_layout does not act on a single block (the boundaries of the single-stage entry points are NHWC): it
# is probed by the ranges below, whose interior tensors take the forward's layout.  xcd_map has tests of its own (XCD_SETTINGS).
SETTINGS = ([{}, {"fuse_front": 0}, {"front_impl": 0}, {"front_impl": 2}, {"se_fuse": 0}, {"se_fuse": 2}, {"se_fuse": 3}, {"front7": 0},
             {"mb7": 1}, {"pw_impl": 1}, {"pw_staged": 0}, {"split_pw": 0}, {"f2s_mask": F2S_ALL}, {"f2s_mask": 0},
             {"se_fuse": 2, "front_impl": 2}, {"mb7": 1, "se_fuse": 0}, {"mb7": 1, "se_fuse": 2}])
# xcd_map (bit 1: front.hip / front2.hip / front2s.hip, 2: front7.hip, 4: head7.hip): the grouped workgroup-to-XCD placement is
# applied when the chip is shared (a launch of >= 128 crops, or option concurrent), and device_math.h's xcd_unit() relabels only the
# whole rounds of eight UNITS of a launch -- (crop, tile) pairs for the front kernels, crop groups (2 crops up to 16 per launch, 4
# above) for front7 / head7: below 8 units every value of xcd_map is the same mapping.  So every value 0..7 runs with concurrent = 1
# at n = 15: front7 / head7 have 8 groups (all relabelled, the last one half full); the front kernels have 15 x tiles units, which is
# 8 or more on every block and leaves a remainder after the rounds of eight wherever the plan's tile count is not a multiple of 8
# (1, 2, 4, 6 or 28 tiles, by block and dtype).  At n = 37 (routing blocks 13-16 and the head: neither depends on the
# gates, which are designed on 17 crops) front7 / head7 have 10 groups of 4: 8 relabelled, 2 behind them, the last one ragged.
XCD_SETTINGS = [{"concurrent": 1, "xcd_map": v} for v in range(8)]
N_XCD, N_XCD_RAGGED = 15, 37
UNFUSED = ({"fuse_front": 0}, {"pw_impl": 1})          # the settings whose launches write the expanded tensor
OTHER = {"routing": "dense_dw", "dense_dw": "routing", "dense_expand": "dense_project", "dense_project": "dense_expand"}
BATCHES = (1, 3, 5, 17)


@pytest.fixture(scope="module")
def handles():
    """get(family, dtype name) -> the handle of that (snapshot, dtype), created on first use; all closed at the end of the module."""
    cache = {}

    def get(family, name):
        if (family, name) not in cache:
            w = (P.premise_snapshot() if family == "premise" else P.forward_snapshot() if family == "forward" else
                 P.head_snapshot(family) if family in P.HEAD_FAMILIES else P.snapshot(family))
            cache[(family, name)] = _lib.Handle(W.pack(w), device=0, dtype=DTYPES[name])
        return cache[(family, name)]

    yield get
    for h in cache.values():
        h.close()


class options:
    """Set options on a handle, restore the defaults on exit."""

    def __init__(self, h, setting):
        self.h, self.setting = h, setting

    def __enter__(self):
        for k, v in self.setting.items():
            self.h.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.setting:
            if k == "split_pw" and self.h.dtype != _lib.F32S:
                continue                         # (a handle that is not f32s accepts 0 only: 0 is what it was set to)
            self.h.set_option(k, DEFAULTS[k])


def applies(setting, name):
    return not ("split_pw" in setting and name != "f32s")


def same(got, want, what):
    """np.array_equal over every element; the message locates a difference: the first 10 (crop, y, x, channel) indices with the two
    values, and the counts per crop and per chunk of 32 channels."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~(got == want))
    first = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:10]]
    per_crop = dict(zip(*(a.tolist() for a in np.unique(bad[:, 0], return_counts=True))))
    per_chunk = dict(zip(*(a.tolist() for a in np.unique(bad[:, -1] // 32, return_counts=True))))
    raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; first (index, got, want): {first}; "
                         f"per crop: {per_crop}; per 32-channel chunk: {per_chunk}")


def scrub_block(h, index, other, want, setting):
    """The block's output buffers live in the handle's arena and keep what the last call left there: the same input's correct bits,
    when the settings of a test run back to back.  A kernel form that skipped a tile, a chunk's tail or the last rows would pass on
    them.  So before every compared call the block runs on ANOTHER input of the same shape (another family's crops) under the
    default options -- and, where `expand` is compared, under the other one of the two unfused settings, which writes that tensor
    with the other kernel -- so that whatever the compared call does not write differs from what is expected."""
    r = h.op_block(index, other)
    assert not np.array_equal(r["dw"], want["dw"]) and not np.array_equal(r["out"], want["out"])
    if setting in UNFUSED and "expand" in want:
        with options(h, UNFUSED[1 - UNFUSED.index(setting)]):
            r = h.op_block(index, other)
        assert not np.array_equal(r["expand"], want["expand"])


def check_block(h, family, index, n, setting, what, x=None, want=None):
    if x is None:
        x, want = P.inputs(family, index, n), P.expected(family, index, n)
    scrub_block(h, index, P.inputs(OTHER[family], index, n), want, setting)
    with options(h, setting):
        r = h.op_block(index, x)
    tag = f"{what} block {index} n={n} {setting}"
    if setting in UNFUSED and "expand" in want:
        same(r["expand"], want["expand"], tag + " expand")
    same(r["dw"], want["dw"], tag + " dw")
    if not np.isnan(r["gate"]).all():            # (NaN where no launch writes the gate: the project GEMM computes it for itself)
        same(r["gate"], want["gate"], tag + " gate")
    same(r["out"], want["out"], tag + " out")
    return r


@pytest.mark.parametrize("name", list(DTYPES))
def test_premise_swish_is_exact_on_the_exact_set(handles, name):
    """The hardware premise, on its own: Swish of every integer of -2048..-104, of 0 and of every integer of 18..2048, as block 16's
    expand conv computes it (pw.hip; then the depthwise conv's Swish on the same values, and the fused front kernel's), is bitwise
    the argument, or zero.  Rests on v_rcp_f32(1.0f) == 1.0f and on v_exp_f32 overflowing to +inf."""
    h = handles("premise", name)
    x = P.premise_input()
    w = P.premise_snapshot()
    pre = x @ w[f"b{P.PREMISE_BLOCK}/expand/kernel"][0, 0]
    assert set(np.unique(pre).astype(int).tolist()) == set(range(-2048, -103)) | {0} | set(range(18, 2049))
    want = np.where(pre >= 18, pre, 0).astype(np.float32)
    with options(h, {"fuse_front": 0}):
        r = h.op_block(P.PREMISE_BLOCK, x)
    same(r["expand"], want, f"{name} expand (Swish of the sweep)")
    same(r["dw"], want, f"{name} depthwise (Swish of the sweep)")
    # (the buffers hold the expected bits now: the reversed sweep overwrites them before the fused kernel is compared)
    assert not np.array_equal(h.op_block(P.PREMISE_BLOCK, np.ascontiguousarray(x[:, ::-1, ::-1]))["dw"], want)
    same(h.op_block(P.PREMISE_BLOCK, x)["dw"], want, f"{name} fused front kernel (Swish of the sweep)")


@pytest.mark.parametrize("index", range(1, 17))
@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("family", P.FAMILIES)
def test_block_under_every_option(handles, family, name, index):
    """op_block at n = 3 under the default options and under every value of every option that chooses a kernel form of one block,
    one option at a time, plus the pairs: expand (where the block runs unfused: fuse_front = 0, pw_impl = 1), dw, gate (where a
    launch writes it) and out are bitwise the expected tensors."""
    h = handles(family, name)
    wrote_gate = False
    for setting in SETTINGS:
        if applies(setting, name):
            r = check_block(h, family, index, 3, setting, f"{family} {name}")
            wrote_gate = wrote_gate or not np.isnan(r["gate"]).any()
    assert wrote_gate, "no setting wrote a gate: it was never compared"


@pytest.mark.parametrize("index", range(1, 17))
@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("family", P.FAMILIES)
def test_block_at_every_batch(handles, family, name, index):
    """n = 1, 3, 5, 17 (the 2- and 4-crop groups of front7.hip, three crops per project workgroup, 16 + 1): every crop is different
    and each is compared with its own expected tensor; with a squeeze-excite launch (se_fuse = 0) the gates are compared too.
    f16: also as one launch per block (mb7)."""
    h = handles(family, name)
    for n in BATCHES:
        check_block(h, family, index, n, {}, f"{family} {name}")
        check_block(h, family, index, n, {"se_fuse": 0}, f"{family} {name}")
        if name == "f16" and index >= 13:
            check_block(h, family, index, n, {"mb7": 1}, f"{family} {name}")


@pytest.mark.parametrize("index", range(1, 17))
@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("family", P.FAMILIES)
def test_block_under_every_xcd_map(handles, family, name, index):
    """Every value of xcd_map with option concurrent, at batches where the grouped placement relabels workgroups (see XCD_SETTINGS):
    n = 15 on every block, and n = 37 on blocks 13-16 of the routing snapshot."""
    h = handles(family, name)
    for setting in XCD_SETTINGS:
        check_block(h, family, index, N_XCD, setting, f"{family} {name}")
    if family == "routing" and index >= 13:
        n = N_XCD_RAGGED
        x = P.inputs(family, index, n)
        ref = P.ref_block(x, P.snapshot(family), index)
        assert ref["bound"] < 2048 and P.in_exact_set(ref["expand_pre"]).all() and P.in_exact_set(ref["dw_pre"]).all()
        assert len({x[i].tobytes() for i in range(n)}) == n
        want = {k: ref[k].astype(np.float32) for k in ("expand", "dw", "gate", "out")}
        for setting in XCD_SETTINGS:
            check_block(h, family, index, n, setting, f"{family} {name}", x, want)


def check_range(h, family, first, last, x, other, want, setting, what):
    """op_block_range under `setting`, after the same range on another input under the default options (see scrub_block)."""
    assert not np.array_equal(h.op_block_range(first, last, other), want)
    with options(h, setting):
        same(h.op_block_range(first, last, x), want, f"{what} blocks {first}..{last} {setting}")


@pytest.mark.parametrize("name", list(DTYPES))
def test_chained_blocks_on_the_routing_snapshot(handles, name):
    """op_block_range(1, 16) at n = 5 with fold12 0 / 1 and act_layout 0 / 1 / 2: bitwise the expected routing image.  The range's
    input and output are NHWC; the tensors between its blocks take the layout the forward gives them, so on the f16 handle
    act_layout 1 and 2 run the blocked epilogue of the split-K project GEMM (outputs of blocks 12-15) and the blocked readers of
    front7.hip and of the skip (blocks 13-16), and act_layout 0 the NHWC ones; f32 and f32s handles have no blocked layout (the
    three values are one schedule there).  head7.hip's blocked reader is reached through a forward only: test_forward_probe
    below (bitwise) and tests/test_act_layout.py."""
    h = handles("routing", name)
    x = P.chain_inputs("routing")
    other = P.chain_inputs("routing", first=200)
    want = P.expected_chain("routing", 1, 16)
    assert (want != 0).mean() > 0.2
    for fold in (0, 1):
        for lay in (0, 1, 2):
            check_range(h, "routing", 1, 16, x, other, want, {"fold12": fold, "act_layout": lay}, f"routing {name}")
    check_range(h, "routing", 1, 16, x, other, want, {"mb7": 1}, f"routing {name}")
    check_range(h, "routing", 1, 16, x, other, want, {"se_fuse": 3, "act_layout": 2}, f"routing {name}")


@pytest.mark.parametrize("name", list(DTYPES))
def test_the_7x7_stage_as_a_range_under_every_layout(handles, name):
    """op_block_range(12, 16) of the routing snapshot at n = 1, 3, 5, 17 on block 12's own probe input (every row and column of the
    image set) with act_layout 0 / 1 / 2, and se_fuse = 3 with act_layout = 2: ragged groups of front7.hip read the blocked tensors
    between blocks 12-16 (f16), the skips of blocks 13-15 add them, and the result is bitwise the reference's blocks chained.  (The
    routing snapshot alone stays exact through a chain: see probe_cases.expected_routing_range.)"""
    h = handles("routing", name)
    for n in BATCHES:
        x = P.inputs("routing", 12, n)
        other = P.inputs("dense_dw", 12, n)
        want = P.expected_routing_range(12, 16, n)
        assert (want != 0).mean() > 0.1
        for setting in ({"act_layout": 0}, {"act_layout": 1}, {"act_layout": 2}, {"se_fuse": 3, "act_layout": 2}):
            check_range(h, "routing", 12, 16, x, other, want, setting, f"routing {name} n={n}")


def kernels_per_forward(h, setting):
    with options(h, setting):
        return h.info().n_kernels_per_forward


@pytest.mark.parametrize("name", list(DTYPES))
def test_folded_weights_on_the_dense_project_snapshot(handles, name):
    """op_block_range(1, 2) with fold12 0 / 1: the composed project1 x expand2 weights are integer products, so both give the bits
    of the expected tensor.  f16 and f32s handles fold (one launch fewer per forward: asserted); an exact-f32 handle never does, so
    its two runs are the same schedule."""
    h = handles("dense_project", name)
    assert kernels_per_forward(h, {"fold12": 0}) - kernels_per_forward(h, {"fold12": 1}) == (0 if name == "f32" else 1)
    x = P.chain_inputs("dense_project")
    other = P.chain_inputs("dense_project", first=200)
    want = P.expected_chain("dense_project", 1, 2)
    for fold in (0, 1):
        check_range(h, "dense_project", 1, 2, x, other, want, {"fold12": fold}, f"dense_project {name}")


U32, U16 = 2.0 ** -24, 2.0 ** -11


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("family", ("routing", "dense_expand"))
def test_head(handles, family, name):
    """op_head with head_fuse 0 / 1 at n = 1, 3, 17.  The head conv's outputs are exact integers (stored exactly in binary16 too:
    below 2048), their sum S over the 49 positions is exact in float32 in any order; feat = S / 49 is held to
    |feat - S/49| <= r |S/49| with r the roundings between the exact sum and the returned value:
      head_fuse = 0 (csrc/head.hip:55, `(...) * (1.0f / 49.0f)`): the constant 1/49 rounded to float32 (2^-24) and the product
                    (2^-24); the feature is returned as float32 (head.hip:61), no binary16 rounding; the logits come from the
                    four-workgroup kernel's own pooling (head.hip:198-199, the same two roundings; split_heads = 1, the default);
      head_fuse = 1 (csrc/head7.hip:136 for f16, :258 for f32 / f32s, `(...) * (1.0f / 49.0f)`): the same two.
    r = 2 * 2^-24 (+ 2^-48 for their product).  Logit j reads ONE pooled feature with weight 1 and bias 0: the same bound plus one
    float32 rounding for the Dense product and one for the sum (head.hip:76, :85-86).
    head_fuse = 1 also runs with option concurrent and xcd_map 0 / 4 / 7 at n = 15 (8 crop groups of 2: head7.hip's grouped workgroup
    placement relabels all of them) and n = 37 (10 groups of 4: 8 relabelled, 2 behind them, the last ragged); below 8 groups the
    placement is the plain one whatever the option says.
    Before every compared call the head runs on another family's input (see scrub_block).
    On inputs that are constant over the 49 positions (probe_cases.head_pooled_inputs) the sum is 49 m and the product rounds back to
    m (test_probe_cpu.test_pooling_49_equal_integers_is_exact): there `feat` is BITWISE the integer features, under the same
    settings and under split_heads = 0."""
    h = handles(family, name)
    r_feat = 2 * U32 + U32 * U32
    r_logit = r_feat + 2 * U32
    w = P.snapshot(family)
    for n in (1, 3, 17, N_XCD, N_XCD_RAGGED):
        x = P.inputs(family, P.HEAD, n)
        ref = P.ref_head(x, w)
        assert P.in_exact_set(ref["pre"]).all() and ref["bound"] < 2048 and ref["conv"].max() <= 2048
        feat = ref["S"] / 49.0
        assert (ref["S"] > 0).mean() > 0.3
        other = P.inputs(OTHER[family], P.HEAD, n)
        xcd = [{"head_fuse": 1, "concurrent": 1, "xcd_map": v} for v in (0, 4, 7)] if n >= N_XCD else []
        for setting in [{"head_fuse": 0}, {"head_fuse": 1}] + xcd:
            h.op_head(other)
            with options(h, setting):
                r = h.op_head(x)
            ef = np.abs(r["feat"].astype(np.float64) - feat)
            el = np.abs(r["logits"].astype(np.float64) - ref["logits"])
            assert (ef <= r_feat * np.abs(feat)).all(), (family, name, n, setting, np.argwhere(ef > r_feat * np.abs(feat))[:10].tolist())
            assert (el <= r_logit * np.abs(ref["logits"])).all(), (family, name, n, setting, np.argwhere(el > r_logit * np.abs(ref["logits"]))[:10].tolist())
        xp = P.head_pooled_inputs(family, n)
        refp = P.ref_head(xp, w)
        assert P.in_exact_set(refp["pre"]).all() and refp["bound"] < 2048 and (refp["conv"] == refp["conv"][:, :1, :1]).all()
        assert (refp["S"] > 0).mean() > 0.3 and len({xp[i].tobytes() for i in range(n)}) == n
        for setting in [{"head_fuse": 0}, {"head_fuse": 1}, {"head_fuse": 0, "split_heads": 0}] + xcd:
            with options(h, setting):
                h.op_head(other)
                r = h.op_head(xp)
            same(r["feat"], refp["conv"][:, 0, 0, :], f"{family} {name} n={n} {setting} feat (pooled integers)")


# ---- the heads stage: op_head launches what the forward launches ----------------------------------------------------------------
HEAD_MATRIX = [{"split_heads": s, "head_fuse": f} for s in (0, 1) for f in (0, 1)]
HEAD_XCD = [{"head_fuse": 1, "concurrent": 1, "xcd_map": v} for v in (0, 4, 7)]
HEAD_OTHER = {"dense_heads": "decode", "decode": "dense_heads"}
DEG = 2e-4          # |ypr - float64 decode|: the bound of test_gpu_parity.test_decode_kernel (the float32 reference alone uses < 1e-4)


def check_heads(h, family, x, want, setting, what, ypr=False):
    """op_head(x) under `setting` after op_head on the other heads family's crops under the same setting: every output buffer (and
    the scratch the features come back through) then holds another input's results -- a workgroup that never drew the last ticket
    leaves visibly wrong logits, not stale correct ones."""
    other = P.head_const_inputs(HEAD_OTHER[family], len(x))
    with options(h, setting):
        r = h.op_head(other)
        assert not np.array_equal(r["logits"], want["logits"]) and not np.array_equal(r["feat"], want["feat"])
        r = h.op_head(x)
    tag = f"{what} n={len(x)} {setting}"
    same(r["logits"], want["logits"], tag + " logits")
    same(r["feat"], want["feat"], tag + " feat")
    assert np.array_equal(r["argmax"], want["argmax"]), (tag, np.argwhere(r["argmax"] != want["argmax"])[:10].tolist())
    if ypr:
        err = np.abs(r["ypr"].astype(np.float64) - want["ypr"])
        assert (err < DEG).all(), (tag, float(err.max()), np.argwhere(err >= DEG)[:10].tolist())


def head_settings(n):
    return HEAD_MATRIX + (HEAD_XCD if n >= N_XCD else [])


@pytest.mark.parametrize("name", list(DTYPES))
def test_dense_heads(handles, name):
    """Dense +-1, +-2 kernels on integer features (0 or 18..2040): the 252 logits are exact integers, so ONE array holds, bit for
    bit, for the single-workgroup kernel (split_heads = 0: 16 waves x 80 features) and for the four-workgroup kernel on pooled
    features (head_fuse = 1: <float, true>, 4 waves x 80) and on the head conv's tensor (head_fuse = 0: <half, false> /
    <float, false>, 8 waves x 40, its own pooling) -- every feature, every wave slice, every partial vector, the bias once.
    n = 1, 3, 5, 17, and 15 / 37 with head7.hip's grouped placement as well."""
    h = handles("dense_heads", name)
    for n in BATCHES + (N_XCD, N_XCD_RAGGED):
        x, want = P.head_const_inputs("dense_heads", n), P.expected_heads("dense_heads", n)
        for setting in head_settings(n):
            check_heads(h, "dense_heads", x, want, setting, f"dense_heads {name}")


@pytest.mark.parametrize("name", list(DTYPES))
def test_decode_rows(handles, name):
    """Designed logit rows (probe_cases.DECODE_ROWS: all equal, single maxima at bins 0 / 63 / 64 / last, exact ties across the lane
    63 / lane 0 boundary, within a lane and between a lane's first and another lane's second element, one-hot, narrow, wide) reach
    the decode of the forward's kernel through routed weights: logits bitwise, argmax the first index among equals, angles within
    2e-4 degrees of the float64 decode -- under the same matrix of settings; op_decode (the single-workgroup kernel's copy of the
    decode, fed logits directly) gets the same rows."""
    h = handles("decode", name)
    for n in BATCHES + (N_XCD, N_XCD_RAGGED):
        x, want = P.head_const_inputs("decode", n), P.expected_heads("decode", n)
        for setting in head_settings(n):
            check_heads(h, "decode", x, want, setting, f"decode {name}", ypr=True)
        h.op_decode(np.ascontiguousarray(want["logits"][::-1]))
        ypr, am = h.op_decode(want["logits"])
        assert np.array_equal(am, want["argmax"]), (name, n, np.argwhere(am != want["argmax"])[:10].tolist())
        assert (np.abs(ypr.astype(np.float64) - want["ypr"]) < DEG).all(), (name, n)


@pytest.mark.parametrize("name", list(DTYPES))
def test_ticket_counters(handles, name):
    """split_heads = 1, back to back on one handle with nothing in between: 17 crops, 3, 17, 1 -- each run a different selection of
    the crops (so that no position finds its own result already there), each bitwise its expectation: the ticket counters are back
    at zero after every launch and no workgroup reads another crop's partial vectors."""
    h = handles("dense_heads", name)
    x, want = P.head_const_inputs("dense_heads", P.N_MAX), P.expected_heads("dense_heads", P.N_MAX)
    runs = (np.arange(17), np.array([16, 15, 14]), np.arange(17)[::-1], np.array([5]))
    for fuse in (1, 0):
        with options(h, {"split_heads": 1, "head_fuse": fuse}):
            got = [h.op_head(np.ascontiguousarray(x[sel])) for sel in runs]
        for sel, r in zip(runs, got):
            tag = f"dense_heads {name} head_fuse={fuse} crops {sel.tolist()}"
            same(r["logits"], want["logits"][sel], tag + " logits")
            same(r["feat"], want["feat"][sel], tag + " feat")
            assert np.array_equal(r["argmax"], want["argmax"][sel]), tag


@pytest.mark.parametrize("name", list(DTYPES))
def test_forward_probe(handles, name):
    """forward_f32 (the real-valued entry point: no byte LUT, eager, stem.hip and block 1's depthwise conv as two kernels) on the
    routing snapshot with a routing stem, images of 0 or 18..24: stem, blocks 1-16, head conv, pooling, Dense and decode as the
    forward chains them, at n = 1, 3, 5, 17 under fold12 0 / 1 x head_fuse 0 / 1 x split_heads 0 / 1 and, on the f16 handle,
    act_layout 0 / 1 / 2 (1 and 2 feed head7.hip its blocked input).  Logit j is float32(S) * float32(1/49) with S the exact
    pooled sum -- one rounding, in every pooling expression (head.hip:55, :198-199, head7.hip:136, :258: a sum of integers in any
    order, one product), then x 1 + 0 in the Dense layer: bitwise.  Argmax equal, angles within 2e-4 degrees.  Before every compared
    run the handle runs another image."""
    h = handles("forward", name)
    layouts = (0, 1, 2) if name == "f16" else (1,)
    for n in BATCHES:
        x, other, want = P.forward_images(n), P.forward_images(n, first=200), P.expected_forward(n)
        for lay in layouts:
            for fold in (0, 1):
                for setting in HEAD_MATRIX:
                    setting = dict(setting, act_layout=lay, fold12=fold)
                    with options(h, setting):
                        assert not np.array_equal(h.forward_f32(other)[2], want["logits"])
                        ypr, am, lg = h.forward_f32(x)
                    tag = f"forward {name} n={n} {setting}"
                    same(lg, want["logits"], tag + " logits")
                    assert np.array_equal(am, want["argmax"]), tag
                    assert (np.abs(ypr.astype(np.float64) - want["ypr"]) < DEG).all(), tag
