"""The exact probe snapshots of tests/probe_cases.py, checked on the CPU: the integer reference against the float64 oracle, the
conditions that keep every value exact (the exact set of Swish, the 2048 bound, saturated gates), the coverage the builders claim,
and -- by mutating the reference the way a broken kernel would -- that the probes can see what they are for.  No GPU."""
import numpy as np
import pytest

from oracle import whenet_oracle as O
from tests import probe_cases as P
from whenet_hip import _lib, spec

BLOCKS = P.BLOCKS
PROBED = [f for f in P.FAMILIES if f != "routing"]


def changed(a: np.ndarray, b: np.ndarray) -> bool:
    """The two expected tensors differ, by an integer >= 1, somewhere (every element is one the GPU test compares)."""
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return bool((d >= 1).any()) and bool(np.all(d == np.rint(d)))


@pytest.mark.parametrize("index", range(1, 17))
@pytest.mark.parametrize("family", P.FAMILIES)
def test_reference_is_the_oracle_and_stays_exact(family, index):
    w = P.snapshot(family)
    x = P.inputs(family, index, 3)
    want = P.expected(family, index, 3)
    b = BLOCKS[index - 1]
    # the oracle on the snapshot as the device gets it.  Its own error: Swish(z) = z (1 - e^-z) falls short of z by up to
    # 18 e^-18 = 2.7e-7 per value -- a single value of 18..24 is an integer to 1e-6, but a sum of them (a dense kernel, a skip) is
    # short by the sum of these.  A value passes two Swishes at the most: 2 e^-18 = 3.05e-8 of it (BatchNorm adds 1e-15), so
    # 3.5e-8 of the block's sum |w||x| (P.stats' `bound`, < 2048: at most 7e-5, far from the 0.5 that would make np.rint ambiguous).
    taps = {}
    O.block(x.astype(np.float64), w, index, taps=taps)
    tol = max(1e-6, 3.5e-8 * P.stats(family, index)["bound"])
    for key in ("expand", "dw", "gate", "out"):
        if key == "expand" and not b.has_expand:
            continue
        t = taps[f"b{index}/{key}"].reshape(want[key].shape)
        assert np.abs(t - np.rint(t)).max() <= tol, (key, np.abs(t - np.rint(t)).max(), tol)
        assert np.array_equal(np.rint(t), want[key]), key
    s = P.stats(family, index)              # over all 17 crops of the GPU tests
    assert s["exact"], "a pre-activation of expand or depthwise outside {z <= -104} u {0} u {18 <= z <= 2048}"
    assert s["bound"] < 2048, s
    assert s["se_limit"] < 2 ** 24, s
    if family == "routing":
        assert s["margin"] == 8, s          # (forced gates: the argument is the bias, 32 >= 24)
    else:
        assert s["margin"] >= 16, s
        assert s["a_min"] >= 2, s          # (no se_reduce output near 0, where a rounding could turn the gate)
    # 17 different crops, values 0 or 18..24
    x17 = P.inputs(family, index, P.N_MAX)
    assert len({x17[i].tobytes() for i in range(P.N_MAX)}) == P.N_MAX
    assert np.isin(x17, [0] + list(range(18, 25))).all()


def test_chained_runs_stay_exact():
    for family, last in (("routing", 16), ("dense_project", 2)):
        w = P.snapshot(family)
        x = P.chain_inputs(family)
        assert len({x[i].tobytes() for i in range(len(x))}) == len(x)
        for index in range(1, last + 1):
            r = P.ref_block(x, w, index)
            assert all(P.in_exact_set(r[k]).all() for k in ("expand_pre", "dw_pre") if k in r), (family, index)
            assert r["bound"] < 2048 and P.gate_margin(r["arg"]) >= (8 if family == "routing" else 16), (family, index, r["bound"])
            assert family == "routing" or np.abs(r["a"]).min() >= 2
            x = r["out"]
        assert np.array_equal(x, P.expected_chain(family, 1, last)) and (x != 0).mean() > 0.2
        if family == "dense_project":       # the composed project1 x expand2 weights and bias are integers exact in binary16
            comp = w["b1/project/kernel"][0, 0] @ w["b2/expand/kernel"][0, 0]
            assert np.abs(comp).max() <= 2048 and np.abs(w["b1/project_bn/beta"] @ w["b2/expand/kernel"][0, 0]).max() <= 2048
            assert (comp > 0).any() and (comp < 0).any()


def test_routing_range_through_the_7x7_stage_stays_exact():
    want = P.expected_routing_range(12, 16, P.N_MAX)          # (asserts the exact set and the 2048 bound block by block)
    assert want.shape == (P.N_MAX, 7, 7, 320) and (want != 0).mean() > 0.1 and np.abs(want).max() <= 2048
    assert len({want[i].tobytes() for i in range(P.N_MAX)}) == P.N_MAX


def test_batchnorm_folds_to_the_identity():
    """In double (as snapshot.cpp folds it and as the oracle evaluates it), so that the weight is the integer in float32 and in
    binary16 AND the f32s image pair, split from the double product scaled by the layer's power of two, has a zero lo half."""
    scale = float(P.GAMMA) / np.sqrt(np.float64(P.VAR) + 1e-3)
    assert abs(scale - 1) <= 1e-15 and P.VAR > 0
    ints = np.arange(-2048, 2049).astype(np.float64)
    assert np.array_equal((ints * scale).astype(np.float32), ints.astype(np.float32))
    assert np.array_equal((ints * scale).astype(np.float16), ints.astype(np.float16))
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    h = h[np.isfinite(h)]
    assert np.array_equal((h.astype(np.float64) * scale).astype(np.float16), h)
    assert np.array_equal((h.astype(np.float64) * scale).astype(np.float32), h.astype(np.float32))
    for shift in range(0, 15):                      # pack_pw_split: the largest |w| 2^shift of a layer lies in [8192, 16384)
        v = ints[np.abs(ints) * 2.0 ** shift < 16384] * scale * 2.0 ** shift
        hi = v.astype(np.float32).astype(np.float16)
        lo = (v - hi.astype(np.float64)).astype(np.float32).astype(np.float16)
        assert np.array_equal(hi.astype(np.float64), np.rint(v)) and (lo == 0).all()
    for family in P.FAMILIES:
        w = P.snapshot(family)
        for name in spec.bn_names():
            assert (w[f"{name}/gamma"] == P.GAMMA).all() and (w[f"{name}/var"] == P.VAR).all() and (w[f"{name}/mean"] == 0).all()
            assert np.array_equal(w[f"{name}/beta"], np.rint(w[f"{name}/beta"]))


def test_swish_is_exact_on_the_exact_set_in_float32():
    z = np.concatenate([np.arange(-2048, -103), [0], np.arange(18, 2049)]).astype(np.float32)
    one = np.float32(1)
    with np.errstate(over="ignore"):
        precise = z * (one / (one + np.exp(-z)))
        fast = z * (one / (one + np.exp2(-z * np.float32(1.4426950408889634))))
    want = np.where(z >= 18, z, 0).astype(np.float32)
    assert np.array_equal(precise, want) and np.array_equal(fast, want)
    for arg, g in ((24, 1), (48, 1), (-104, 0), (-128, 0)):
        with np.errstate(over="ignore"):
            assert one / (one + np.exp(np.float32(-arg))) == g
    x, w = P.premise_input(), P.premise_snapshot()
    pre = x @ w[f"b{P.PREMISE_BLOCK}/expand/kernel"][0, 0]
    assert set(np.unique(pre).astype(int).tolist()) == set(range(-2048, -103)) | {0} | set(range(18, 2049))


def plans(index):
    """The tile plans of block `index` that the library reports: (kind, dtype name, plan) of dw.hip's `plan_dw` and front.hip's
    `plan_front`, for the two storage types (the f32s kernels run the float32 plans).  front2.hip, front2s.hip, front7.hip and
    mb7.hip tile by plans of their own, which the C ABI does not report."""
    out = []
    for name, dt in (("f32", _lib.F32), ("f16", _lib.F16)):
        out.append(("dw", name, _lib.dw_plan(dt, index)))
        if index >= 2:
            out.append(("front", name, _lib.front_plan(dt, index)))
    return out


def test_routing_snapshot_is_what_it_claims():
    w = P.snapshot("routing")
    maps = []
    for b in BLOCKS:
        p = f"b{b.index}"
        for name in ("expand", "project"):
            if name == "expand" and not b.has_expand:
                continue
            m = w[f"{p}/{name}/kernel"][0, 0]
            assert ((m != 0).sum(axis=0) == 1).all() and set(np.unique(m)) == {0, 1}, (p, name)
            src = m.argmax(axis=0)
            assert not np.array_equal(src, np.arange(len(src)) % m.shape[0]), (p, name)          # not the identity
            maps.append(tuple(src[:16]))
            if name == "expand":
                assert set(src) == set(range(b.cin)), p               # every k index is read
        k3 = w[f"{p}/dw/kernel"][:, :, :, 0].reshape(b.k * b.k, b.cexp)
        assert ((k3 != 0).sum(axis=0) == 1).all() and set(np.unique(k3)) == {0, 1}
        tap = k3.argmax(axis=0)
        for kind, name, plan in plans(b.index):
            cc = plan["CC"] if "CC" in plan else b.cexp // plan["chunks"]          # (front plans: the last chunk may be short)
            for c0 in range(0, b.cexp, cc):
                # every tap occurs in every chunk that has the channels for it (a 16-channel chunk holds 16 of the 25)
                width = min(cc, b.cexp - c0)
                assert len(set(tap[c0:c0 + width])) == min(width, b.k * b.k), (p, kind, name, c0)
        assert (w[f"{p}/se_expand/kernel"] == 0).all() and (w[f"{p}/se_expand/bias"] == 32).all()
    assert len(set(maps)) == len(maps), "two layers share a channel map"
    m = w["head/conv/kernel"][0, 0]
    assert ((m != 0).sum(axis=0) == 1).all() and set(m.argmax(axis=0)) == set(range(320))
    for name in ("yaw", "pitch", "roll"):
        d = w[f"{name}/kernel"]
        assert ((d != 0).sum(axis=0) == 1).all() and set(np.unique(d)) == {0, 1} and (w[f"{name}/bias"] == 0).all()


@pytest.mark.parametrize("family", PROBED)
def test_dense_snapshots_are_what_they_claim(family):
    w = P.snapshot(family)
    for b in BLOCKS:
        p = f"b{b.index}"
        ce = np.arange(b.cexp)
        k3 = w[f"{p}/dw/kernel"][:, :, :, 0].reshape(b.k * b.k, b.cexp)
        d_neg = ce % 8 == P.DW_NEG
        # the non-positive classes: all weights <= 0 and a multiple of 8; every other channel all >= 0
        assert (k3[:, d_neg] <= 0).all() and (k3[:, d_neg] % 8 == 0).all() and (k3[:, d_neg] < 0).any(axis=0).all()
        assert (k3[:, ~d_neg] >= 0).all()
        if family == "dense_dw":
            assert (k3 != 0).all() and np.isin(k3[:, ~d_neg], (1, 2)).all() and {1, 2} <= set(np.unique(k3))
        else:
            centre = (b.k // 2) * b.k + b.k // 2
            assert (k3[centre] != 0).all() and (np.delete(k3, centre, axis=0) == 0).all()
        if b.has_expand:
            m = w[f"{p}/expand/kernel"][0, 0]
            e_neg = ce % 8 == P.EXPAND_NEG
            assert (m[:, e_neg] <= 0).all() and (m[:, e_neg] % 8 == 0).all() and (m[:, e_neg] < 0).any(axis=0).all()
            assert (m[:, ~e_neg] >= 0).all()
            if family == "dense_expand":
                assert (m != 0).all() and {1, 2, -8} == set(np.unique(m))          # every (k, cout) entry
            else:
                assert ((m != 0).sum(axis=0) == 1).all() and set(np.abs(m).argmax(axis=0)) == set(range(b.cin))
        pk = w[f"{p}/project/kernel"][0, 0]
        beta = w[f"{p}/project_bn/beta"]
        if family == "dense_project":
            assert (pk != 0).all() and (pk > 0).any() and (pk < 0).any() and np.abs(pk).max() <= 7
            assert b.index == 1 or ((beta > 0).any() and (beta < 0).any())
        else:
            assert ((pk != 0).sum(axis=0) == 1).all() and set(np.unique(pk)) == {0, 1} and (beta == 0).all()
        # the outputs of the non-positive classes are exactly 0; the gates are 0 / 1, differ between the crops of a batch of 3,
        # and are not constant over the channels of the batch
        e = P.expected(family, b.index, 3)
        if b.has_expand:
            assert (e["expand"][..., ce % 8 == P.EXPAND_NEG] == 0).all() and (e["expand"][..., ce % 8 != P.EXPAND_NEG] != 0).any()
        assert (e["dw"][..., d_neg] == 0).all()
        g = e["gate"]
        assert np.isin(g, (0, 1)).all() and len({g[i].tobytes() for i in range(3)}) >= 2 and 0.05 < g.mean() < 0.95, (p, g.mean())
        assert (w[f"{p}/se_expand/bias"] == -128).all()
        w1 = w[f"{p}/se_reduce/kernel"][0, 0]
        assert ((w1 != 0).sum(axis=0) == 1).all() and np.array_equal(w1, np.rint(w1))          # one channel each, integer weights


@pytest.mark.parametrize("family", ("routing", "dense_dw"))
def test_impulses_fall_on_every_tile_and_halo_edge(family):
    """For every reported tile plan (dw.hip, front.hip; see plans()): the first and last row and column of the image, and the first and last row and
    column of every tile and of every tile's halo (where it lies inside the image), carry an impulse in a batch of 3 -- in every
    channel, since every channel's pattern has every row and column of the image in some crop or a third of them in each."""
    for b in BLOCKS:
        x = P.inputs(family, b.index, 3)
        rows = (x != 0).any(axis=(0, 2, 3))
        cols = (x != 0).any(axis=(0, 1, 3))
        assert rows.all() and cols.all(), b.index
        per_channel_rows = (x != 0).any(axis=(0, 2))          # [H, C]
        assert per_channel_rows[[0, b.h_in - 1]].any(axis=1).all()
        pad = spec.same_pad(b.h_in, b.k, b.s)[1]
        for kind, name, plan in plans(b.index):
            edges = set()
            for spans in (P.tile_rows(plan, b), P.tile_cols(plan, b)):
                for y0, y1 in spans:
                    edges |= {y0 * b.s, (y1 - 1) * b.s, y0 * b.s - pad, (y1 - 1) * b.s - pad + b.k - 1}
            inside = sorted(e for e in edges if 0 <= e < b.h_in)
            assert inside and rows[inside].all() and cols[inside].all(), (b.index, kind, name)
        # stride-2 blocks pad bottom / right only (or one more there): the last input row and column are read by the last outputs
        if b.s == 2:
            assert pad == (b.k - 2) // 2


def test_dense_expand_inputs_excite_every_k_index():
    for b in BLOCKS:
        x = P.inputs("dense_expand", b.index, 3)
        assert (x != 0).any(axis=(0, 1, 2)).all(), b.index


# ---- the probes can see what they are for -----------------------------------------------------------------------------------------
def mutated_weights(w, name, edit):
    w2 = dict(w)
    a = w[name].copy()
    edit(a)
    w2[name] = a
    return w2


@pytest.mark.parametrize("index", (7, 9, 16))
def test_a_dropped_tap_is_visible(index):
    """Every tap (all 9 or 25) of a channel of the dense depthwise snapshot, and the one tap of a routing channel."""
    b = BLOCKS[index - 1]
    for family in ("dense_dw", "routing"):
        w = P.snapshot(family)
        x = P.inputs(family, index, 3)
        base = P.ref_block(x, w, index)
        c = 1
        for ky in range(b.k):
            for kx in range(b.k):
                if w[f"b{index}/dw/kernel"][ky, kx, c, 0] == 0:
                    continue

                def drop(a):
                    a[ky, kx, c, 0] = 0
                r = P.ref_block(x, mutated_weights(w, f"b{index}/dw/kernel", drop), index)
                assert changed(r["dw"], base["dw"]), (family, index, ky, kx)


@pytest.mark.parametrize("index", (2, 7, 16))
def test_a_dropped_k_index_is_visible(index):
    """Every k of the dense expand conv (in `expand` and `dw`), and every k of the dense project conv whose channel is not of a
    non-positive class (in `out`, in one of the 17 crops: a channel's gate is open in some crops only)."""
    b = BLOCKS[index - 1]
    w = P.snapshot("dense_expand")
    x = P.inputs("dense_expand", index, 3)
    base = P.ref_block(x, w, index)
    for k in range(b.cin):
        def drop(a):
            a[0, 0, k, :] = 0
        r = P.ref_block(x, mutated_weights(w, f"b{index}/expand/kernel", drop), index)
        assert changed(r["expand"], base["expand"]) and changed(r["dw"], base["dw"]), (index, k)
    e = P.expected("dense_project", index, P.N_MAX)
    seen = ((e["dw"] * e["gate"][:, None, None, :]) != 0).any(axis=(0, 1, 2))          # out changes by |p| d >= 18 where this is set
    ce = np.arange(b.cexp)
    live = (ce % 8 != P.DW_NEG) & ((ce % 8 != P.EXPAND_NEG) | (not b.has_expand))
    assert seen[live].all() and not seen[~live].any(), (index, np.flatnonzero(live & ~seen)[:10])


MUTATIONS = {"squeeze_drop_last": {"squeeze_drop_last": 1}, "mean_halved": {"mean_scale": 0.5},
             "gate_of_next_crop": {"gate_from": 1}, "gate_of_crop_after_next": {"gate_from": 2}}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_a_squeeze_excite_mutation_is_visible(mutation):
    """The squeeze sum without its last pixel, 1/(H W) halved, the gate of crop i + 1 / i + 2: each changes `gate` and `out` of a batch
    of 3 -- in every probed family, and in every block for all but the missing pixel (the fine threshold needs a crop whose last
    pixel is non-zero in a channel whose sums fit: it exists in some blocks of each family; they are listed)."""
    seen = {}
    for family in PROBED:
        w = P.snapshot(family)
        for b in BLOCKS:
            x = P.inputs(family, b.index, 3)
            base = P.ref_block(x, w, b.index)
            r = P.ref_block(x, w, b.index, mut=MUTATIONS[mutation])
            ok = changed(r["gate"], base["gate"]) and changed(r["out"], base["out"])
            if ok:
                seen.setdefault(family, []).append(b.index)
            if mutation != "squeeze_drop_last":
                assert ok, (mutation, family, b.index)
    for family in PROBED:
        assert seen.get(family), (mutation, family)
    if mutation == "squeeze_drop_last":
        big = {i for f in PROBED for i in seen[f] if BLOCKS[i - 1].h_out >= 56}
        assert big, "no block with a 112 x 112 or 56 x 56 squeeze sum sees the missing pixel"


@pytest.mark.parametrize("mutation", ("halo_shift", "halo_neighbour"))
def test_a_halo_mutation_is_visible(mutation):
    """One tile's top halo row shifted by one input row, or taken from the neighbour crop's last row: visible in `dw` for every tile
    (below the first) of every reported tile plan (dw.hip, front.hip) of every block, on the dense depthwise snapshot.  The tile
    rows of front2.hip, front2s.hip, front7.hip and mb7.hip are not visited (not reported); every row and column of the image
    carries an impulse, so their edges are touched all the same."""
    w = P.snapshot("dense_dw")
    for b in BLOCKS:
        x = P.inputs("dense_dw", b.index, 3)
        base = P.ref_block(x, w, b.index)
        pad = spec.same_pad(b.h_in, b.k, b.s)[1]
        done = set()
        for kind, name, plan in plans(b.index):
            for y0, y1 in P.tile_rows(plan, b):
                if y0 * b.s - pad < 1 or (y0, y1) in done:
                    continue
                done.add((y0, y1))
                r = P.ref_block(x, w, b.index, mut={mutation: (y0, y1)})
                assert changed(r["dw"], base["dw"]), (mutation, b.index, kind, name, y0, y1)
        if mutation == "halo_neighbour" and not done:
            # a single tile per image: its top halo is the padding; a kernel that reads the neighbour crop's last row there is
            # seen because that row is not zero
            assert (x[:, b.h_in - 1] != 0).any(axis=(1, 2)).all()


def test_routing_blocks_of_the_7x7_stage_stay_exact_at_37_crops():
    """The batch at which front7.hip's grouped placement leaves groups behind its rounds of eight (test_probe_gpu.py): the routing
    snapshot's gates are forced, so crops beyond the 17 the other families' gates are designed on are as good as the first."""
    w = P.snapshot("routing")
    for index in (13, 14, 15, 16):
        x = P.inputs("routing", index, 37)
        assert len({x[i].tobytes() for i in range(37)}) == 37 and np.array_equal(x[:P.N_MAX], P.inputs("routing", index, P.N_MAX))
        r = P.ref_block(x, w, index)
        assert r["bound"] < 2048 and P.in_exact_set(r["expand_pre"]).all() and P.in_exact_set(r["dw_pre"]).all() and (r["gate"] == 1).all()
        assert np.array_equal(r["out"][:3], P.expected("routing", index, 3)["out"])


def test_head_probes():
    for family in ("routing", "dense_expand"):
        w = P.snapshot(family)
        x = P.inputs(family, P.HEAD, 37)
        r = P.ref_head(x, w)
        assert P.in_exact_set(r["pre"]).all() and r["bound"] < 2048 and r["conv"].max() <= 2048 and r["S"].max() < 2 ** 24
        f = O.swish(O.batchnorm(O.conv2d(x[:3].astype(np.float64), w["head/conv/kernel"], 1), w, "head/bn"))
        assert np.array_equal(np.rint(f), r["conv"][:3]) and np.abs(f - np.rint(f)).max() <= 1e-6
        lg = O.heads(f, w)
        assert np.allclose(lg, r["logits"][:3], rtol=1e-7, atol=1e-12)
        assert len({x[i].tobytes() for i in range(37)}) == 37


# ---- the heads stage and the whole forward ----------------------------------------------------------------------------------------
PACKED_SHA256 = {"routing": "0228c2b29f3be46294bd626d7cad723ed9b331b84057dac93dcb65d2e53f9bd0",
                 "dense_expand": "4bdc22b725527414b16b03190f02c8bde106dfce8c5cdee3dab10bb11fda936e",
                 "dense_dw": "c9918f786d6d3b552398ae3be8c7de6ae5bc8087a4cede7ba96697e1759d7649",
                 "dense_project": "a2b31dc4c0a2464c60b4b3b445d6e6f114308ee799bd6c3feb449bcfad3207df"}
N_HEADS_BIG = 37          # the largest batch of the heads tests on the GPU (test_probe_gpu.N_XCD_RAGGED)


@pytest.mark.parametrize("family", P.FAMILIES)
def test_the_block_families_pack_to_the_same_bytes(family):
    """The four families of the MBConv probes are what they were before the heads families were added: the sha256 of W.pack of
    each, taken before that edit."""
    import hashlib
    from whenet_hip import weights as W
    assert P.FAMILIES == tuple(PACKED_SHA256)
    assert hashlib.sha256(bytes(W.pack(P.snapshot(family)))).hexdigest() == PACKED_SHA256[family]


def test_pooling_49_equal_integers_is_exact():
    """float32(49 m) * (float32(1) / float32(49)) == m for m = 0..4096 (the rounded constant is 2.05e-8 below 1/49, relatively:
    less than 2^-25), and 49 m is exact in float32 in any order of the additions (partial sums are multiples of m below 2^24)."""
    m = np.arange(4097, dtype=np.float32)
    assert abs(float(P.INV49) * 49 - 1) < 2.0 ** -25
    assert np.array_equal((m * np.float32(49)) * P.INV49, m)
    s = np.zeros(4097, np.float32)
    for _ in range(49):
        s = s + m
    assert np.array_equal(s, m * np.float32(49)) and np.array_equal(s * P.INV49, m)


@pytest.mark.parametrize("family", P.HEAD_FAMILIES)
def test_heads_reference_is_the_oracle_and_stays_exact(family):
    w = P.head_snapshot(family)
    x = P.head_const_inputs(family, N_HEADS_BIG)
    assert np.isin(x, [0] + list(range(18, 25))).all() and (x == x[:, :1, :1, :]).all()
    assert len({x[i].tobytes() for i in range(len(x))}) == len(x)
    assert np.array_equal(x[:P.N_MAX], P.head_const_inputs(family, P.N_MAX))          # crop i is a function of i alone
    r = P.ref_heads(x, w)
    for key in ("feat", "logits"):
        assert np.array_equal(r[key], np.rint(r[key])), key
    assert 0 <= r["feat"].min() and r["feat"].max() <= 2048 and r["bound"] < 2 ** 24          # (every partial sum is below `bound`)
    conv = w["head/conv/kernel"][0, 0]
    assert ((conv != 0).sum(axis=0) == 1).all() and (conv >= 0).all()          # one positive weight per feature
    e = P.expected_heads(family, N_HEADS_BIG)
    assert e["feat"].dtype == np.float32 and np.array_equal(e["logits"], r["logits"]) and np.array_equal(e["argmax"], r["argmax"])
    # the float64 oracle on the same weights and inputs.  Its own error: Swish(z) = z (1 - e^-z) is short of z by up to 18 e^-18 =
    # 2.7e-7 per feature (BatchNorm adds 1e-15 of it): 3.5e-8 of the sum |feat||W|, as in test_reference_is_the_oracle_and_stays_exact
    f = O.swish(O.batchnorm(O.conv2d(x[:5].astype(np.float64), w["head/conv/kernel"], 1), w, "head/bn"))
    assert np.abs(f - np.rint(f)).max() <= 1e-6 and np.array_equal(np.rint(f.mean(axis=(1, 2))), r["feat"][:5])
    lg = O.heads(f, w)
    tol = max(1e-6, 3.5e-8 * float(r["bound"]))
    assert tol < 0.25 and np.abs(lg - r["logits"][:5]).max() <= tol, (np.abs(lg - r["logits"][:5]).max(), tol)
    assert np.array_equal(O.argmax_bins(r["logits"]), r["argmax"])
    assert np.array_equal(np.stack(O.decode(r["logits"]), axis=1), r["ypr"])
    D, bias = P.dense_matrix(w)
    if family == "dense_heads":
        assert (D != 0).all() and set(np.unique(D)) == {-2, -1, 1, 2} and (bias != 0).all() and np.array_equal(bias, np.rint(bias))
        assert {1, 2, 3, 5, 8, 13, 40, 85} == set(np.unique(conv[conv != 0])) and set(conv.argmax(axis=0)) == set(range(320))
    else:
        j = np.arange(spec.N_LOGITS)
        assert len(set(P.decode_channel(j))) == spec.N_LOGITS and len(set(P.decode_feature(j))) == spec.N_LOGITS
        assert ((D != 0).sum(axis=0) == 1).all() and np.array_equal(D.argmax(axis=0), P.decode_feature(j))
        assert np.array_equal(conv.argmax(axis=0)[P.decode_feature(j)], P.decode_channel(j))
        assert np.array_equal(r["logits"], P.DECODE_GAIN * x[:, 0, 0, P.decode_channel(j)])          # injective in ONE channel
        # the features behind the logits lie in every workgroup quarter and every 40-channel wave slice
        assert set(P.decode_feature(j) // 40) == set(range(32))


def test_dense_heads_coverage():
    """In the batch of 17: every one of the 1280 features is non-zero in some crop, and every (workgroup quarter, wave slice) of
    the contraction -- 40 features for the 8-wave form of the four-workgroup kernel, 80 for its 4-wave form and for the 16 waves of
    the single-workgroup kernel -- contributes a non-zero amount to every logit in some crop."""
    w = P.head_snapshot("dense_heads")
    r = P.ref_heads(P.head_const_inputs("dense_heads", P.N_MAX), w)
    assert (r["feat"] != 0).any(axis=0).all()
    D, _ = P.dense_matrix(w)
    for width in (40, 80, 320):
        for c0 in range(0, spec.FEAT, width):
            part = r["feat"][:, c0:c0 + width] @ D[c0:c0 + width]
            assert (part != 0).any(axis=0).all(), (width, c0)


def test_decode_rows_are_what_they_claim():
    x = P.head_const_inputs("decode", N_HEADS_BIG)
    e = P.expected_heads("decode", N_HEADS_BIG)
    lg = e["logits"].astype(np.float64)
    for n in (P.N_MAX, 15, 11):          # every kind of row on the 120-bin head and on a 66-bin head (on both of them, in fact)
        for h in range(3):
            assert {P.decode_kind(i, h) for i in range(n)} == set(P.DECODE_ROWS), (n, h)
    for i in range(N_HEADS_BIG):
        for h, (_, lo, nb) in enumerate(P.HEADS):
            kind, row, am = P.decode_kind(i, h), lg[i, lo:lo + nb], int(e["argmax"][i, h])
            top = np.flatnonzero(row == row.max())
            if kind == "equal":
                assert len(top) == nb and am == 0
            elif kind in P.DECODE_MAXIMA:
                assert tuple(top) == P.DECODE_MAXIMA[kind][0 if nb == 120 else 1] and am == top[0]
            elif kind == "one_hot":
                assert len(top) == 1 and np.sort(row)[-2] <= row.max() - 104 and np.exp(np.float32(-104)) == 0
            elif kind == "narrow":
                assert row.max() - row.min() <= 6 and 0.25 * nb < len(top) < 0.75 * nb
            else:
                assert kind == "wide" and len(top) > 1 and row.max() - row.min() == 30 and am == top[0]


def softmax_expectation_f32(logits):
    """utils.softmax plus the expectation, plainly in float32 numpy (what any float32 kernel computes, up to the order of the sums)."""
    out = []
    for h, (_, lo, nb) in enumerate(P.HEADS):
        z = logits[:, lo:lo + nb].astype(np.float32)
        z = z - z.max(axis=1, keepdims=True)
        a = np.exp(z)
        p = a / a.sum(axis=1, keepdims=True, dtype=np.float32)
        ex = (p * np.arange(nb, dtype=np.float32)).sum(axis=1, dtype=np.float32)
        out.append(ex * np.float32(3) - np.float32(180 if h == 0 else 99))
    return np.stack(out, axis=1)


def test_decode_reference_sits_inside_the_gpu_bound():
    """The GPU tests hold ypr to 2e-4 degrees of the float64 decode (the bound of test_decode_kernel): a plain float32 restatement is
    within 1e-4 degrees of it on every designed row and on the forward probe's logits -- half of that bound is the kernel's own."""
    e = P.expected_heads("decode", N_HEADS_BIG)
    got = softmax_expectation_f32(e["logits"])
    assert got.dtype == np.float32 and np.abs(got - e["ypr"]).max() < 1e-4, np.abs(got - e["ypr"]).max()
    f = P.expected_forward(P.N_MAX)
    assert np.abs(softmax_expectation_f32(f["logits"]) - f["ypr"]).max() < 1e-4


def test_heads_mutations_are_visible():
    """What a broken heads kernel would compute, restated, changes an expected tensor that the GPU tests compare -- at every batch
    size they run (1, 3, 5, 17) where the mutation does not need a neighbour crop or a particular row."""
    w = P.head_snapshot("dense_heads")
    for n in (1, 3, 5, P.N_MAX):
        x = P.head_const_inputs("dense_heads", n)
        base = P.ref_heads(x, w)
        for c0 in range(0, spec.FEAT, 40):                    # one 40-channel slice dropped: every logit of every crop moves
            r = P.ref_heads(x, w, {"drop_slice": (c0, c0 + 40)})
            assert changed(r["logits"], base["logits"]), (n, c0)
            assert n < P.N_MAX or (r["logits"] != base["logits"]).any(axis=0).all(), c0
        for q in range(4):                                    # partial vector p_q dropped (p3 among them)
            assert changed(P.ref_heads(x, w, {"drop_partial": q})["logits"], base["logits"]), (n, q)
        assert changed(P.ref_heads(x, w, {"bias_per_workgroup": 1})["logits"], base["logits"]), n
        assert (P.ref_heads(x, w, {"bias_per_workgroup": 1})["logits"] != base["logits"]).all()
    w = P.head_snapshot("decode")
    for n in (3, 5, P.N_MAX):
        x = P.head_const_inputs("decode", n)
        base = P.ref_heads(x, w)
        for mut in ({"logits_from": 1}, {"logits_from": n - 1}, {"pitch_from": 119}):
            r = P.ref_heads(x, w, mut)
            assert not np.array_equal(r["argmax"], base["argmax"]), (n, mut)
            assert (np.abs(r["ypr"] - base["ypr"]) > 1).any(), (n, mut)          # (degrees: far beyond the 2e-4 of the GPU test)
        assert np.array_equal(P.ref_heads(x, w, {"logits_from": 1})["logits"], base["logits"])
    x = P.head_const_inputs("decode", P.N_MAX)
    base = P.ref_heads(x, w)
    for mut, kinds in (({"argmax_last": 1}, ("equal", "tie_63_64", "tie_1_65", "tie_5_100", "narrow", "wide")),
                       ({"argmax_first_64": 1}, ("max_64", "max_last"))):
        r = P.ref_heads(x, w, mut)
        for h in range(3):
            for kind in kinds:
                rows = [i for i in range(P.N_MAX) if P.decode_kind(i, h) == kind]
                assert rows and all(r["argmax"][i, h] != base["argmax"][i, h] for i in rows), (mut, h, kind)
    # n = 1: the rows of crop 0 (equal | max_64 | tie_5_100) see both argmax mutations
    for mut in ({"argmax_last": 1}, {"argmax_first_64": 1}):
        assert not np.array_equal(P.ref_heads(x[:1], w, mut)["argmax"], base["argmax"][:1]), mut


def test_forward_probe_stays_exact_and_is_the_oracle():
    w = P.forward_snapshot()
    k = w["stem/conv/kernel"]
    assert ((k != 0).reshape(27, spec.STEM_C).sum(axis=0) == 1).all() and set(np.unique(k)) == {0, 1}
    assert (k != 0).reshape(27, spec.STEM_C).any(axis=1).all()                      # every tap of every input channel is read
    for key in w:
        if not key.startswith("stem/conv"):
            assert w[key] is P.snapshot("routing")[key], key
    x = P.forward_images(P.N_MAX)
    assert np.isin(x, [0] + list(range(18, 25))).all() and len({x[i].tobytes() for i in range(P.N_MAX)}) == P.N_MAX
    stem = P.ref_stem(x[:3], w)
    assert (stem["out"] != 0).any(axis=(0, 1, 2)).all(), "a stem channel is zero: its tap sees no diagonal"
    e = P.expected_forward(P.N_MAX)
    assert e["exact"] and e["bound"] < 2048, e["bound"]
    S = e["S"]
    assert np.array_equal(S, np.rint(S)) and S.max() < 2 ** 24 and ((S > 0).mean(axis=1) >= 0.3).all(), (S > 0).mean(axis=1).min()
    lg = e["logits"]
    assert lg.dtype == np.float32 and len({lg[i].tobytes() for i in range(P.N_MAX)}) == P.N_MAX
    # one rounding: the float32 product of the exact sum and the rounded constant
    sel = S[:, P.head_feature(np.arange(spec.N_LOGITS))]
    assert np.abs(lg.astype(np.float64) - sel / 49).max() <= (2.0 ** -24 + 2.06e-8) * (sel / 49).max()
    # the other image of the GPU test (run before every compared run) gives other logits
    assert not np.array_equal(P.expected_forward(3, first=200)["logits"], lg[:3])
    # the float64 oracle, stem to logits, on two crops.  Its own error: a value passes at most two Swishes per block, one in the stem
    # and one in the head (34), each short by at most e^-18 of it; the sums have non-negative terms only (routing weights of 1, skips)
    ref = O.heads(O.backbone(x[:2].astype(np.float64), w), w)
    want = sel[:2] / 49
    assert (np.abs(ref - want) <= 34 * np.exp(-18.0) * want + 1e-9).all(), np.abs(ref - want).max()
