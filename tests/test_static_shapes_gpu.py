"""Options pw_static and front_static (f16 handles): the project 1x1 GEMMs and block 6's front kernel run, where the per-layer
tables say so, the instantiation of their kernel whose layer shape -- K, N, the pixels per crop, tile and chunk counts, the
squeeze-excite sizes, the tile plan -- is compile-time constants instead of kernel arguments.  Only index arithmetic differs:
tiles, k-group ownership, the combine order, the LDS layout, the roundings and every summation order are the generic form's.
So every output is BITWISE that of pw_static = 0 / front_static = 0: whole forwards at 1, 3, 7, 9 and 65 crops (the smallest
that reach a 64-row tile holding rows of three crops at HW = 49, a partial last tile, a last workgroup past MT's multiple of 8
and both sides of xcd_unit()'s split; at 65 crops every layer of the tables runs its static form), with the arena poisoned, as
one chain and on every engine with forwards in flight, and block by block.  Launches outside the tables keep the generic form."""
import numpy as np
import pytest

from whenet_hip import _lib, spec, synth, weights as W

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 7, 9, 65)
# the layers whose launch at 65 crops in one chain is the static form: {layer: row of the kernel's shape table}
PW_STATIC = {"b2/project": 0, "b3/project": 1, "b4/project": 2, "b7/project": 5, "b9/project": 6,
             "b13/project": 9, "b14/project": 9, "b15/project": 9, "b16/project": 10}
FRONT_STATIC = {"b6/front": 0}
OPTIONS = ("pw_static", "front_static")


@pytest.fixture(scope="module")
def blob(weights):
    return W.pack(weights)


@pytest.fixture(scope="module")
def crops():
    return synth.noise_crops(65, seed=4321)


@pytest.fixture(scope="module")
def h16(blob):
    with _lib.Handle(blob, device=0, dtype=_lib.F16) as h:
        yield h


def set_both(h, pw, front):
    h.set_option("pw_static", pw)
    h.set_option("front_static", front)


@pytest.fixture(scope="module")
def generic(h16, crops):
    """pw_static = 0, front_static = 0: ypr, argmax, logits of every batch size (computed once, never changed)."""
    set_both(h16, 0, 0)
    try:
        return {n: h16.forward(crops[:n]) for n in BATCHES}
    finally:
        set_both(h16, 1, 1)


def same(got, want):
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def launches(h, crops, n=65):
    """whenet_profile()'s launch list of ONE chain of n crops."""
    d = h.device_alloc(crops[:n].nbytes)
    h.set_option("lanes", 1)
    try:
        h.h2d(d, crops[:n])
        return h.profile(d, n, 2)
    finally:
        h.set_option("lanes", 2)
        h.device_free(d)


def static_row(kernel):
    """The shape-table row of a static instantiation (its last template argument: the sixth of a project GEMM as the profile
    spells it, the seventh of the front kernel), or None for the generic form."""
    if "<" not in kernel:
        return None
    args = kernel[kernel.index("<") + 1:-1].split(", ")
    if kernel.startswith("whenet_pw_") and len(args) == 6 and args[-1].isdigit():
        return int(args[-1])
    if kernel.startswith("whenet_front_kernel<") and len(args) == 7:
        return int(args[-1])
    return None


@pytest.mark.parametrize("pw,front", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("poison", [0, 1])
def test_static_forms_are_bitwise_the_generic_forms(h16, crops, generic, pw, front, poison):
    h16.set_option("poison", poison)
    set_both(h16, pw, front)
    try:
        for n in BATCHES:
            assert same(h16.forward(crops[:n]), generic[n]), (pw, front, poison, n)
    finally:
        set_both(h16, 1, 1)
        h16.set_option("poison", 0)


def test_static_forms_as_one_chain(h16, crops, generic):
    h16.set_option("lanes", 1)
    try:
        for n in BATCHES:
            assert same(h16.forward(crops[:n]), generic[n]), n
    finally:
        h16.set_option("lanes", 2)


def test_static_forms_on_every_engine_in_flight(blob, crops, generic):
    with _lib.Handle(blob, device=0, dtype=_lib.F16) as h:
        h.set_option("inflight", 3)                 # (each forward is one chain; also switches the grouped XCD placement on)
        for n in BATCHES:
            for slot in range(3):                   # blocking forwards go round robin over the engines
                assert same(h.forward(crops[:n]), generic[n]), (n, slot)
            tickets = [h.submit(crops[:n]) for _ in range(3)]
            for slot, t in enumerate(tickets):
                assert same(h.collect(t, n, want_logits=True), generic[n]), (n, slot)


# n = 1 and 3, and the smallest batch at which the block's launch is the table's (the split-K GEMMs take 2 x 2 tiles from 21
# crops on; block 6's front kernel runs 256 lanes from 33 crops on)
@pytest.mark.parametrize("index,more", [(2, ()), (3, ()), (4, ()), (5, ()), (6, (33,)), (7, (21,)), (9, (21,)), (10, (21,))])
def test_block_outputs_are_bitwise_the_generic_forms(h16, index, more):
    """whenet_op_block: the depthwise output, the gate where it is read back, and the block output -- behind the gate that blocks
    4 to 6 compute in their project GEMM from the front kernel's squeeze-excite partial vectors, so a changed partial shows."""
    b = spec.blocks()[index - 1]
    rng = np.random.default_rng(200 + index)
    for n in (1, 3) + more:
        x = rng.standard_normal((n, b.h_in, b.h_in, b.cin)).astype(np.float32)
        outs = {}
        try:
            for static in (0, 1):
                set_both(h16, static, static)
                outs[static] = h16.op_block(index, x)
        finally:
            set_both(h16, 1, 1)
        for key in ("dw", "out"):
            assert outs[1][key].tobytes() == outs[0][key].tobytes(), (index, n, key)
            assert np.isfinite(outs[1][key]).all()


def test_block_6_squeeze_excite_partials_are_bitwise_the_generic_forms(h16):
    """The partial vectors block 6's front kernel writes, seen through the stand-alone excite kernel (se_fuse = 0: the gate is
    computed from them by se.hip and read back, and the depthwise output next to it) -- at 33 crops the launch is the table's."""
    b = spec.blocks()[5]
    rng = np.random.default_rng(306)
    try:
        h16.set_option("se_fuse", 0)
        for n in (1, 3, 33):
            x = rng.standard_normal((n, b.h_in, b.h_in, b.cin)).astype(np.float32)
            outs = {}
            for static in (0, 1):
                h16.set_option("front_static", static)
                outs[static] = h16.op_block(6, x)
            for key in ("dw", "gate", "out"):
                assert outs[1][key].tobytes() == outs[0][key].tobytes(), (n, key)
            assert np.isfinite(outs[1]["gate"]).all() and outs[1]["gate"].any()
    finally:
        h16.set_option("se_fuse", 1)
        set_both(h16, 1, 1)


def test_blocks_12_to_16_with_the_blocked_layout(h16):
    """The 7 x 7 blocks' static forms store (and read the skip in) 16-channel blocks: reached through the range entry point, at
    the smallest batch whose 49-pixel maps fill 128 workgroups of 2 x 2 tiles (55 crops)."""
    b = spec.blocks()[11]
    rng = np.random.default_rng(212)
    for n in (1, 3, 55):
        x = rng.standard_normal((n, b.h_in, b.h_in, b.cin)).astype(np.float32)
        outs = {}
        try:
            for static in (0, 1):
                set_both(h16, static, static)
                outs[static] = h16.op_block_range(12, 16, x)
        finally:
            set_both(h16, 1, 1)
        assert outs[1].tobytes() == outs[0].tobytes() and np.isfinite(outs[1]).all(), n


def test_profile_reports_the_kernel_that_runs(h16, crops):
    prof = {}
    try:
        for static in (0, 1):
            set_both(h16, static, static)
            prof[static] = launches(h16, crops)
    finally:
        set_both(h16, 1, 1)
    assert len(prof[0]) == len(prof[1])
    for a, b in zip(prof[0], prof[1]):
        assert (a["layer"], a["kind"], a["alg_bytes"], a["alg_flops"], a["crops"]) == (b["layer"], b["kind"], b["alg_bytes"], b["alg_flops"], b["crops"])
        want = {**PW_STATIC, **FRONT_STATIC}.get(a["layer"])
        assert static_row(a["kernel"]) is None, a
        if want is None:
            assert a["kernel"] == b["kernel"], (a, b)
        else:
            assert static_row(b["kernel"]) == want, (a, b)
            assert b["kernel"].startswith(a["kernel"].rstrip(">").removesuffix(", false")), (a, b)      # the same instantiation + its row


@pytest.mark.parametrize("key,generic_layers", [
    ("se_fuse", set(PW_STATIC)),                                                          # every gate from global memory
    ("act_layout", {"b12/project", "b13/project", "b14/project", "b15/project", "b16/project"}),
    ("pw_staged", {"b13/project", "b14/project", "b15/project", "b16/project"}),
    ("fold12", {"b1/project"}),
])
def test_launches_outside_the_tables_keep_the_generic_form(h16, crops, key, generic_layers):
    """With the option off the affected blocks' launches are no row of the tables: generic kernels there, static ones elsewhere,
    and the same bits for both values of pw_static / front_static."""
    try:
        h16.set_option(key, 0)
        names = {s["layer"]: s["kernel"] for s in launches(h16, crops)}
        outs = {}
        for static in (0, 1):
            set_both(h16, static, static)
            outs[static] = {n: h16.forward(crops[:n]) for n in (9, 65)}
    finally:
        h16.set_option(key, 1)
        set_both(h16, 1, 1)
    for n in (9, 65):
        assert same(outs[1][n], outs[0][n]), (key, n)
    for layer in generic_layers:
        assert static_row(names[layer]) is None, (key, layer, names[layer])
    for layer, row in PW_STATIC.items():
        if layer not in generic_layers:
            assert static_row(names[layer]) == row, (key, layer, names[layer])


def test_small_batches_keep_the_generic_form_where_the_blocking_differs(h16, crops):
    """At 9 crops the deep GEMMs run 1 x 1 tiles and block 6's front kernel 512 lanes: neither is the table's launch."""
    names = {s["layer"]: s["kernel"] for s in launches(h16, crops, 9)}
    for layer in ("b6/front", "b7/project", "b12/project", "b16/project"):
        assert static_row(names[layer]) is None, (layer, names[layer])
    assert static_row(names["b2/project"]) == 0, names["b2/project"]


def test_option_ranges(h16):
    for key in OPTIONS:
        for bad in (-1, 2):
            assert h16._lib.whenet_set_option(h16._h, key.encode(), bad) == _lib.EINVAL
        for ok in (0, 1):
            h16.set_option(key, ok)
