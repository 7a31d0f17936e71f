"""Option front2_static (f16 handles): the layers that run front2.hip use the form of the kernel whose tile geometry -- H, Cin,
Cexp, the tile and strip shapes, the LDS offsets, the launch's tile and chunk counts -- is compile-time constants (the plan of
the layer's row in front2_tuned.inc) instead of fields of the kernel's parameter block.  Only index arithmetic differs: the
MFMAs, the Swish, the roundings, the LDS layout, the tile -> partial-sum slot mapping and every summation order are the generic
form's.  So every output is BITWISE that of front2_static = 0: whole forwards at batch sizes on both sides of xcd_unit()'s
whole-rounds / remainder split, with the arena poisoned, as one chain and as two, on every engine with forwards in flight, and
block by block behind the squeeze-excite gate.  Shapes and plans outside the table keep the generic form."""
import os
import subprocess
import sys

import numpy as np
import pytest

from whenet_hip import _lib, spec, synth, weights as W

pytestmark = pytest.mark.gpu

BATCHES = (1, 7, 8, 9, 65)
COVERED = (2, 3, 4, 5, 7, 8, 9, 10, 11, 12)      # blocks whose front2 launch has a static form


@pytest.fixture(scope="module")
def blob(weights):
    return W.pack(weights)


@pytest.fixture(scope="module")
def crops():
    return synth.noise_crops(65, seed=1234)


@pytest.fixture(scope="module")
def h16(blob):
    with _lib.Handle(blob, device=0, dtype=_lib.F16) as h:
        yield h


@pytest.fixture(scope="module")
def generic(h16, crops):
    """front2_static = 0: ypr, argmax, logits of every batch size."""
    h16.set_option("front2_static", 0)
    try:
        return {n: h16.forward(crops[:n]) for n in BATCHES}
    finally:
        h16.set_option("front2_static", 1)


def same(got, want):
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def front_launches(h, crops, n=8):
    d = h.device_alloc(crops[:n].nbytes)
    try:
        h.h2d(d, crops[:n])
        return h.profile(d, n, 2)
    finally:
        h.device_free(d)


@pytest.mark.parametrize("poison", [0, 1])
def test_static_form_is_bitwise_the_generic_form(h16, crops, generic, poison):
    h16.set_option("poison", poison)
    try:
        for n in BATCHES:
            assert same(h16.forward(crops[:n]), generic[n]), (poison, n)
    finally:
        h16.set_option("poison", 0)


@pytest.mark.parametrize("lanes", [1, 2])
def test_static_form_is_bitwise_the_generic_form_for_one_and_two_chains(h16, crops, generic, lanes):
    h16.set_option("lanes", lanes)
    h16.set_option("min_lane_crops", 2)            # (7 crops travel as 3 + 4 with two chains)
    try:
        for n in BATCHES:
            assert same(h16.forward(crops[:n]), generic[n]), (lanes, n)
    finally:
        h16.set_option("min_lane_crops", 16)
        h16.set_option("lanes", 2)


def test_static_form_is_bitwise_the_generic_form_on_every_engine_in_flight(blob, crops, generic):
    with _lib.Handle(blob, device=0, dtype=_lib.F16) as h:
        h.set_option("inflight", 3)                 # (also switches the grouped XCD placement on)
        for n in BATCHES:
            for slot in range(3):                   # blocking forwards go round robin over the engines
                assert same(h.forward(crops[:n]), generic[n]), (n, slot)
            tickets = [h.submit(crops[:n]) for _ in range(3)]
            for slot, t in enumerate(tickets):
                assert same(h.collect(t, n, want_logits=True), generic[n]), (n, slot)


def test_static_form_without_the_xcd_map(h16, crops, generic):
    h16.set_option("xcd_map", 0)
    try:
        for n in BATCHES:
            assert same(h16.forward(crops[:n]), generic[n]), n
    finally:
        h16.set_option("xcd_map", 7)


@pytest.mark.parametrize("index", [2, 3, 4, 5, 7, 9, 10, 12])
def test_block_outputs_are_bitwise_the_generic_forms(h16, index):
    """whenet_op_block: the depthwise output and the block output (behind the gate: a changed squeeze-excite partial shows; the
    gate itself is read back only on blocks whose project conv does not compute it)."""
    b = spec.blocks()[index - 1]
    rng = np.random.default_rng(100 + index)
    for n in (1, 9):
        x = rng.standard_normal((n, b.h_in, b.h_in, b.cin)).astype(np.float32)
        outs = {}
        try:
            for static in (0, 1):
                h16.set_option("front2_static", static)
                outs[static] = h16.op_block(index, x)
        finally:
            h16.set_option("front2_static", 1)
        for key in ("dw", "out"):
            assert outs[1][key].tobytes() == outs[0][key].tobytes(), (index, n, key)
            assert np.isfinite(outs[1][key]).all()


def test_blocks_1_and_2_with_the_folded_project(h16):
    """Block 2's static form is the GATED kernel (option fold12): reached through the range entry point, as in the forward."""
    b = spec.blocks()[0]
    rng = np.random.default_rng(99)
    for n in (1, 9):
        x = rng.standard_normal((n, b.h_in, b.h_in, b.cin)).astype(np.float32)
        outs = {}
        try:
            for static in (0, 1):
                h16.set_option("front2_static", static)
                outs[static] = h16.op_block_range(1, 2, x)
        finally:
            h16.set_option("front2_static", 1)
        assert outs[1].tobytes() == outs[0].tobytes() and np.isfinite(outs[1]).all(), n


def test_shapes_outside_the_table_keep_the_generic_form(h16, crops):
    """fold12 = 0 (block 2 with 16 input channels), front_impl = 0 (no front2 launch at all): same bits for both option values,
    and no static kernel where the table has no row."""
    try:
        for key in ("fold12", "front_impl"):
            h16.set_option(key, 0)
            outs = {}
            for static in (0, 1):
                h16.set_option("front2_static", static)
                outs[static] = {n: h16.forward(crops[:n]) for n in (7, 9)}
            names = {s["layer"]: s["kernel"] for s in front_launches(h16, crops)}
            h16.set_option(key, 1)
            for n in (7, 9):
                assert same(outs[1][n], outs[0][n]), (key, n)
            if key == "fold12":
                assert names["b2/front"].startswith("whenet_front2_kernel<3, 2, 1, "), names["b2/front"]
                assert names["b3/front"].startswith("whenet_front2_static_kernel<"), names["b3/front"]
            else:
                assert not any("front2" in k for k in names.values())
    finally:
        for key in ("fold12", "front_impl", "front2_static"):
            h16.set_option(key, 1)


CHILD = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1] + '/headposeestimation-whenet_amd'); sys.path.insert(0, sys.argv[1]);"
         "import torch; from whenet_hip import _lib, synth, weights as W;"
         "h = _lib.Handle(W.pack(W.synthetic(1234)), device=0, dtype=_lib.F16); c = synth.noise_crops(9, seed=1234); outs = {};\n"
         "for s in (0, 1):\n"
         "    h.set_option('front2_static', s); outs[s] = h.forward(c)\n"
         "d = h.device_alloc(c.nbytes); h.h2d(d, c); names = {s['layer']: s['kernel'] for s in h.profile(d, 9, 2)}; h.device_free(d); h.close()\n"
         "assert all(a.tobytes() == b.tobytes() for a, b in zip(outs[0], outs[1])), 'bits differ'\n"
         "print('B2=' + names['b2/front']); print('B4=' + names['b4/front']); print('B7=' + names['b7/front'])")


@pytest.mark.parametrize("var,value", [("WHENET_FRONT_THREADS", "256"), ("WHENET_FRONT_NO_TUNED", "1")])
def test_forced_plans_keep_the_generic_form(var, value):
    """The probes' environment variables are read once per process: a child process each.  A 256-lane block 2 is not the
    table's plan (512 lanes); without the tuned table a layer keeps the static form only where the fallback plan IS the
    table's (block 4: 32 channels x 7 rows x the full width), block 7's fallback plan (7 rows) is not."""
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, "-c", CHILD, root], env=dict(os.environ, **{var: value}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    names = dict(line.split("=", 1) for line in r.stdout.splitlines() if line[:3] in ("B2=", "B4=", "B7="))
    if var == "WHENET_FRONT_THREADS":
        assert names["B2"].startswith("whenet_front2_kernel<3, 2, 2, 256, 0, true>"), names
        assert names["B4"].startswith("whenet_front2_static_kernel<"), names
    else:
        assert names["B4"].startswith("whenet_front2_static_kernel<"), names
        assert names["B7"].startswith("whenet_front2_kernel<"), names


def test_profile_reports_the_kernel_that_runs(h16, crops):
    prof = {}
    try:
        for static in (0, 1):
            h16.set_option("front2_static", static)
            prof[static] = front_launches(h16, crops)
    finally:
        h16.set_option("front2_static", 1)
    assert len(prof[0]) == len(prof[1])
    for a, b in zip(prof[0], prof[1]):
        assert (a["layer"], a["kind"], a["alg_bytes"], a["alg_flops"], a["crops"]) == (b["layer"], b["kind"], b["alg_bytes"], b["alg_flops"], b["crops"])
        if a["layer"] in {f"b{i}/front" for i in COVERED}:
            assert a["kernel"].startswith("whenet_front2_kernel<") and b["kernel"].startswith("whenet_front2_static_kernel<"), (a, b)
            assert b["kernel"].split("<")[1].startswith(a["kernel"].split("<")[1].rstrip(">"))      # the same instantiation + its row
        else:
            assert a["kernel"] == b["kernel"], (a, b)


def test_front2_static_range(h16):
    for bad in (-1, 2):
        assert h16._lib.whenet_set_option(h16._h, b"front2_static", bad) == _lib.EINVAL
    for ok in (0, 1):
        h16.set_option("front2_static", ok)
