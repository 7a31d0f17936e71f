"""Option act_layout (f16 handles): the 7 x 7 tensors between the blocks -- the outputs of the project convs of blocks 12-16 --
stored as 16-channel blocks [crop][C/16][HW][16] instead of NHWC.  The producer (the split-K project
epilogue) and the consumers (front7.hip, head7.hip, the skip operand of the next project) only change addresses: no
arithmetic, no order of summation.  So every output is BITWISE the NHWC schedule's -- for ragged and whole batches, with the
arena poisoned (every element read was written by this forward, in the layout it is read in), on every engine of a handle
with forwards in flight, as one chain and as two, and where kernels that do not know the layout (mb7.hip, front.hip, the
un-fused head conv) sit between kernels that do."""
import numpy as np
import pytest

from whenet_hip import _lib, synth, weights as W

pytestmark = pytest.mark.gpu

BATCHES = (1, 7, 64, 65)


@pytest.fixture(scope="module")
def blob(weights):
    return W.pack(weights)


@pytest.fixture(scope="module")
def crops():
    return np.concatenate([synth.scene_crops(40, seed=71), synth.noise_crops(25, seed=72)])       # 65 seeded crops


@pytest.fixture(scope="module")
def h16(blob):
    with _lib.Handle(blob, device=0, dtype=_lib.F16) as h:
        yield h


@pytest.fixture(scope="module")
def nhwc(h16, crops):
    """act_layout = 0: ypr, argmax, logits of every batch size under the default schedule."""
    h16.set_option("act_layout", 0)
    try:
        return {n: h16.forward(crops[:n]) for n in BATCHES}
    finally:
        h16.set_option("act_layout", 1)


def same(got, want):
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("layout", [2, 1])
@pytest.mark.parametrize("poison", [0, 1])
def test_blocked_layout_is_bitwise_nhwc(h16, crops, nhwc, layout, poison):
    h16.set_option("act_layout", layout)
    h16.set_option("poison", poison)
    try:
        for n in BATCHES:
            assert same(h16.forward(crops[:n]), nhwc[n]), (layout, poison, n)
    finally:
        h16.set_option("poison", 0)
        h16.set_option("act_layout", 1)


@pytest.mark.parametrize("layout", [2, 1])
@pytest.mark.parametrize("lanes", [1, 2])
def test_blocked_layout_is_bitwise_nhwc_for_one_and_two_chains(h16, crops, nhwc, layout, lanes):
    h16.set_option("act_layout", layout)
    h16.set_option("lanes", lanes)
    h16.set_option("min_lane_crops", 2)            # (7 crops travel as 3 + 4 with two chains)
    try:
        for n in BATCHES:
            assert same(h16.forward(crops[:n]), nhwc[n]), (layout, lanes, n)
    finally:
        h16.set_option("min_lane_crops", 16)
        h16.set_option("lanes", 2)
        h16.set_option("act_layout", 1)


@pytest.mark.parametrize("layout", [2, 1])
def test_blocked_layout_is_bitwise_nhwc_on_every_engine_in_flight(blob, crops, nhwc, layout):
    with _lib.Handle(blob, device=0, dtype=_lib.F16) as h:
        h.set_option("inflight", 3)
        h.set_option("act_layout", layout)          # (reaches every engine of the handle)
        for n in BATCHES:
            for slot in range(3):                   # blocking forwards go round robin over the engines
                assert same(h.forward(crops[:n]), nhwc[n]), (layout, n, slot)
            tickets = [h.submit(crops[:n]) for _ in range(3)]          # and three submissions in flight at once
            for slot, t in enumerate(tickets):
                assert same(h.collect(t, n, want_logits=True), nhwc[n]), (layout, n, slot)


def test_kernels_without_the_layout_keep_nhwc(h16, crops, nhwc):
    """mb7.hip (blocks 13-16) and front.hip (front_impl = 0) read and write NHWC only: the tensors they touch stay NHWC whatever
    act_layout says, the others may be blocked -- each of those schedules gives the same bits for act_layout 0 and 2."""
    try:
        for key, value in (("mb7", 1), ("front_impl", 0), ("front7", 0), ("head_fuse", 0), ("fuse_front", 0)):
            h16.set_option(key, value)
            outs = {}
            for layout in (0, 2):
                h16.set_option("act_layout", layout)
                outs[layout] = {n: h16.forward(crops[:n]) for n in (7, 65)}
            h16.set_option(key, {"mb7": 0, "front_impl": 1, "front7": 1, "head_fuse": 1, "fuse_front": 1}[key])
            for n in (7, 65):
                assert same(outs[2][n], outs[0][n]), (key, n)
                assert np.isfinite(outs[2][n][2]).all()
    finally:
        for key, value in (("mb7", 0), ("front_impl", 1), ("front7", 1), ("head_fuse", 1), ("fuse_front", 1), ("act_layout", 1)):
            h16.set_option(key, value)


def test_act_layout_range(h16):
    for bad in (-1, 3):
        assert h16._lib.whenet_set_option(h16._h, b"act_layout", bad) == _lib.EINVAL
        with pytest.raises(ValueError):
            h16.set_option("act_layout", bad)
    for ok in (0, 2, 1):
        h16.set_option("act_layout", ok)
