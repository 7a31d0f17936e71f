"""Default Huffman tables on the GPU: `default_tables=True` on jpeg.decode / decode_clip and FramePipeline.begin_jpeg /
begin_clip_jpeg completes an MJPG frame without DHT on the host (whenet_jpeg_add_default_tables) and hands it to the calls that
exist: the frames, status words and collect results are those of the unstripped streams, bit for bit, and without the argument a
stripped stream is refused before a slot is taken, as before.  Small streams: 35 x 50 and 64 x 48."""
import json
import os

import numpy as np
import pytest

from tests import jpeg_default_tables_cases as DT
from tests.test_clip_gpu import assert_same, kwargs
from tests.test_yuv_gpu import seeded_model
from whenet_hip import _lib, jpeg
from whenet_hip.frames import FramePipeline

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL = DT.STRIPS["all"]


@pytest.fixture(scope="module")
def post():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def model():
    m = seeded_model()
    yield m
    m.close()


@pytest.fixture(scope="module")
def kw():
    with open(os.path.join(GOLDEN, "reference_detector.json")) as f:
        return kwargs(json.load(f)["detect"], "tiny", score=0.0)       # threshold 0: the seeded detector fires on small frames


def stream(name):
    return DT.sources()[name]


# ---- 1. the kernels alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pil_444_35x50", "pil_422_35x50_dri", "pil_420_35x50", "pil_grey_35x50", "pil_420_64x48", "own_422_35x50",
                                  "pil_prog_420_35x50"])
def test_decode_of_a_stripped_stream_equals_the_host_statement(post, name):
    data, sof2 = stream(name)
    stripped = DT.strip(data, DT.STRIPS["ac"] if sof2 else ALL)
    for rule in ("own", "libjpeg"):
        want = jpeg.decode_host(data, rule=rule, progressive=sof2)
        assert jpeg.decode_host(stripped, rule=rule, progressive=sof2, default_tables=True).tobytes() == want.tobytes()
        got = jpeg.decode(stripped, handle=post, rule=rule, progressive=sof2, default_tables=True)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (name, rule)
    if not sof2:
        with pytest.raises(ValueError, match="missing Huffman table"):
            jpeg.decode(stripped, handle=post)


def test_decode_clip_of_complete_stripped_and_progressive_streams(post):
    names = ["pil_420_35x50", "pil_422_35x50_dri", "pil_prog_420_35x50", "pil_420_64x48", "pil_grey_35x50"]
    whole = [stream(n)[0] for n in names]
    clip = [whole[0], DT.strip(whole[1], ALL), DT.strip(whole[2], DT.STRIPS["ac"]), DT.strip(whole[3], DT.STRIPS["id1"]), DT.strip(whole[4], ALL)]
    want, want_status = jpeg.decode_clip(whole, handle=post, progressive=True)
    got, status = jpeg.decode_clip(clip, handle=post, progressive=True, default_tables=True)
    assert status.tolist() == want_status.tolist() == [[_lib.OK, -1]] * 5
    for g, w, n in zip(got, want, names):
        assert g.tobytes() == w.tobytes() == jpeg.decode_host(stream(n)[0], progressive=True).tobytes(), n
    with pytest.raises(ValueError, match="frame 1: .*missing Huffman table"):
        jpeg.decode_clip(clip, handle=post, progressive=True)


# ---- 2. the pipeline ----------------------------------------------------------------------------------------------------------------
def run_frame(fp, kw, data, **begin_kw):
    st = fp.begin_jpeg(data, **begin_kw)
    fp.detect_heads(**kw)
    return fp.collect(detections=True), st


def run_clip(fp, kw, datas, **begin_kw):
    sts = fp.begin_clip_jpeg(datas, **begin_kw)
    fp.detect_heads_clip(**kw)
    return fp.collect_clip(detections=True), sts


def test_begin_jpeg_of_a_stripped_stream_equals_the_unstripped_submission(model, kw):
    with FramePipeline(model, depth=1) as fp:
        fired = 0
        for name in ("pil_420_64x48", "pil_422_35x50_dri", "pil_prog_420_35x50"):
            data, sof2 = stream(name)
            stripped = DT.strip(data, DT.STRIPS["ac"] if sof2 else ALL)
            want, wst = run_frame(fp, kw, data, progressive=sof2)
            got, gst = run_frame(fp, kw, stripped, progressive=sof2, default_tables=True)
            assert_same(got, want)
            assert (gst.ok, gst.interval) == (wst.ok, wst.interval) == (True, -1)
            fired += len(want[4])
            if not sof2:
                with pytest.raises(ValueError, match="missing Huffman table"):
                    fp.begin_jpeg(stripped)
                assert fp.in_flight == 0
        assert fired > 0                                # the detector fired: windows, angles and logits were compared


def test_begin_clip_jpeg_of_complete_stripped_and_progressive_streams(model, kw):
    names = ["pil_420_35x50", "pil_422_35x50_dri", "pil_prog_420_35x50", "pil_420_64x48"]      # two sizes: a mixed clip
    whole = [stream(n)[0] for n in names]
    clip = [whole[0], DT.strip(whole[1], ALL), DT.strip(whole[2], DT.STRIPS["ac"]), DT.strip(whole[3], ALL)]
    with FramePipeline(model, depth=1) as fp:
        (want, wcount), wsts = run_clip(fp, kw, whole, progressive=True)
        for _ in range(2):                              # (the slot's buffers reused)
            (got, gcount), gsts = run_clip(fp, kw, clip, progressive=True, default_tables=True)
            assert gcount == wcount and len(got) == len(want) == 4
            for g, w in zip(got, want):
                assert_same(g, w)
            assert [(s.ok, s.interval) for s in gsts] == [(s.ok, s.interval) for s in wsts] == [(True, -1)] * 4
        with pytest.raises(ValueError, match="frame 1: .*missing Huffman table"):
            fp.begin_clip_jpeg(clip, progressive=True)
        assert fp.in_flight == 0 and fp._begun_clip is None


def test_the_default_still_refuses_before_a_slot_is_taken():
    good = stream("pil_420_35x50")[0]
    stripped = DT.strip(good, ALL)

    def next_ticket(h):
        t = h.frame_begin_jpeg(good, np.zeros(2, np.int32))
        h.frame_heads(t, np.zeros((0, 4), np.int32))
        h.collect(t, 0)
        return t

    m, twin = seeded_model(), seeded_model()            # the twin sees the accepted submissions alone
    try:
        want = [next_ticket(twin._handle) for _ in range(3)]
        got = [next_ticket(m._handle)]
        for _ in range(2):
            for _ in range(_lib.MAX_INFLIGHT + 1):      # (a leak would use up the slots)
                with pytest.raises(ValueError, match="missing Huffman table"):
                    m._handle.frame_begin_jpeg(stripped, np.zeros(2, np.int32))
                with pytest.raises(ValueError, match="frame 1: .*missing Huffman table"):
                    m._handle.clip_begin_jpeg([good, stripped], np.zeros((2, 2), np.int32))
            got.append(next_ticket(m._handle))
        assert got == want
    finally:
        m.close()
        twin.close()
