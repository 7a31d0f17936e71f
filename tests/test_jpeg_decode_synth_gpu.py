"""Constructed JPEG streams (tests/jpeg_synth.py) through the decoder's kernels, no tolerance anywhere.  The expected planes and
frames come from the coefficients the WRITER was given (tests/test_jpeg_decode_synth_cpu.py holds the statements to the same), so
what is pinned here is the kernels' own part of csrc/jpeg_dec.hip and csrc/jpeg_dec_seg.hip: the marker scan, the segment table's
carry, the LDS scan of the saturating DC maps, the lane -> segment maps of 16, 32 and 64 decoding lanes per wave, the staging of
blocks, and the bit reader's 16-byte window on entropy data that does not begin on a 16-byte boundary.  Every stream is at most
72 KB and none without DRI is above 20 KB (asserted on the CPU)."""
import numpy as np
import pytest
import torch

from tests import jpeg_decode_cases as DC
from tests import jpeg_synth as S
from tests.test_jpeg_decode_seg_gpu import DEV, delta, device_packed, guarded_rows, post, read_packed, untouched  # noqa: F401 (post: a fixture)
from whenet_hip import _lib, jpeg

pytestmark = pytest.mark.gpu
FORMS = [(0, 128), (1, 4), (1, 8), (1, 128)]                     # (entropy form, seg_bytes)
LANE_CASES = ("sat_grey", "sat_420", "len16_444", "phantom_grey", "ri1_grey", "sample_001")
UNALIGNED_CASES = ("sat_grey", "ri1_grey", "fill_420", "sample_012")
MARKERS = bytes(b for n in range(8) for b in (0xFF, 0xD0 + n))   # FF D0 FF D1 .. FF D7: what a read outside the data would meet


def stream_and_truth(name):
    """(the stream, the frame, the status, the planes): the writer's for a synthetic case, the host statement's for a sample still"""
    if name in S.CASES:
        e = S.expected(name)
        return S.case(name).data, e.frame, e.status, e.planes
    data = DC.case(name)
    i = _lib.jpeg_parse(data)
    frame = np.empty((i.h, i.w, 3), np.uint8)
    status = _lib.jpeg_decode_host(data, jpeg.packed_surface(frame), True)
    return data, frame, status, jpeg.decode_planes_host(data)[0]


@pytest.fixture(scope="module")
def truth():
    """name -> stream_and_truth(name): computed once, shared, never modified"""
    return {name: stream_and_truth(name) for name in S.CASE_NAMES + ["sample_001", "sample_012"]}


# ---- 1. both entropy forms return the construction ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,seg_bytes", FORMS)
@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_both_forms_equal_the_construction(post, truth, name, form, seg_bytes):
    data, want, want_status, planes = truth[name]
    i = _lib.jpeg_parse(data)
    block, view, pitch = guarded_rows(i.h, 3 * i.w, 7, 3)                      # an odd pitch between guard bytes
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = view.ctypes.data, pitch, _lib.SURF_PACKED, 0
    status, stats = post.op_jpeg_decode_ex(data, s, True, form, seg_bytes)
    assert status.tolist() == want_status.tolist() == [_lib.OK, -1]
    assert np.array_equal(view.reshape(i.h, i.w, 3), want)
    assert untouched(block, view)
    assert stats[7] == form and stats[0] == i.intervals
    if form == 1:
        _, host_status, host_stats = jpeg.decode_segmented_host(data, seg_bytes, _lib.JPEG_SEG_WINDOW, stats=True)
        assert host_status.tolist() == want_status.tolist()
        assert stats[:5].tolist() == host_stats[:5].tolist()                    # intervals, segments, windows, sync rounds, stitch walks
        assert stats[6] == seg_bytes
    if (i.components, i.hs, i.vs) == (3, 2, 2):
        h, w, ch, cw = i.h, i.w, (i.h + 1) // 2, (i.w + 1) // 2
        blocks = [guarded_rows(*g) for g in [(h, w, 3, 1), (ch, cw, 5, 2), (ch, cw, 2, 3)]]
        s = _lib.SurfaceC()
        for p, (_, v, pt) in enumerate(blocks):
            s.plane[p], s.pitch[p] = v.ctypes.data, pt
        s.format, s.matrix, s.on_device = _lib.YUV_I420, _lib.YUV_JFIF, 0
        status, _ = post.op_jpeg_decode_ex(data, s, True, form, seg_bytes)
        assert status.tolist() == want_status.tolist()
        for (blk, v, _), ref in zip(blocks, planes):
            assert np.array_equal(v, ref) and untouched(blk, v)


# ---- 2. 16 and 64 decoding lanes per wave ---------------------------------------------------------------------------------------------
def forced(post, data, seg_bytes):
    i = _lib.jpeg_parse(data)
    frame = np.zeros((i.h, i.w, 3), np.uint8)
    status, stats = post.op_jpeg_decode_ex(data, jpeg.packed_surface(frame), True, 1, seg_bytes)
    return frame, status.tolist(), stats


@pytest.fixture(scope="module")
def default_lanes(post, truth):
    """(name, seg_bytes) -> the segmented decode at the default lanes (option jpeg_seg_lanes = 0)"""
    post.set_option("jpeg_seg_lanes", 0)
    return {(name, seg_bytes): forced(post, truth[name][0], seg_bytes) for name in LANE_CASES for seg_bytes in (4, 128)}


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("name", LANE_CASES)
def test_lane_widths_give_the_same_output_and_statistics(post, truth, default_lanes, name, lanes):
    """The sync kernel's workgroup is WINDOW x 64 / lanes threads and lane -> segment is (wave x lanes + lane) in the sync, count and
    write kernels.  The statistics are compared too, the sync rounds [3] and the bytes a lane fetched [5] included: a window's rounds
    are taken in lockstep by all of its segments behind barriers whatever wave holds them, so nothing in the header's text depends
    on the lanes."""
    data, want, want_status, _ = truth[name]
    try:
        post.set_option("jpeg_seg_lanes", lanes)
        for seg_bytes in (4, 128):
            frame, status, stats = forced(post, data, seg_bytes)
            ref_frame, ref_status, ref_stats = default_lanes[(name, seg_bytes)]
            assert status == ref_status == want_status.tolist()
            assert np.array_equal(frame, ref_frame) and np.array_equal(frame, want)
            assert stats[:6].tolist() == ref_stats[:6].tolist() and stats[6] == seg_bytes and stats[7] == 1
    finally:
        post.set_option("jpeg_seg_lanes", 0)


def test_other_lane_widths_are_refused(post):
    for bad in (8, 48, 128, -16):
        with pytest.raises(ValueError):
            post.set_option("jpeg_seg_lanes", bad)


# ---- 3. entropy data that does not begin on a 16-byte boundary ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_handle():
    h = _lib.Handle.postproc(0)
    yield h
    h.close()


@pytest.mark.parametrize("form,seg_bytes", [(0, 128), (1, 4), (1, 128)])
@pytest.mark.parametrize("name", UNALIGNED_CASES)
def test_unaligned_entropy_pointer(device_handle, truth, name, form, seg_bytes):
    """whenet_jpeg_decode_device with d_entropy = a 16-byte boundary + k and nbytes exact.  The header asks no alignment of d_entropy:
    the bit reader's window (JpegBitReader::byte_at) and the marker scan take their 16-byte loads from the address, not the index.
    The allocation holds FF D0 FF D1 .. in front of and behind the data: a byte read outside [0, nbytes) is a restart marker too
    many (or a marker that ends an interval's bits early) and shows in the status or the picture."""
    data, want, want_status, _ = truth[name]
    info = _lib.jpeg_parse(data)
    ent = np.frombuffer(data, np.uint8)[info.data_offset:]
    h = device_handle
    got = {}
    try:
        h.set_option("jpeg_entropy", form)
        h.set_option("jpeg_seg_bytes", seg_bytes)
        for k in (0, 1, 7, 15):
            at = 32 + k
            host = np.frombuffer((MARKERS * (ent.size // 16 + 8))[:at + ent.size + 48], np.uint8).copy()
            host[:at] = np.frombuffer(MARKERS * 3, np.uint8)[-at:]              # .. FF Dn ends right in front of the data
            host[at:at + ent.size] = ent
            host[at + ent.size:] = np.frombuffer(MARKERS * 3, np.uint8)[:48]    # FF D0 .. begins right behind it
            buf = torch.from_numpy(host).to(DEV)
            assert buf.data_ptr() % 16 == 0
            status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
            out, s_dst = device_packed(info.h, info.w, 5, 3)
            before = h.jpeg_decode_counters()
            h.jpeg_decode_device(info, buf.data_ptr() + at, ent.size, s_dst, True, status.data_ptr())
            torch.cuda.synchronize()
            assert delta(h.jpeg_decode_counters(), before) == {"interval": 1 - form, "segmented": form}
            frame, clean = read_packed(out, info.h, info.w, 5, 3)
            got[k] = (frame, status.cpu().tolist())
            assert clean, k
            assert buf.cpu().numpy().tobytes() == host.tobytes()
    finally:
        h.set_option("jpeg_entropy", 2)
        h.set_option("jpeg_seg_bytes", 128)
    for k in (0, 1, 7, 15):
        assert got[k][1] == got[0][1] == want_status.tolist(), k
        assert np.array_equal(got[k][0], got[0][0]) and np.array_equal(got[k][0], want), k


# ---- 4. the form that "auto" takes ----------------------------------------------------------------------------------------------------
def test_auto_takes_the_segmented_form_for_a_long_interval_and_the_other_for_600_short_ones(truth):
    h = _lib.Handle.postproc(0)
    try:
        for name, form in (("idct_extreme", "segmented"), ("ri1_grey", "interval")):
            s = S.case(name)
            data, want, want_status, _ = truth[name]
            per_interval = (len(data) - s.data_offset) // s.header.intervals        # from the writer, not from a parser
            assert (per_interval >= _lib.JPEG_SEG_AUTO_BYTES) == (form == "segmented")
            before = h.jpeg_decode_counters()
            got = np.zeros_like(want)
            status = h.op_jpeg_decode(data, jpeg.packed_surface(got), True)
            assert np.array_equal(got, want) and status.tolist() == want_status.tolist()
            d = delta(h.jpeg_decode_counters(), before)
            assert d[form] == 1 and sum(d.values()) == 1, (name, d)
    finally:
        h.close()
