"""Constructed JPEG streams (tests/jpeg_synth.py) through the decoder's statements on the CPU.  Every other stream of the suite comes
from an encoder and every other expected value from a decoder; here the expected coefficients are the writer's own, so the numpy
statement of tests/jpeg_decode_cases.py is itself held to something that is no decoder, and the host statement
(`whenet_jpeg_decode_host`, `whenet_jpeg_decode_planes_host`) and the host emulation of the segmented form
(`whenet_jpeg_decode_segmented_host`) are held to the planes and the frame derived from those coefficients -- on saturating DC
predictors, 9 / 10 / 16-bit codes, complete codes whose padding is a code word, value sizes up to 15, crossed table ids, other EOB
symbols, a ZRL onto k = 64, fill bytes, bytes behind an interval's last block, 600 intervals and the inverse DCT at the end of its
int32 headroom.  What makes a case a case is asserted from the writer's bookkeeping, never from a decoder.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import jpeg_decode_cases as DC
from tests import jpeg_synth as S
from whenet_hip import jpeg

SEG_BYTES = (4, 8, 64, 1024)
WINDOWS = (2, 5, 256)


# ---- 1. the cases are what the table says, by the writer's bookkeeping --------------------------------------------------------------
def _sat_grey(s):
    assert s.header.intervals == 1 and s.pred.max() == 32767 and s.pred.min() == -32768
    assert not np.array_equal(np.clip(s.raw_pred, -32768, 32767), s.pred)       # a clipped prefix sum is wrong behind a bound
    assert s.body_bytes // 4 > 256                                             # more than 256 segments of 4 bytes: a scan carry
    differs, segment = s.pred != s.raw_pred, s.dc_offset // 4
    assert (differs & (segment < 256)).any() and (differs & (segment > 256)).any()
    assert len({(z, c) for z, c in zip(s.zrls, np.diff(np.append(s.dc_offset, s.body_bytes)))}) > 4      # blocks of several lengths


def _sat_420(s):
    assert s.bound == [{"lo"}, {"hi"}, set()]                                   # where the clamp changed a predictor, per component
    luma, cb, cr = (s.pred[s.comp == c] for c in range(3))
    assert luma.min() == -32768 and luma.max() < 32767 and cb.max() == 32767 and cb.min() > -32768
    assert cr.min() > -32768 and cr.max() < 32767
    assert not np.array_equal(s.pred[s.comp < 2], s.raw_pred[s.comp < 2])


def _len16_444(s):
    assert set(s.lengths[0]) == {16} and set(s.lengths[1]) == {16}
    assert s.sizes[1][15] > 0 and s.sizes[1][11] + s.sizes[1][12] + s.sizes[1][13] + s.sizes[1][14] > 0
    assert (s.header.qt, s.header.dc, s.header.ac) == ([3, 0, 2], [1, 0, 1], [0, 1, 1])
    assert np.abs(s.coef).max() >= 2047 and (s.coef == -2048).any()             # value x Q meets the clamp


def _edge910_grey(s):
    assert set(s.lengths[0]) == {9, 10} and set(s.lengths[1]) == {9, 10}


def _phantom(s):
    for cls in (0, 1):
        assert S.kraft(S.PHANTOM[(cls, 0)][0]) == 1.0                           # complete: every bit string is code words
    assert S.PHANTOM[(0, 0)][1][-1] == 0                                        # the all-ones DC code is category 0
    assert max(s.pad_bits) >= 3                                                 # so some padding is a whole phantom DC symbol


def _ri1_grey(s):
    assert s.header.intervals == 600 == len(s.pad_bits) and s.rst == [k % 8 for k in range(599)]
    assert set(s.lengths[0]) == {16} and set(s.lengths[1]) == {16} and s.closed["eob"] > 500


def _idct_extreme(s):
    assert set(np.unique(s.coef).tolist()) == {-2048, 2047}
    c = s.coef.reshape(-1, 8, 8)
    r = (np.einsum("vy,nvu->nyu", DC.DCT, c) + 128) >> 8
    b = np.abs(np.einsum("ux,nyu->nyx", DC.DCT, r)).max()                       # int64: the second pass, before the shift
    assert 9e8 <= b < 2 ** 31, b
    assert s.header.intervals == 1 and s.body_bytes >= 4096


def _zrl_close_422(s):
    assert s.closed["full"] > 0 and s.closed["zrl"] > 0 and s.closed["eob"] > 0
    alone = [b for b in range(len(s.zrls)) if s.zrls[b] == 3 and np.count_nonzero(s.coef[b, 1:]) == 1 and s.coef[b, 63] != 0]
    assert alone and (s.header.hs, s.header.vs, s.header.intervals) == (2, 1, 3)


def _tail_bytes_420(s):
    assert s.header.intervals == 5 and s.data.count(bytes([0x12, 0x34, 0x00, 0x56]) * 9) == 5


def _fill_420(s):
    assert len(s.rst) == 4 and s.data.count(b"\xff\xff\xff\xff") == 5          # three fill bytes before four RSTn and EOI


def _multi_table_segments(s):
    assert s.data.count(b"\xff\xc4") == 1 and s.data.count(b"\xff\xdb") == 1
    assert [s.data[s.data.index(b"\xff\xc0") + 10 + 3 * c] for c in range(3)] == [82, 71, 66]


CONDITIONS = {
    "sat_grey": _sat_grey, "sat_420": _sat_420, "len16_444": _len16_444, "edge910_grey": _edge910_grey, "phantom_grey": _phantom,
    "phantom_pad0": _phantom, "ri1_grey": _ri1_grey, "tail_bytes_420": _tail_bytes_420, "fill_420": _fill_420,
    "idct_extreme": _idct_extreme, "zrl_close_422": _zrl_close_422, "multi_table_segments": _multi_table_segments,
}


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_the_case_is_what_the_table_says(name):
    s = S.case(name)
    assert len(s.data) <= S.MAX_BYTES
    assert s.header.intervals > 1 or s.body_bytes <= 20 * 1024                  # the one-lane form walks a stream without DRI alone
    CONDITIONS[name](s)


# ---- 2. the numpy statement is the construction ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_numpy_statement_returns_the_writers_coefficients(name):
    s = S.case(name)
    d = DC.decode(s.data)
    assert d.status.tolist() == [DC.OK, -1]
    assert np.array_equal(d.coef, s.coef)
    hd, want = d.header, s.header
    assert (hd.h, hd.w, hd.comps, hd.hs, hd.vs, hd.qt, hd.dc, hd.ac, hd.ri, hd.intervals, hd.data_offset) == \
        (want.h, want.w, want.comps, want.hs, want.vs, want.qt, want.dc, want.ac, want.ri, want.intervals, want.data_offset)


# ---- 3. the host statement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_host_statement_returns_the_constructed_planes_and_frame(name):
    s, want = S.case(name), S.expected(name)
    i = jpeg.info(s.data)
    assert (i["h"], i["w"], i["components"], i["intervals"], i["data_offset"]) == (want.header.h, want.header.w, want.header.comps,
                                                                                  want.header.intervals, s.data_offset)
    planes, status = jpeg.decode_planes_host(s.data)
    assert status.tolist() == want.status.tolist()
    assert len(planes) == len(want.planes)
    for p, q in zip(planes, want.planes):
        assert np.array_equal(p, q)
    assert np.array_equal(jpeg.decode_host(s.data), want.frame)
    assert np.array_equal(jpeg.decode_host(s.data, bgr=False), want.frame[..., ::-1])


# ---- 4. the host emulation of the segmented form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_segmented_host_returns_the_constructed_planes_and_frame(name):
    s, want = S.case(name), S.expected(name)
    for seg_bytes in SEG_BYTES:
        for window in WINDOWS:
            got, status, stats = jpeg.decode_segmented_host(s.data, seg_bytes, window, stats=True)
            assert status.tolist() == want.status.tolist(), (seg_bytes, window)
            assert np.array_equal(got, want.frame), (seg_bytes, window)
            assert stats[0] == want.header.intervals and stats[6] == seg_bytes and stats[7] == 1
            planes, status, _ = jpeg.decode_segmented_planes_host(s.data, seg_bytes, window)
            assert status.tolist() == want.status.tolist(), (seg_bytes, window)
            for p, q in zip(planes, want.planes):
                assert np.array_equal(p, q), (seg_bytes, window)


def test_the_scan_carries_of_the_segmented_form_are_reached():
    """sat_grey at seg_bytes 4 is more than 256 segments of one interval, ri1_grey more than 512 intervals"""
    assert jpeg.decode_segmented_host(S.case("sat_grey").data, 4, stats=True)[2][1] > 256
    stats = jpeg.decode_segmented_host(S.case("ri1_grey").data, 4, stats=True)[2]
    assert stats[0] == 600 and stats[1] >= 600


# ---- 5. the sanitizer program -----------------------------------------------------------------------------------------------------------
def test_seg_host_check_program_runs_the_synthetic_streams_under_the_sanitizers(tmp_path):
    """tools/jpeg_dec_seg_host_check.cpp, built stand-alone with -fsanitize=address,undefined as tests/test_jpeg_decode_seg_cpu.py
    builds it, on the synthetic streams and their cut and flipped copies: the program is run on its own, never loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_dec_seg_host_check"
    src = os.path.join(DC.ROOT, "tools", "jpeg_dec_seg_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in S.CASE_NAMES:
        (tmp_path / f"{name}.jpg").write_bytes(S.case(name).data)
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.jpg") for n in S.CASE_NAMES], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "no report" in r.stderr
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    for name in S.CASE_NAMES:
        assert lines[f"{name}.jpg"].startswith("status 0 -1 segments"), lines[f"{name}.jpg"]
