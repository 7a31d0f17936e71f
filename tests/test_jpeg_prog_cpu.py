"""The progressive JPEG decoder's host statement (csrc/jpeg_prog_host.h behind whenet_jpeg_parse_scans,
whenet_jpeg_decode_progressive_host, ..._planes_host and whenet_jpeg_progressive_coefficients_host) against three references, with no
tolerance anywhere:
  1. the numpy / Python statement of tests/jpeg_prog_cases.py (raw coefficients, finished records, planes, frames, status, counters);
  2. the baseline TWIN of every Pillow stream -- the same picture, quality, sampling and DRI written with optimize=True holds the
     same quantised coefficients -- through the baseline decoder, which earlier tests pin;
  3. executed Pillow: rule 1 is `Image.open(...).convert("RGB")` byte for byte, on Pillow's streams and on the scan writer's, which
     Pillow must open -- that pins the writer.
Streams are made at test time (Pillow 12.2.0, the scan writer); no test needs a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import jpeg_decode_cases as DC
from tests import jpeg_exact_cases as EX
from tests import jpeg_prog_cases as PC
from whenet_hip import _lib, jpeg

ROOT = DC.ROOT
COMPLETE = PC.PILLOW_NAMES + PC.CONSTRUCTED_NAMES


def stream_of(name):
    if name in PC.PILLOW:
        return PC.pillow_case(name)
    if name in PC.DAMAGED:
        return PC.DAMAGED[name]
    return PC.constructed(name)


def blocks_of(hd):
    return hd.mcu_cols * hd.mcu_rows * hd.bpm


def host_frame(data, bgr, rule):
    return jpeg.decode_host(data, bgr=bgr, rule=rule, progressive=True, strict=False)


# The first bad item of every damaged stream, worked out by hand, not taken from either statement.  The damaged Pillow stream is
# 35 x 50 4:2:2 with 3-unit intervals: its ten scans have 7, 12, 7, 7, 12, 12, 7, 7, 7, 12 intervals (3 x 7 MCUs or chroma blocks, 5 x 7
# luma blocks), so they begin at items 0, 7, 19, 26, 33, 45, 57, 64, 71, 78.
#   a cut in the middle of scan i: the stream ends inside one of scan i's intervals; the markers behind it are missing, so the bad item
#       is the interval the cut falls in (the table's entry lies inside scan i's range, asserted below)
#   cut in front of the last two scans: all 71 items of scans 0..7 are good, the progression is incomplete: the item count, 71
#   scan 3 (items 26..32): marker 1 renumbered: item 26 + 1; marker 2 removed: the markers behind it carry the wrong numbers from
#       position 2 on: 26 + 2; a marker too many: its last interval, 26 + 6
#   the constructed grey 9 x 7 streams have 2 blocks and no DRI: one item per scan, and the damage sits in scan 1 or scan 2
SCAN_FIRST_ITEM = [0, 7, 19, 26, 33, 45, 57, 64, 71, 78, 90]
FIRST_BAD = {"truncated_in_scan_0": 3, "truncated_in_scan_1": 12, "truncated_in_scan_2": 22, "truncated_in_scan_3": 29, "truncated_in_scan_4": 38,
             "truncated_in_scan_5": 50, "truncated_in_scan_6": 60, "truncated_in_scan_7": 67, "truncated_in_scan_8": 74, "truncated_in_scan_9": 83,
             "cut_before_last_two_scans": 71, "incomplete_no_eoi": 71, "wrong_rst_scan_3": 27, "missing_rst_scan_3": 28, "extra_rst_scan_3": 32,
             "noncode": 1, "run_past_se": 1, "s2_in_refinement": 2, "eobrun_past_interval": 1, "ends_in_correction_bits": 2}


def test_the_expected_bad_items_lie_in_their_scans():
    assert set(FIRST_BAD) == set(PC.DAMAGED)
    scans = jpeg.info(PC._base10(), progressive=True)["scans"]
    assert [s["first_item"] for s in scans] + [scans[-1]["first_item"] + scans[-1]["intervals"]] == SCAN_FIRST_ITEM
    for i in range(10):
        assert SCAN_FIRST_ITEM[i] <= FIRST_BAD[f"truncated_in_scan_{i}"] < SCAN_FIRST_ITEM[i + 1]


# ---- 1. the library's host statement is the numpy statement ----------------------------------------------------------------------
@pytest.mark.parametrize("name", COMPLETE + PC.DAMAGED_NAMES)
def test_host_statement_equals_the_numpy_statement(name):
    data = stream_of(name)
    st = PC.decode(data)
    hd = st.header
    coef, raw, cnt, status = _lib.jpeg_progressive_coefficients_host(data, blocks_of(hd))
    assert status.tolist() == st.status.tolist()
    assert np.array_equal(raw, st.raw) and np.array_equal(coef, st.coef)
    assert cnt == st.counters
    planes, pstatus = jpeg.decode_planes_host(data, progressive=True)
    assert pstatus.tolist() == st.status.tolist() and len(planes) == hd.comps
    for got, want in zip(planes, st.planes):
        assert np.array_equal(got, want)
    for got, want in zip(jpeg.decode_planes_host(data, progressive=True, rule="libjpeg")[0], EX.planes(st)):
        assert np.array_equal(got, want)
    for bgr in (True, False):
        assert np.array_equal(host_frame(data, bgr, "own"), DC.frame(st, bgr))
        assert np.array_equal(host_frame(data, bgr, "libjpeg"), EX.frame(st, bgr))
    if name in PC.DAMAGED:
        assert status.tolist() == [PC.EFORMAT, FIRST_BAD[name]]
        with pytest.raises(jpeg.DecodeError) as err:
            jpeg.decode_host(data, progressive=True)
        assert err.value.interval == status[1]
    else:
        assert status.tolist() == [PC.OK, -1]


@pytest.mark.parametrize("name", [n for n in COMPLETE if "_420_" in n] + ["noisy_q100"])
def test_a_420_stream_decodes_into_i420_and_nv12_surfaces(name):
    data = PC.noisy_q100() if name == "noisy_q100" else stream_of(name)
    st = PC.decode(data)
    h, w = st.header.h, st.header.w
    ch, cw = (h + 1) // 2, (w + 1) // 2
    for fmt in ("i420", "nv12"):
        y = np.full((h, w + 5), 0xC7, np.uint8)
        s = _lib.SurfaceC()
        s.plane[0], s.pitch[0] = y.ctypes.data, w + 5
        if fmt == "i420":
            u, v = np.full((ch, cw + 3), 0xC7, np.uint8), np.full((ch, cw + 1), 0xC7, np.uint8)
            s.plane[1], s.pitch[1], s.plane[2], s.pitch[2] = u.ctypes.data, cw + 3, v.ctypes.data, cw + 1
            s.format = _lib.YUV_I420
        else:
            uv = np.full((ch, 2 * cw + 2), 0xC7, np.uint8)
            s.plane[1], s.pitch[1] = uv.ctypes.data, 2 * cw + 2
            s.format = _lib.YUV_NV12
        s.matrix, s.on_device = _lib.YUV_JFIF, 0
        assert _lib.jpeg_decode_progressive_host(data, s, True).tolist() == [PC.OK, -1]
        assert np.array_equal(y[:, :w], st.planes[0]) and (y[:, w:] == 0xC7).all()
        if fmt == "i420":
            assert np.array_equal(u[:, :cw], st.planes[1]) and np.array_equal(v[:, :cw], st.planes[2])
            assert (u[:, cw:] == 0xC7).all() and (v[:, cw:] == 0xC7).all()
        else:
            assert np.array_equal(uv[:, 0:2 * cw:2], st.planes[1]) and np.array_equal(uv[:, 1:2 * cw:2], st.planes[2])
            assert (uv[:, 2 * cw:] == 0xC7).all()


# ---- 2. the twin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.PILLOW_NAMES)
def test_a_pillow_stream_decodes_to_its_baseline_twin(name):
    data, twin = PC.pillow_case(name), PC.pillow_twin(name)
    assert jpeg.info(twin)["h"] > 0                      # the twin is a stream the baseline decoder accepts
    hd = PC.decode(data).header
    coef = _lib.jpeg_progressive_coefficients_host(data, blocks_of(hd))[0]
    assert np.array_equal(coef, DC.decode(twin).coef)    # (the baseline statement's records, which the baseline host test pins)
    for rule in ("own", "libjpeg"):
        for bgr in (True, False):
            assert np.array_equal(host_frame(data, bgr, rule), jpeg.decode_host(twin, bgr=bgr, rule=rule))


# ---- 3. executed Pillow ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", COMPLETE)
def test_rule_1_is_pillows_rgb_byte_for_byte(name):
    data = stream_of(name)
    assert PC.off_the_clamp(PC.decode(data)), "the pictures are chosen off the +-2048 clamp: rule 1's condition"
    assert np.array_equal(host_frame(data, False, "libjpeg"), EX.pillow(data))


# ---- 4. the scan plan: geometry, levels, counters --------------------------------------------------------------------------------
def test_the_scan_plan_of_pillows_script():
    """35 x 50 4:2:2 with 3-MCU intervals: 7 intervals in the DC scans (3 x 7 frame MCUs), 12 in the luma AC scans (5 x 7 blocks: the
    component's own grid, not the plane padded to whole MCUs), 7 in the chroma ones (3 x 7); three levels."""
    i = jpeg.info(PC.pillow_case("pil_422_35x50_q75_blocks3"), progressive=True)
    scans = i["scans"]
    assert (i["h"], i["w"], i["sampling"], len(scans)) == (50, 35, (2, 1), 10)
    dc = [s for s in scans if s["ss"] == 0]
    assert [s["intervals"] for s in dc] == [7, 7] and all(s["components"] == (0, 1, 2) for s in dc)
    assert all(s["intervals"] == 12 for s in scans if s["ss"] > 0 and s["components"] == (0,))
    assert all(s["intervals"] == 7 for s in scans if s["ss"] > 0 and s["components"] != (0,))
    assert [s["level"] for s in scans] == [1, 1, 1, 1, 1, 2, 2, 2, 2, 3]
    assert [s["first_item"] for s in scans] == list(np.cumsum([0] + [s["intervals"] for s in scans[:-1]]))
    assert all(s["ri"] == 3 for s in scans)
    # 17 x 17 4:2:0: 3 x 3 luma blocks against 4 x 4 padded
    i = jpeg.info(PC.pillow_case("pil_420_17x17_q75_rows1"), progressive=True)
    # (libjpeg writes a DRI per scan for "one row": 2 MCUs in the DC scans, 3 blocks in the luma AC scans, whose rows are 3 blocks)
    assert {(s["ri"], s["intervals"]) for s in i["scans"] if s["ss"] > 0 and s["components"] == (0,)} == {(3, 3)}
    assert {(s["ri"], s["intervals"]) for s in i["scans"] if s["ss"] == 0} == {(2, 2)}


def test_a_baseline_stream_is_one_scan_and_the_existing_result():
    data = PC.pillow_twin("pil_420_17x17_q75_blocks3")
    i = jpeg.info(data, progressive=True)
    base = jpeg.info(data)
    assert len(i["scans"]) == 1 and i["intervals"] == base["intervals"] and i["data_offset"] == base["data_offset"]
    s = i["scans"][0]
    assert (s["ss"], s["se"], s["ah"], s["al"], s["level"], s["intervals"]) == (0, 63, 0, 0, 1, base["intervals"])
    for rule in ("own", "libjpeg"):
        assert np.array_equal(jpeg.decode_host(data, rule=rule, progressive=True), jpeg.decode_host(data, rule=rule))
    for a, b in zip(jpeg.decode_planes_host(data, progressive=True)[0], jpeg.decode_planes_host(data)[0]):
        assert np.array_equal(a, b)


def test_levels_of_the_constructed_scripts():
    levels = lambda name: max(s["level"] for s in jpeg.info(PC.constructed(name), progressive=True)["scans"])      # noqa: E731
    assert levels("minimal_420_17x17_fixed") == 1 and levels("approx3_420_17x17_fixed") == 4 and levels("bands_grey_9x7_ranked") == 1
    # the deepest script the rules allow: every step of a chain of overlapping scans lowers Al, from 13 to 0
    assert levels("levels14_420_17x17_fixed") == 14 and levels("levels14_grey_9x7_ranked") == 14
    i = jpeg.info(PC.constructed("dri_changes_420_17x17_fixed"), progressive=True)
    assert [s["ri"] for s in i["scans"]] == [2, 1, 2, 3, 3, 4, 4]      # luma: 9 blocks; chroma: 4 (Ri 0 or >= the units: one interval)
    assert [s["intervals"] for s in i["scans"]] == [2, 9, 2, 2, 3, 1, 1]
    i = jpeg.info(PC.constructed("ids23_420_17x17_ranked"), progressive=True)
    assert i["scans"][0]["dc_ids"] == (2, 3, 3) and [s["ac_ids"] for s in i["scans"][1:]] == [(2,), (3,), (3,)]


def test_long_eob_runs_and_refinement_counters():
    """1024 x 1024 of one level: 16,384 blocks, every AC scan one EOB run over all of them (EOBRUN as libjpeg counts it: the block
    in hand included).  A noisy picture at quality 100 meets ZRLs in refinement scans and correction bits that change a value."""
    data = PC.flat_grey_1024()
    coef, raw, cnt, status = _lib.jpeg_progressive_coefficients_host(data, 16384)
    assert status.tolist() == [PC.OK, -1] and cnt["max_eobrun"] >= 16384 and cnt["levels"] == 3
    assert not coef[:, 1:].any() and len(set(coef[:, 0].tolist())) == 1
    assert np.array_equal(host_frame(data, False, "libjpeg"), EX.pillow(data))
    data = PC.noisy_q100()
    st = PC.decode(data)
    coef, raw, cnt, status = _lib.jpeg_progressive_coefficients_host(data, blocks_of(st.header))
    assert cnt == st.counters and cnt["refine_zrl"] > 0 and cnt["corrections"] > 0 and cnt["correction_bits"] > cnt["corrections"]
    assert np.array_equal(raw, st.raw) and PC.off_the_clamp(st)
    assert np.array_equal(host_frame(data, False, "libjpeg"), EX.pillow(data))
    assert np.array_equal(host_frame(data, False, "libjpeg"), jpeg.decode_host(PC.noisy_q100(False), bgr=False, rule="libjpeg"))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
REASONS = {
    "ss_above_se": "Ss > Se", "se_above_63": "Se > 63", "dc_with_ac": "Ss = 0 with Se != 0", "interleaved_ac": "Ss > 0 with several",
    "al_above_13": "above 13", "ah_above_13": "above 13", "second_first_scan": "already had one", "refine_without_first": "no first scan",
    "refine_wrong_ah": "Ah is not", "refine_al_not_ah_minus_1": "Al is not Ah - 1", "ac_before_dc": "DC coefficient has had no scan",
    "missing_table": "missing Huffman table", "dqt_behind_sos": "DQT", "scans_129": "more than 128 scans", "ns_2": "two components",
}


@pytest.mark.parametrize("name", list(PC.REFUSED))
def test_script_violations_are_refused_with_the_reason_and_nothing_is_written(name):
    data = PC.REFUSED[name]
    with pytest.raises(PC.Refused):
        PC.parse(data)
    with pytest.raises(ValueError, match=REASONS[name]):
        jpeg.info(data, progressive=True)
    frame = np.full((17, 17, 3), 0xC7, np.uint8)
    with pytest.raises(ValueError, match=REASONS[name]):
        _lib.jpeg_decode_progressive_host(data, jpeg.packed_surface(frame), True)
    assert (frame == 0xC7).all()


def test_a_header_that_claims_a_million_intervals_costs_what_its_bytes_hold():
    """A few hundred bytes that say 8192 x 8192 with DRI 1: every one of 128 scans claims 2^20 intervals.  The plan lists an item
    where the data holds its start, so the parse neither takes long nor holds gigabytes -- whatever it ends in."""
    import resource
    import time

    def inflate(data):
        d = bytearray(data)
        p = d.find(b"\xff\xc2")
        d[p + 5:p + 9] = bytes([0x20, 0, 0x20, 0])                    # h = w = 8192
        p = d.find(b"\xff\xda")
        return bytes(d[:p]) + bytes([0xFF, 0xDD, 0, 4, 0, 1]) + bytes(d[p:])      # DRI 1 in front of the first scan

    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    t = time.perf_counter()
    with pytest.raises(ValueError, match="more than 128 scans"):
        jpeg.info(inflate(PC.REFUSED["scans_129"]), progressive=True)
    i = jpeg.info(inflate(PC.constructed("minimal_grey_9x7_fixed")), progressive=True)
    assert [(s["ri"], s["intervals"], s["first_item"]) for s in i["scans"]] == [(1, 1 << 20, 0), (1, 1 << 20, 1 << 20)]
    assert time.perf_counter() - t < 2.0
    assert resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before < 256 * 1024      # KiB: the old lists alone were 4 GB


def test_the_defaults_still_refuse_progressive_streams():
    data = PC.pillow_case("pil_420_17x17_q75_nodri")
    for call in (jpeg.info, jpeg.decode_host, jpeg.decode_planes_host, lambda d: jpeg.decode_host(d, rule="libjpeg")):
        with pytest.raises(ValueError, match="progressive"):
            call(data)


def test_bad_arguments_are_einval():
    data = PC.pillow_case("pil_420_17x17_q75_nodri")
    with pytest.raises(ValueError, match="progressive=True"):      # (not rule 0's planes in silence)
        jpeg.decode_planes_host(PC.pillow_twin("pil_420_17x17_q75_nodri"), rule="libjpeg")
    with pytest.raises(ValueError, match="blocks"):
        _lib.jpeg_progressive_coefficients_host(data, 23)                      # 2 x 2 MCUs of 6 blocks
    with pytest.raises(ValueError, match="baseline"):
        _lib.jpeg_progressive_coefficients_host(PC.pillow_twin("pil_420_17x17_q75_nodri"), 24)
    lib = _lib.load()
    import ctypes as C
    info, n = _lib.JpegInfoC(), C.c_int(0)
    a = np.frombuffer(data, np.uint8)
    scans = (_lib.JpegScanC * 4)()
    assert lib.whenet_jpeg_parse_scans(a.ctypes.data, a.size, C.byref(info), scans, 4, C.byref(n)) == _lib.EINVAL and n.value == 10
    grey = np.empty((17, 17, 3), np.uint8)
    s = jpeg.packed_surface(grey)
    s.format, s.matrix = _lib.YUV_I420, _lib.YUV_JFIF
    with pytest.raises(ValueError, match="rule 1"):
        _lib.jpeg_decode_progressive_host(data, s, True, "libjpeg")


# ---- 6. the sanitizer check and the symbols --------------------------------------------------------------------------------------
def test_host_check_program_runs_the_table_under_the_sanitizers(tmp_path):
    """tools/jpeg_prog_host_check.cpp: csrc/jpeg_prog_host.h -- the scan decode the kernels share -- built stand-alone with
    -fsanitize=address,undefined and run on every stream of the table (Pillow's, the constructed, the damaged and the refused
    ones, the two large ones), and on cut and bit-flipped copies of each."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_prog_host_check"
    src = os.path.join(ROOT, "tools", "jpeg_prog_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    streams = {n: stream_of(n) for n in PC.PILLOW_NAMES + PC.CONSTRUCTED_NAMES + PC.DAMAGED_NAMES}
    streams.update(PC.REFUSED)
    streams["flat_grey_1024"], streams["noisy_q100"] = PC.flat_grey_1024(), PC.noisy_q100()
    for name, data in streams.items():
        (tmp_path / f"{name}.jpg").write_bytes(data)
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.jpg") for n in streams], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    import zlib
    for name, data in streams.items():
        if name in PC.REFUSED:
            assert lines[f"{name}.jpg"].startswith("refused"), lines[f"{name}.jpg"]
            continue
        frame = np.empty(host_frame(data, True, "own").shape, np.uint8)
        status = _lib.jpeg_decode_progressive_host(data, jpeg.packed_surface(frame), True)
        want = f"status {status[0]} {status[1]} crc {zlib.crc32(host_frame(data, True, 'own').tobytes()):08x} " \
               f"{zlib.crc32(host_frame(data, True, 'libjpeg').tobytes()):08x}"
        # (behind it: the checksum of the scan plan, which tests/test_jpeg_parse_pins_cpu.py compares)
        frame_part, plan = lines[f"{name}.jpg"].rsplit(" plan ", 1)
        assert frame_part == want and len(plan) == 16, name


def test_new_symbols_are_exported_and_bound():
    lib = _lib.load()
    for s in ("whenet_jpeg_parse_scans", "whenet_jpeg_decode_progressive_host", "whenet_jpeg_decode_progressive_planes_host",
              "whenet_jpeg_progressive_coefficients_host", "whenet_op_jpeg_decode_progressive", "whenet_frame_begin_jpeg_progressive",
              "whenet_jpeg_progressive_counters"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    import ctypes
    assert ctypes.sizeof(_lib.JpegScanC) == 4 * 20 + 16 and _lib.ABI_VERSION == 6
    info, scans = _lib.jpeg_parse_scans(PC.pillow_case("pil_420_17x17_q75_nodri"))
    assert all(s.progressive == 1 for s in scans)
    assert [s.progressive for s in _lib.jpeg_parse_scans(PC.pillow_twin("pil_420_17x17_q75_nodri"))[1]] == [0]
