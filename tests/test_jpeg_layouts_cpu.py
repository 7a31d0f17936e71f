"""The JPEG decoder's LAYOUTS section (include/whenet_hip.h, JPEG DECODER, LAYOUTS), the parts that need no GPU: the host statement
behind the ..._accept calls against the independent numpy statement of tests/jpeg_layout_cases.py, byte for byte, planes and frame,
both rules; rule 1 against executed Pillow on EVERY stream (none skipped: every stream is built off the +-2048 clamp, which is
asserted); the segmented form's host emulation; what is refused without the argument (with today's texts, nothing written) and with
it; damaged streams; the routing; the stand-alone checker under the host sanitizers; the entry points.

The kernels are held to this host statement in tests/test_jpeg_layouts_gpu.py."""
import ctypes
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import jpeg_layout_cases as LC
from whenet_hip import _lib, jpeg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RULES = ((0, "own"), (1, "libjpeg"))
LAYOUTS, PROGRESSIVE = _lib.JPEG_ACCEPT_LAYOUTS, _lib.JPEG_ACCEPT_PROGRESSIVE
BOTH = LAYOUTS | PROGRESSIVE
GAP = 0xC3

# every stream the section accepts: name -> (bytes, the sequential stream whose numpy statement is this stream's, needs SOF2?)
def _accepted():
    t = {}
    for n in LC.SINGLE_NAMES:
        t[n] = (LC.single(n), LC.single(n), False)
    for n in LC.SOF1_NAMES:
        t[n] = (LC.sof1(n), LC.sof1(n), False)
    for n in LC.MULTI_NAMES:
        t[n] = (LC.multi(n), LC.multi(n), False)
    for n in LC.SOF2_NAMES:
        t[n] = (LC.sof2(n), LC.sof2_twin(n), True)
    for s, first in (("411", (0, 1)), ("440", (1, 2)), ("410", (0, 2)), ("420", (0, 1))):
        b, hs, vs = LC._blocks(s, 17, 33)
        t[f"{s}_33x17_sof2_ns2_{first[0]}{first[1]}"] = (LC.sof2_ns2(s, 17, 33, first), LC.write(b, 17, 33, hs, vs), True)
    return t


ACCEPTED = _accepted()
ACCEPTED_NAMES = list(ACCEPTED)
# the streams the argument alone admits (the old samplings' single-scan SOF0 twins are not among them)
NEW_NAMES = [n for n in ACCEPTED_NAMES if not n.startswith("42") or "sof1" in n or n in LC.MULTI or "ns2" in n]


def host_planes(data, rule, accept=BOTH):
    i = _lib.jpeg_parse_scans_accept(data, accept)[0]
    shapes = [(i.h, i.w)] + [(-(-i.h // i.vs), -(-i.w // i.hs))] * (i.components - 1)
    planes = [np.full(s, GAP, np.uint8) for s in shapes]
    return planes, _lib.jpeg_decode_accept_planes_host(data, planes, rule, accept)


def host_frame(data, rule, bgr=True, accept=BOTH):
    i = _lib.jpeg_parse_scans_accept(data, accept)[0]
    frame = np.full((i.h, i.w, 3), GAP, np.uint8)
    status, _ = _lib.jpeg_decode_accept_host(data, jpeg.packed_surface(frame), bgr, rule, accept, False)
    return frame, status


# ---- 1. the host statement against numpy, and rule 1 against executed Pillow -------------------------------------------------------
@pytest.mark.parametrize("name", ACCEPTED_NAMES)
def test_host_statement_equals_the_numpy_statement_and_rule_1_equals_pillow(name):
    data, twin, sof2 = ACCEPTED[name]
    dec = LC.decode(twin)
    assert LC.off_the_clamp(dec), "the case table holds no stream on the +-2048 clamp"      # rule 1's SCOPE condition: asserted, not skipped
    assert dec.status.tolist() == [LC.OK, -1]
    accept = BOTH if sof2 else LAYOUTS
    for rule, rname in RULES:
        planes, status = host_planes(data, rname, accept)
        want = LC.planes(dec, rule)
        assert status.tolist() == [LC.OK, -1]
        assert len(planes) == len(want) and all(np.array_equal(p, w) for p, w in zip(planes, want)), (name, rule)
        for bgr in (True, False):
            frame, status = host_frame(data, rname, bgr, accept)
            assert status.tolist() == [LC.OK, -1] and np.array_equal(frame, LC.frame(dec, rule, bgr)), (name, rule, bgr)
        assert np.array_equal(jpeg.decode_host(data, rule=rname, progressive=sof2, layouts=True), LC.frame(dec, rule))
    # the executed library: the RGB frame and its own planes (chroma as it upsamples them)
    assert np.array_equal(LC.pillow_rgb(data), LC.frame(dec, 1, bgr=False)), name
    if dec.header.comps == 3:
        ycc, up = LC.pillow_ycc(data), LC.upsampled(dec, 1)
        assert np.array_equal(ycc[..., 0], LC.planes(dec, 1)[0]) and np.array_equal(ycc[..., 1], up[0]) and np.array_equal(ycc[..., 2], up[1]), name
    else:
        assert np.array_equal(LC.pillow_ycc(data, "L"), LC.planes(dec, 1)[0]), name


def test_rule_1_of_440_filters_a_two_pixel_wide_picture_and_411_410_replicate():
    """the lines of the header's RULE 1 paragraph on the shapes that tell them apart: 17 x 2 at 4:4:0 is filtered vertically (no
    narrow-width switch), 4:1:1 / 4:1:0 take in[y >> log2 vs][x >> 2]"""
    dec = LC.decode(LC.single("440_2x17"))
    cb = LC.planes(dec, 1)[1].astype(np.int64)
    up = LC.upsampled(dec, 1)[0]
    assert cb.shape == (9, 2) and not np.array_equal(up, cb[np.arange(17) >> 1])      # replication would be another picture
    assert np.array_equal(up[2], (3 * cb[1] + cb[0] + 1) >> 2) and np.array_equal(up[3], (3 * cb[1] + cb[2] + 2) >> 2)
    assert np.array_equal(up[0], cb[0]) and np.array_equal(up[16], (3 * cb[8] + cb[7] + 1) >> 2)
    assert np.array_equal(LC.pillow_ycc(LC.single("440_2x17"))[..., 1], up)
    for s, vs in (("411", 1), ("410", 2)):
        dec = LC.decode(LC.single(f"{s}_65x33"))
        cb = LC.planes(dec, 1)[1]
        assert np.array_equal(LC.pillow_ycc(LC.single(f"{s}_65x33"))[..., 1], cb[np.arange(33) >> (vs - 1)][:, np.arange(65) >> 2])


# ---- 2. the segmented form's host emulation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.SINGLE_NAMES + LC.SOF1_NAMES + LC.DAMAGED_NAMES)
def test_segmented_emulation_gives_the_same_bytes(name):
    data = LC.DAMAGED[name] if name in LC.DAMAGED else ACCEPTED[name][0]
    for rule, rname in RULES:
        want, want_status = host_frame(data, rname, True, LAYOUTS)
        want_planes, _ = host_planes(data, rname, LAYOUTS)
        for seg_bytes in (4, 16, 128):
            for window in (1, 3, 256):
                frame, status, stats = jpeg.decode_segmented_host(data, seg_bytes, window, stats=True, rule=rname, layouts=True)
                assert np.array_equal(frame, want) and status.tolist() == want_status.tolist(), (name, rule, seg_bytes, window)
        planes = [np.full_like(p, GAP) for p in want_planes]
        status, _ = _lib.jpeg_decode_segmented_accept_planes_host(data, planes, 16, 3, rname, LAYOUTS)
        assert all(np.array_equal(p, w) for p, w in zip(planes, want_planes)) and status.tolist() == want_status.tolist()
        if rule == 0:
            planes, status, _ = jpeg.decode_segmented_planes_host(data, 16, 3, layouts=True)
            assert all(np.array_equal(p, w) for p, w in zip(planes, want_planes)) and status.tolist() == want_status.tolist()
    with pytest.raises(ValueError, match="luma sampling must be|SOF1"):
        jpeg.decode_segmented_host(data, 16, 3)


# ---- 3. without the bit ------------------------------------------------------------------------------------------------------------
TODAY = {"single": "luma sampling must be 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4)",
         "sof1": "extended sequential DCT (SOF1): baseline sequential streams only",
         "scans": "several scans (a scan that does not hold every component): one interleaved scan only",
         "ids": "a Huffman table class or id above 1 (baseline: ids 0..1)",
         "ns2": "a scan of two components: scans hold one component or all of them"}


def todays_reason(name, data):
    """what the parsers say about the stream today: the first thing they meet"""
    sof = next(data[p + 1] for p in range(2, len(data) - 1) if data[p] == 0xFF and data[p + 1] in (0xC0, 0xC1, 0xC2))
    if sof == 0xC1:
        return TODAY["sof1"]
    i = _lib.jpeg_parse_scans_accept(data, BOTH)[0]
    if (i.hs, i.vs) in LC.SAMPLINGS.values():
        return TODAY["single"]
    if "ns2" in name:
        return TODAY["ns2"]
    return TODAY["ids"] if "ids" in name else TODAY["scans"]


@pytest.mark.parametrize("name", NEW_NAMES)
def test_without_the_bit_every_call_refuses_with_todays_text_and_writes_nothing(name):
    data, _, sof2 = ACCEPTED[name]
    why = todays_reason(name, data)
    i = _lib.jpeg_parse_scans_accept(data, BOTH)[0]
    frame = np.full((i.h, i.w, 3), GAP, np.uint8)
    surface = jpeg.packed_surface(frame)
    planes = [np.full((i.h, i.w), GAP, np.uint8) for _ in range(i.components)]
    lib = _lib.load()
    a = _lib._stream_array(data)
    status = np.full(2, 77, np.int32)
    calls = {
        "jpeg_parse": lambda: _lib.jpeg_parse(data),
        "jpeg_parse_scans": lambda: _lib.jpeg_parse_scans(data),
        "jpeg_decode_host": lambda: _lib.jpeg_decode_host(data, surface, True),
        "jpeg_decode_rule_host": lambda: _lib.jpeg_decode_rule_host(data, surface, True, "libjpeg"),
        "jpeg_decode_planes_host": lambda: _lib.jpeg_decode_planes_host(data, planes),
        "jpeg_decode_progressive_host": lambda: _lib.jpeg_decode_progressive_host(data, surface, True),
        "jpeg_decode_progressive_planes_host": lambda: _lib.jpeg_decode_progressive_planes_host(data, planes),
        "jpeg_decode_oriented_host": lambda: _lib.jpeg_decode_oriented_host(data, surface, True, "own", True),
        "jpeg_decode_segmented_host": lambda: _lib.jpeg_decode_segmented_host(data, surface, True, 16, 3),
        "jpeg_clip_plan_progressive": lambda: _lib.jpeg_clip_plan_progressive([data]),
        "jpeg_parse_scans_accept": lambda: _lib.jpeg_parse_scans_accept(data, PROGRESSIVE),
        "jpeg_decode_accept_host": lambda: _lib.jpeg_decode_accept_host(data, surface, True, "own", PROGRESSIVE),
        "jpeg_decode_accept_planes_host": lambda: _lib.jpeg_decode_accept_planes_host(data, planes, "own", PROGRESSIVE),
        "jpeg_decode_segmented_accept_host": lambda: _lib.jpeg_decode_segmented_accept_host(data, surface, True, 16, 3, "own", 0),
        "jpeg_clip_plan_accept": lambda: _lib.jpeg_clip_plan_accept([data], accept=PROGRESSIVE),
    }
    for who, call in calls.items():
        with pytest.raises(ValueError) as err:
            call()
        text = str(err.value)
        # a SOF2 stream through a call that does not take SOF2 is refused for that first, as it is today
        takes_sof2 = "progressive" in who or "scans" in who or "oriented" in who or who.endswith(("accept_host", "accept_planes_host", "plan_accept"))
        want = why if (not sof2 or (takes_sof2 and "segmented" not in who)) else "progressive DCT (SOF2): baseline sequential streams only"
        assert text.endswith(want), (name, who, text)
        assert (frame == GAP).all() and all((p == GAP).all() for p in planes), (name, who)
    for accept in (0, PROGRESSIVE):      # the status words of a refused call stay what they were
        rc = lib.whenet_jpeg_decode_accept_host(_lib._ptr(a), int(a.size), ctypes.byref(surface), _lib.BGR, 0, accept, 0, _lib._ptr(status), None)
        assert rc == _lib.EFORMAT and status.tolist() == [77, 77] and (frame == GAP).all()
    # (jpeg.py with its defaults)
    for call in (lambda: jpeg.decode_host(data, progressive=sof2), lambda: jpeg.info(data, progressive=sof2),
                 lambda: jpeg.decode_planes_host(data, progressive=sof2)):
        with pytest.raises(ValueError, match=why.split("(")[0].strip()[:30]):
            call()


def test_an_old_stream_is_the_same_bytes_with_and_without_the_bit():
    for s in ("420", "422", "444", "grey"):
        data = LC.plain(s, 17, 33)
        for _, rname in RULES:
            want = jpeg.decode_host(data, rule=rname)
            assert np.array_equal(jpeg.decode_host(data, rule=rname, layouts=True), want)
            assert np.array_equal(jpeg.decode_host(data, rule=rname, layouts=True, progressive=True), want)
        a, b = jpeg.info(data), jpeg.info(data, layouts=True)
        assert all(np.array_equal(a[k], b[k]) for k in a) and len(b["scans"]) == 1


# ---- 4. refused with the bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LC.REFUSED))
def test_refused_with_the_bit_with_its_reason_before_anything_is_written(name):
    data, why = LC.REFUSED[name]
    frame = np.full((17, 33, 3), GAP, np.uint8)
    planes = [np.full((17, 33), GAP, np.uint8) for _ in range(3)]
    for accept in (LAYOUTS, BOTH):
        for call in (lambda: _lib.jpeg_parse_scans_accept(data, accept),
                     lambda: _lib.jpeg_decode_accept_host(data, jpeg.packed_surface(frame), True, "own", accept),
                     lambda: _lib.jpeg_decode_accept_planes_host(data, planes, "libjpeg", accept),
                     lambda: _lib.jpeg_clip_plan_accept([LC.single("411_33x17"), data], accept=accept)):
            with pytest.raises(ValueError) as err:
                call()
            assert why in str(err.value), (name, str(err.value))
            assert (frame == GAP).all() and all((p == GAP).all() for p in planes)
    with pytest.raises(ValueError, match="frame 1: "):
        _lib.jpeg_clip_plan_accept([LC.single("411_33x17"), data], accept=BOTH)
    for kw in ({}, {"progressive": True}):
        with pytest.raises(ValueError):
            jpeg.decode_host(data, layouts=True, **kw)


def test_the_accept_argument_is_checked():
    data = LC.single("411_33x17")
    frame = np.empty((17, 33, 3), np.uint8)
    for bad in (-1, 4, 8):
        with pytest.raises(ValueError, match="accept must be a set of WHENET_JPEG_ACCEPT"):
            _lib.jpeg_parse_scans_accept(data, bad)
        with pytest.raises(ValueError, match="accept must be a set of WHENET_JPEG_ACCEPT"):
            _lib.jpeg_decode_accept_host(data, jpeg.packed_surface(frame), True, "own", bad)
    with pytest.raises(ValueError, match="accept must be 0 or WHENET_JPEG_ACCEPT_LAYOUTS"):
        _lib.jpeg_decode_segmented_accept_host(data, jpeg.packed_surface(frame), True, 16, 3, "own", BOTH)
    # I420 / NV12 destinations stay 4:2:0-only
    y, u, v = np.empty((17, 33), np.uint8), np.empty((9, 9), np.uint8), np.empty((9, 9), np.uint8)
    s = _lib.SurfaceC()
    for k, p in enumerate((y, u, v)):
        s.plane[k], s.pitch[k] = p.ctypes.data, p.strides[0]
    s.format, s.matrix, s.on_device = _lib.YUV_I420, _lib.YUV_JFIF, 0
    with pytest.raises(ValueError, match="only a 4:2:0 stream decodes into an I420 or NV12 surface"):
        _lib.jpeg_decode_accept_host(data, s, True, "own", LAYOUTS)


# ---- 5. damaged streams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.DAMAGED_NAMES + LC.MULTI_DAMAGED_NAMES)
def test_a_damaged_stream_has_the_statements_status_and_fully_defined_frame(name):
    data = LC.DAMAGED[name] if name in LC.DAMAGED else LC.MULTI_DAMAGED[name]
    dec = LC.decode(data)
    assert dec.status[0] == LC.EFORMAT
    for rule, rname in RULES:
        planes, status = host_planes(data, rname, LAYOUTS)
        assert status.tolist() == dec.status.tolist(), (name, rule)
        assert all(np.array_equal(p, w) for p, w in zip(planes, LC.planes(dec, rule))), (name, rule)
        frame, status = host_frame(data, rname, True, LAYOUTS)
        assert status.tolist() == dec.status.tolist() and np.array_equal(frame, LC.frame(dec, rule)), (name, rule)
    with pytest.raises(jpeg.DecodeError) as err:
        jpeg.decode_host(data, layouts=True)
    assert err.value.interval == dec.status[1]


def test_the_status_pairs_of_the_multi_scan_damage():
    """ITEMS are numbered scan by scan, one per restart interval; a missing component is the item count"""
    scans = jpeg.info(LC.multi("missing_last_scan"), layouts=True)["scans"]
    assert [(s["components"], s["first_item"], s["intervals"]) for s in scans] == [((0,), 0, 8), ((1,), 8, 5)]      # 15 luma blocks at Ri 2, 5 chroma
    st = {n: LC.decode(LC.multi(n)).status.tolist() for n in LC.MULTI_DAMAGED_NAMES}
    cut = st.pop("truncated_in_scan_2")
    assert cut[0] == LC.EFORMAT and 8 <= cut[1] < 13      # an item of scan 2: the cut lies in the middle of its bytes
    assert st == {"missing_last_scan": [LC.EFORMAT, 13], "noncode_in_scan_1": [LC.EFORMAT, 0], "run_past_63_in_scan_3": [LC.EFORMAT, 2],
                  "wrong_rst_in_scan_1": [LC.EFORMAT, 1]}, st
    # the planes of the missing component come from zero coefficients: grey
    planes, _ = host_planes(LC.multi("missing_last_scan"), "own", LAYOUTS)
    assert (planes[2] == 128).all() and planes[1].std() > 0


# ---- 6. routing --------------------------------------------------------------------------------------------------------------------
def test_single_scan_ids_up_to_1_is_the_baseline_decoder_and_the_rest_is_one_level_of_the_scan_plan():
    for name in LC.SINGLE_NAMES + LC.SOF1_NAMES:
        data = ACCEPTED[name][0]
        i = jpeg.info(data, layouts=True)
        assert len(i["scans"]) == 1 and i["scans"][0]["level"] == 1 and i["sampling"] in (tuple(LC.SAMPLINGS.values()) + ((2, 2), (1, 1)))
        for entropy, form in ((0, 0), (1, 1)):
            plan = _lib.jpeg_clip_plan_accept([data], entropy, 16, LAYOUTS)
            fr = plan["frames"][0]
            assert fr["form"] == form and plan["progressive"] == 0 and plan["scan_launches"] == 0 and fr["nscans"] == 0, name
            assert fr["coef"][1] == LC.decode(data).coef.shape[0] * 128      # the records: MCUs x bpm x 128 bytes, from the stream's own count
    for name in LC.MULTI_NAMES:
        data = LC.multi(name)
        i = jpeg.info(data, layouts=True)
        want = LC.parse(data)[1]
        assert [s["components"] for s in i["scans"]] == [tuple(s["comps"]) for s in want], name
        assert [(s["ri"], s["intervals"], s["level"]) for s in i["scans"]] == [(s["ri"], s["intervals"], 1) for s in want], name
        plan = _lib.jpeg_clip_plan_accept([data, LC.single("411_33x17")], 2, 128, LAYOUTS)
        fr = plan["frames"][0]
        assert fr["form"] == _lib.JPEG_CLIP_FORM_PROGRESSIVE and fr["levels"] == 1 and fr["nscans"] == len(want), name
        assert plan["progressive"] == 1 and plan["scan_launches"] == 1      # ONE launch of the scan kernel, however many scans
        assert fr["huff"][1] == 6 * (2 * 512 + 4 * 17 + 4 * 17 + 256) * len(want)      # six tables per sequential scan
    # a clip of SOF2 and multi-scan frames: the SOF2 frames' levels and one launch for the sequential ones
    sof2 = LC.sof2("440_33x17_minimal")
    levels = max(s["level"] for s in jpeg.info(sof2, progressive=True, layouts=True)["scans"])
    plan = _lib.jpeg_clip_plan_accept([sof2, LC.multi("411_33x17_y_cb_cr"), LC.multi("422_33x17_cb_cr_y")], accept=BOTH)
    assert plan["progressive"] == 3 and plan["scan_launches"] == levels + 1


def test_the_reader_passes_the_argument_on(tmp_path):
    from whenet_hip.mjpeg import MJPGReader, MJPGWriter
    frames = [LC.single("411_65x33"), LC.strip_dht(LC.annexk_411())]
    path = str(tmp_path / "dv.avi")
    with MJPGWriter(path, 25, (65, 33)) as out:
        for f in frames:
            out.write(f)
    with MJPGReader(path, default_tables=True, layouts=True) as r:
        assert r.layouts and len(r) == 2 and r.info(0)["sampling"] == (4, 1) and r.info(1)["sampling"] == (4, 1)
        assert np.array_equal(jpeg.decode_host(r[1], layouts=r.layouts), jpeg.decode_host(LC.annexk_411(), layouts=True))
    with MJPGReader(path) as r:
        assert not r.layouts
        with pytest.raises(ValueError, match="luma sampling must be"):
            r.info(0)
    assert np.array_equal(jpeg.decode_host(frames[1], layouts=True, default_tables=True), jpeg.decode_host(LC.annexk_411(), layouts=True))
    with pytest.raises(ValueError, match="missing Huffman table"):
        jpeg.decode_host(frames[1], layouts=True)


# ---- 7. the stand-alone checker and the symbols ------------------------------------------------------------------------------------
def test_host_check_program_runs_under_the_sanitizers(tmp_path):
    """tools/jpeg_layouts_host_check.cpp: the shared headers built stand-alone with -fsanitize=address,undefined and run on every
    stream of the table, the damaged and the refused ones included, their truncations and bit flips"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_layouts_host_check"
    src = os.path.join(ROOT, "tools", "jpeg_layouts_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    streams = {n: ACCEPTED[n][0] for n in ACCEPTED_NAMES if "33x17" in n or n in LC.SINGLE_NAMES}
    streams.update(LC.DAMAGED)
    streams.update(LC.MULTI_DAMAGED)
    streams.update({n: d for n, (d, _) in LC.REFUSED.items()})
    for n, d in streams.items():
        (tmp_path / f"{n}.jpg").write_bytes(d)
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.jpg") for n in streams], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == ""
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert len(lines) == len(streams)
    for n, (d, why) in LC.REFUSED.items():
        assert lines[f"{n}.jpg"].startswith("refused") and why in lines[f"{n}.jpg"], lines[f"{n}.jpg"]
    for n in LC.SINGLE_NAMES:
        words = lines[f"{n}.jpg"].split()
        frame, status = host_frame(streams[n], "own", True, LAYOUTS)
        frame1, _ = host_frame(streams[n], "libjpeg", True, LAYOUTS)
        assert words[0] == "baseline" and words[words.index("seg") + 1] == "same", lines[f"{n}.jpg"]
        assert words[words.index("crc") + 1:words.index("crc") + 3] == [f"{zlib.crc32(frame.tobytes()):08x}", f"{zlib.crc32(frame1.tobytes()):08x}"]
        assert "without: luma sampling must be" in lines[f"{n}.jpg"]
    for n in list(LC.MULTI_DAMAGED) + [m for m in LC.MULTI_NAMES if "33x17" in m]:
        words = lines[f"{n}.jpg"].split()
        _, status = host_frame(streams[n], "own", True, LAYOUTS)
        assert words[0] == "sequential" and words[words.index("levels") + 1] == "1", lines[f"{n}.jpg"]
        assert [int(v) for v in words[words.index("status") + 1:words.index("status") + 3]] == status.tolist()


def test_new_symbols_are_exported_and_bound_and_the_structs_keep_their_layout():
    lib = _lib.load()
    names = ("whenet_jpeg_parse_scans_accept", "whenet_jpeg_decode_accept_host", "whenet_jpeg_decode_accept_planes_host",
             "whenet_jpeg_decode_segmented_accept_host", "whenet_jpeg_decode_segmented_accept_planes_host", "whenet_op_jpeg_decode_accept",
             "whenet_op_jpeg_decode_clip_accept", "whenet_frame_begin_jpeg_accept", "whenet_clip_begin_jpeg_accept", "whenet_jpeg_clip_plan_accept")
    assert set(names) == set(_lib.EXPORTS_ACCEPT) and not set(names) & set(_lib.EXPORTS)
    for s in names:
        assert hasattr(lib, s)
    assert _lib.ABI_VERSION == 6 and ctypes.sizeof(_lib.JpegScanC) == 4 * 20 + 16
    assert ctypes.sizeof(_lib.JpegInfoC) == 72 + 256 + 4 + 64 + 1024 + 4
    # declared in the companion header, which includes the main one; the main header documents them and declares what it declared
    header = open(os.path.join(ROOT, "include", "whenet_hip_jpeg_accept.h")).read()
    main = open(os.path.join(ROOT, "include", "whenet_hip.h")).read()
    assert '#include "whenet_hip.h"' in header and "JPEG DECODER, LAYOUTS" in main
    for s in names:
        assert f"WHENET_API int {s}(" in header and header.count(s + "(") == 1 and f"WHENET_API int {s}(" not in main
    assert "#define WHENET_JPEG_ACCEPT_PROGRESSIVE 1" in header and "#define WHENET_JPEG_ACCEPT_LAYOUTS 2" in header
