"""EXIF orientation on the host (csrc/jpeg_dec_host.h: jpeg_exif_orientation, jpeg_dec_frame_oriented_host; `whenet_jpeg_orientation`,
`whenet_jpeg_decode_oriented_host`): the parser on hand-built APP1 segments, the oriented host statement against the numpy table of
include/whenet_hip.h (JPEG DECODER, ORIENTATION) and, under rule 1, against executed Pillow's `ImageOps.exif_transpose`.  Every
comparison is `array_equal`.  No GPU.

Where Pillow 12.2.0 and the parser differ (measured, not asserted): Pillow also reads the tag with count 2, with a TIFF magic other
than 42 and from an IFD whose entry count leaves the segment; the parser answers 1 for all three, as for every malformed structure."""
import io
import warnings

import numpy as np
import pytest

from tests import jpeg_orient_cases as OC
from tests import jpeg_prog_cases as PC
from whenet_hip import _lib, jpeg


def pillow_tag(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Image.open(io.BytesIO(data)).getexif().get(OC.ORIENTATION)


def pillow_upright(data):
    from PIL import Image, ImageOps
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(data))).convert("RGB"))


# ---- 1. the parser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("progressive", [False, True])
@pytest.mark.parametrize("name", list(OC.SEGMENTS))
def test_the_parser_on_constructed_segments(name, progressive):
    segments, where, want = OC.SEGMENTS[name]
    data = OC.splice(OC.stream("420_17x35", progressive), segments, where)
    assert jpeg.orientation(data) == want
    assert jpeg.orientation(np.frombuffer(data, np.uint8)) == want
    # the header is read as it was: broken EXIF never refuses a stream
    i = _lib.jpeg_parse_scans(data)[0]
    assert (i.h, i.w) == (35, 17)
    if name in OC.WELL_FORMED:
        p = pillow_tag(data)
        assert p == want if isinstance(p, int) and 1 <= p <= 8 else want == 1


@pytest.mark.parametrize("name", OC.MALFORMED)
def test_everything_malformed_or_out_of_scope_gives_1(name):
    assert OC.SEGMENTS[name][2] == 1
    assert jpeg.orientation(OC.splice(OC.stream("420_17x35"), *OC.SEGMENTS[name][:2])) == 1


def test_the_parser_reads_nothing_it_should_not():
    good = OC.tagged("420_17x35", 6)
    assert jpeg.orientation(good) == 6
    for data in (b"", b"\xff", b"\xff\xd8", b"\xff\xd8\xff", b"\x00" * 64, good[:2] + good[4:]):
        assert jpeg.orientation(data) == 1
    at = good.index(b"Exif")
    for cut in range(len(good)):                       # every truncation: an answer in 1..8, and 1 until the entry is whole
        v = jpeg.orientation(good[:cut])
        assert 1 <= v <= 8
    assert jpeg.orientation(good[:at + 6 + 8 + 2 + 11]) == 1
    # an Exif APP1 behind SOS is not looked for
    sos = OC.stream("420_17x35").index(b"\xff\xda")
    base = OC.stream("420_17x35")
    assert jpeg.orientation(base[:sos] + base[sos:] + OC.exif_app1(OC.tiff(6))) == 1
    # info() keeps its keys
    assert set(jpeg.info(good)) == set(jpeg.info(base))


# ---- 2. the oriented host statement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.PICTURE_NAMES)
def test_decode_host_oriented_is_the_numpy_table_of_decode_host(name):
    h, w = OC.PICTURES[name][:2]
    for progressive in (False, True):
        plain = OC.stream(name, progressive)
        for rule in ("own", "libjpeg"):
            for bgr in (True, False):
                u = jpeg.decode_host(plain, bgr=bgr, rule=rule, progressive=progressive)
                assert u.shape == (h, w, 3)
                for v in OC.VALUES:
                    d = OC.tagged(name, v, progressive, order="II" if v & 1 else "MM")
                    got = jpeg.decode_host(d, bgr=bgr, rule=rule, progressive=progressive, orient=True)
                    assert got.shape == ((w, h, 3) if v >= 5 else (h, w, 3))
                    assert np.array_equal(got, OC.transform(u, v)), (name, progressive, rule, bgr, v)
                    # without the argument the tag is ignored: today's bytes
                    if v in (3, 6):
                        assert np.array_equal(jpeg.decode_host(d, bgr=bgr, rule=rule, progressive=progressive), u)
                # an untagged stream, and value 1: the plain call's bytes
                assert np.array_equal(jpeg.decode_host(plain, bgr=bgr, rule=rule, progressive=progressive, orient=True), u)


@pytest.mark.parametrize("name", OC.PICTURE_NAMES)
def test_rule_1_oriented_is_executed_pillow(name):
    for progressive in (False, True):
        for v in OC.VALUES:
            d = OC.tagged(name, v, progressive, where="soi" if v == 4 else "app0", typ=4 if v == 7 else 3)
            got = jpeg.decode_host(d, bgr=False, rule="libjpeg", progressive=progressive, orient=True)
            assert np.array_equal(got, pillow_upright(d)), (name, progressive, v)


@pytest.mark.parametrize("progressive", [False, True])
def test_a_damaged_oriented_stream_keeps_its_status_and_turns_its_defined_frame(progressive):
    cuts = [PC.DAMAGED["truncated_in_scan_5"], PC.DAMAGED["wrong_rst_scan_3"], PC.DAMAGED["cut_before_last_two_scans"]] if progressive \
        else [OC.baseline_cut(), OC.baseline_cut("420_33x65")]
    for cut in cuts:
        for rule in ("own", "libjpeg"):
            i = _lib.jpeg_parse_scans(cut)[0]
            u = np.empty((i.h, i.w, 3), np.uint8)
            if progressive:
                want_status = _lib.jpeg_decode_progressive_host(cut, jpeg.packed_surface(u), True, rule)
            else:
                want_status = _lib.jpeg_decode_rule_host(cut, jpeg.packed_surface(u), True, rule)
            assert want_status[0] == PC.EFORMAT
            for v in (1, 2, 6, 7):
                d = OC.oriented(cut, v)
                got = np.empty((i.w, i.h, 3) if v >= 5 else (i.h, i.w, 3), np.uint8)
                status = _lib.jpeg_decode_oriented_host(d, jpeg.packed_surface(got), True, rule, progressive)
                assert status.tolist() == want_status.tolist()
                assert np.array_equal(got, OC.transform(u, v))
                with pytest.raises(jpeg.DecodeError) as err:
                    jpeg.decode_host(d, rule=rule, progressive=progressive, orient=True)
                assert err.value.interval == want_status[1] and np.array_equal(err.value.frame, got)


def test_pitched_destinations_and_refusals_of_the_host_statement():
    d = OC.tagged("420_17x35", 6)
    want = jpeg.decode_host(d, orient=True)
    block = np.full((17, 3 * 35 + 11), 0xC3, np.uint8)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = block.ctypes.data, block.strides[0], _lib.SURF_PACKED, 0
    assert _lib.jpeg_decode_oriented_host(d, s, True).tolist() == [PC.OK, -1]
    assert np.array_equal(block[:, :105].reshape(17, 35, 3), want) and (block[:, 105:] == 0xC3).all()
    # the destination is checked against the ORIENTED size: the upright pitch (3 * 17) is too small for rows of 35 pixels
    s.pitch[0] = 3 * 17
    with pytest.raises(ValueError, match="pitch"):
        _lib.jpeg_decode_oriented_host(d, s, True)
    # a planar destination and a turned stream
    planes = [np.full((36, 18), 0xC3, np.uint8), np.full((18, 9), 0xC3, np.uint8), np.full((18, 9), 0xC3, np.uint8)]
    y = _lib.SurfaceC()
    for k, p in enumerate(planes):
        y.plane[k], y.pitch[k] = p.ctypes.data, p.strides[0]
    y.format, y.matrix, y.on_device = _lib.YUV_I420, _lib.YUV_JFIF, 0
    with pytest.raises(ValueError, match="packed surfaces only"):
        _lib.jpeg_decode_oriented_host(d, y, True)
    assert all((p == 0xC3).all() for p in planes)
    # a progressive stream needs progressive=True here as everywhere
    with pytest.raises(ValueError, match="progressive"):
        jpeg.decode_host(OC.tagged("420_17x35", 6, True), orient=True)


def test_host_check_program_runs_the_segments_under_the_sanitizers(tmp_path):
    """tools/jpeg_orient_host_check.cpp: the parser and the oriented host statement built stand-alone (its own main, CPU only) with
    -fsanitize=address,undefined: every constructed APP1, every truncation and 96 bit-flipped copies of each in exact-size heap
    blocks, and a few pictures decoded into destinations of exactly the oriented size."""
    import os
    import shutil
    import subprocess
    import zlib
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_orient_host_check"
    src = os.path.join(root, "tools", "jpeg_orient_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    streams = {f"seg_{n}": OC.splice(OC.stream("420_17x35", k & 1 == 1), segs, where) for k, (n, (segs, where, _)) in enumerate(OC.SEGMENTS.items())}
    pictures = {}
    for k, name in enumerate(("420_17x35", "422_35x50_blocks3", "444_33x65", "grey_9x7", "420_4x9_cw2", "420_1x1", "422_7x1")):
        for v in (2, 5, 6, 7):
            pictures[f"pic_{name}_{v}"] = OC.tagged(name, v, (k + v) & 1 == 1)
    pictures["cut_prog_6"] = OC.oriented(PC.DAMAGED["truncated_in_scan_5"], 6)
    pictures["cut_base_8"] = OC.oriented(OC.baseline_cut(), 8)
    streams.update(pictures)
    for n, d in streams.items():
        (tmp_path / f"{n}.jpg").write_bytes(d)
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.jpg") for n in streams], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    for n, (_, _, want) in OC.SEGMENTS.items():
        assert lines[f"seg_{n}.jpg"].startswith(f"orientation {want} "), (n, lines[f"seg_{n}.jpg"])
    for n, d in pictures.items():
        word = lines[f"{n}.jpg"].split()
        own = jpeg.decode_host(d, strict=False, progressive=True, orient=True)
        lib = jpeg.decode_host(d, strict=False, progressive=True, orient=True, rule="libjpeg")
        assert word[1] == str(jpeg.orientation(d)) and word[2] == f"{own.shape[0]}x{own.shape[1]}", (n, word)
        assert word[-2:] == [f"{zlib.crc32(own.tobytes()):08x}", f"{zlib.crc32(lib.tobytes()):08x}"], (n, word)
        assert (word[4] != "0") == n.startswith("cut_")


def test_python_surface():
    import inspect
    from whenet_hip.frames import FramePipeline, JpegStatus
    for fn, default in ((jpeg.decode, False), (jpeg.decode_host, False), (jpeg.decode_clip, False), (FramePipeline.begin_clip_jpeg, False),
                        (FramePipeline.begin_jpeg, None)):
        assert inspect.signature(fn).parameters["orient"].default is default
    assert JpegStatus().orientation == 1
    assert jpeg.oriented_shape(3, 5, 4) == (3, 5) and jpeg.oriented_shape(3, 5, 5) == (5, 3)
