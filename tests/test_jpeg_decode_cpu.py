"""The JPEG decoder's host statement (csrc/jpeg_dec_host.h through whenet_jpeg_parse / whenet_jpeg_decode_host /
whenet_jpeg_decode_planes_host) against the numpy statement of tests/jpeg_decode_cases.py, byte for byte on every case of the table,
damaged streams included; against executed Pillow where Pillow itself stays within one level of the float64 inverse DCT; and the
round trip through the library's own encoder within the bound its quantisers allow.  No GPU."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_decode_cases as DC
from whenet_hip import _lib, jpeg
from whenet_hip.yuv import YUVFrame

ROOT = DC.ROOT


def library_frame(data, bgr=True):
    return jpeg.decode_host(data, bgr=bgr, strict=False)


# ---- 1. the host statement is the numpy statement -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.CASE_NAMES)
def test_decode_host_equals_the_numpy_statement(name):
    data, want = DC.case(name), DC.statement(name)
    hd = want.header
    i = jpeg.info(data)
    assert (i["h"], i["w"], i["components"], i["intervals"], i["data_offset"]) == (hd.h, hd.w, hd.comps, hd.intervals, hd.data_offset)
    assert i["sampling"] == (hd.hs, hd.vs) and i["restart_interval"] == hd.ri
    for c in range(hd.comps):
        assert i["quantisers"][i["quantiser_ids"][c]].tolist() == hd.q[hd.qt[c]]
    planes, status = jpeg.decode_planes_host(data)
    assert status.tolist() == want.status.tolist() == [DC.OK, -1]
    assert len(planes) == hd.comps
    for got, ref in zip(planes, want.planes):
        assert got.shape == ref.shape and np.array_equal(got, ref)
    assert np.array_equal(library_frame(data, True), DC.frame(want, True))
    assert np.array_equal(library_frame(data, False), DC.frame(want, False))


FOUR_TWO_ZERO = [n for n in DC.CASE_NAMES if n.startswith(("pil_420", "own_", "sample_"))]


@pytest.mark.parametrize("name", FOUR_TWO_ZERO)
def test_a_420_frame_is_yuv_to_bgr_host_of_the_decoded_i420_planes(name):
    data = DC.case(name)
    i = jpeg.info(data)
    assert i["sampling"] == (2, 2)
    h, w = i["h"], i["w"]
    for fmt in ("i420", "nv12"):                       # the planes through the surface destinations, pitched
        ch, cw = (h + 1) // 2, (w + 1) // 2
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
        assert _lib.jpeg_decode_host(data, s, True).tolist() == [DC.OK, -1]
        want = DC.statement(name).planes
        assert np.array_equal(y[:, :w], want[0]) and (y[:, w:] == 0xC7).all()
        if fmt == "i420":
            assert np.array_equal(u[:, :cw], want[1]) and np.array_equal(v[:, :cw], want[2])
            assert (u[:, cw:] == 0xC7).all() and (v[:, cw:] == 0xC7).all()
            yuv = YUVFrame.i420(np.ascontiguousarray(y[:, :w]), np.ascontiguousarray(u[:, :cw]), np.ascontiguousarray(v[:, :cw]), "jfif")
        else:
            assert np.array_equal(uv[:, 0:2 * cw:2], want[1]) and np.array_equal(uv[:, 1:2 * cw:2], want[2]) and (uv[:, 2 * cw:] == 0xC7).all()
            yuv = YUVFrame.nv12(np.ascontiguousarray(y[:, :w]), np.ascontiguousarray(uv[:, :2 * cw]), "jfif")
        assert np.array_equal(yuv.to_bgr(), library_frame(data, True))          # whenet_yuv_to_bgr_host


def test_other_samplings_do_not_decode_into_yuv_surfaces():
    data = DC.case("pil_444_17x17")
    y, c = np.zeros((17, 17), np.uint8), np.zeros((9, 9), np.uint8)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.plane[1], s.pitch[1], s.plane[2], s.pitch[2] = y.ctypes.data, 17, c.ctypes.data, 9, c.ctypes.data, 9
    s.format, s.matrix = _lib.YUV_I420, _lib.YUV_JFIF
    with pytest.raises(ValueError, match="4:2:0"):
        _lib.jpeg_decode_host(data, s, True)
    s.matrix = _lib.YUV_BT601
    with pytest.raises(ValueError):
        _lib.jpeg_decode_host(DC.case("pil_420_17x17"), s, True)


# ---- 2. pinned to executed Pillow -----------------------------------------------------------------------------------------------
def pillow_planes(data, mode):
    im = Image.open(io.BytesIO(data))
    im.draft(mode, im.size)
    im.load()
    assert im.mode == mode and im.size == Image.open(io.BytesIO(data)).size
    return np.asarray(im)


def within(a, b, tol):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= tol


@pytest.mark.parametrize("name", DC.CASE_NAMES)
def test_luma_is_within_one_level_of_the_float_idct_wherever_pillow_is(name):
    """Pillow's own Y (`draft('L')`: the decoder's luma plane) within 1 of the rounded float64 inverse DCT of the statement's
    coefficients -> this decoder's Y within 1 of it too, and within 2 of Pillow's (the sum of the two bounds, not a measurement).
    A case where Pillow is not within 1 does not belong in the table: that is asserted, not skipped."""
    data, dec = DC.case(name), DC.statement(name)
    ref = np.clip(np.rint(DC.float_planes(dec)[0]), 0, 255)
    pil = pillow_planes(data, "L")
    mine = jpeg.decode_planes_host(data)[0][0]
    assert within(pil, ref, 1), "Pillow itself leaves the float inverse DCT by more than a level: take the case out of the table"
    print(f"{name}: share of luma samples equal to Pillow's {float((mine == pil).mean()):.4f}, to the rounded float IDCT "
          f"{float((mine == ref).mean()):.4f}")
    assert within(mine, ref, 1)
    assert within(mine, pil, 2)


@pytest.mark.parametrize("name", [n for n in DC.CASE_NAMES if n.startswith("pil_444")])
def test_chroma_of_444_streams_is_within_one_level_of_the_float_idct_wherever_pillow_is(name):
    data, dec = DC.case(name), DC.statement(name)
    ref = [np.clip(np.rint(p), 0, 255) for p in DC.float_planes(dec)]
    pil = pillow_planes(data, "YCbCr")
    mine = jpeg.decode_planes_host(data)[0]
    for c in range(3):
        assert within(pil[..., c], ref[c], 1), "Pillow itself leaves the float inverse DCT by more than a level"
        assert within(mine[c], ref[c], 1) and within(mine[c], pil[..., c], 2)


def test_difference_to_pillows_rgb_on_the_samples_is_measured_not_asserted():
    """Nearest-neighbour chroma against libjpeg's triangle filter: a stated difference.  The figures go to docs/experiments.md."""
    for name in ("sample_001", "sample_012"):
        data = DC.case(name)
        pil = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(np.int64)
        mine = library_frame(data, bgr=False).astype(np.int64)
        d = np.abs(pil - mine)
        print(f"{name}: |RGB - Pillow's RGB| mean {d.mean():.3f}, max {d.max()}, equal share {float((d == 0).mean()):.4f}")
        assert mine.shape == pil.shape


# ---- 3. round trip through the library's encoder --------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", [10, 50, 95, 100])
@pytest.mark.parametrize("size", [(17, 17), (70, 50), (33, 40)])
def test_round_trip_stays_within_the_quantisers_bound(size, quality):
    """decode_host(encode_host(frame, q)): every sample within sum_vu (Q[vu] / 2) |basis_vu(y, x)| + 1 of the plane the encoder
    compressed -- half a quantiser step per coefficient, taken through the float64 inverse DCT, plus 1 for the decoder's rounding;
    computed from the stream's own quantisers."""
    from tests import jpeg_cases as JC
    h, w = size
    frame = np.ascontiguousarray(DC.picture(h, w, seed=quality)[..., ::-1])
    data = jpeg.encode_host(frame, quality)
    src = JC.planes_of_packed(frame, bgr=True)
    i = jpeg.info(data)
    planes, status = jpeg.decode_planes_host(data)
    assert status.tolist() == [DC.OK, -1]
    basis = np.abs(np.einsum("vy,ux->vuyx", DC.DCT_F, DC.DCT_F))               # |basis_vu(y, x)|
    for c in range(3):
        q = i["quantisers"][i["quantiser_ids"][c]].reshape(8, 8).astype(np.float64)
        bound = np.einsum("vu,vuyx->yx", q / 2, basis) + 1
        ph, pw = planes[c].shape
        tiled = np.tile(bound, (-(-ph // 8), -(-pw // 8)))[:ph, :pw]
        err = np.abs(planes[c].astype(np.float64) - np.asarray(src[c], np.float64))
        assert (err <= tiled).all(), (c, float((err - tiled).max()))


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
REASONS = {"progressive": "progressive", "sof1": "SOF1", "arithmetic": "arithmetic", "12bit": "12-bit", "4_components": "4 components",
           "two_scans": "several scans", "missing_dht": "missing Huffman table", "dqt_16bit": "16-bit", "truncated_header": "truncated",
           "not_a_jpeg": "SOI"}


@pytest.mark.parametrize("name", list(DC.REFUSED))
def test_unsupported_streams_are_refused_with_the_reason(name):
    data = DC.REFUSED[name]()
    with pytest.raises(DC.Refused):
        DC.parse(data)
    lib = _lib.load()
    a = np.frombuffer(data, np.uint8)
    info = _lib.JpegInfoC()
    assert lib.whenet_jpeg_parse(a.ctypes.data, a.size, info) == _lib.EFORMAT
    assert REASONS[name] in lib.whenet_last_error(None).decode()
    frame = np.full((64, 64, 3), 0xC7, np.uint8)
    status = np.full(2, 77, np.int32)
    assert lib.whenet_jpeg_decode_host(a.ctypes.data, a.size, jpeg.packed_surface(frame), _lib.BGR, status.ctypes.data) == _lib.EFORMAT
    assert (frame == 0xC7).all() and (status == 77).all()
    with pytest.raises(ValueError, match=REASONS[name]):
        jpeg.decode_host(data)


def test_bad_arguments_are_einval():
    lib = _lib.load()
    data = np.frombuffer(DC.case("pil_420_17x17"), np.uint8)
    info, status = _lib.JpegInfoC(), np.zeros(2, np.int32)
    frame = np.zeros((17, 17, 3), np.uint8)
    s = jpeg.packed_surface(frame)
    assert lib.whenet_jpeg_parse(None, 10, info) == _lib.EINVAL
    assert lib.whenet_jpeg_parse(data.ctypes.data, 0, info) == _lib.EINVAL
    assert lib.whenet_jpeg_parse(data.ctypes.data, data.size, None) == _lib.EINVAL
    assert lib.whenet_jpeg_decode_host(data.ctypes.data, 0, s, _lib.BGR, status.ctypes.data) == _lib.EINVAL
    assert lib.whenet_jpeg_decode_host(data.ctypes.data, data.size, None, _lib.BGR, status.ctypes.data) == _lib.EINVAL
    assert lib.whenet_jpeg_decode_host(data.ctypes.data, data.size, s, _lib.BGR, None) == _lib.EINVAL
    assert lib.whenet_jpeg_decode_host(data.ctypes.data, data.size, s, 7, status.ctypes.data) == _lib.EINVAL          # channel order
    s.pitch[0] = 3 * 17 - 1
    assert lib.whenet_jpeg_decode_host(data.ctypes.data, data.size, s, _lib.BGR, status.ctypes.data) == _lib.EINVAL
    assert "pitch" in lib.whenet_last_error(None).decode()
    s.pitch[0], s.on_device = 3 * 17, 1
    assert lib.whenet_jpeg_decode_host(data.ctypes.data, data.size, s, _lib.BGR, status.ctypes.data) == _lib.EINVAL
    assert lib.whenet_jpeg_decode_planes_host(data.ctypes.data, data.size, None, None, status.ctypes.data) == _lib.EINVAL
    assert not frame.any()


# ---- 5. damaged streams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.DAMAGED_NAMES)
def test_damaged_streams_give_the_status_and_the_statements_output(name):
    data, interval = DC.DAMAGED[name]()
    want = DC.statement(name)
    assert want.status.tolist() == [DC.EFORMAT, interval]
    planes, status = jpeg.decode_planes_host(data)
    assert status.tolist() == [_lib.EFORMAT, interval]
    for got, ref in zip(planes, want.planes):
        assert np.array_equal(got, ref)
    assert np.array_equal(library_frame(data, True), DC.frame(want, True))
    assert np.array_equal(library_frame(data, False), DC.frame(want, False))
    with pytest.raises(jpeg.DecodeError) as err:
        jpeg.decode_host(data)
    assert err.value.interval == interval and np.array_equal(err.value.frame, DC.frame(want, True))


def test_a_stream_without_its_eoi_is_whole():
    data = DC.case("pil_420_rst_rows")
    assert data[-2:] == b"\xff\xd9"
    planes, status = jpeg.decode_planes_host(data[:-2])
    assert status.tolist() == [DC.OK, -1]
    for got, ref in zip(planes, DC.statement("pil_420_rst_rows").planes):
        assert np.array_equal(got, ref)


def test_the_damaged_output_is_the_whole_output_up_to_the_damage():
    """Intervals before the bad one are untouched, the rows of the intervals behind a bad marker are the flat 128 of zero
    coefficients."""
    good = DC.statement("pil_420_rst_rows").planes[0]
    data, interval = DC.DAMAGED["wrong_rst"]()
    y = jpeg.decode_planes_host(data)[0][0]
    assert np.array_equal(y[:16 * (interval + 1)], good[:16 * (interval + 1)]) and (y[16 * (interval + 1):] == 128).all()
    data, interval = DC.DAMAGED["stray_marker"]()
    y = jpeg.decode_planes_host(data)[0][0]
    assert np.array_equal(y[:16 * interval], good[:16 * interval]) and np.array_equal(y[16 * (interval + 1):], good[16 * (interval + 1):])
    assert not np.array_equal(y[16 * interval:16 * (interval + 1)], good[16 * interval:16 * (interval + 1)])


# ---- 6. the sanitizer check and the symbols -------------------------------------------------------------------------------------
def test_host_check_program_runs_the_table_under_the_sanitizers(tmp_path):
    """tools/jpeg_dec_host_check.cpp: csrc/jpeg_dec_host.h -- the bit reader the kernels share -- built stand-alone with
    -fsanitize=address,undefined and run on every stream of the table, the damaged and the refused ones included."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_dec_host_check"
    src = os.path.join(ROOT, "tools", "jpeg_dec_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = []
    for name in DC.CASE_NAMES:
        (tmp_path / f"{name}.jpg").write_bytes(DC.case(name))
        names.append(name)
    for name in DC.DAMAGED_NAMES:
        (tmp_path / f"{name}.jpg").write_bytes(DC.DAMAGED[name]()[0])
        names.append(name)
    for name in DC.REFUSED:
        (tmp_path / f"{name}.jpg").write_bytes(DC.REFUSED[name]())
        names.append(name)
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.jpg") for n in names], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    for name in DC.CASE_NAMES:
        assert lines[f"{name}.jpg"].startswith("status 0 -1"), lines[f"{name}.jpg"]
    for name in DC.DAMAGED_NAMES:
        assert lines[f"{name}.jpg"].startswith(f"status {DC.EFORMAT} {DC.DAMAGED[name]()[1]}"), lines[f"{name}.jpg"]
    for name in DC.REFUSED:
        assert lines[f"{name}.jpg"].startswith("refused"), lines[f"{name}.jpg"]
    # the program's checksum of a frame is the library's frame (behind it: the checksum of the decode tables, which
    # tests/test_jpeg_parse_pins_cpu.py compares)
    import zlib
    for name in ("pil_420_17x17", "pil_444_q50", "noncode"):
        data = DC.DAMAGED[name]()[0] if name in DC.DAMAGED else DC.case(name)
        frame_part, tables = lines[f"{name}.jpg"].rsplit(" tables ", 1)
        assert frame_part.split()[-1] == f"{zlib.crc32(library_frame(data, True).tobytes()):08x}" and len(tables) == 16


def test_new_symbols_are_exported_and_bound():
    lib = _lib.load()
    for s in ("whenet_jpeg_parse", "whenet_jpeg_decode_host", "whenet_jpeg_decode_planes_host", "whenet_op_jpeg_decode",
              "whenet_jpeg_decode_device", "whenet_frame_begin_jpeg"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    import ctypes
    assert ctypes.sizeof(_lib.JpegInfoC) == 72 + 256 + 4 + 64 + 1024 + 4
