"""Rule 1 of the JPEG decoder (libjpeg's bytes) without a GPU: the numpy statement of tests/jpeg_exact_cases.py = the host statement
(csrc/jpeg_dec_host.h through whenet_jpeg_decode_rule_host and whenet_jpeg_decode_segmented_rule_host) = executed Pillow
(`Image.open(...).convert("RGB")`, its bundled libjpeg-turbo with its defaults), byte for byte; rule 0 through the new entry points
is rule 0; the refusals; the damaged streams; the six symbols."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import jpeg_decode_cases as DC
from tests import jpeg_exact_cases as EC
from whenet_hip import _lib, frames, jpeg

ROOT = DC.ROOT
SYMBOLS = ("whenet_jpeg_decode_rule_host", "whenet_jpeg_decode_segmented_rule_host", "whenet_op_jpeg_decode_rule",
           "whenet_op_jpeg_decode_clip_rule", "whenet_frame_begin_jpeg_rule", "whenet_clip_begin_jpeg_rule")


def three_way(data, dec, seg_bytes=128):
    """numpy statement = host (plain and segmented) = Pillow on the RGB frame; BGR is the RGB result reversed"""
    assert EC.off_the_clamp(dec), "a coefficient sits at the clamp: the stream is outside the claim"
    want = EC.pillow(data)
    assert np.array_equal(EC.frame(dec, bgr=False), want)
    host = jpeg.decode_host(data, bgr=False, rule="libjpeg")
    assert host.shape == want.shape and np.array_equal(host, want)
    assert np.array_equal(jpeg.decode_segmented_host(data, seg_bytes=seg_bytes, bgr=False, rule="libjpeg"), want)
    assert np.array_equal(jpeg.decode_host(data, bgr=True, rule="libjpeg"), want[..., ::-1])
    assert np.array_equal(EC.frame(dec, bgr=True), want[..., ::-1])


# ---- 1. three-way equality ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.CASE_NAMES)
def test_statement_host_and_pillow_agree_on_every_case(name):
    """Every Pillow-made stream of the table (16 x 8192 and the 300-interval stream among them), the library's own `encode_host`
    streams and the two committed stills."""
    three_way(DC.case(name), DC.statement(name))


@pytest.mark.parametrize("sampling", [0, 1, 2])
def test_statement_host_and_pillow_agree_on_the_size_sweep(sampling):
    """192 sizes per sampling: h in 1..18, w in 1..33 -- cw <= 2 (replication), cw = 3 (the first filtered width), both vertical
    clamps, planes whose padding holds decoded samples."""
    n = 0
    for s, h, w in EC.SWEEP:
        if s != sampling:
            continue
        data = EC.sweep_stream(s, h, w)
        dec = DC.decode(data)
        assert (dec.header.h, dec.header.w) == (h, w) and (dec.header.hs, dec.header.vs) == {0: (1, 1), 1: (2, 1), 2: (2, 2)}[s]
        three_way(data, dec, seg_bytes=4 if (h + w) % 2 else 64)
        n += 1
    assert n == 192


def test_the_segmented_host_form_gives_the_same_frame_at_every_window():
    data = DC.case("pil_420_50x70")
    want = EC.statement_frame("pil_420_50x70")
    for seg, window in ((4, 1), (4, 256), (16, 3), (4096, 1024)):
        got, status, st = jpeg.decode_segmented_host(data, seg_bytes=seg, window=window, rule="libjpeg", stats=True)
        assert status.tolist() == [DC.OK, -1] and st[7] == 1 and np.array_equal(got, want)


# ---- 2. rule 0 is untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pil_420_50x70", "pil_422_33x8", "pil_444_q50", "pil_grey_17x17", "own_17x17", "pil_420_1x1", "sample_001"])
def test_rule_0_through_the_new_entry_points_is_the_old_entry_points_bytes(name):
    data = DC.case(name)
    i = _lib.jpeg_parse(data)
    for bgr in (True, False):
        old = jpeg.decode_host(data, bgr=bgr)
        new = np.full((i.h, i.w, 3), 0x5A, np.uint8)
        assert _lib.jpeg_decode_rule_host(data, jpeg.packed_surface(new), bgr, "own").tolist() == [DC.OK, -1]
        assert np.array_equal(new, old)
        seg = np.full((i.h, i.w, 3), 0x5A, np.uint8)
        status, _ = _lib.jpeg_decode_segmented_rule_host(data, jpeg.packed_surface(seg), bgr, 16, 8, "own")
        assert status.tolist() == [DC.OK, -1] and np.array_equal(seg, old)
        assert np.array_equal(old, DC.frame(DC.statement(name), bgr))      # (and both are the rule-0 statement)
    if i.components == 3:
        assert not np.array_equal(jpeg.decode_host(data, rule="libjpeg"), jpeg.decode_host(data)) or i.h * i.w == 1


def test_a_pitched_destination_keeps_every_byte_outside_the_rows():
    data = DC.case("pil_420_17x17")
    buf = np.full((17, 17 * 3 + 7), 0xC7, np.uint8)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.format, s.on_device = buf.ctypes.data, buf.shape[1], _lib.SURF_PACKED, 0
    assert _lib.jpeg_decode_rule_host(data, s, True, "libjpeg").tolist() == [DC.OK, -1]
    assert np.array_equal(buf[:, :51].reshape(17, 17, 3), EC.statement_frame("pil_420_17x17")) and (buf[:, 51:] == 0xC7).all()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_rule_1_with_a_yuv_destination_is_einval(fmt):
    data = DC.case("pil_420_16x16")
    y, c = np.zeros((16, 16), np.uint8), np.zeros((8, 16), np.uint8)
    s = _lib.SurfaceC()
    s.plane[0], s.pitch[0], s.plane[1], s.pitch[1], s.plane[2], s.pitch[2] = y.ctypes.data, 16, c.ctypes.data, 16, c.ctypes.data, 16
    s.format, s.matrix, s.on_device = (_lib.YUV_I420 if fmt == "i420" else _lib.YUV_NV12), _lib.YUV_JFIF, 0
    assert _lib.jpeg_decode_rule_host(data, s, True, "own").tolist() == [DC.OK, -1]      # rule 0 takes the surface
    lib = _lib.load()
    a = np.frombuffer(data, np.uint8)
    status = np.zeros(2, np.int32)
    for plain in (True, False):
        if plain:
            rc = lib.whenet_jpeg_decode_rule_host(a.ctypes.data, a.size, C.byref(s), _lib.BGR, 1, status.ctypes.data)
        else:
            rc = lib.whenet_jpeg_decode_segmented_rule_host(a.ctypes.data, a.size, C.byref(s), _lib.BGR, 128, 256, 1, status.ctypes.data, None)
        assert rc == _lib.EINVAL
        assert b"WHENET_SURF_PACKED only" in lib.whenet_last_error(None)


def test_a_rule_outside_0_and_1_is_einval_and_python_names_the_choices():
    data = DC.case("pil_420_16x16")
    frame = np.zeros((16, 16, 3), np.uint8)
    lib = _lib.load()
    a = np.frombuffer(data, np.uint8)
    s = jpeg.packed_surface(frame)
    status = np.zeros(2, np.int32)
    for rule in (-1, 2):      # (the pure-host calls have no handle whose option -1 could mean)
        assert lib.whenet_jpeg_decode_rule_host(a.ctypes.data, a.size, C.byref(s), _lib.BGR, rule, status.ctypes.data) == _lib.EINVAL
    for call in (jpeg.decode_host, jpeg.decode_segmented_host):
        with pytest.raises(ValueError, match="'own' or 'libjpeg'"):
            call(data, rule="turbo")
    with pytest.raises(ValueError, match="'own' or 'libjpeg'"):
        jpeg.decode(data, rule="turbo", handle=object())
    with pytest.raises(ValueError, match="'own' or 'libjpeg'"):
        jpeg.decode_clip([data], rule=1, handle=object())


# ---- 4. damaged streams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.DAMAGED_NAMES)
def test_damaged_streams_keep_their_status_and_host_is_the_statement(name):
    data, bad = DC.DAMAGED[name]()
    i = _lib.jpeg_parse(data)
    want = EC.statement_frame(name)
    for segmented in (False, True):
        status = {}
        for rule in ("own", "libjpeg"):
            frame = np.full((i.h, i.w, 3), 0x5A, np.uint8)
            if segmented:
                status[rule] = _lib.jpeg_decode_segmented_rule_host(data, jpeg.packed_surface(frame), True, 16, 4, rule)[0].tolist()
            else:
                status[rule] = _lib.jpeg_decode_rule_host(data, jpeg.packed_surface(frame), True, rule).tolist()
            if rule == "libjpeg":
                assert np.array_equal(frame, want)
        assert status["own"] == status["libjpeg"] == [DC.EFORMAT, bad] == DC.statement(name).status.tolist()
    with pytest.raises(jpeg.DecodeError) as e:
        jpeg.decode_host(data, rule="libjpeg")
    assert e.value.interval == bad and np.array_equal(e.value.frame, want)


# ---- 5. the stand-alone sanitizer program walks rule 1 ---------------------------------------------------------------------------
def test_host_check_program_walks_rule_1_under_the_sanitizers(tmp_path):
    """tools/jpeg_dec_host_check.cpp (ASan + UBSan, its own main, CPU only) decodes every stream and every cut or flipped copy under
    rule 1 too; its rule-1 checksum is the library's rule-1 frame.  The streams: the sizes where the clamped neighbours sit at a
    plane's edge, and two damaged ones (tests/test_jpeg_decode_cpu.py runs the program on the whole table)."""
    import shutil
    import subprocess
    import zlib
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_dec_host_check"
    src = os.path.join(ROOT, "tools", "jpeg_dec_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    streams = {f"sweep_{s}_{h}x{w}": EC.sweep_stream(s, h, w) for s in (1, 2) for h, w in ((1, 1), (2, 4), (3, 5), (1, 6), (17, 17), (9, 33))}
    streams.update({n: DC.case(n) for n in ("pil_444_17x17", "pil_grey_17x17", "own_17x17")})
    streams.update({n: DC.DAMAGED[n]()[0] for n in ("run_past_63", "truncated_no_dri")})      # (small ones: every copy is decoded twice)
    for name, data in streams.items():
        (tmp_path / f"{name}.jpg").write_bytes(data)
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.jpg") for n in streams], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    for name, data in streams.items():
        want = jpeg.decode_host(data, bgr=True, strict=False, rule="libjpeg")
        status = f"status {DC.EFORMAT} {DC.DAMAGED[name]()[1]}" if name in DC.DAMAGED else "status 0 -1"
        assert lines[f"rule1:{name}.jpg"] == f"{status} crc {zlib.crc32(want.tobytes()):08x}", name
        assert lines[f"{name}.jpg"].startswith(status)


# ---- 6. the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_six_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "whenet_hip.h")) as f:
        text = f.read()
    for s in SYMBOLS:
        assert f"WHENET_API int {s}(" in text and text.count(s + "(") == 1 and s in _lib.EXPORTS and hasattr(lib, s)
    assert "#define WHENET_ABI_VERSION 6" in text and _lib.ABI_VERSION == 6      # additions only
    assert "JPEG DECODER, RULE 1" in text and '"jpeg_rule"' in text
    assert _lib.JPEG_RULE == {"own": 0, "libjpeg": 1}
    for name in ("op_jpeg_decode_rule", "op_jpeg_decode_clip_rule"):
        assert hasattr(_lib.Handle, name)
    import inspect
    for fn in (jpeg.decode, jpeg.decode_host, jpeg.decode_segmented_host, jpeg.decode_clip):
        assert inspect.signature(fn).parameters["rule"].default == "own"
    for fn in (frames.FramePipeline.begin_jpeg, frames.FramePipeline.begin_clip_jpeg):
        assert inspect.signature(fn).parameters["rule"].default is None      # None: the handle's option "jpeg_rule"
