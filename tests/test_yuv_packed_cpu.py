"""Packed 4:2:2 ingest (YUYV / UYVY) without a GPU: the codes of include/whenet_hip.h, the host form of the conversion
(whenet_yuv_to_bgr_host) against its numpy statement (tests/yuv_packed_cases.py) on the case table and on every (Y, U, V) triple,
the tie to the pinned 4:2:0 path, the case table's power to see wrong implementations, the argument checks and the YUVFrame
constructors.  Everything is bitwise."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import yuv_packed_cases as PC
from whenet_hip import _lib, yuv
from whenet_hip.yuv import YUVFrame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- codes -------------------------------------------------------------------------------------------------------------------
def test_header_lib_and_package_agree_on_the_codes():
    with open(os.path.join(ROOT, "include", "whenet_hip.h")) as f:
        text = f.read()
    codes = {name: int(re.search(rf"#define WHENET_YUV_{name}\s+(\d+)", text).group(1)) for name in ("NV12", "I420", "YUYV", "UYVY")}
    assert (codes["YUYV"], codes["UYVY"]) == (PC.YUYV, PC.UYVY) == (_lib.YUV_YUYV, _lib.YUV_UYVY) == (3, 4)
    assert yuv.FORMATS["yuyv"] == yuv.FORMATS["yuy2"] == _lib.YUV_YUYV and yuv.FORMATS["uyvy"] == _lib.YUV_UYVY
    assert len(set(codes.values())) == 4 and 2 not in codes.values() and 7 not in codes.values()
    assert int(re.search(r"#define WHENET_SURF_PACKED\s+(\d+)", text).group(1)) == 2
    # the coefficient rows this file's statement restates are the header's
    m = re.search(r"#define WHENET_YUV_COEFFS((?:.*\\\n)*.*)\n", text)
    rows = [tuple(int(v) for v in r.split(",")) for r in re.findall(r"\{\s*(\d+(?:\s*,\s*\d+){5})\s*\}", m.group(1))]
    assert rows == [PC.COEFFS[0], PC.COEFFS[1], PC.COEFFS[2]]
    # one entry point more than before (the default-tables call), none for this format family
    declared = re.findall(r"WHENET_API\s+[\w\s\*]+?\b(whenet_\w+)\s*\(", text)
    assert len(declared) == len(set(declared)) == len(_lib.EXPORTS) == 131
    assert int(re.search(r"#define WHENET_ABI_VERSION\s+(\d+)", text).group(1)) == 6


# ---- the host function is the numpy statement --------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,matrix", PC.MATRICES)
@pytest.mark.parametrize("fname,fmt", PC.FORMATS)
def test_host_function_equals_numpy_on_every_case(fname, fmt, mname, matrix):
    for case in PC.CASES:
        b = PC.build(case, fmt)
        frame = PC.frame_of(b, mname)
        assert frame.format == fmt and frame.matrix == matrix
        if b["h"] > 1:
            assert frame.pitches == (b["pitch"],)
        got = frame.to_bgr()
        want = PC.expected(b, matrix)
        assert got.dtype == np.uint8 and got.shape == want.shape == (b["h"], b["w"], 3)
        assert got.tobytes() == want.tobytes(), (case[0], fname, mname)
        assert PC.build(case, fmt)["flat"].tobytes() == b["flat"].tobytes()      # the source is not written


def test_both_formats_of_one_picture_give_one_frame():
    for case in PC.CASES:
        a, b = PC.build(case, PC.YUYV), PC.build(case, PC.UYVY)
        assert PC.frame_of(a, "bt709").to_bgr().tobytes() == PC.frame_of(b, "bt709").to_bgr().tobytes(), case[0]


@pytest.mark.parametrize("mutation", PC.MUTATIONS)
def test_every_mutation_is_seen_by_its_case(mutation):
    name = PC.SEEN_BY[mutation]
    for _, fmt in PC.FORMATS:
        b = PC.built(name, fmt)
        want = PC.expected(b, 0)
        assert PC.expected(b, 0, mutation).tobytes() != want.tobytes(), (mutation, name, fmt)
        assert PC.frame_of(b, "bt601").to_bgr().tobytes() == want.tobytes()


@pytest.mark.parametrize("mname,matrix", PC.MATRICES)
def test_host_function_equals_numpy_on_all_triples(mname, matrix):
    fmt = PC.FORMATS[matrix % 2][1]                     # (the formats differ in byte positions only, which the case table covers)
    rows = PC.all_triples(fmt)
    seen = np.zeros(1 << 24, bool)
    step = 256
    for r0 in range(0, PC.TRIPLES_H, step):
        part = rows[r0:r0 + step]
        got = YUVFrame((part,), fmt, mname, step, PC.TRIPLES_W).to_bgr()
        assert got.tobytes() == PC.all_triples_expected(matrix, r0, step).tobytes(), (mname, r0)
        q = part.reshape(step, -1, 4).astype(np.int64)
        y0, u, y1, v = (q[..., i] for i in ((0, 1, 2, 3) if fmt == PC.YUYV else (1, 0, 3, 2)))
        seen[(y0 << 16) | (u << 8) | v] = True
        seen[(y1 << 16) | (u << 8) | v] = True
    assert seen.all()                                   # every triple was in the frame


# ---- the tie to the pinned 4:2:0 path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,matrix", PC.MATRICES)
def test_a_frame_whose_row_pairs_share_chroma_equals_its_i420_frame(mname, matrix):
    for h, w in ((2, 2), (5, 17), (10, 18), (33, 7), (64, 130)):
        Y, U, V = PC.content(f"shared_{h}x{w}", "random", h, w)
        U[1::2], V[1::2] = U[0:2 * (h // 2):2], V[0:2 * (h // 2):2]
        want = YUVFrame.i420(np.ascontiguousarray(Y[:, :w]), np.ascontiguousarray(U[0::2]), np.ascontiguousarray(V[0::2]), matrix=mname).to_bgr()
        for _, fmt in PC.FORMATS:
            rows = PC.interleave(Y, U, V, fmt)
            assert YUVFrame((rows,), fmt, mname, h, w).to_bgr().tobytes() == want.tobytes(), (h, w, fmt)


# ---- YUVFrame -------------------------------------------------------------------------------------------------------------------
def test_constructors_shapes_and_pitches():
    b = PC.built("random_5x17", PC.YUYV)
    rows = b["rows"]                                    # [5, 36]
    want = PC.expected(b, 0).tobytes()
    f = YUVFrame.yuyv(rows, w=17)
    assert (f.h, f.w, f.format, f.pitches, f.on_device) == (5, 17, _lib.YUV_YUYV, (36,), False) and f.to_bgr().tobytes() == want
    assert YUVFrame.yuyv(rows).w == 18 and YUVFrame.uyvy(rows, matrix="jfif").format == _lib.YUV_UYVY
    even = PC.built("random_10x18", PC.UYVY)
    f3 = YUVFrame.uyvy(even["rows"].reshape(10, 18, 2), matrix="bt709")          # [h, w, 2] for even w
    assert (f3.h, f3.w, f3.pitches) == (10, 18, (36,)) and f3.to_bgr().tobytes() == PC.expected(even, 1).tobytes()
    # from_buffer: tight, pitched, the alias, bytes
    g = YUVFrame.from_buffer(rows.tobytes(), 5, 17, "yuy2")
    assert g.format == _lib.YUV_YUYV and g.pitches == (36,) and not g.writable and g.to_bgr().tobytes() == want
    p = PC.built("random_pitched_64x130", PC.UYVY)
    g = YUVFrame.from_buffer(p["flat"], 64, 130, "uyvy", pitch=544, matrix="jfif")
    assert g.pitches == (544,) and g.to_bgr().tobytes() == PC.expected(p, 2).tobytes()
    d = g.descriptor()
    assert (d.format, d.matrix, d.h, d.w, d.pitch[0]) == (_lib.YUV_UYVY, _lib.YUV_JFIF, 64, 130, 544) and not d.plane[1] and not d.plane[2]
    # refusals
    for call, text in ((lambda: YUVFrame((rows, rows), "yuyv", "bt601", 5, 17), "YUYV has 1 plane, got 2"),
                       (lambda: YUVFrame((rows[:, :35],), "yuyv", "bt601", 5, 17), r"\[5,36\]"),
                       (lambda: YUVFrame((rows,), "yuyv", "bt601", 5, 19), r"\[5,40\]"),
                       (lambda: YUVFrame((rows[:, ::2],), "uyvy", "bt601", 5, 8), "contiguous|\\[5,16\\]"),
                       (lambda: YUVFrame((rows.astype(np.int8),), "yuyv", "bt601", 5, 17), "uint8"),
                       (lambda: YUVFrame.yuyv(rows, w=16), "w = 16"),
                       (lambda: YUVFrame.yuyv(rows[:, :34]), "4 cw"),
                       (lambda: YUVFrame.from_buffer(rows.tobytes(), 5, 17, "yuyv", pitch=35), "pitch 35 is below"),
                       (lambda: YUVFrame.from_buffer(rows.tobytes()[:-1], 5, 17, "yuyv"), "the frame needs 180"),
                       (lambda: YUVFrame.from_buffer(rows.tobytes(), 5, 17, "yvyu"), "unknown format"),
                       (lambda: YUVFrame((rows,), 2, "bt601", 5, 17), "unknown format"),
                       (lambda: YUVFrame.from_buffer(rows.tobytes(), 0, 17, "yuyv"), "sides must be 1..8192")):
        with pytest.raises(ValueError, match=text):
            call()


def test_a_packed_destination_is_refused_before_the_library():
    from whenet_hip.overlay import surface_of
    rows = np.zeros((4, 16), np.uint8)
    for f in (YUVFrame.yuyv(rows), YUVFrame.uyvy(rows)):
        assert f.writable
        with pytest.raises(ValueError, match="as a destination is not built"):
            surface_of(f, 4, 8)


# ---- the library's own argument checks ---------------------------------------------------------------------------------------------
def test_wrong_descriptors_are_refused_with_the_frames_index():
    lib = _lib.load()
    b = PC.built("random_5x17", PC.YUYV)
    out = np.empty((5, 17, 3), np.uint8)

    def refused(fn):
        d = PC.frame_of(b, "bt601").descriptor()
        fn(d)
        assert lib.whenet_yuv_to_bgr_host(C.byref(d), out.ctypes.data) == _lib.EINVAL
        return lib.whenet_last_error(None).decode()

    assert "frame 0: pitch 35 of plane 0 is below its row of 36 bytes" in refused(lambda d: d.pitch.__setitem__(0, 35))
    assert "frame 0: plane 0 is NULL" in refused(lambda d: d.plane.__setitem__(0, None))
    assert "sides must be 1..8192" in refused(lambda d: setattr(d, "w", 8193))
    assert "unknown matrix" in refused(lambda d: setattr(d, "matrix", 3))
    for code in (2, 7, -1, 5):
        msg = refused(lambda d: setattr(d, "format", code))
        assert f"frame 0: unknown format {code} (WHENET_YUV_NV12, WHENET_YUV_I420, WHENET_YUV_YUYV or WHENET_YUV_UYVY)" in msg
    # planes 1 and 2 are ignored: NULL and nonsense pitches are fine
    d = PC.frame_of(b, "bt601").descriptor()
    d.plane[1], d.plane[2], d.pitch[1], d.pitch[2] = None, None, -5, 0
    assert lib.whenet_yuv_to_bgr_host(C.byref(d), out.ctypes.data) == _lib.OK and out.tobytes() == PC.expected(b, 0).tobytes()
