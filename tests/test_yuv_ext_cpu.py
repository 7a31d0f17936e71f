"""The extended YUV ingest (include/whenet_hip_yuv_ext.h) without a GPU: the host statement (whenet_yuvx_to_bgr_host) against its
numpy statement (tests/yuv_ext_cases.py) on the case table, the tie of the 16-bit arithmetic to the pinned 8-bit path
(whenet_yuv_to_bgr_host) on the table and on every (Y, U, V) triple, the old formats through the new call, the float64 distance,
the case table's power to see wrong implementations, the companion header, the refusals, the YUVFrame constructors and the host
sanitizer program.  Everything but the float64 distance is bitwise."""
import ctypes as C
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import yuv_cases as YC
from tests import yuv_ext_cases as XC
from tests import yuv_packed_cases as PC
from whenet_hip import _lib, yuv
from whenet_hip.yuv import YUVFrame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "whenet_hip_yuv_ext.h")


# ---- 1. the host function is the numpy statement ------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,matrix", XC.MATRICES)
@pytest.mark.parametrize("fmt", XC.FORMATS, ids=XC.FORMAT_NAMES)
def test_host_function_equals_numpy_on_every_case(fmt, mname, matrix):
    for case in XC.CASES:
        b = XC.build(case, fmt)
        before = [f.copy() for f in b["flats"]]
        frame = XC.frame_of(b, mname)
        assert (frame.format, frame.container, frame.shift, frame.matrix) == (b["layout"], b["bits"], b["shift"], matrix) and frame.needs_ext
        if b["h"] > 1:
            assert frame.pitches == b["pitches"]
        got = frame.to_bgr()
        assert got.dtype == np.uint8 and got.shape == (b["h"], b["w"], 3)
        assert got.tobytes() == XC.expected_bytes(case[0], fmt[0], matrix), (case[0], fmt[0], mname)
        assert all(a.tobytes() == f.tobytes() for a, f in zip(before, b["flats"]))      # the source is not written


@pytest.mark.parametrize("shift", range(9))
def test_every_shift_uses_the_low_bits_and_masks_the_high_ones(shift):
    b = XC.build(XC.CASES[XC.CASE_NAMES.index("random_5x17")], ("i420_16", XC.I420, 16, shift))
    assert any((f.view("<u2") & 0xFF).any() and (f.view("<u2") >> 10).any() for f in b["flats"])      # low bits set, junk above bit 9
    assert XC.frame_of(b, "bt2020").to_bgr().tobytes() == XC.expected(b, XC.BT2020).tobytes()


# ---- 2. the tie to the pinned path: samples << 8 give the bytes of whenet_yuv_to_bgr_host ----------------------------------------
def _widened(planes8, layout, shift, matrix):
    """The 16-bit frame whose samples are the 8-bit samples << 8, stored under `shift`."""
    words = [(w >> shift).astype("<u2") for w in XC.widen(planes8)]
    h, w = planes8[0].shape
    return YUVFrame(words, layout, matrix, h, w, container=16, shift=shift), words


@pytest.mark.parametrize("mname,matrix", YC.MATRICES)
def test_samples_shifted_by_8_give_the_pinned_bytes_on_the_table(mname, matrix):
    for case in YC.CASES[:22]:                          # (the small and the pitched cases; the sample frames add nothing here)
        for fname, fmt in YC.FORMATS:
            b = YC.build(case, fmt)
            want = YC.frame_of(b, mname).to_bgr().tobytes()      # the existing call
            assert want == YC.expected(b, matrix).tobytes()
            tight = [np.ascontiguousarray(v) for v in b["views"]]
            for shift in (0, 4, 6):
                f, keep = _widened(tight, fmt, shift, mname)
                assert f.to_bgr().tobytes() == want, (case[0], fname, shift)
        b = YC.build(case, YC.I420)                     # 4:4:4 at 16 bits: the I420 frame's chroma repeated 2 x 2
        y, u, v = (np.ascontiguousarray(p) for p in b["views"])
        h, w = y.shape
        full = [y] + [np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w] for p in (u, v)]
        f, keep = _widened(full, XC.I444, 0, mname)
        assert f.to_bgr().tobytes() == YC.frame_of(b, mname).to_bgr().tobytes(), case[0]


def test_samples_shifted_by_8_give_the_pinned_bytes_on_all_triples():
    yp, uv = YC.all_triples()                           # every (Y, U, V) exactly once, 4096 x 4096
    want = YUVFrame.nv12(yp, uv, matrix="bt709").to_bgr()
    y16, uv16 = XC.widen([yp, uv])
    got = YUVFrame.p016(y16, uv16, matrix="bt709").to_bgr()
    assert got.tobytes() == want.tobytes()
    # a 2^18 sample for the others; BT.2020 has no old call: its 8-bit container through the new one (held to numpy above)
    rng = np.random.default_rng(2018)
    y, uv = rng.integers(0, 256, (512, 512), dtype=np.uint8), rng.integers(0, 256, (256, 512), dtype=np.uint8)
    y16, uv16 = XC.widen([y, uv])
    for mname in ("bt601", "jfif"):
        assert YUVFrame.p016(y16, uv16, matrix=mname).to_bgr().tobytes() == YUVFrame.nv12(y, uv, matrix=mname).to_bgr().tobytes(), mname
    narrow = YUVFrame((y, uv), "nv12", "bt2020", 512, 512, container=8)
    assert narrow.needs_ext and YUVFrame.p016(y16, uv16, matrix="bt2020").to_bgr().tobytes() == narrow.to_bgr().tobytes()
    assert narrow.to_bgr().tobytes() == XC.yuvx_to_bgr([y, uv], (512, 512), XC.NV12, 8, 0, XC.BT2020, 512, 512).tobytes()


# ---- 3. / 4. one picture in two formats ----------------------------------------------------------------------------------------------
def test_p016_and_the_16_bit_i420_frame_of_one_picture_give_one_frame():
    for case in XC.CASES:
        b = XC.build(case, ("i420_16", XC.I420, 16, 0))
        y, u, v = (np.ascontiguousarray(p).view("<u2") for p in b["views"])
        planar = YUVFrame.i010(y, u, v, depth=16, matrix="bt2020")
        semi = YUVFrame.p016(y, np.stack([u, v], axis=2), matrix="bt2020")
        assert (semi.format, planar.format, semi.shift, planar.shift) == (XC.NV12, XC.I420, 0, 0)
        assert semi.to_bgr().tobytes() == planar.to_bgr().tobytes(), case[0]


def test_an_i444_frame_of_repeated_chroma_gives_the_i420_frames_bytes():
    for case in YC.CASES[:22]:
        b = YC.build(case, YC.I420)
        y, u, v = (np.ascontiguousarray(p) for p in b["views"])
        h, w = y.shape
        full = YUVFrame.i444(y, *[np.ascontiguousarray(np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w]) for p in (u, v)], matrix="bt709")
        assert full.format == XC.I444 and full.container == 8 and full.needs_ext
        assert full.to_bgr().tobytes() == YC.frame_of(b, "bt709").to_bgr().tobytes(), case[0]


# ---- 5. an old format through the new call is the old call -----------------------------------------------------------------------
def test_old_formats_through_the_new_call_equal_the_old_call():
    n = 0
    for cases, mod in ((YC.CASES[:22], YC), (PC.CASES, PC)):
        for case in cases:
            for _, fmt in mod.FORMATS:
                b = mod.build(case, fmt)
                for mname, _ in YC.MATRICES:
                    frame = mod.frame_of(b, mname)
                    old = frame.descriptor()
                    assert isinstance(old, _lib.YuvFrameC) and not frame.needs_ext      # the old struct, as before
                    ext = frame.descriptor_ext()
                    assert (ext.layout, ext.container, ext.shift, ext.matrix) == (fmt, 8, 0, frame.matrix)
                    assert _lib.yuvx_to_bgr_host(ext).tobytes() == _lib.yuv_to_bgr_host(old).tobytes(), (case[0], fmt, mname)
                    assert _lib.yuvx_to_bgr_host(_lib.yuvx_desc(old)).tobytes() == frame.to_bgr().tobytes()
                    n += 1
    assert n >= 200


# ---- 6. float64 with the unrounded constants --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,matrix", XC.MATRICES)
def test_every_byte_is_within_one_level_of_float64(mname, matrix):
    """The coefficient rounding moves a value by under 4e-4 of a level, so only values near a tie (or, for BT.601, whose integer
    row is TRUNCATED from three-decimal constants, within its larger coefficient error) move; the share is reported, not capped."""
    differing = total = 0
    for fmt in XC.FORMATS:
        for name in ("random_10x18", "extremes_10x18", "random_pitched_64x130", "random_97x131"):
            b = XC.built(name, fmt[0])
            want = XC.float_reference(b["flats"], b["pitches"], b["layout"], b["bits"], b["shift"], matrix, b["h"], b["w"])
            got = XC.frame_of(b, mname).to_bgr().astype(np.int64)
            diff = np.abs(got - want)
            assert diff.max() <= 1, (mname, fmt[0], name, int(diff.max()))
            differing += int((diff != 0).sum())
            total += diff.size
    print(f"{mname}: {differing} of {total} bytes differ from float64 by one level ({100.0 * differing / total:.4f} %)")


# ---- 7. the table sees wrong implementations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", XC.MUTATIONS)
def test_each_wrong_implementation_differs_on_a_case(mutation):
    """A check of the case table first (numpy against numpy): a wrong implementation of this kind would be seen.  Then the
    library itself on the first such case: its bytes are the statement's and not the mutation's."""
    seen = []
    for fmt in XC.WIDE_FORMATS:
        if mutation == "chroma_row_y" and fmt[1] == XC.I444:
            continue
        for case in XC.CASES:
            b = XC.build(case, fmt)
            if XC.expected(b, XC.BT2020, mutation).tobytes() != XC.expected_bytes(case[0], fmt[0], XC.BT2020):
                seen.append((fmt[0], case[0]))
    assert seen, mutation
    fname, name = seen[0]
    b = XC.built(name, fname)
    got = XC.frame_of(b, "bt2020").to_bgr().tobytes()
    assert got == XC.expected_bytes(name, fname, XC.BT2020) and got != XC.expected(b, XC.BT2020, mutation).tobytes()
    if mutation == "wrap32":                            # the blue and red terms at Y16 = U16 = V16 = 65535
        assert any(name.startswith("extremes") for _, name in seen)


# ---- 8. the companion header -------------------------------------------------------------------------------------------------------
def test_companion_header_is_valid_c_and_agrees_with_library_and_package(tmp_path):
    with open(HEADER) as f:
        text = f.read()
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc is not None, "a host C compiler is needed"
    src = tmp_path / "use.c"
    src.write_text('#include "whenet_hip_yuv_ext.h"\nstatic const int k[WHENET_YUVX_MATRICES][6] = WHENET_YUVX_COEFFS;\n'
                   "int main(void) { whenet_yuvx_frame_t f; f.layout = WHENET_YUVX_I444; f.container = WHENET_YUVX_U16; "
                   "return k[WHENET_YUV_BT2020][0] + f.layout + f.container == 48 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(HEADER), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    declared = re.findall(r"WHENET_API\s+[\w\s\*]+?\b(whenet_\w+)\s*\(", text)
    assert len(declared) == 7 and tuple(declared) == _lib.EXPORTS_YUVX
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name) and name not in _lib.EXPORTS
    codes = {n: int(re.search(rf"#define WHENET_{n}\s+(\d+)", text).group(1)) for n in
             ("YUVX_I444", "YUVX_U8", "YUVX_U16", "YUV_BT2020", "YUVX_MATRICES", "YUVX_MAX_SHIFT")}
    assert codes == dict(YUVX_I444=16, YUVX_U8=8, YUVX_U16=16, YUV_BT2020=3, YUVX_MATRICES=4, YUVX_MAX_SHIFT=8)
    assert (_lib.YUVX_I444, _lib.YUVX_U8, _lib.YUVX_U16, _lib.YUV_BT2020) == (16, 8, 16, 3) == (XC.I444, 8, 16, XC.BT2020)
    assert yuv.LAYOUTS["i444"] == 16 and yuv.MATRICES_EXT["bt2020"] == 3 and "bt2020" not in yuv.MATRICES and "bt2020" not in yuv.COEFFS
    assert C.sizeof(_lib.YuvxFrameC) == 3 * C.sizeof(C.c_void_p) + 9 * 4 + (4 if C.sizeof(C.c_void_p) == 8 else 0)
    m = re.search(r"#define WHENET_YUVX_COEFFS((?:.*\\\n)*.*)\n", text)
    rows = [tuple(int(v) for v in r.split(",")) for r in re.findall(r"\{\s*(\d+(?:\s*,\s*\d+){5})\s*\}", m.group(1))]
    assert rows == [XC.COEFFS[i] for i in range(4)] and rows[:3] == [YC.COEFFS[i] for i in range(3)]
    assert rows[3] == XC.BT2020_DERIVED == yuv.COEFFS_EXT["bt2020"] == (16, 1220945, 1760217, 196426, 682019, 2245811)
    # whenet_hip.h is what it was: 131 declarations, three matrices, ABI 6
    with open(os.path.join(ROOT, "include", "whenet_hip.h")) as f:
        main = f.read()
    old = re.findall(r"WHENET_API\s+[\w\s\*]+?\b(whenet_\w+)\s*\(", main)
    assert len(old) == len(set(old)) == len(_lib.EXPORTS) == 131 and not set(old) & set(declared)
    assert "#define WHENET_YUV_MATRICES 3" in main and "yuvx" not in main.lower()
    assert int(re.search(r"#define WHENET_ABI_VERSION\s+(\d+)", main).group(1)) == 6
    for item in ("Y210", "NV16", "ig-endian", "PQ", "ull-range", "DESTINATIONS"):      # the "not built" list
        assert item in text.split("Not built:")[-1], item


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
def _valid(fname="p016"):
    b = XC.built("random_5x17", fname)
    return b, XC.frame_of(b, "bt2020")


def _odd_address(d):
    d.plane[1] = d.plane[1] + 1


BAD = [
    ("plane 0 is NULL", lambda d: d.plane.__setitem__(0, None), "p016"),
    ("plane 1 is NULL", lambda d: d.plane.__setitem__(1, None), "p016"),
    ("plane 2 is NULL", lambda d: d.plane.__setitem__(2, None), "yuv444p16"),
    ("pitch 32 of plane 0 is below its row of 34 bytes", lambda d: d.pitch.__setitem__(0, 32), "p016"),
    ("pitch 16 of plane 2 is below its row of 17 bytes", lambda d: d.pitch.__setitem__(2, 16), "i444"),
    ("unknown layout 2", lambda d: setattr(d, "layout", 2), "p016"),
    ("unknown layout 5", lambda d: setattr(d, "layout", 5), "p016"),
    ("unknown layout 7", lambda d: setattr(d, "layout", 7), "p016"),
    ("unknown layout -1", lambda d: setattr(d, "layout", -1), "i444"),
    ("unknown container 10", lambda d: setattr(d, "container", 10), "p016"),
    ("unknown container 0", lambda d: setattr(d, "container", 0), "i444"),
    ("unknown matrix 4", lambda d: setattr(d, "matrix", 4), "p016"),
    ("unknown matrix -1", lambda d: setattr(d, "matrix", -1), "i444"),
    ("shift 9 is outside 0..8", lambda d: setattr(d, "shift", 9), "p016"),
    ("shift -1 is outside 0..8", lambda d: setattr(d, "shift", -1), "yuv420p10le"),
    ("shift 6 with an 8-bit container", lambda d: setattr(d, "shift", 6), "i444"),
    ("a packed layout has an 8-bit container", lambda d: setattr(d, "layout", 3), "p016"),
    ("sides must be 1..8192", lambda d: setattr(d, "h", 0), "p016"),
    ("sides must be 1..8192", lambda d: setattr(d, "w", 8193), "i444"),
    ("plane 1 of 16-bit samples lies at an odd address", _odd_address, "p016"),
    ("pitch 35 of plane 0 of 16-bit samples is odd", lambda d: d.pitch.__setitem__(0, 35), "p016"),
]


@pytest.mark.parametrize("text,spoil,fname", BAD, ids=[f"{i}_{b[0].split()[0]}" for i, b in enumerate(BAD)])
def test_bad_descriptor_is_einval_naming_the_frame_and_the_next_call_succeeds(text, spoil, fname):
    lib = _lib.load()
    b, frame = _valid(fname)
    d = frame.descriptor()
    assert isinstance(d, _lib.YuvxFrameC)
    spoil(d)
    out = np.full((64, 64, 3), 7, np.uint8)
    assert lib.whenet_yuvx_to_bgr_host(d, _lib._ptr(out)) == _lib.EINVAL
    msg = lib.whenet_last_error(None).decode()
    assert "frame 0" in msg and text in msg, msg
    assert (out == 7).all()                                               # nothing was written
    with pytest.raises(ValueError, match="frame 0"):
        _lib.yuvx_to_bgr_host(d)
    assert frame.to_bgr().tobytes() == XC.expected_bytes("random_5x17", fname, XC.BT2020)      # the next valid call
    assert lib.whenet_yuvx_to_bgr_host(None, None) == _lib.EINVAL and lib.whenet_yuvx_to_bgr_host(frame.descriptor(), None) == _lib.EINVAL


# ---- 10. YUVFrame -------------------------------------------------------------------------------------------------------------------
def test_constructors_take_words_or_bytes_and_pitches_from_strides():
    h, w = 6, 10
    rng = np.random.default_rng(5)
    big = rng.integers(0, 65536, (h, 32), dtype=np.uint16)
    uvbig = rng.integers(0, 65536, (3, 24), dtype=np.uint16)
    f = YUVFrame.p010(big[:, :w], uvbig[:, :10], matrix="bt2020")
    assert f.pitches == (64, 48) and (f.h, f.w, f.format, f.container, f.shift, f.matrix) == (h, w, 0, 16, 0, 3)
    want = XC.yuvx_to_bgr([big.view(np.uint8).reshape(-1), uvbig.view(np.uint8).reshape(-1)], (64, 48), XC.NV12, 16, 0, XC.BT2020, h, w)
    assert f.to_bgr().tobytes() == want.tobytes()
    assert YUVFrame.p016(big[:, :w], np.ascontiguousarray(uvbig[:, :10]).reshape(3, 5, 2), matrix="bt2020").to_bgr().tobytes() == want.tobytes()
    assert YUVFrame.p010(big.view(np.uint8)[:, :2 * w], uvbig.view(np.uint8)[:, :20], matrix="bt2020").to_bgr().tobytes() == want.tobytes()
    d = f.descriptor()
    assert isinstance(d, _lib.YuvxFrameC) and (d.layout, d.container, d.shift, d.matrix, d.h, d.w, list(d.pitch)) == (0, 16, 0, 3, h, w, [64, 48, 0])
    assert d.plane[0] == big.ctypes.data and d.plane[1] == uvbig.ctypes.data
    u, v = rng.integers(0, 1024, (2, 3, 16), dtype=np.uint16)
    g = YUVFrame.i010(big[:, :w] >> 6, u[:, :5], v[:, 3:8])
    assert g.pitches == (20, 32, 32)                # (big >> 6 is a fresh tight array)
    assert (g.format, g.container, g.shift, g.matrix) == (1, 16, 6, _lib.YUV_BT709)
    assert YUVFrame.i010(big[:, :w], u[:, :5], v[:, 3:8], depth=12).shift == 4
    y8 = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    k = YUVFrame.i444(*y8)
    assert (k.format, k.container, k.pitches, k.matrix) == (16, 8, (w, w, w), _lib.YUV_BT601)
    assert k.to_bgr().tobytes() == XC.yuvx_to_bgr(list(y8.reshape(3, -1)), (w, w, w), XC.I444, 8, 0, XC.BT601, h, w).tobytes()
    k16 = YUVFrame.i444(big[:, :w], big[:, 10:20], big[:, 20:30], matrix="bt2020")
    assert (k16.container, k16.pitches) == (16, (64, 64, 64))


@pytest.mark.parametrize("fmt", XC.FORMATS, ids=XC.FORMAT_NAMES)
def test_from_buffer_is_a_decoders_single_allocation(fmt):
    fname, layout, bits, shift = fmt
    b = XC.built("random_5x17", fname)
    tight = XC.tight_buffer(b)
    f = YUVFrame.from_buffer(tight.tobytes(), 5, 17, fname, matrix="bt2020")
    assert (f.format, f.container, f.shift) == (layout, bits, shift) and f.pitches == b["pitches"]
    assert f.to_bgr().tobytes() == XC.expected_bytes("random_5x17", fname, XC.BT2020)
    with pytest.raises(ValueError, match="needs"):
        YUVFrame.from_buffer(tight[:-1], 5, 17, fname)
    with pytest.raises(ValueError, match="pitch"):
        YUVFrame.from_buffer(tight, 5, 17, fname, pitch=b["pitches"][0] - bits // 8)
    # pitched: the luma rows at 48 bytes, the chroma rows where the docstring puts them
    bs = bits // 8
    cpitch = 48 if layout != XC.I420 else 24
    rows = [v.shape[0] for v in b["views"]]
    buf = np.full(48 * rows[0] + cpitch * sum(rows[1:]), XC.GAP, np.uint8)
    off, flats, pitches = 0, [], []
    for v, p in zip(b["views"], [48] + [cpitch] * (len(rows) - 1)):
        np.lib.stride_tricks.as_strided(buf[off:], v.shape, (p, 1))[...] = v
        flats.append(buf[off:]), pitches.append(p)
        off += p * v.shape[0]
    g = YUVFrame.from_buffer(buf, 5, 17, fname, pitch=48, matrix="bt601")
    assert g.pitches == tuple(pitches) and bs * 17 <= 48
    assert g.to_bgr().tobytes() == XC.yuvx_to_bgr(flats, pitches, layout, bits, shift, XC.BT601, 5, 17).tobytes()


def test_names_of_from_buffer():
    assert {n: yuv.FORMATS_EXT[n] for n in ("p010", "p016", "yuv420p10le", "yuv420p12le", "i444", "yuv444p16")} == {
        "p010": (0, 16, 0), "p016": (0, 16, 0), "yuv420p10le": (1, 16, 6), "yuv420p12le": (1, 16, 4), "i444": (16, 8, 0), "yuv444p16": (16, 16, 0)}
    assert not set(yuv.FORMATS_EXT) & set(yuv.FORMATS)
    buf = np.zeros(5 * 17 * 2 + 3 * 18 * 2, np.uint8)
    assert YUVFrame.from_buffer(buf, 5, 17, "P010").matrix == _lib.YUV_BT601      # (from_buffer's default, as for the old formats)


def test_constructors_refuse_what_they_cannot_describe():
    y8, y16 = np.zeros((4, 6), np.uint8), np.zeros((4, 6), np.uint16)
    uv16, u16 = np.zeros((2, 6), np.uint16), np.zeros((2, 3), np.uint16)
    YUVFrame.p010(y16, uv16), YUVFrame.i010(y16, u16, u16), YUVFrame.i444(y16, y16, y16), YUVFrame.i444(y8, y8, y8)
    for bad in (lambda: YUVFrame.nv12(y16, uv16), lambda: YUVFrame.i420(y8, u16, u16.view(np.uint8)[:, :3])):
        with pytest.raises(ValueError, match="uint8"):                    # the 8-bit constructors keep refusing anything but uint8
            bad()
    with pytest.raises(ValueError, match="matrix"):
        YUVFrame.nv12(y8, np.zeros((2, 6), np.uint8), matrix="bt2020")        # (as before: the old constructors keep their three matrices)
    with pytest.raises(ValueError, match="matrix"):
        YUVFrame((y8, np.zeros((2, 6), np.uint8)), "nv12", "bt2020", 4, 6)      # (the plain constructor too, and its formats)
    with pytest.raises(ValueError, match="format"):
        YUVFrame((y8, y8, y8), "i444", "bt601", 4, 6)
    assert YUVFrame((y8, np.zeros((2, 6), np.uint8)), "nv12", "bt2020", 4, 6, container=8).needs_ext      # naming the container opens the new tables
    with pytest.raises(ValueError, match="uint16"):
        YUVFrame.p010(y16.astype(np.float32), uv16)
    with pytest.raises(ValueError, match="uint16"):
        YUVFrame.p010(y16, uv16.astype(">u2"))                             # big-endian samples are not built
    with pytest.raises(ValueError, match="even"):
        YUVFrame.p010(np.zeros((4, 13), np.uint8), np.zeros((2, 14), np.uint8))      # bytes: an odd row
    with pytest.raises(ValueError, match="UV plane"):
        YUVFrame.p010(y16, u16)
    with pytest.raises(ValueError, match="V plane"):
        YUVFrame.i444(y8, y8, np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError, match="V plane"):
        YUVFrame.i444(y16, y16, y8)                                        # 16-bit Y and U, a V plane of half the bytes
    with pytest.raises(ValueError, match="contiguous"):
        YUVFrame.p010(np.zeros((4, 12), np.uint16)[:, ::2], uv16)
    with pytest.raises(ValueError, match="depth"):
        YUVFrame.i010(y16, u16, u16, depth=7)
    with pytest.raises(ValueError, match="even"):
        YUVFrame.p010(np.zeros((4, 14), np.uint8)[:, 1:13], np.zeros((2, 12), np.uint8))      # an odd address
    with pytest.raises(ValueError, match="8-bit container"):
        YUVFrame((np.zeros((4, 12), np.uint8),), "yuyv", "bt601", 4, 6, container=16)
    with pytest.raises(ValueError, match="shift"):
        YUVFrame((y8, y8, y8), "i444", "bt601", 4, 6, container=8, shift=2)
    with pytest.raises(ValueError, match="extended calls"):
        _lib._yuv_descs([YUVFrame.i444(y8, y8, y8)])
    from whenet_hip import overlay
    with pytest.raises(ValueError, match="not built"):
        overlay.surface_of(YUVFrame.p010(y16, uv16), 4, 6, "annotate")


# ---- the host sanitizer program --------------------------------------------------------------------------------------------------
def test_host_check_program_runs_the_table_under_the_sanitizers(tmp_path):
    """tools/yuvx_host_check.cpp: csrc/yuvx_host.h -- the per-pixel function the kernels share, the staging layout, the checks --
    built stand-alone with -fsanitize=address,undefined and run on clips of the table: the program is never loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "yuvx_host_check"
    src = os.path.join(ROOT, "tools", "yuvx_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def write(name, b, layout, bits, shift, matrix):
        path = tmp_path / f"{name}.bin"
        with open(path, "wb") as f:
            f.write(np.array([layout, bits, shift, matrix, b["h"], b["w"]] + list(b["pitches"]) + [0] * (3 - len(b["pitches"])), "<i4").tobytes())
            for flat, v, p in zip(b["flats"], b["views"], b["pitches"]):
                f.write(flat[:p * (v.shape[0] - 1) + v.shape[1]].tobytes())
        return str(path)

    odd8 = YC.build(YC.CASES[YC.CASE_NAMES.index("random_3x5")], YC.I420)      # 15 + 2 * 6 = 27 bytes: the next frame would start odd
    assert sum(v.size for v in odd8["views"]) % 2 == 1
    for i, fmt in enumerate(XC.FORMATS):
        files, want = [], []
        for j, case in enumerate(XC.CASES):
            if len(files) == 15:
                break
            if j % 3 == 1:                                                  # an odd-sized 8-bit frame in front of the next one
                files.append(write(f"odd_{i}_{j}", odd8, YC.I420, 8, 0, XC.JFIF))
                want.append(zlib.crc32(YC.expected(odd8, YC.JFIF).tobytes()))
            b = XC.build(case, fmt)
            files.append(write(f"{fmt[0]}_{case[0]}", b, b["layout"], b["bits"], b["shift"], (i + j) % 4))
            want.append(zlib.crc32(XC.expected_bytes(case[0], fmt[0], (i + j) % 4)))
        if fmt[2] == 16:
            files, want = files[1:] + files[:1], want[1:] + want[:1]       # (the refusals run on the first frame: a 16-bit one)
        r = subprocess.run([str(exe)] + files, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(files) + 1 and lines[-1].startswith("refusals ") and lines[-1].endswith(" ok")
        for line, crc in zip(lines, want):
            parts = line.split()
            assert int(parts[3], 16) == int(parts[5], 16) == crc, line
        if fmt[2] == 16:
            assert any(int(line.split()[7]) > 0 and int(line.split()[7]) % 2 == 0 for line in lines[1:-1])
