"""YUV 4:2:0 ingest without a GPU: the constants of include/whenet_hip.h, the host form of the conversion
(whenet_yuv_to_bgr_host) against its numpy statement (tests/yuv_cases.py) on the case table and on every (Y, U, V) triple, the
JFIF row against executed Pillow, the case table's power to see wrong implementations, the argument checks and the YUVFrame
constructors.  Everything but the Pillow bound (1 level: Pillow's tables carry 6 fractional bits, the product's 20) is bitwise."""
import os
import re
import warnings

import numpy as np
import pytest

from tests import yuv_cases as YC
from whenet_hip import _lib
from whenet_hip import yuv as Y
from whenet_hip.yuv import YUVFrame

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def triples():
    return YC.all_triples()


# ---- constants ---------------------------------------------------------------------------------------------------------------
def test_constants_equal_the_table_and_the_expressions():
    with open(os.path.join(ROOT, "include", "whenet_hip.h")) as f:
        text = f.read()
    m = re.search(r"#define WHENET_YUV_COEFFS((?:.*\\\n)*.*)\n", text)
    rows = re.findall(r"\{\s*(\d+(?:\s*,\s*\d+){5})\s*\}", m.group(1))
    header = [tuple(int(v) for v in r.split(",")) for r in rows]
    assert len(header) == 3
    codes = {name: int(re.search(rf"#define WHENET_YUV_{name}\s+(\d+)", text).group(1)) for name in ("NV12", "I420", "BT601", "BT709", "JFIF")}
    assert (codes["NV12"], codes["I420"]) == (YC.NV12, YC.I420) == (_lib.YUV_NV12, _lib.YUV_I420)
    assert (codes["BT601"], codes["BT709"], codes["JFIF"]) == (YC.BT601, YC.BT709, YC.JFIF) == (_lib.YUV_BT601, _lib.YUV_BT709, _lib.YUV_JFIF)
    assert YC.COEFFS[YC.BT601] == (16, 1220542, 1673527, 409993, 852492, 2116026)
    assert YC.COEFFS[YC.JFIF] == (0, 1048576, 1470104, 360853, 748826, 1858077)
    for name, code in YC.MATRICES:
        assert YC.COEFFS[code] == YC.COEFF_EXPRESSIONS[code], name
        assert header[code] == YC.COEFFS[code], name
        assert Y.COEFFS[name] == YC.COEFFS[code], name
        yoff, cy, cvr, cug, cvg, cub = YC.COEFFS[code]
        assert cy * (255 - yoff) + max(cvr, cub) * 127 + (1 << 19) < 2 ** 31          # no sum leaves int32
        assert cy * (255 - yoff) + (cug + cvg) * 128 + (1 << 19) < 2 ** 31 and -(cug + cvg) * 127 > -2 ** 31
    assert 1220542 * 239 + 2116026 * 127 < 2 ** 30


# ---- the host function is the numpy statement --------------------------------------------------------------------------------
@pytest.mark.parametrize("mname,matrix", YC.MATRICES)
@pytest.mark.parametrize("fname,fmt", YC.FORMATS)
def test_host_function_equals_numpy_on_every_case(fname, fmt, mname, matrix):
    for case in YC.CASES:
        b = YC.build(case, fmt)
        frame = YC.frame_of(b, mname)
        assert frame.pitches == b["pitches"], case[0]                    # strides -> pitches
        got = frame.to_bgr()
        want = YC.expected(b, matrix)
        assert got.dtype == np.uint8 and got.shape == (b["h"], b["w"], 3)
        assert got.tobytes() == want.tobytes(), (case[0], fname, mname)


@pytest.mark.parametrize("mname,matrix", YC.MATRICES)
def test_host_function_equals_numpy_on_all_triples(triples, mname, matrix):
    yp, uv = triples
    got = YUVFrame.nv12(yp, uv, matrix=mname).to_bgr()
    want = YC.yuv_to_bgr([yp, uv], (4096, 4096), YC.NV12, matrix, 4096, 4096)
    assert got.tobytes() == want.tobytes()
    seen = np.zeros(1 << 24, bool)                                        # (the frame does hold every triple)
    t = YC.triples_per_pixel(yp, uv).astype(np.int64)
    seen[(t[..., 0] << 16) | (t[..., 1] << 8) | t[..., 2]] = True
    assert seen.all()


# ---- JFIF against executed Pillow ---------------------------------------------------------------------------------------------
def test_jfif_is_within_one_level_of_executed_pillow(triples):
    from PIL import Image
    yp, uv = triples
    ycc = np.ascontiguousarray(YC.triples_per_pixel(yp, uv))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)               # (the mode argument of fromarray)
        rgb = np.asarray(Image.fromarray(ycc, "YCbCr").convert("RGB"))
    ours = YC.yuv_to_bgr([yp, uv], (4096, 4096), YC.NV12, YC.JFIF, 4096, 4096)[..., ::-1]
    diff = np.abs(rgb.astype(np.int16) - ours.astype(np.int16))
    equal = float((diff == 0).mean())
    print(f"JFIF against Pillow over 2^24 triples: max |delta| = {int(diff.max())}, equal {equal:.1%}, off by one {float((diff == 1).mean()):.1%}")
    assert int(diff.max()) <= 1


# ---- the table sees wrong implementations ------------------------------------------------------------------------------------
def _applies(mutation, case, fmt, matrix):
    name, kind, h, w, pitched = case
    if mutation == "pitch_as_width":
        return pitched
    if mutation == "nv12_as_i420":
        return fmt == YC.NV12 and kind == "random" and ((h + 1) // 2) * ((w + 1) // 2) >= 2
    if mutation == "chroma_row_y":
        return kind == "random" and h >= 3
    if mutation == "no_max0":
        return kind == "extremes" and matrix != YC.JFIF and h * w >= 10      # (luma 0 among the extremes; JFIF has no offset)
    if mutation == "swap_uv":
        return kind == "random" and h * w >= 4
    return kind == "random" and h * w >= 4                                   # no_rounding


@pytest.mark.parametrize("mutation", YC.MUTATIONS)
def test_each_mutation_changes_the_cases_it_applies_to(mutation):
    applied = 0
    for case in YC.CASES:
        for _, fmt in YC.FORMATS:
            for _, matrix in YC.MATRICES:
                if not _applies(mutation, case, fmt, matrix):
                    continue
                b = YC.build(case, fmt)
                changed = int((YC.expected(b, matrix, mutation) != YC.expected(b, matrix)).sum())
                assert changed >= 1, (mutation, case[0], fmt, matrix)
                applied += 1
    assert applied >= 3, mutation


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def _valid_desc(fmt=YC.NV12):
    b = YC.build(YC.CASES[YC.CASE_NAMES.index("random_5x17")], fmt)
    return b, YC.frame_of(b, "bt601")


BAD = [
    ("plane 0 is NULL", lambda d: d.plane.__setitem__(0, None), YC.NV12),
    ("plane 1 is NULL", lambda d: d.plane.__setitem__(1, None), YC.NV12),
    ("plane 2 is NULL", lambda d: d.plane.__setitem__(2, None), YC.I420),
    ("pitch", lambda d: d.pitch.__setitem__(0, 16), YC.NV12),
    ("pitch", lambda d: d.pitch.__setitem__(1, 17), YC.NV12),
    ("pitch", lambda d: d.pitch.__setitem__(2, 8), YC.I420),
    ("unknown format", lambda d: setattr(d, "format", 2), YC.NV12),
    ("unknown format", lambda d: setattr(d, "format", -1), YC.NV12),
    ("unknown matrix", lambda d: setattr(d, "matrix", 3), YC.NV12),
    ("sides must be 1..8192", lambda d: setattr(d, "h", 0), YC.NV12),
    ("sides must be 1..8192", lambda d: setattr(d, "w", 8193), YC.NV12),
    ("sides must be 1..8192", lambda d: setattr(d, "h", -4), YC.I420),
]


@pytest.mark.parametrize("text,spoil,fmt", BAD, ids=[f"{i}_{b[0].split()[0]}" for i, b in enumerate(BAD)])
def test_bad_descriptor_is_einval_naming_the_frame_and_the_next_call_succeeds(text, spoil, fmt):
    lib = _lib.load()
    b, frame = _valid_desc(fmt)
    d = frame.descriptor()
    spoil(d)
    out = np.full((64, 64, 3), 7, np.uint8)
    rc = lib.whenet_yuv_to_bgr_host(d, _lib._ptr(out))
    assert rc == _lib.EINVAL
    msg = lib.whenet_last_error(None).decode()
    assert "frame 0" in msg and text in msg, msg
    assert (out == 7).all()                                               # nothing was written
    with pytest.raises(ValueError, match="frame 0"):
        _lib.yuv_to_bgr_host(d)
    assert frame.to_bgr().tobytes() == YC.expected(b, YC.BT601).tobytes()      # the next valid call


def test_null_arguments_are_einval():
    lib = _lib.load()
    _, frame = _valid_desc()
    assert lib.whenet_yuv_to_bgr_host(None, None) == _lib.EINVAL
    assert lib.whenet_yuv_to_bgr_host(frame.descriptor(), None) == _lib.EINVAL


# ---- YUVFrame ----------------------------------------------------------------------------------------------------------------
def test_constructors_take_pitches_from_strides():
    h, w = 6, 10
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, (h, 32), dtype=np.uint8)
    uvbig = rng.integers(0, 256, (3, 24), dtype=np.uint8)
    f = YUVFrame.nv12(big[:, :w], uvbig[:, :10], matrix="jfif")
    assert f.pitches == (32, 24) and (f.h, f.w, f.format, f.matrix) == (h, w, _lib.YUV_NV12, _lib.YUV_JFIF)
    want = YC.yuv_to_bgr([big.reshape(-1), uvbig.reshape(-1)], (32, 24), YC.NV12, YC.JFIF, h, w)
    assert f.to_bgr().tobytes() == want.tobytes()
    # the interleaved plane as [ch, cw, 2]
    uv3 = np.ascontiguousarray(uvbig[:, :10]).reshape(3, 5, 2)
    assert YUVFrame.nv12(big[:, :w], uv3, matrix="jfif").to_bgr().tobytes() == want.tobytes()
    u, v = rng.integers(0, 256, (2, 3, 16), dtype=np.uint8)
    g = YUVFrame.i420(big[:, :w], u[:, :5], v[:, 3:8], matrix=_lib.YUV_BT709)
    assert g.pitches == (32, 16, 16) and g.matrix == _lib.YUV_BT709
    want = YC.yuv_to_bgr([big.reshape(-1), u.reshape(-1), v.reshape(-1)[3:]], (32, 16, 16), YC.I420, YC.BT709, h, w)
    assert g.to_bgr().tobytes() == want.tobytes()
    d = g.descriptor()
    assert (d.h, d.w, d.format, d.matrix, list(d.pitch)) == (h, w, 1, 1, [32, 16, 16]) and d.plane[2] == v[:, 3:8].ctypes.data


@pytest.mark.parametrize("fname,fmt", YC.FORMATS)
def test_from_buffer_is_a_decoders_single_allocation(fname, fmt):
    h, w, pitch = 7, 13, 32
    ch, cw = 4, 7
    rng = np.random.default_rng(11)
    cpitch = pitch if fmt == YC.NV12 else 16
    n = pitch * h + (ch if fmt == YC.NV12 else 2 * ch) * cpitch
    buf = rng.integers(0, 256, n, dtype=np.uint8)
    f = YUVFrame.from_buffer(buf.tobytes(), h, w, fname, pitch=pitch, matrix="bt709")
    planes = [buf, buf[pitch * h:]] if fmt == YC.NV12 else [buf, buf[pitch * h:], buf[pitch * h + cpitch * ch:]]
    pitches = (pitch, cpitch) if fmt == YC.NV12 else (pitch, cpitch, cpitch)
    assert f.pitches == pitches
    assert f.to_bgr().tobytes() == YC.yuv_to_bgr(planes, pitches, fmt, YC.BT709, h, w).tobytes()
    # tight, and exactly as many bytes as the frame needs
    tight = rng.integers(0, 256, h * w + 2 * ch * cw, dtype=np.uint8)
    t = YUVFrame.from_buffer(tight, h, w, fname)
    assert t.pitches == ((w, 2 * cw) if fmt == YC.NV12 else (w, cw, cw)) and t.matrix == _lib.YUV_BT601
    with pytest.raises(ValueError, match="needs"):
        YUVFrame.from_buffer(tight[:-1], h, w, fname)
    with pytest.raises(ValueError, match="pitch"):
        YUVFrame.from_buffer(buf, h, w, fname, pitch=w - 1)


def test_constructors_reject_wrong_dtypes_and_shapes():
    y = np.zeros((4, 6), np.uint8)
    uv = np.zeros((2, 6), np.uint8)
    u = np.zeros((2, 3), np.uint8)
    YUVFrame.nv12(y, uv), YUVFrame.i420(y, u, u)
    with pytest.raises(ValueError, match="uint8"):
        YUVFrame.nv12(y.astype(np.float32), uv)
    with pytest.raises(ValueError, match="uint8"):
        YUVFrame.i420(y, u.astype(np.int16), u)
    with pytest.raises(ValueError, match="UV plane"):
        YUVFrame.nv12(y, u)                                   # a single chroma plane where the interleaved one belongs
    with pytest.raises(ValueError, match="V plane"):
        YUVFrame.i420(y, u, np.zeros((2, 4), np.uint8))
    with pytest.raises(ValueError, match="U plane"):
        YUVFrame.i420(y, np.zeros((3, 3), np.uint8), u)
    with pytest.raises(ValueError, match="Y plane"):
        YUVFrame.nv12(np.zeros((4, 6, 1), np.uint8), uv)
    with pytest.raises(ValueError, match="contiguous"):
        YUVFrame.nv12(np.zeros((4, 12), np.uint8)[:, ::2], uv)
    with pytest.raises(ValueError, match="matrix"):
        YUVFrame.nv12(y, uv, matrix="bt2020")
    with pytest.raises(ValueError, match="format"):
        YUVFrame.from_buffer(np.zeros(36, np.uint8), 4, 6, "yuy2")
    with pytest.raises(ValueError, match="sides"):
        YUVFrame.nv12(np.zeros((0, 6), np.uint8), np.zeros((0, 6), np.uint8))
    with pytest.raises(ValueError, match="planes"):
        YUVFrame((y, uv), "i420", "bt601", 4, 6)
    # odd sizes round the chroma planes up
    f = YUVFrame.i420(np.zeros((5, 7), np.uint8), np.zeros((3, 4), np.uint8), np.zeros((3, 4), np.uint8))
    assert f.pitches == (7, 4, 4)
    with pytest.raises(ValueError, match="U plane"):
        YUVFrame.i420(np.zeros((5, 7), np.uint8), np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8))
