"""The JPEG encoder without a GPU: `whenet_jpeg_encode_host` against the numpy statement of tests/jpeg_cases.py byte for byte on the
case table, the header and the IJG quantiser scaling at every quality, the test's own parser, EXECUTED Pillow (libjpeg-turbo) as
the third-party decoder and as the encoder to stay next to, the overflow and EINVAL rules and the bound."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image, features

from tests import jpeg_cases as JC
from whenet_hip import _lib, jpeg
from whenet_hip.yuv import YUVFrame

# Measured on the host statement (docs/experiments.md section 29), never on the kernels:
PILLOW_Y_BOUND = 1            # levels: Pillow's decoded Y plane against the float64 inverse DCT of the dequantised coefficients
PSNR_GAP_DB = 0.002           # the largest luma PSNR deficit against Pillow's own encoder on the six comparisons (0.0015 dB) ...
PSNR_MARGIN_DB = PSNR_GAP_DB + 0.05
SIZE_GAP = 0.020              # ... and the largest byte excess (1.99 %: chroma from summed RGB, DC predictors reset per MCU row)
SIZE_MARGIN = SIZE_GAP + 0.01


def restart_overhead(h):
    """bytes the restart intervals cost at most: the DRI segment, and per marker its two bytes and up to one byte of padding"""
    return 6 + 3 * ((h + 15) // 16 - 1)


@pytest.fixture(scope="module")
def statements():
    return {name: JC.statement(c) for name, c in JC.CASES.items()}


@pytest.fixture(scope="module")
def digests():
    return JC.load_digests()


# ---- 1. the host statement against the numpy statement -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(JC.CASES))
def test_encode_host_equals_the_statement(name, statements, digests):
    case = JC.CASES[name]
    _, frame = case.source()
    got = jpeg.encode_host(frame, case.quality, bgr=case.bgr)
    assert got == statements[name].data
    assert JC.digest(got) == digests[name]["sha256"] and len(got) == digests[name]["bytes"]


def test_the_designed_cases_hit_what_they_are_designed_for(statements):
    s = statements
    assert s["flat"].coef.any() == 0                                          # every block an EOB, every DC difference 0
    assert len(s["flat"].data) == JC.HEADER_BYTES + 2 * (12 + 2)              # two intervals of 96 bits and a marker each
    dc = s["black_white_q100"].coef[0, :, 0]
    assert int(abs(dc[6] - dc[3])).bit_length() == 11                         # Y00 of the white MCU against Y11 of the black one
    luma = s["checkerboard_q50"].coef[0].reshape(-1, 6, 64)[:, :4]
    assert (luma[..., 63] == -1).all() and (luma[..., :63] == 0).all()         # 62 zeros in front of the one coefficient: three ZRLs
    luma = s["checkerboard_q100"].coef[0].reshape(-1, 6, 64)[:, :4]
    assert (luma[..., 63] != 0).all()                                         # no EOB behind these blocks
    assert s["noise_q100_stuffed"].stuffed >= 1
    assert any(n % 8 == 0 for n in s["unpadded"].interval_bits) and JC.find_unpadded_seed() == JC.UNPADDED_SEED
    assert JC.parse(s["tall_160x16"].data).rst == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    assert s["wide_16x272"].coef.shape == (1, 17 * 6, 64)


def test_flat_frame_is_all_eobs(statements):
    # luma block: DC category 0 (2 bits) + EOB (4 bits); chroma block: 2 + 2 bits; an MCU 4 x 6 + 2 x 4 = 32 bits
    assert statements["flat"].interval_bits == [3 * 32, 3 * 32]


@pytest.mark.parametrize("quality", range(1, 101))
def test_header_and_quantisers_at_every_quality(quality):
    head, q = _lib.jpeg_header(33, 47, quality)
    assert head == JC.header(33, 47, quality) and len(head) == JC.HEADER_BYTES == jpeg.HEADER_BYTES
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    for row, base in zip(q, (JC.Q_LUMA, JC.Q_CHROMA)):
        assert list(row) == [min(max((b * scale + 50) // 100, 1), 255) for b in base]
    assert jpeg.header(33, 47, quality) == head and np.array_equal(jpeg.quantisers(quality), q)


def test_header_depends_on_size_and_quality_only(statements):
    for name, case in JC.CASES.items():
        planes, _ = case.source()
        h, w = planes[0].shape
        assert statements[name].data[:JC.HEADER_BYTES] == jpeg.header(h, w, case.quality)


# ---- 2. the parser, and Pillow as the decoder -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(JC.CASES))
def test_parser_recovers_the_quantised_coefficients(name, statements):
    enc = statements[name]
    p = JC.parse(enc.data)
    assert np.array_equal(p.coef, enc.coef)
    assert [m for m, _ in p.segments] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert p.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    assert p.rst == [r & 7 for r in range(enc.coef.shape[0] - 1)]


def test_pillow_is_built_with_a_jpeg_decoder():
    assert features.check("jpg")


@pytest.mark.parametrize("name", list(JC.CASES))
def test_pillow_decodes_every_stream(name, statements):
    enc = statements[name]
    planes, _ = JC.CASES[name].source()
    h, w = planes[0].shape
    im = Image.open(io.BytesIO(enc.data))
    assert im.format == "JPEG" and im.size == (w, h) and im.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    im.load()                                                        # the whole entropy-coded data, every restart marker
    im = Image.open(io.BytesIO(enc.data))
    im.draft("YCbCr", im.size)                                       # the decoder's own planes, no colour conversion
    im.load()
    assert im.mode == "YCbCr"
    y = np.asarray(im)[..., 0].astype(np.int64)
    p = JC.parse(enc.data)
    want = np.clip(np.rint(JC.reconstruct_luma(p.coef, p.qtables[0], h, w)), 0, 255).astype(np.int64)
    worst = int(np.abs(y - want).max())
    print(f"{name}: Pillow's Y plane within {worst} level(s) of the float64 inverse DCT")
    assert worst <= PILLOW_Y_BOUND


# ---- 3. quality and size against Pillow's own encoder ------------------------------------------------------------------------------
def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def _decoded_luma(data):
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    im.load()
    return np.asarray(im)[..., 0]


@pytest.mark.parametrize("name", ["130x250_noise", "130x250_gradient"])
@pytest.mark.parametrize("quality", [50, 75, 95])
def test_quality_and_size_next_to_pillows_encoder(name, quality):
    px = JC.CASES[name].source()[1]
    h, w = px.shape[:2]
    planes = JC.planes_of_packed(px)
    # the same pixels as full-resolution Y, Cb, Cr for Pillow: the packed rule with one pixel in the place of the four
    one = JC.planes_of_packed(np.repeat(np.repeat(px, 2, 0), 2, 1))
    ycc = np.stack([planes[0], one[1], one[2]], -1)
    assert np.array_equal(one[0][::2, ::2], planes[0])
    ours = JC.encode(planes, h, w, quality).data
    assert jpeg.encode_host(px, quality) == ours
    buf = io.BytesIO()
    Image.frombytes("YCbCr", (w, h), ycc.tobytes()).save(buf, format="JPEG", quality=quality, subsampling=2)
    theirs = buf.getvalue()
    ours_db, theirs_db = _psnr(_decoded_luma(ours), planes[0]), _psnr(_decoded_luma(theirs), planes[0])
    print(f"{name} q{quality}: luma PSNR {ours_db:.4f} dB (Pillow {theirs_db:.4f}), {len(ours)} bytes (Pillow {len(theirs)})")
    assert theirs_db - ours_db <= PSNR_MARGIN_DB
    assert len(ours) <= len(theirs) * (1 + SIZE_MARGIN) + restart_overhead(h)


# ---- 4. overflow, EINVAL, the bound -------------------------------------------------------------------------------------------------
def _encode_raw(surface, h, w, quality, cap, room, channel_order=_lib.BGR):
    """whenet_jpeg_encode_host with `cap` on a buffer of `room` bytes filled with a canary: (code, size, buffer)"""
    lib = _lib.load()
    buf = np.full(room, 0xC5, np.uint8)
    size = C.c_int64(-1)
    rc = lib.whenet_jpeg_encode_host(C.byref(surface), h, w, channel_order, quality, buf.ctypes.data_as(C.c_void_p), cap, C.byref(size))
    return rc, int(size.value), buf


def test_overflow_reports_the_size_and_leaves_the_tail(statements):
    case = JC.CASES["noise_q100_stuffed"]
    _, frame = case.source()
    full = statements[case.name].data
    surface, h, w, _keep = jpeg.source_of(frame)
    rc, size, buf = _encode_raw(surface, h, w, case.quality, len(full), len(full) + 64)
    assert rc == _lib.OK and size == len(full) and buf[:size].tobytes() == full and (buf[size:] == 0xC5).all()
    for cap in (len(full) - 1, JC.HEADER_BYTES, 0):
        rc, size, buf = _encode_raw(surface, h, w, case.quality, cap, len(full) + 64)
        assert rc == _lib.EOVERFLOW == -75 and size == len(full)
        assert buf[:cap].tobytes() == full[:cap] and (buf[cap:] == 0xC5).all()
    with pytest.raises(jpeg.CapacityError) as err:
        jpeg.encode_host(frame, case.quality, capacity=len(full) - 1)
    assert err.value.needed == len(full) and str(len(full)) in str(err.value)
    assert jpeg.encode_host(frame, case.quality, capacity=len(full)) == full


def test_einval():
    y, u, v = np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)
    good = jpeg.source_of(YUVFrame.i420(y, u, v, "jfif"))[0]
    assert _encode_raw(good, 16, 16, 95, 4096, 4096)[0] == _lib.OK
    for matrix in ("bt601", "bt709"):
        for frame in (YUVFrame.i420(y, u, v, matrix), YUVFrame.nv12(y, np.zeros((8, 16), np.uint8), matrix)):
            with pytest.raises(ValueError, match="JFIF"):
                jpeg.encode_host(frame)
    for h, w, q in ((0, 16, 95), (16, 0, 95), (8193, 16, 95), (16, 8193, 95), (16, 16, 0), (16, 16, 101)):
        assert _encode_raw(good, h, w, q, 4096, 4096)[0] == _lib.EINVAL
        if q == 95:
            with pytest.raises(ValueError):
                jpeg.bound(h, w)
        with pytest.raises(ValueError):
            jpeg.header(h, w, q)
    for p in range(3):
        bad = jpeg.source_of(YUVFrame.i420(y, u, v, "jfif"))[0]
        bad.plane[p] = None
        assert _encode_raw(bad, 16, 16, 95, 4096, 4096)[0] == _lib.EINVAL
        bad = jpeg.source_of(YUVFrame.i420(y, u, v, "jfif"))[0]
        bad.pitch[p] = (16, 8, 8)[p] - 1
        assert _encode_raw(bad, 16, 16, 95, 4096, 4096)[0] == _lib.EINVAL
    packed = jpeg.source_of(np.zeros((16, 16, 3), np.uint8))[0]
    assert _encode_raw(packed, 16, 16, 95, 4096, 4096, channel_order=7)[0] == _lib.EINVAL
    packed.pitch[0] = 47
    assert _encode_raw(packed, 16, 16, 95, 4096, 4096)[0] == _lib.EINVAL
    packed.pitch[0], packed.format = 48, 9
    assert _encode_raw(packed, 16, 16, 95, 4096, 4096)[0] == _lib.EINVAL
    lib = _lib.load()
    assert lib.whenet_jpeg_encode_host(None, 16, 16, _lib.BGR, 95, None, 0, None) == _lib.EINVAL
    assert "jpeg_encode_host" in (lib.whenet_last_error(None) or b"").decode()
    with pytest.raises(ValueError):
        jpeg.encode_host(np.zeros((16, 16, 3), np.float32))
    with pytest.raises(ValueError):
        jpeg.encode_host(np.zeros((16, 16, 4), np.uint8))


def test_bound_holds_on_the_table_and_on_the_worst_blocks(statements):
    for name, case in JC.CASES.items():
        planes, _ = case.source()
        h, w = planes[0].shape
        assert jpeg.bound(h, w) >= len(statements[name].data)
    # the derivation: 629 + ceil(h / 16) (2 ceil(1660 x 6 ceil(w / 16) / 8) + 2)
    for h, w in ((1, 1), (16, 16), (33, 47), (1080, 1920), (8192, 8192)):
        blocks = 6 * ((w + 15) // 16)
        assert jpeg.bound(h, w) == 629 + ((h + 15) // 16) * (2 * ((1660 * blocks + 7) // 8) + 2)
    # the worst blocks that can be coded: every AC coefficient +-1023 (16 + 10 bits in the luma table), DC differences of category 11
    codes = [JC.huffman_codes(*t) for t in JC.HUFF]
    h, w, R, M = 32, 48, 2, 3
    total = JC.HEADER_BYTES
    for r in range(R):
        acc, nbits, pred = 0, 0, [0, 0, 0]
        for i in range(6 * M):
            comp = 0 if i % 6 < 4 else i % 6 - 3
            zz = np.array([1023 if k % 2 else -1023 for k in range(64)])
            zz[0] = -1024 if pred[comp] >= 0 else 1016
            symbols = JC.block_symbols(zz, pred[comp], codes[0 if comp == 0 else 2], codes[1 if comp == 0 else 3])
            bits = sum(n for _, n in symbols)
            assert bits <= 1660 and (comp != 0 or bits == 9 + 11 + 63 * 26)
            for code, n in symbols:
                acc, nbits = (acc << n) | code, nbits + n
            pred[comp] = int(zz[0])
        raw = ((acc << (-nbits % 8)) | ((1 << (-nbits % 8)) - 1)).to_bytes((nbits + 7) // 8, "big")
        total += len(raw) + raw.count(b"\xff") + 2
    assert jpeg.bound(h, w) >= total > 629 + R * (6 * M * 1500 // 8)
