"""The JPEG encoder's samplings and optimised Huffman tables without a GPU: `whenet_jpeg_encode_host_ex` against the numpy statement
of tests/jpeg_sampling_cases.py byte for byte, the header and the bound per sampling, `whenet_jpeg_optimal_table` on constructed
frequencies and against EXECUTED Pillow's (libjpeg-turbo's) own optimised tables, Pillow as the decoder of every stream and as
the encoder to stay next to, the round trip through the project's decoder, and the argument errors."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image, ImageFile, JpegImagePlugin

from tests import jpeg_cases as JC
from tests import jpeg_decode_cases as JD
from tests import jpeg_sampling_cases as SC
from tests import test_jpeg_cpu as T420      # the margins of the 4:2:0 pin: no new numbers here
from whenet_hip import _lib, jpeg
from whenet_hip.yuv import YUVFrame

SAMPLINGS = list(SC.SAMPLINGS)
LAYER = {s: [(1, hs, vs, 0), (2, 1, 1, 1), (3, 1, 1, 1)] for s, (hs, vs) in SC.SAMPLINGS.items()}


def _host(case, optimize, **kw):
    return jpeg.encode_host(case.pixels, case.quality, bgr=case.bgr, sampling=case.sampling, optimize=optimize, **kw)


_STREAMS = {}


def _library(case, optimize):
    """(the library's stream of a case, its histograms), encoded once; the statement's Encoded beside it only after the two streams
    were found equal, so that what a test reads from the statement (coefficients, interval bits) describes the LIBRARY's bytes"""
    key = (case.name, bool(optimize))
    if key not in _STREAMS:
        hist = np.zeros((4, 256), np.uint32)
        _STREAMS[key] = (_host(case, optimize, hist=hist), hist)
    data, hist = _STREAMS[key]
    enc = SC.statement(case, optimize)
    assert data == enc.data, case.name
    return data, hist, enc


# ---- 1. the host statement against the numpy statement -----------------------------------------------------------------------
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_encode_host_equals_the_statement(sampling, optimize):
    for case in SC.by_sampling()[sampling]:
        want = SC.statement(case, optimize)
        hist = np.full((4, 256), 0xABCD, np.uint32)
        assert _host(case, optimize, hist=hist) == want.data, case.name
        if optimize:
            assert np.array_equal(hist, want.hist), case.name
        else:
            assert (hist == 0xABCD).all()                            # written by an optimised encode only


def test_the_defaults_are_the_existing_calls():
    px = JC.smooth(33, 47, 5)
    assert jpeg.encode_host(px, 75, sampling="4:2:0", optimize=False) == jpeg.encode_host(px, 75) == JC.encode(JC.planes_of_packed(px), 33, 47, 75).data
    assert jpeg.header(33, 47, 75, sampling="4:2:0") == jpeg.header(33, 47, 75) == JC.header(33, 47, 75)
    assert jpeg.bound(33, 47, sampling="4:2:0") == jpeg.bound(33, 47)
    for c in (c for c in SC.CASES.values() if c.sampling == "4:2:0"):
        assert np.array_equal(np.stack(c.planes()[1:]), np.stack(JC.planes_of_packed(c.pixels, c.bgr)[1:]))


def test_the_geometry_cases_hit_what_they_are_designed_for():
    g = SC.GEOMETRY
    for case in g.values():
        for optimize in (False, True):
            data = _library(case, optimize)[0]
            p = SC.parse(data)                                       # the library's own bytes, through the test-side parser
            assert np.array_equal(p.coef, SC.statement(case, optimize).coef) and (p.hs, p.vs) == SC.SAMPLINGS[case.sampling]
    assert SC.statement(g["8x704_444"], False).coef.shape == (1, 264, 64) and SC.statement(g["8x1040_422"], False).coef.shape == (1, 260, 64)
    for s in ("444", "422"):
        assert SC.statement(g[f"8x24_{s}"], False).coef.shape[0] == 1 and SC.statement(g[f"9x24_{s}"], False).coef.shape[0] == 2
    assert any(SC.statement(c, False).stuffed for c in SC.CASES.values())


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_header_and_bound_per_sampling(sampling):
    hs, vs = SC.SAMPLINGS[sampling]
    for h, w, q in ((1, 1, 95), (33, 47, 30), (1080, 1920, 100), (8192, 8192, 1)):
        head = jpeg.header(h, w, q, sampling)
        assert head == SC.header(h, w, q, sampling) and len(head) == jpeg.HEADER_BYTES == 629
        base = jpeg.header(h, w, q)
        differ = [i for i in range(629) if head[i] != base[i]]
        # the SOF0 sampling byte of Y and the two DRI bytes: 2 + 18 + 2 x 69 bytes, then SOF0's marker, length, P, Y, X, Nf, id
        assert set(differ) <= {158 + 11, 629 - 14 - 2, 629 - 14 - 1}
        assert head[169] == (hs << 4) | vs and (head[613] << 8) | head[614] == -(-w // (8 * hs))
        blocks = (hs * vs + 2) * -(-w // (8 * hs))
        assert jpeg.bound(h, w, sampling) == SC.bound(h, w, sampling) == 629 + -(-h // (8 * vs)) * (2 * ((1660 * blocks + 7) // 8) + 2)
    for case in SC.by_sampling()[sampling]:
        h, w = case.pixels.shape[:2]
        for optimize in (False, True):
            enc = SC.statement(case, optimize)
            assert len(enc.data) <= jpeg.bound(h, w, sampling)
            head_bytes = enc.data.index(b"\xff\xda") + 14
            assert head_bytes == 629 if not optimize else 177 + 4 * 22 + 20 <= head_bytes <= 629


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_bound_holds_on_the_worst_blocks(sampling):
    # every AC coefficient +-1023 (16 + 10 bits in the luma table), DC differences of category 11, as the 4:2:0 test builds them
    hs, vs = SC.SAMPLINGS[sampling]
    codes = [JC.huffman_codes(*t) for t in JC.HUFF]
    R, M, bpm = 2, 3, hs * vs + 2
    h, w = R * 8 * vs, M * 8 * hs
    total = 629
    for r in range(R):
        acc, nbits, pred = 0, 0, [0, 0, 0]
        for i in range(bpm * M):
            comp = SC.block_component(i, sampling)
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
    assert jpeg.bound(h, w, sampling) >= total > 629 + R * (bpm * M * 1500 // 8)


# ---- 2. the tables ------------------------------------------------------------------------------------------------------------
def _check_table(freq, bits, vals):
    bits, vals = [int(b) for b in bits], [int(v) for v in vals]
    assert len(bits) == 16 and sum(bits) == len(vals)
    assert sorted(vals) == [s for s in range(256) if freq[s]]        # only the occurring symbols, each once
    kraft = sum(n / (1 << (l + 1)) for l, n in enumerate(bits))
    assert kraft < 1                                                 # room for the reserved code point
    codes = JC.huffman_codes(bits, vals)
    assert all(code != (1 << length) - 1 for code, length in codes.values())      # no code is all ones
    # symbols of equal code size in increasing value: where figure K.3 did not run the sizes are the lengths (where it ran, a
    # length holds symbols of several sizes, still listed size by size: libjpeg's order, which the Pillow pin requires)
    if max(SC.code_sizes(freq)) <= 16:
        at = 0
        for n in bits:
            assert vals[at:at + n] == sorted(vals[at:at + n])
            at += n
    else:
        size = SC.code_sizes(freq)
        assert vals == sorted(vals, key=lambda s: (size[s], s))


@pytest.mark.parametrize("name", list(SC.FREQUENCIES))
def test_optimal_table_on_constructed_frequencies(name):
    freq = SC.FREQUENCIES[name]
    assert freq.max() < 1 << 32
    bits, vals = jpeg.optimal_table(freq.astype(np.uint32))
    want_bits, want_vals = SC.optimal_table(freq)
    assert list(bits) == want_bits and list(vals) == want_vals
    _check_table(freq, bits, vals)
    if name == "single":
        assert list(bits) == [1] + [0] * 15 and list(vals) == [5]   # one 1-bit code
    if name == "two":
        # a tie of 3 and 3: the LARGER value is the second least, merges with the reserved symbol and shares the 2-bit level with it
        assert list(bits) == [1, 1] + [0] * 14 and list(vals) == [0, 0xF0]
    if name == "all_equal":
        assert list(bits) == [0] * 7 + [255, 1] + [0] * 7
    if name == "fibonacci":                                          # the unlimited code is deeper than 16: figure K.3 ran
        assert bits[15] > 0 and len(vals) == 40
    if name == "large":
        assert freq.sum() >= 1 << 27 and list(vals)[0] == 0x01


def test_optimal_table_on_seeded_frequencies():
    rs = np.random.RandomState(77)
    for i in range(200):
        n = rs.randint(1, 257)
        freq = np.zeros(256, np.int64)
        syms = rs.choice(256, n, replace=False)
        freq[syms] = rs.randint(1, 4, n) if i % 3 == 0 else np.floor(rs.pareto(0.4, n) * 3 + 1).clip(1, 1 << 28)
        bits, vals = jpeg.optimal_table(freq.astype(np.uint32))
        want_bits, want_vals = SC.optimal_table(freq)
        assert list(bits) == want_bits and list(vals) == want_vals
        _check_table(freq, bits, vals)


def test_optimal_table_einval():
    lib = _lib.load()
    bits, vals, count = np.zeros(16, np.uint8), np.zeros(256, np.uint8), C.c_int(0)
    freq = np.zeros(256, np.uint32)
    args = (bits.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), C.byref(count))
    assert lib.whenet_jpeg_optimal_table(freq.ctypes.data_as(C.c_void_p), *args) == _lib.EINVAL      # no symbol occurs
    assert lib.whenet_jpeg_optimal_table(None, *args) == _lib.EINVAL
    freq[3] = 1
    assert lib.whenet_jpeg_optimal_table(freq.ctypes.data_as(C.c_void_p), None, args[1], args[2]) == _lib.EINVAL
    assert lib.whenet_jpeg_optimal_table(freq.ctypes.data_as(C.c_void_p), *args) == _lib.OK and count.value == 1


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_optimised_streams_carry_proper_tables_and_are_not_longer(sampling):
    for case in SC.by_sampling()[sampling]:
        (std_data, _, std), (opt_data, hist, opt) = _library(case, False), _library(case, True)
        assert np.array_equal(std.coef, opt.coef)                    # the same pixels
        carried = SC.parse(opt_data).tables                          # the DHT segments of the library's stream
        for t in range(4):
            bits, vals = jpeg.optimal_table(hist[t])                 # the library's table of the library's histogram
            _check_table(hist[t], bits, vals)
            assert carried[SC.TC_TH[t]] == ([int(b) for b in bits], [int(v) for v in vals]), case.name
        # the entropy-coded bits before padding and stuffing, interval by interval
        assert all(o <= s for o, s in zip(opt.interval_bits, std.interval_bits)), case.name
        assert len(opt_data) <= len(std_data), case.name             # the whole stream: holds on every case of the table


# ---- 3. pinned to executed Pillow ---------------------------------------------------------------------------------------------
def _float_luma(enc, quality, sampling, h, w):
    """float64 [h,w]: the inverse DCT (float64, orthonormal basis) of the dequantised luma coefficients, + 128, unclipped"""
    hs, vs = SC.SAMPLINGS[sampling]
    R, B, _ = enc.coef.shape
    M = B // (hs * vs + 2)
    nat = np.zeros((R, M, hs * vs, 64))
    nat[..., JC.ZIGZAG] = enc.coef.reshape(R, M, hs * vs + 2, 64)[:, :, :hs * vs] * np.array(JC.scaled_q(JC.Q_LUMA, quality), np.float64)[JC.ZIGZAG]
    pix = np.einsum("vy,...vu,ux->...yx", JD.DCT_F, nat.reshape(R, M, vs, hs, 8, 8), JD.DCT_F) + 128
    return pix.transpose(0, 2, 4, 1, 3, 5).reshape(R * vs * 8, M * hs * 8)[:h, :w]      # [R, M, dy, dx, y, x] -> [R, dy, y, M, dx, x]


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_pillow_decodes_every_stream(sampling, optimize):
    worst = 0
    for case in SC.by_sampling()[sampling]:
        data, _, enc = _library(case, optimize)
        h, w = case.pixels.shape[:2]
        im = Image.open(io.BytesIO(data))
        assert im.format == "JPEG" and im.mode == "RGB" and im.size == (w, h) and im.layer == LAYER[sampling], case.name
        assert JpegImagePlugin.get_sampling(im) == SC.PILLOW_SUBSAMPLING[sampling]
        im.draft("YCbCr", im.size)                                   # the decoder's own planes, no colour conversion
        im.load()                                                    # the whole entropy-coded data, every restart marker
        assert im.mode == "YCbCr"
        y = np.asarray(im)[..., 0].astype(np.int64)
        want = np.clip(np.rint(_float_luma(enc, case.quality, sampling, h, w)), 0, 255).astype(np.int64)
        worst = max(worst, int(np.abs(y - want).max()))
        assert np.abs(y - want).max() <= T420.PILLOW_Y_BOUND, case.name
    print(f"{sampling} optimize={optimize}: Pillow's Y plane within {worst} level(s) of the float64 inverse DCT")


def _chroma(rgb):
    r, g, b = (rgb[..., i].astype(np.float64) for i in range(3))
    return np.stack([-0.168736 * r - 0.331264 * g + 0.5 * b, 0.5 * r - 0.418688 * g - 0.081312 * b])


@pytest.mark.parametrize("optimize", [False, True])
def test_chroma_error_on_the_line_frame_falls_with_the_sampling(optimize):
    px = SC.lines(64, 48)
    src = _chroma(px[..., ::-1])
    err = {}
    for sampling in SAMPLINGS:
        data = jpeg.encode_host(px, 95, sampling=sampling, optimize=optimize)
        got = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        err[sampling] = float(np.mean((_chroma(got) - src) ** 2))
    print("chroma mean squared error of the Pillow-decoded line frame:", {k: round(v, 2) for k, v in err.items()})
    # measured on the host statement: 1868 / 1026 / 6.3 -- a one-pixel line loses half of its chroma per halved direction
    assert err["4:4:4"] < err["4:2:2"] < err["4:2:0"]


@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_optimal_table_returns_pillows_own_tables(sampling):
    """Pillow's optimize=True baseline streams, one restart interval per MCU row: their symbols are counted by the test-side parser
    and `whenet_jpeg_optimal_table` of the four histograms must return the DHT segments' bits / vals byte for byte."""
    for content in SC.CONTENT:
        for (h, w) in ((33, 18), (35, 50), (64, 48)):
            for quality in SC.QUALITIES:
                rgb = np.ascontiguousarray(SC.CONTENT[content](h, w)[..., ::-1])
                buf = io.BytesIO()
                Image.fromarray(rgb).save(buf, format="JPEG", quality=quality, subsampling=SC.PILLOW_SUBSAMPLING[sampling], optimize=True,
                                          restart_marker_rows=1)
                p = SC.parse(buf.getvalue())
                assert (p.hs, p.vs) == SC.SAMPLINGS[sampling] and sorted(p.tables) == sorted(SC.TC_TH)
                for t in range(4):
                    bits, vals = jpeg.optimal_table(p.hist[t].astype(np.uint32))
                    assert (list(bits), list(vals)) == p.tables[SC.TC_TH[t]], (content, h, w, quality, t)


def _decoded_luma(data):
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    im.load()
    return np.asarray(im)[..., 0]


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("sampling", ["4:2:2", "4:4:4"])
@pytest.mark.parametrize("name", ["130x250_noise", "130x250_gradient"])
@pytest.mark.parametrize("quality", [50, 75, 95])
def test_quality_and_size_next_to_pillows_encoder(name, quality, sampling, optimize, monkeypatch):
    """test_jpeg_cpu.py's comparison at the other samplings and with optimised tables on both sides: its frames, its margins"""
    monkeypatch.setattr(ImageFile, "MAXBLOCK", 1 << 20)             # Pillow's optimize=True needs the whole stream in one buffer
    px = JC.CASES[name].source()[1]
    h, w = px.shape[:2]
    planes = SC.planes_of_packed(px, True, sampling)
    one = SC.planes_of_packed(px, True, "4:4:4")                      # full-resolution Y, Cb, Cr for Pillow, which subsamples itself
    ycc = np.stack(one, -1)
    ours = SC.encode(planes, h, w, quality, sampling, optimize).data
    assert jpeg.encode_host(px, quality, sampling=sampling, optimize=optimize) == ours
    buf = io.BytesIO()
    Image.frombytes("YCbCr", (w, h), ycc.tobytes()).save(buf, format="JPEG", quality=quality, subsampling=SC.PILLOW_SUBSAMPLING[sampling],
                                                         optimize=optimize)
    theirs = buf.getvalue()
    ours_db, theirs_db = T420._psnr(_decoded_luma(ours), planes[0]), T420._psnr(_decoded_luma(theirs), planes[0])
    print(f"{name} q{quality} {sampling} optimize={optimize}: luma PSNR {ours_db:.4f} dB (Pillow {theirs_db:.4f}), {len(ours)} bytes "
          f"(Pillow {len(theirs)})")
    assert theirs_db - ours_db <= T420.PSNR_MARGIN_DB
    assert SC.restart_overhead(16, 16) == T420.restart_overhead(16) and SC.restart_overhead(h, 16) == T420.restart_overhead(h)
    assert len(ours) <= len(theirs) * (1 + T420.SIZE_MARGIN) + SC.restart_overhead(h, 8)


# ---- 4. the round trip through the project's own decoder --------------------------------------------------------------------------
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_the_projects_decoder_accepts_every_stream(sampling, optimize):
    for case in SC.by_sampling()[sampling]:
        data, _, enc = _library(case, optimize)
        planes, status = jpeg.decode_planes_host(data)
        assert list(status) == [_lib.OK, -1], case.name
        hd = JD.parse(data)
        assert (hd.hs, hd.vs) == SC.SAMPLINGS[sampling]
        q = [JC.scaled_q(JC.Q_LUMA, case.quality), JC.scaled_q(JC.Q_CHROMA, case.quality)]
        zz_q = [[t[JC.ZIGZAG[k]] for k in range(64)] for t in q]
        want = JD._place(hd, JD.idct_int(SC.natural_dequantised(enc.coef, zz_q, sampling)), np.uint8)
        for got, w in zip(planes, want):
            assert np.array_equal(got, w), case.name
        frame = jpeg.decode_host(data, bgr=case.bgr)
        assert frame.shape == case.pixels.shape


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------------
def _encode_raw(surface, h, w, quality, sampling, optimize, cap, room, channel_order=_lib.BGR):
    """whenet_jpeg_encode_host_ex with `cap` on a buffer of `room` bytes filled with a canary: (code, size, buffer)"""
    lib = _lib.load()
    buf = np.full(room, 0xC5, np.uint8)
    size = C.c_int64(-1)
    rc = lib.whenet_jpeg_encode_host_ex(C.byref(surface), h, w, channel_order, quality, sampling, optimize, buf.ctypes.data_as(C.c_void_p), cap,
                                        C.byref(size), None)
    return rc, int(size.value), buf


def test_einval():
    lib = _lib.load()
    packed = jpeg.source_of(np.zeros((16, 16, 3), np.uint8))[0]
    for sampling in (0, 1, 2):
        assert _encode_raw(packed, 16, 16, 95, sampling, 1, 4096, 4096)[0] == _lib.OK
    for sampling in (-1, 3, 444):
        assert _encode_raw(packed, 16, 16, 95, sampling, 0, 4096, 4096)[0] == _lib.EINVAL
        assert "sampling" in (lib.whenet_last_error(None) or b"").decode()
        assert lib.whenet_jpeg_bound_ex(16, 16, sampling) == _lib.EINVAL
        assert lib.whenet_jpeg_header_ex(16, 16, 95, sampling, None, 0, None) == _lib.EINVAL
    for bad in ("4:1:1", "444", 2, None):
        with pytest.raises(ValueError, match="sampling"):
            jpeg.encode_host(np.zeros((16, 16, 3), np.uint8), sampling=bad)
        with pytest.raises(ValueError, match="sampling"):
            jpeg.bound(16, 16, bad)
        with pytest.raises(ValueError, match="sampling"):
            jpeg.header(16, 16, 95, bad)
    y, u, v = np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)
    for frame in (YUVFrame.i420(y, u, v, "jfif"), YUVFrame.nv12(y, np.zeros((8, 16), np.uint8), "jfif")):
        assert jpeg.encode_host(frame, sampling="4:2:0", optimize=True)      # planar sources carry 4:2:0 chroma: that they encode
        for sampling in ("4:2:2", "4:4:4"):
            with pytest.raises(ValueError, match="4:2:0 chroma"):
                jpeg.encode_host(frame, sampling=sampling)
            s = jpeg.source_of(frame)[0]
            assert _encode_raw(s, 16, 16, 95, _lib.jpeg_sampling_code(sampling), 0, 4096, 4096)[0] == _lib.EINVAL
            assert "4:2:0 chroma" in (lib.whenet_last_error(None) or b"").decode()


@pytest.mark.parametrize("optimize", [0, 1])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_overflow_reports_the_size_and_leaves_the_tail(sampling, optimize):
    case, = (c for n, c in SC.CASES.items() if n.startswith("35x50_") and n.endswith(f"_q100_bgr_{sampling}"))
    full = SC.statement(case, bool(optimize)).data
    head = full.index(b"\xff\xda") + 14
    assert (head < 629) == bool(optimize)
    surface, h, w, _keep = jpeg.source_of(case.pixels)
    code = _lib.jpeg_sampling_code(sampling)
    rc, size, buf = _encode_raw(surface, h, w, case.quality, code, optimize, len(full), len(full) + 64)
    assert rc == _lib.OK and size == len(full) and buf[:size].tobytes() == full and (buf[size:] == 0xC5).all()
    for cap in (len(full) - 1, 629, head, head - 1, 0):
        rc, size, buf = _encode_raw(surface, h, w, case.quality, code, optimize, cap, len(full) + 64)
        assert rc == _lib.EOVERFLOW and size == len(full)
        assert buf[:cap].tobytes() == full[:cap] and (buf[cap:] == 0xC5).all()
    with pytest.raises(jpeg.CapacityError) as err:
        jpeg.encode_host(case.pixels, case.quality, capacity=len(full) - 1, sampling=sampling, optimize=bool(optimize))
    assert err.value.needed == len(full)


# ---- 6. the host sanitizers ----------------------------------------------------------------------------------------------------------
def test_host_check_program_runs_under_the_sanitizers(tmp_path):
    """tools/jpeg_opt_host_check.cpp: csrc/jpeg_host.h -- the table builder and the host encoder the kernels share their arithmetic
    with -- built stand-alone with -fsanitize=address,undefined and run on the table's sizes and on 4,000 seeded frequency vectors"""
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_opt_host_check"
    src = os.path.join(JC.ROOT, "tools", "jpeg_opt_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "jpeg_opt_host_check OK: 198 frames, 4000 tables" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
