"""Default Huffman tables without a GPU (whenet_jpeg_add_default_tables; csrc/jpeg_dec_host.h's jpeg_add_default_tables): MJPG
frames whose DHT segments were left out are completed with libjpeg's std_huff_tables -- read here from executed Pillow streams, not
restated -- and then decode to the bytes of the complete stream and, under rule 1, to the bytes executed Pillow (libjpeg-turbo, which
installs the same tables itself) returns for the STRIPPED stream.

PROGRESSIVE.  libjpeg always optimises the tables of a progressive stream, and such a stream defines only its DC tables in front of
the first SOS (the AC tables stand in front of their own scans).  So "stripped" has one well-defined equal for SOF2: the AC slots,
which are missing in front of the first SOS as the stream stands -- the completed stream gets the Annex K AC tables there, every AC
scan's own DHT replaces them, and the frame is the original's and Pillow's.  Cutting a progressive stream's optimised DC tables
leaves entropy data no table describes: Pillow reports a broken stream, and the test holds those copies to the structure only (the
segment's bytes and position), not to a frame."""
import io
import warnings

import numpy as np
import pytest

from tests import jpeg_default_tables_cases as DT
from whenet_hip import _lib, jpeg
from whenet_hip.mjpeg import MJPGReader, MJPGWriter

MISSING_TEXT = "missing Huffman table"


def pillow_rgb(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def missing_slots(stream):
    have = DT.tables_before_sos(stream)
    return [k for k in DT.SLOTS if k not in have]


NAMES = sorted(DT.sources())


@pytest.mark.parametrize("sname", sorted(DT.STRIPS))
@pytest.mark.parametrize("name", NAMES)
def test_a_stripped_stream_is_restored(name, sname):
    data, sof2 = DT.sources()[name]
    stripped = DT.strip(data, DT.STRIPS[sname])
    missing = missing_slots(stripped)
    assert missing, (name, sname)                       # (a grey or progressive stream misses id 1 / AC slots as it stands)
    got = jpeg.add_default_tables(stripped)
    # the inserted segment is exactly the Annex K bytes of the missing slots, in order, directly in front of the first SOS
    at = DT.sos_at(stripped)
    seg = DT.annex_k_segment(missing)
    assert len(seg) <= 420 and got == stripped[:at] + seg + stripped[at:], (name, sname)
    assert missing_slots(got) == [] and jpeg.add_default_tables(got) == got
    # the frame is the unstripped stream's under both rules, and under rule 1 what Pillow makes of the STRIPPED stream
    cut_own_tables = sof2 and any(k in DT.STRIPS[sname] for k in DT.tables_before_sos(data))
    if cut_own_tables:                                  # (optimised DC tables are gone: no frame is defined, see the docstring)
        return
    for rule in ("own", "libjpeg"):
        want = jpeg.decode_host(data, rule=rule, progressive=sof2, bgr=False)
        assert jpeg.decode_host(got, rule=rule, progressive=sof2, bgr=False).tobytes() == want.tobytes(), (name, sname, rule)
        assert jpeg.decode_host(stripped, rule=rule, progressive=sof2, bgr=False, default_tables=True).tobytes() == want.tobytes()
    assert jpeg.decode_host(got, rule="libjpeg", progressive=sof2, bgr=False).tobytes() == pillow_rgb(stripped).tobytes(), (name, sname)
    planes, status = jpeg.decode_planes_host(stripped, progressive=sof2, default_tables=True)
    want_planes, want_status = jpeg.decode_planes_host(data, progressive=sof2)
    assert status.tolist() == want_status.tolist() and all(a.tobytes() == b.tobytes() for a, b in zip(planes, want_planes))
    i = jpeg.info(stripped, progressive=sof2, default_tables=True)
    assert (i["h"], i["w"]) == tuple(jpeg.info(data, progressive=sof2)[k] for k in ("h", "w"))
    assert i["data_offset"] == jpeg.info(data, progressive=sof2)["data_offset"] + len(got) - len(data)


def test_the_annex_k_tables_are_the_encoders():
    """libjpeg's tables (from Pillow) are the ones the library's own encoder writes: one source for both directions."""
    own = DT.tables_before_sos(DT.sources()["own_420_35x50"][0])
    assert own == DT.annex_k()
    assert len(DT.annex_k_segment(DT.SLOTS)) == 420


def test_a_complete_stream_comes_back_byte_for_byte():
    complete = [n for n in NAMES if not missing_slots(DT.sources()[n][0])]
    assert len(complete) >= 10                          # (every colour baseline stream; grey and progressive ones miss slots as they stand)
    for name in complete:
        data, _ = DT.sources()[name]
        assert jpeg.add_default_tables(data) == data, name
        assert jpeg.add_default_tables(np.frombuffer(data, np.uint8)) == data


def test_an_optimised_stream_defines_all_four_and_comes_back_unchanged():
    data = DT.pillow_stream(35, 50, 2, optimize=True)
    assert missing_slots(data) == [] and DT.tables_before_sos(data) != DT.annex_k()
    assert jpeg.add_default_tables(data) == data
    # ... and an optimised table that stays is not replaced: only the missing slots are filled
    stripped = DT.strip(data, {(1, 1)})
    got = jpeg.add_default_tables(stripped)
    have = DT.tables_before_sos(got)
    assert have[(1, 1)] == DT.annex_k()[(1, 1)] and all(have[k] == DT.tables_before_sos(data)[k] for k in DT.SLOTS[:3])


def test_a_stream_missing_id_2_stays_refused():
    """A scan that names table id 2: the call fills 0 and 1 only and the decoder gives its own reason."""
    data = DT.strip(DT.pillow_stream(35, 50, 2), DT.STRIPS["all"])
    segs = DT.segments(data)
    m, a, b = segs[-1]
    sos = bytearray(data[a:b])
    sos[8] = 0x22                                       # component 2: Td = 2, Ta = 2
    bad = data[:a] + bytes(sos) + data[b:]
    got = jpeg.add_default_tables(bad)
    assert len(got) == len(bad) + 420 and set(DT.tables_before_sos(got)) == set(DT.SLOTS)
    for call in (lambda: jpeg.info(got), lambda: jpeg.decode_host(bad, default_tables=True), lambda: jpeg.info(got, progressive=True)):
        with pytest.raises(ValueError, match="Huffman table"):
            call()


def test_garbage_and_truncated_headers_come_back_unchanged():
    data = DT.strip(DT.pillow_stream(35, 50, 2), DT.STRIPS["all"])
    at = DT.sos_at(data)
    rng = np.random.default_rng(77)
    cases = [b"", b"\xff", b"\xff\xd8", b"\xff\xd8\xff", b"RIFF" + bytes(100), bytes(rng.integers(0, 256, 500, dtype=np.uint8)),
             data[:at], data[:at + 1], data[:at + 3], data[:at + 5], data[:40], b"\xff\xd8" + data[3:],
             data[:2] + b"\xff\xd9" + data[2:],                                  # EOI before SOS
             data[:2] + b"\xff\xc4\x00\x05\x00\x01\x02" + data[2:],              # a short DHT
             data[:2] + b"\xff\xc4\x00\x13\x20" + bytes(16) + data[2:],          # a DHT of class 2
             data[:2] + b"\xff\xe0\xff\xff" + data[2:]]                          # a segment that passes the end
    for c in cases:
        assert jpeg.add_default_tables(c) == c, c[:16]
    end = DT.segments(data)[-1][2]
    for cut in range(0, end):                           # every truncation of the header
        assert jpeg.add_default_tables(data[:cut]) == data[:cut], cut
    assert jpeg.add_default_tables(data[:end]) == data[:at] + DT.annex_k_segment(DT.SLOTS) + data[at:end]      # (the SOS header is whole)
    lib = _lib.load()                                   # NULL arguments and a small capacity are the only refusals
    import ctypes as C
    src, out, n = np.frombuffer(data, np.uint8), np.empty(len(data) + 420, np.uint8), C.c_int64(0)
    assert lib.whenet_jpeg_add_default_tables(src.ctypes.data, src.size, out.ctypes.data, out.size, C.byref(n)) == _lib.OK and n.value == len(data) + 420
    assert lib.whenet_jpeg_add_default_tables(src.ctypes.data, src.size, out.ctypes.data, out.size - 1, C.byref(n)) == _lib.EINVAL
    assert "capacity" in lib.whenet_last_error(None).decode()
    for args in ((None, src.size, out.ctypes.data, out.size, C.byref(n)), (src.ctypes.data, src.size, None, out.size, C.byref(n)),
                 (src.ctypes.data, src.size, out.ctypes.data, out.size, None)):
        assert lib.whenet_jpeg_add_default_tables(*args) == _lib.EINVAL


def test_without_the_argument_every_stripped_stream_is_refused_as_before():
    for name in NAMES:
        data, sof2 = DT.sources()[name]
        if sof2:
            continue
        stripped = DT.strip(data, DT.STRIPS["all"])
        for call in (lambda: jpeg.info(stripped), lambda: jpeg.decode_host(stripped), lambda: jpeg.decode_host(stripped, rule="libjpeg"),
                     lambda: jpeg.decode_planes_host(stripped), lambda: jpeg.info(stripped, default_tables=False)):
            with pytest.raises(ValueError, match=MISSING_TEXT):
                call()
    data, _ = DT.sources()["pil_prog_420_35x50"]
    with pytest.raises(ValueError, match="Huffman table"):
        jpeg.decode_host(DT.strip(data, DT.STRIPS["all"]), progressive=True)


def test_mjpg_reader_completes_the_frames_of_an_avi_without_dht(tmp_path):
    frames = [DT.pillow_stream(64, 48, 2), DT.pillow_stream(64, 48, 1), DT.pillow_stream(64, 48, 2, dri=1)]
    stripped = [DT.strip(f, DT.STRIPS["all"]) for f in frames]
    path = tmp_path / "camera.avi"
    with MJPGWriter(path, 30, (48, 64)) as out:
        for s in stripped:
            out.write(s)
    with MJPGReader(path) as src:                       # the default: the chunks as they are, refused by the decoder
        assert list(src) == stripped
        with pytest.raises(ValueError, match=MISSING_TEXT):
            jpeg.decode_host(src[0])
    with MJPGReader(path, default_tables=True) as src:
        assert len(src) == 3
        got = list(src)
        assert got == [jpeg.add_default_tables(s) for s in stripped] and src[1] == got[1]
        assert [c for clip in src.clips(2) for c in clip] == got
        for g, f in zip(got, frames):
            assert jpeg.decode_host(g).tobytes() == jpeg.decode_host(f).tobytes()


def test_host_check_program_runs_under_the_sanitizers(tmp_path):
    """tools/jpeg_default_tables_host_check.cpp (ASan + UBSan, its own main, CPU only): the function on every stream of the table, on
    the stripped copies and on cut and bit-flipped copies of each, the results through the decoder's header parsers.  It must give
    no report, and its checksum of every completed stream is the library's."""
    import os
    import shutil
    import subprocess
    import zlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_default_tables_host_check"
    src = os.path.join(root, "tools", "jpeg_default_tables_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    streams = {}
    for name in NAMES:
        data, _ = DT.sources()[name]
        streams[f"{name}.jpg"] = data
        for sname, drop in DT.STRIPS.items():
            streams[f"{name}.{sname}.jpg"] = DT.strip(data, drop)
    streams["garbage.jpg"] = bytes(np.random.default_rng(3).integers(0, 256, 700, dtype=np.uint8))
    streams["empty.jpg"] = b""
    for name, data in streams.items():
        (tmp_path / name).write_bytes(data)
    r = subprocess.run([str(exe)] + [str(tmp_path / n) for n in streams], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert set(lines) == set(streams)
    for name, data in streams.items():
        want = jpeg.add_default_tables(data)
        assert lines[name].startswith(f"{len(data)} -> {len(want)} ") and lines[name].endswith(f"crc {zlib.crc32(want):08x}"), (name, lines[name])
        baseline_ok = not DT.sources().get(name.split(".")[0], (b"", True))[1]
        assert ("accepted" in lines[name]) == baseline_ok, (name, lines[name])
