"""The segmented form of the JPEG decoder's entropy stage as its host emulation (csrc/jpeg_dec_seg_host.h through
whenet_jpeg_decode_segmented_host / whenet_jpeg_decode_segmented_planes_host): byte for byte what the host statement
(whenet_jpeg_decode_host) gives on every case of tests/jpeg_decode_cases.py, the damaged streams included, at segment sizes from 4
bytes up and sync windows from 2 segments up; on streams designed against the method; the saturating DC scan against a clamped running
sum; and the stand-alone sanitizer program.  No GPU."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_decode_cases as DC
from whenet_hip import _lib, jpeg

ROOT = DC.ROOT
SEG_BYTES = (4, 8, 64, 1024)
WINDOWS = (2, 5, 256)
NOISE_SEED = 0      # the first seed whose stream has a stuffed 0x00 as the first byte of a 4-byte segment (checked below)


def stream_of(name):
    return DC.DAMAGED[name]()[0] if name in DC.DAMAGED else DC.case(name)


def host(data):
    """(frame, status) of the host statement"""
    i = _lib.jpeg_parse(data)
    frame = np.empty((i.h, i.w, 3), np.uint8)
    status = _lib.jpeg_decode_host(data, jpeg.packed_surface(frame), True)
    return frame, status


def assert_equal_to_host(data, seg_bytes, window):
    want, want_status = host(data)
    got, status, stats = jpeg.decode_segmented_host(data, seg_bytes, window, stats=True)
    assert status.tolist() == want_status.tolist()
    assert np.array_equal(got, want)
    assert stats[6] == seg_bytes and stats[7] == 1
    return stats


def flat_stream(mode):
    """A flat picture, 256 x 256: every block is a DC difference of 0 and an EOB, a period of a few bits"""
    im = Image.new(mode, (256, 256), (90, 140, 200) if mode == "RGB" else 117)
    out = io.BytesIO()
    im.save(out, "JPEG", quality=90, **({"subsampling": 2} if mode == "RGB" else {}))
    return out.getvalue()


def noise_stream(seed):
    rng = np.random.default_rng(seed)
    out = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)).save(out, "JPEG", quality=100, subsampling=0)
    return out.getvalue()


# ---- 1. equality on the whole table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DC.CASE_NAMES + DC.DAMAGED_NAMES)
def test_segmented_host_equals_decode_host(name):
    data = stream_of(name)
    want, want_status = host(data)
    planes_want, _ = jpeg.decode_planes_host(data)
    for seg_bytes in SEG_BYTES:
        for window in WINDOWS:
            got, status, stats = jpeg.decode_segmented_host(data, seg_bytes, window, stats=True)
            assert status.tolist() == want_status.tolist(), (seg_bytes, window)
            assert np.array_equal(got, want), (seg_bytes, window)
            assert stats[6] == seg_bytes and stats[7] == 1
            i = jpeg.info(data)
            assert 1 <= stats[1] <= -(-(len(data) - i["data_offset"]) // seg_bytes) + i["intervals"]      # the host's bound
            assert stats[2] == -(-stats[1] // window) and stats[3] <= window
        planes, status, _ = jpeg.decode_segmented_planes_host(data, seg_bytes, 5)
        assert status.tolist() == want_status.tolist()
        for p, q in zip(planes, planes_want):
            assert np.array_equal(p, q)
    if name in DC.DAMAGED:
        with pytest.raises(jpeg.DecodeError) as err:
            jpeg.decode_segmented_host(data, 64)
        assert err.value.interval == DC.DAMAGED[name]()[1]


# ---- 2. designed streams --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["RGB", "L"])
def test_flat_pictures_whose_guessed_walks_stay_out_of_phase(mode):
    """1,030 and 771 bytes of entropy data with a period of 5 and 6 bits: a guessed walk keeps its distance to the true one for long
    (the grey stream needs 96 sync rounds for its 97 segments of 8 bytes).  Nothing about rounds is asserted: equality, and that the
    stream is cut into more than 100 segments -- at seg_bytes 8 for the colour stream; the grey one has 771 bytes, which is 97 segments
    of 8 bytes whatever its grey level (1,024 blocks of a 2-bit DC symbol and a 4-bit EOB), so it is held to the bound at seg_bytes 4."""
    data = flat_stream(mode)
    stats = assert_equal_to_host(data, 8, 256)
    if mode == "RGB":
        assert stats[1] > 100
    else:
        assert stats[1] == 97 and assert_equal_to_host(data, 4, 256)[1] > 100
    for seg_bytes, window in ((4, 2), (4, 256), (64, 5)):
        assert_equal_to_host(data, seg_bytes, window)


def stuffed_zero_at_a_segment_start(data, seg_bytes):
    off = jpeg.info(data)["data_offset"]
    ent = data[off:]
    return any(ent[p] == 0 and ent[p - 1] == 0xFF for p in range(seg_bytes, len(ent), seg_bytes))


def test_noise_at_quality_100_has_segments_without_a_code_word_start():
    seed = next(s for s in range(64) if stuffed_zero_at_a_segment_start(noise_stream(s), 4))
    assert seed == NOISE_SEED
    data = noise_stream(NOISE_SEED)
    assert stuffed_zero_at_a_segment_start(data, 4)
    for seg_bytes in (4, 8, 64):
        for window in WINDOWS:
            assert_equal_to_host(data, seg_bytes, window)


def test_damage_deep_inside_a_chain():
    """truncated_no_dri, and a byte flip in the middle of sample_001's entropy data: the segments behind the damage write nothing"""
    data = stream_of("truncated_no_dri")
    for seg_bytes in (4, 8, 64):
        assert_equal_to_host(data, seg_bytes, 256)
    good = DC.case("sample_001")
    off = jpeg.info(good)["data_offset"]
    at = off + (len(good) - off) // 2
    flipped = good[:at] + bytes([good[at] ^ 0x5A]) + good[at + 1:]
    want, status = host(flipped)
    for seg_bytes, window in ((8, 256), (64, 5), (128, 256)):
        assert_equal_to_host(flipped, seg_bytes, window)
    assert not np.array_equal(want, host(good)[0])


def test_a_buffer_that_continues_with_zeros_behind_eoi():
    """the device-to-device capacity case: nbytes is a buffer's capacity, zero-filled behind the stream"""
    data = DC.case("pil_420_50x70") + bytes(4096)
    want, status = host(data)
    assert status.tolist() == [_lib.OK, -1] and np.array_equal(want, host(DC.case("pil_420_50x70"))[0])
    for seg_bytes, window in ((4, 256), (64, 2), (1024, 5)):
        assert_equal_to_host(data, seg_bytes, window)


# ---- 3. the segmented path really ran -------------------------------------------------------------------------------------------
def test_the_statistics_show_segments_windows_and_the_stitch():
    data = DC.case("sample_001")
    assert len(data) - jpeg.info(data)["data_offset"] == 21376
    stats = assert_equal_to_host(data, 8, 256)
    assert stats[0] == 1 and stats[1] == 21376 // 8 and stats[2] >= 10 and stats[7] == 1
    assert stats[4] >= 1          # every later window's first segment starts from a guess: the stitch walked (the GPU test relies on it)
    assert stats[3] >= 1 and stats[5] >= 8


# ---- 4. the saturating DC scan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_dc_maps_compose_to_the_clamped_running_sum(seed):
    rng = np.random.default_rng(seed)
    n = 5000
    diff = rng.integers(-2047, 2048, n).astype(np.int32)
    diff[1000:1400] = 2047           # leaves +32767 ...
    diff[3000:3500] = -2047          # ... and -32768: a plain prefix sum is wrong behind these
    want = np.empty(n, np.int64)
    p = 0
    for i, d in enumerate(diff.tolist()):
        p = min(max(p + d, -32768), 32767)
        want[i] = p
    assert want.max() == 32767 and want.min() == -32768
    assert not np.array_equal(np.clip(np.cumsum(diff.astype(np.int64)), -32768, 32767), want)
    for chunk in (1, 7, 64, 4096, n + 1):
        assert np.array_equal(_lib.jpeg_seg_dc_scan_host(diff, chunk), want), chunk


# ---- 5. the sanitizer program ---------------------------------------------------------------------------------------------------
def test_seg_host_check_program_runs_the_table_under_the_sanitizers(tmp_path):
    """tools/jpeg_dec_seg_host_check.cpp: csrc/jpeg_dec_seg_host.h -- what the kernels of csrc/jpeg_dec_seg.hip share -- built
    stand-alone with -fsanitize=address,undefined and run on the table's streams and their cut and flipped copies."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_dec_seg_host_check"
    src = os.path.join(ROOT, "tools", "jpeg_dec_seg_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = DC.CASE_NAMES + DC.DAMAGED_NAMES
    for name in names:
        (tmp_path / f"{name}.jpg").write_bytes(stream_of(name))
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.jpg") for n in names], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "no report" in r.stderr
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    for name in DC.CASE_NAMES:
        assert lines[f"{name}.jpg"].startswith("status 0 -1 segments"), lines[f"{name}.jpg"]
    for name in DC.DAMAGED_NAMES:
        assert lines[f"{name}.jpg"].startswith(f"status {DC.EFORMAT} {DC.DAMAGED[name]()[1]} segments"), lines[f"{name}.jpg"]


# ---- 6. bindings and arguments --------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    lib = _lib.load()
    for s in ("whenet_jpeg_decode_segmented_host", "whenet_jpeg_decode_segmented_planes_host", "whenet_op_jpeg_decode_ex",
              "whenet_jpeg_decode_counters", "whenet_jpeg_seg_dc_scan_host"):
        assert s in _lib.EXPORTS and hasattr(lib, s)
    with open(os.path.join(ROOT, "include", "whenet_hip.h")) as f:
        text = f.read()
    assert "#define WHENET_ABI_VERSION 6" in text                       # additions only
    assert f"#define WHENET_JPEG_SEG_WINDOW {_lib.JPEG_SEG_WINDOW}" in text
    assert hasattr(_lib.Handle, "op_jpeg_decode_ex") and hasattr(_lib.Handle, "jpeg_decode_counters")


def test_bad_arguments_are_einval():
    lib = _lib.load()
    data = np.frombuffer(DC.case("pil_420_17x17"), np.uint8)
    status, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
    frame = np.zeros((17, 17, 3), np.uint8)
    s = jpeg.packed_surface(frame)

    def call(seg_bytes, window, d=data.ctypes.data, size=data.size, dst=s, st=status.ctypes.data):
        return lib.whenet_jpeg_decode_segmented_host(d, size, dst, _lib.BGR, seg_bytes, window, st, stats.ctypes.data)

    for seg_bytes in (0, 2, 3, 6, 100, 8192, -4):
        assert call(seg_bytes, 256) == _lib.EINVAL
        assert "seg_bytes" in lib.whenet_last_error(None).decode()
    for window in (0, -1, 1025):
        assert call(64, window) == _lib.EINVAL
        assert "window" in lib.whenet_last_error(None).decode()
    assert call(64, 256, d=None) == _lib.EINVAL
    assert call(64, 256, dst=None) == _lib.EINVAL
    assert call(64, 256, st=None) == _lib.EINVAL
    assert not frame.any()
    assert call(64, 256) == _lib.OK and frame.any()
    assert lib.whenet_jpeg_decode_segmented_host(data.ctypes.data, data.size, s, _lib.BGR, 64, 256, status.ctypes.data, None) == _lib.OK
    with pytest.raises(ValueError, match="entropy"):
        jpeg.decode(DC.case("pil_420_17x17"), entropy="both")
    assert lib.whenet_jpeg_seg_dc_scan_host(None, 4, 2, None) == _lib.EINVAL
    assert lib.whenet_jpeg_decode_counters(None, None) == _lib.EINVAL
