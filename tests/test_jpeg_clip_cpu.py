"""Clips of JPEG streams, the parts that need no GPU: the four entry points are declared, exported and bound; the plan
(`whenet_jpeg_clip_plan`, csrc/jpeg_dec_clip_host.h: the layout the engine uses) keeps what the kernels rely on; the plan's header
runs stand-alone under the host sanitizers; `MJPGReader.clips(n)` cuts a file into clips."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import jpeg_decode_cases as DC
from whenet_hip import _lib, frames, jpeg, mjpeg

ROOT = DC.ROOT
SYMBOLS = ("whenet_clip_begin_jpeg", "whenet_op_jpeg_decode_clip", "whenet_jpeg_clip_plan", "whenet_jpeg_clip_counters")
# 4:2:0, 4:2:2, 4:4:4 and grey, with and without DRI, 1 x 1 to 70 x 50, and two camera stills without DRI (auto: the segmented form)
SET = ["pil_420_50x70", "pil_422_50x70", "pil_444_q50", "pil_grey_50x70", "pil_420_rst_rows", "pil_444_rst_blocks3", "pil_420_1x1",
       "sample_001", "pil_grey_rst_blocks3", "pil_422_33x8", "pil_420_8x8", "sample_012", "own_17x17", "pil_grey_1x1", "pil_420_16x16",
       "pil_420_optimize"]
JPEG_DEC_TABLES_BYTES = 4 * (2 * 512 + 4 * 17 + 4 * 17 + 256) + 2 * 4 * 64 + 64      # JpegDecTables: four JpegDecHuff, q, zz


def parsed(names):
    datas = [DC.case(n) for n in names]
    infos = [_lib.jpeg_parse(d) for d in datas]
    return datas, infos, [len(d) - i.data_offset for d, i in zip(datas, infos)]


def test_the_four_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "whenet_hip.h")) as f:
        text = f.read()
    for s in SYMBOLS:
        assert f"WHENET_API int {s}(" in text and s in _lib.EXPORTS and hasattr(lib, s)
    assert "#define WHENET_ABI_VERSION 6" in text                       # additions only
    assert f"#define WHENET_JPEG_CLIP_PLAN_FRAME_WORDS {_lib.JPEG_CLIP_PLAN_FRAME_WORDS}" in text
    assert f"#define WHENET_JPEG_CLIP_PLAN_TOTAL_WORDS {_lib.JPEG_CLIP_PLAN_TOTAL_WORDS}" in text
    assert "clips of JPEG streams" not in text.split("Not built:")[-1].split("*/")[0]
    nm = shutil.which("nm")
    if nm is not None:                                                   # the library's own export list
        out = subprocess.run([nm, "-D", "--defined-only", _lib.load()._name], capture_output=True, text=True).stdout
        for s in SYMBOLS:
            assert f" T {s}\n" in out
    for name in ("clip_begin_jpeg", "op_jpeg_decode_clip", "jpeg_clip_counters"):
        assert hasattr(_lib.Handle, name)
    assert hasattr(frames.FramePipeline, "begin_clip_jpeg") and hasattr(jpeg, "decode_clip") and hasattr(mjpeg.MJPGReader, "clips")


def geometry(i):
    hs, vs = (i.hs, i.vs) if i.components == 3 else (1, 1)
    cols, rows = -(-i.w // (8 * hs)), -(-i.h // (8 * vs))
    bpm = hs * vs + 2 if i.components == 3 else 1
    mcus = cols * rows
    ri = i.restart_interval if 0 < i.restart_interval < mcus else mcus
    planes = [cols * 8 * hs * rows * 8 * vs] + [cols * 8 * rows * 8] * (i.components - 1) + [0] * (3 - i.components)
    return -(-mcus // ri), mcus * bpm, planes


def predicted_form(entropy, nbytes, intervals):
    return entropy if entropy != 2 else int(nbytes // max(intervals, 1) >= _lib.JPEG_SEG_AUTO_BYTES)


def check_plan(infos, nbytes, entropy, seg_bytes):
    plan = _lib.jpeg_clip_plan(infos, nbytes, entropy, seg_bytes)
    F = len(infos)
    assert len(plan["frames"]) == F
    regions = [("records", -1) + plan["records"]]
    for f, (fr, i, nb) in enumerate(zip(plan["frames"], infos, nbytes)):
        intervals, blocks, planes = geometry(i)
        assert intervals == i.intervals
        form = predicted_form(entropy, nb, intervals)                    # what jpeg_entropy / jpeg_seg_bytes give the stream alone
        assert fr["form"] == form and fr["seg_bytes"] == (seg_bytes if form else 0)
        cap = -(-nb // seg_bytes) + intervals if form else 0
        assert fr["seg_cap"] == cap
        # the lengths are those of the single-stream layout
        want = {"tables": JPEG_DEC_TABLES_BYTES, "data": nb, "start": 4 * intervals, "meta": 64, "seg_stats": 64, "coef": blocks * 128,
                "plane0": planes[0], "plane1": planes[1], "plane2": planes[2], "first_seg": 4 * (intervals + 1) if form else 0,
                "seg_exit": 8 * cap, "seg_count": 56 * cap, "seg_blk": 16 * cap}
        for name in _lib.JPEG_CLIP_REGIONS:
            off, length = fr[name]
            assert length == want[name], (f, name)
            if length:
                regions.append((name, f, off, length))
                # planes need 8 (one 8-byte store per block row), vector loads of the data and the int4 of seg_blk 16
                assert off % 256 == 0 or (name == "seg_stats" and off == fr["meta"][0] + 64), (f, name)
        z0, zn = plan["zero"]
        for name in ("start", "meta", "seg_stats", "coef"):
            assert z0 <= fr[name][0] and fr[name][0] + fr[name][1] <= z0 + zn
        for name in ("tables", "data"):
            assert fr[name][0] + fr[name][1] <= plan["upload_bytes"]
    assert plan["records"][0] == 0 and plan["records"][1] == 512 * F and plan["records"][1] <= plan["upload_bytes"] <= plan["zero"][0]
    assert plan["forms"] == (sum(fr["form"] == 0 for fr in plan["frames"]), sum(fr["form"] == 1 for fr in plan["frames"]))
    regions.sort(key=lambda r: r[2])
    for a, b in zip(regions, regions[1:]):
        assert a[2] + a[3] <= b[2], (a, b)                               # pairwise disjoint
    assert regions[-1][2] + regions[-1][3] <= plan["bytes"]              # inside the total
    return plan


@pytest.mark.parametrize("seg_bytes", [4, 128])
@pytest.mark.parametrize("entropy", [0, 1, 2])
def test_the_plan_of_mixed_clips(entropy, seg_bytes):
    datas, infos, nbytes = parsed(SET)
    for F in (1, 2, 3, 7, 16):
        for first in (0, 5):
            pick = [(first + k) % len(SET) for k in range(F)]
            check_plan([infos[k] for k in pick], [nbytes[k] for k in pick], entropy, seg_bytes)
    plan = check_plan(infos[::-1], nbytes[::-1], entropy, seg_bytes)
    if entropy == 2:                                                     # auto: the camera stills alone take the segmented form
        assert [fr["form"] for fr in plan["frames"]] == [int(n.startswith("sample_")) for n in SET[::-1]]


def test_a_one_frame_clip_has_the_single_stream_sizes():
    datas, infos, nbytes = parsed(SET)
    for i, nb in zip(infos, nbytes):
        for entropy, seg_bytes in itertools.product((0, 1), (8, 128)):
            plan = check_plan([i], [nb], entropy, seg_bytes)             # (the region lengths are checked there)
            fr = plan["frames"][0]
            # back to back, each rounded up to 256: the bytes of the single-stream buffer plus the one record
            sizes = [plan["records"][1]] + [fr[n][1] for n in ("tables", "data", "start")] + [128] + \
                    [fr[n][1] for n in ("coef", "plane0", "plane1", "plane2", "first_seg", "seg_exit", "seg_count", "seg_blk")]
            assert plan["bytes"] == sum(-(-s // 256) * 256 for s in sizes)


def test_the_plan_refuses_bad_arguments():
    datas, infos, nbytes = parsed(SET[:2])
    for kw in (dict(entropy=3), dict(entropy=-1), dict(seg_bytes=100), dict(seg_bytes=2), dict(seg_bytes=8192)):
        with pytest.raises(ValueError):
            _lib.jpeg_clip_plan(infos, nbytes, **kw)
    with pytest.raises(ValueError, match="1..16"):
        _lib.jpeg_clip_plan(infos * 9, nbytes * 9)
    with pytest.raises(ValueError, match="1..16"):
        _lib.jpeg_clip_plan([], [])
    with pytest.raises(ValueError, match="nbytes"):
        _lib.jpeg_clip_plan(infos, [nbytes[0], -1])
    bad = _lib.JpegInfoC.from_buffer_copy(bytes(infos[0]))
    bad.components = 4
    with pytest.raises(ValueError, match="frame 1"):
        _lib.jpeg_clip_plan([infos[0], bad], nbytes)
    lib = _lib.load()
    assert lib.whenet_jpeg_clip_plan(None, None, 1, 0, 128, None) == _lib.EINVAL
    assert lib.whenet_jpeg_clip_counters(None, None) == _lib.EINVAL


def test_the_python_layer_refuses_before_the_library_is_touched():
    good = DC.case("pil_420_17x17")
    for datas in ([], [good] * 17):
        with pytest.raises(ValueError, match="1..16"):
            jpeg.decode_clip(datas)
    with pytest.raises(ValueError, match="frame 2.*progressive"):
        jpeg.decode_clip([good, good, DC.REFUSED["progressive"](), good])
    with pytest.raises(ValueError, match="entropy"):
        jpeg.decode_clip([good], entropy="both")


def test_clip_host_check_program_runs_under_the_sanitizers(tmp_path):
    """tools/jpeg_dec_clip_host_check.cpp: csrc/jpeg_dec_clip_host.h built stand-alone with -fsanitize=address,undefined; every
    plan's regions are filled in a heap block of exactly the plan's size."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_dec_clip_host_check"
    src = os.path.join(ROOT, "tools", "jpeg_dec_clip_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in SET:
        (tmp_path / f"{name}.jpg").write_bytes(DC.case(name))
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.jpg") for n in SET], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "no report" in r.stderr
    words = r.stdout.split()
    plans = 16 * len(SET) * 9
    assert words[:2] == ["plans", str(plans)] and words[2:4] == ["frames", str(sum(range(1, 17)) * len(SET) * 9)]
    assert int(words[5]) + int(words[7]) == int(words[3]) and int(words[5]) > 0 and int(words[7]) > 0


@pytest.mark.parametrize("n", [1, 3, 16, 40])
def test_mjpg_reader_clips(tmp_path, n):
    path = str(tmp_path / "clip.avi")
    streams = [DC.own_stream(16, 16, 90, seed=k) for k in range(7)]
    with mjpeg.MJPGWriter(path, 25, (16, 16)) as out:
        for s in streams:
            out.write(s)
    with mjpeg.MJPGReader(path) as src:
        flat = list(src)
        clips = list(src.clips(n))
        assert flat == streams
        assert [d for c in clips for d in c] == flat                     # the concatenation is the file
        assert all(len(c) >= 1 for c in clips) and all(len(c) == n for c in clips[:-1]) and len(clips[-1]) == (len(flat) - 1) % n + 1
        assert len(clips) == -(-len(flat) // n)
        with pytest.raises(ValueError):
            next(src.clips(0))
