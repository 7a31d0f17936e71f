"""Progressive JPEG streams in clips, the parts that need no GPU: the three entry points are declared, exported and bound; the plan
(`whenet_jpeg_clip_plan_progressive`, csrc/jpeg_dec_clip_host.h: the layout the engine uses) keeps what the kernels rely on, and
for baseline streams alone it is `whenet_jpeg_clip_plan`'s; a refused stream names its frame and the scan parser's reason; the plan's
header runs stand-alone under the host sanitizers, staged and decoded the way the clip kernels walk it."""
import os
import shutil
import subprocess

import pytest

from tests import jpeg_decode_cases as DC
from tests import jpeg_prog_cases as PC
from whenet_hip import _lib, frames, jpeg

ROOT = DC.ROOT
SYMBOLS = ("whenet_op_jpeg_decode_clip_progressive", "whenet_clip_begin_jpeg_progressive", "whenet_jpeg_clip_plan_progressive")
# progressive: the four samplings, 1 x 1 to 64 x 48, without DRI, 3-block and row intervals, and two constructed scripts (14 levels,
# DRI changing between scans); baseline: twins of two of them, two small streams and a camera still (auto: the segmented form)
PROGRESSIVE = ["pil_420_17x17_q75_nodri", "pil_422_35x50_q75_blocks3", "pil_444_9x7_q75_nodri", "pil_grey_1x1_q75_nodri",
               "pil_420_64x48_q75_rows1", "pil_grey_35x50_q95_blocks3", "pil_444_64x48_q75_rows1", "pil_422_17x17_q30_nodri"]
CONSTRUCTED = ["levels14_420_17x17_ranked", "dri_changes_grey_9x7_fixed"]
BASELINE = ["pil_420_17x17", "pil_grey_rst_blocks3", "sample_001"]
JPEG_DEC_TABLES_BYTES = 4 * (2 * 512 + 4 * 17 + 4 * 17 + 256) + 2 * 4 * 64 + 64      # JpegDecTables (tests/test_jpeg_clip_cpu.py)
JPEG_DEC_HUFF_BYTES = 2 * 512 + 4 * 17 + 4 * 17 + 256
SCAN_BYTES, ITEM_BYTES = 4 * 21, 16                                                   # JpegProgScan, JpegProgItem


def table():
    """name -> stream, in an order that puts baseline frames between progressive ones"""
    t = {n: PC.pillow_case(n) for n in PROGRESSIVE}
    t.update({n: PC.constructed(n) for n in CONSTRUCTED})
    t.update({"twin_" + n: PC.pillow_twin(n) for n in PROGRESSIVE[:2]})
    t.update({n: DC.case(n) for n in BASELINE})
    names = sorted(t, key=lambda n: (len(n) * 7 + sum(map(ord, n))) % 13)
    return {n: t[n] for n in names}


def test_the_three_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "whenet_hip.h")) as f:
        text = f.read()
    for s in SYMBOLS:
        assert f"WHENET_API int {s}(" in text and s in _lib.EXPORTS and hasattr(lib, s)
    assert "#define WHENET_ABI_VERSION 6" in text                       # additions only
    assert f"#define WHENET_JPEG_CLIP_PROG_PLAN_FRAME_WORDS {_lib.JPEG_CLIP_PROG_PLAN_FRAME_WORDS}" in text
    assert f"#define WHENET_JPEG_CLIP_PROG_PLAN_TOTAL_WORDS {_lib.JPEG_CLIP_PROG_PLAN_TOTAL_WORDS}" in text
    assert f"#define WHENET_JPEG_CLIP_PLAN_FRAME_WORDS {_lib.JPEG_CLIP_PLAN_FRAME_WORDS}" in text     # the first plan's words stay
    for part in text.split("Not built:")[1:]:
        assert "progressive streams in clips" not in " ".join(part.split("*/")[0].split())
    nm = shutil.which("nm")
    if nm is not None:                                                   # the library's own export list
        out = subprocess.run([nm, "-D", "--defined-only", _lib.load()._name], capture_output=True, text=True).stdout
        for s in SYMBOLS:
            assert f" T {s}\n" in out
    for name in ("op_jpeg_decode_clip_progressive", "clip_begin_jpeg"):
        assert hasattr(_lib.Handle, name)
    import inspect
    assert inspect.signature(jpeg.decode_clip).parameters["progressive"].default is False
    assert inspect.signature(frames.FramePipeline.begin_clip_jpeg).parameters["progressive"].default is False
    assert inspect.signature(_lib.Handle.clip_begin_jpeg).parameters["progressive"].default is False


def geometry(i):
    hs, vs = (i.hs, i.vs) if i.components == 3 else (1, 1)
    cols, rows = -(-i.w // (8 * hs)), -(-i.h // (8 * vs))
    bpm = hs * vs + 2 if i.components == 3 else 1
    planes = [cols * 8 * hs * rows * 8 * vs] + [cols * 8 * rows * 8] * (i.components - 1) + [0] * (3 - i.components)
    return cols * rows * bpm, planes


def check_plan(datas, entropy, seg_bytes):
    plan = _lib.jpeg_clip_plan_progressive(datas, entropy, seg_bytes)
    F = len(datas)
    assert len(plan["frames"]) == F and plan["record_stride"] == 512 and 288 <= plan["prog_record_offset"] <= 512 - 184
    regions = [("records", -1) + plan["records"]]
    z0, zn = plan["zero"]
    levels, nprog = [], 0
    for f, (fr, data) in enumerate(zip(plan["frames"], datas)):
        i, scans = _lib.jpeg_parse_scans(data)
        blocks, planes = geometry(i)
        want = {"coef": blocks * 128, "plane0": planes[0], "plane1": planes[1], "plane2": planes[2], "meta": 64}
        if scans[0].progressive:
            nprog += 1
            assert fr["form"] == _lib.JPEG_CLIP_FORM_PROGRESSIVE and fr["seg_bytes"] == 0 and fr["seg_cap"] == 0
            lv = max(s.level for s in scans)
            levels.append(lv)
            assert fr["nscans"] == len(scans) and fr["levels"] == lv
            # the item list: a scan's share is its intervals (all of them: the streams of the table are undamaged), padded to 16
            assert fr["list"] == sum(-(-s.intervals // 16) * 16 for s in scans)
            end = scans[-1].data_offset + scans[-1].data_bytes
            want.update({"scans": SCAN_BYTES * len(scans), "huff": 3 * JPEG_DEC_HUFF_BYTES * len(scans), "qz": 3 * 64 * 2, "items": ITEM_BYTES * fr["list"],
                         "data": end - scans[0].data_offset, "raw": blocks * 128, "tables": 0, "start": 0, "seg_stats": 0, "first_seg": 0,
                         "seg_exit": 0, "seg_count": 0, "seg_blk": 0})
            zeroed, uploaded = ("meta", "raw"), ("scans", "huff", "qz", "items", "data")
            # scans | huff | qz | items | data, the content jpeg_prog_stage writes, in that order
            assert fr["scans"][0] < fr["huff"][0] < fr["qz"][0] < fr["items"][0] < fr["data"][0]
            assert fr["coef"][0] >= z0 + zn                                 # the finished records: work, written whole by the finish kernel
        else:
            nb = len(data) - i.data_offset
            form = entropy if entropy != 2 else int(nb // max(i.intervals, 1) >= _lib.JPEG_SEG_AUTO_BYTES)
            cap = -(-nb // seg_bytes) + i.intervals if form else 0
            assert (fr["form"], fr["seg_bytes"], fr["seg_cap"]) == (form, seg_bytes if form else 0, cap)
            assert (fr["nscans"], fr["levels"], fr["list"]) == (0, 0, 0)
            want.update({"tables": JPEG_DEC_TABLES_BYTES, "data": nb, "start": 4 * i.intervals, "seg_stats": 64,
                         "first_seg": 4 * (i.intervals + 1) if form else 0, "seg_exit": 8 * cap, "seg_count": 56 * cap, "seg_blk": 16 * cap,
                         "scans": 0, "huff": 0, "qz": 0, "items": 0, "raw": 0})
            zeroed, uploaded = ("start", "meta", "seg_stats", "coef"), ("tables", "data")
        for name in _lib.JPEG_CLIP_REGIONS + _lib.JPEG_CLIP_PROG_REGIONS:
            off, length = fr[name]
            assert length == want[name], (f, name)
            if length:
                regions.append((name, f, off, length))
                assert off % 256 == 0 or (name == "seg_stats" and off == fr["meta"][0] + 64), (f, name)
        for name in zeroed:                                                 # ONE memset covers them
            assert z0 <= fr[name][0] and fr[name][0] + fr[name][1] <= z0 + zn, (f, name)
        for name in uploaded:                                               # ONE copy covers them
            assert plan["records"][1] <= fr[name][0] and fr[name][0] + fr[name][1] <= plan["upload_bytes"], (f, name)
    assert plan["records"][0] == 0 and plan["records"][1] == 512 * F and plan["records"][1] <= plan["upload_bytes"] <= z0
    assert plan["upload_bytes"] % 256 == 0 and z0 % 256 == 0
    assert plan["progressive"] == nprog and plan["scan_launches"] == max(levels, default=0) <= 14
    assert plan["forms"] == (sum(fr["form"] == 0 for fr in plan["frames"]), sum(fr["form"] == 1 for fr in plan["frames"]))
    assert sum(plan["forms"]) + nprog == F
    regions.sort(key=lambda r: r[2])
    for a, b in zip(regions, regions[1:]):
        assert a[2] + a[3] <= b[2], (a, b)                               # pairwise disjoint
    assert regions[-1][2] + regions[-1][3] <= plan["bytes"]              # inside the total
    return plan


@pytest.mark.parametrize("entropy,seg_bytes", [(0, 128), (1, 16), (2, 128)])
def test_the_plan_of_mixed_clips(entropy, seg_bytes):
    t = table()
    names = list(t)
    assert len(names) == 15
    for F in (1, 2, 3, 7, 15):
        for first in (0, 4, 9):
            check_plan([t[names[(first + k) % len(names)]] for k in range(F)], entropy, seg_bytes)
    plan = check_plan([t[n] for n in names] + [t[names[0]]], entropy, seg_bytes)      # sixteen frames
    assert plan["progressive"] >= 10 and sum(plan["forms"]) >= 5
    assert plan["scan_launches"] == 14                                   # the 14-level script among 3-level ones: the largest, not the sum
    if entropy == 2:                                                     # auto: the camera still alone takes the segmented form
        assert plan["forms"][1] == 1


def test_a_clip_of_baseline_streams_gets_the_plan_it_always_got():
    names = ["pil_420_50x70", "pil_444_q50", "pil_grey_rst_blocks3", "sample_001", "pil_420_1x1", "pil_422_33x8"]
    datas = [DC.case(n) for n in names] + [PC.pillow_twin(n) for n in PROGRESSIVE[:3]]
    infos = [_lib.jpeg_parse(d) for d in datas]
    nbytes = [len(d) - i.data_offset for d, i in zip(datas, infos)]
    for entropy, seg_bytes in ((0, 128), (1, 4), (1, 128), (2, 8)):
        for pick in (range(len(datas)), [3], [0, 3, 8], list(range(len(datas))) + list(range(7))):
            old = _lib.jpeg_clip_plan([infos[k] for k in pick], [nbytes[k] for k in pick], entropy, seg_bytes)
            new = check_plan([datas[k] for k in pick], entropy, seg_bytes)
            for key in old:                                              # records, upload_bytes, zero, bytes, forms
                if key != "frames":
                    assert new[key] == old[key], key
            for a, b in zip(old["frames"], new["frames"]):               # region for region
                for key in a:
                    assert a[key] == b[key], key
            assert new["progressive"] == 0 and new["scan_launches"] == 0


def reason_of(data):
    """what jpeg.info(..., progressive=True) says of a refused stream, without the call's own name in front"""
    with pytest.raises(ValueError) as err:
        jpeg.info(data, progressive=True)
    text = str(err.value)
    return text.split("jpeg_parse_scans: ", 1)[1] if "jpeg_parse_scans: " in text else text


def test_refusals_name_the_frame_and_the_reason():
    good, base = PC.pillow_case(PROGRESSIVE[0]), DC.case("pil_420_17x17")
    for name, bad in PC.REFUSED.items():
        reason = reason_of(bad)
        assert len(reason) > 8, name
        with pytest.raises(ValueError) as err:
            _lib.jpeg_clip_plan_progressive([good, base, bad, good])
        assert f"frame 2: {reason}" in str(err.value), (name, str(err.value))
        # the Python layer refuses the same way before the library's clip calls are touched (no GPU is opened: handle=None is never reached)
        with pytest.raises(ValueError) as err:
            jpeg.decode_clip([good, base, bad, good], progressive=True)
        assert "frame 2" in str(err.value) and reason in str(err.value), (name, str(err.value))
    with pytest.raises(ValueError, match="frame 1.*not a JPEG"):
        _lib.jpeg_clip_plan_progressive([good, b"\x00" * 40])
    for kw in (dict(entropy=3), dict(entropy=-1), dict(seg_bytes=100), dict(seg_bytes=2)):
        with pytest.raises(ValueError):
            _lib.jpeg_clip_plan_progressive([good, base], **kw)
    with pytest.raises(ValueError, match="1..16"):
        _lib.jpeg_clip_plan_progressive([good] * 17)
    with pytest.raises(ValueError, match="1..16"):
        _lib.jpeg_clip_plan_progressive([])
    assert _lib.load().whenet_jpeg_clip_plan_progressive(None, None, 1, 0, 128, None) == _lib.EINVAL


def test_without_the_flag_a_clip_still_refuses_a_progressive_stream():
    good, prog = DC.case("pil_420_17x17"), PC.pillow_case(PROGRESSIVE[0])
    with pytest.raises(ValueError, match="frame 2.*progressive"):
        jpeg.decode_clip([good, good, prog, good])
    with pytest.raises(ValueError, match="frame 0.*progressive"):
        jpeg.decode_clip([prog], progressive=False)


def test_clip_host_check_program_runs_under_the_sanitizers(tmp_path):
    """tools/jpeg_prog_clip_host_check.cpp: the host headers built stand-alone with -fsanitize=address,undefined; clips of 1, 3 and
    16 of the table's streams and of their cut and bit-flipped copies are planned, staged into a heap block of exactly upload_bytes
    and decoded from a block of exactly the plan's bytes in the clip kernels' order; the result is the host statement's."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    exe = tmp_path / "jpeg_prog_clip_host_check"
    src = os.path.join(ROOT, "tools", "jpeg_prog_clip_host_check.cpp")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t = table()
    del t["sample_001"]                                                  # (21 KB under the sanitizers in every clip: the small streams say the same)
    for name, data in t.items():
        (tmp_path / f"{name}.jpg").write_bytes(data)
    r = subprocess.run([str(exe)] + [str(tmp_path / f"{n}.jpg") for n in t], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "no report" in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    words = r.stdout.split()
    assert words[0::2] == ["plans", "frames", "progressive", "baseline", "launches", "variants"]
    plans, nframes, prog, base, launches, variants = (int(w) for w in words[1::2])
    streams = len(t) + variants
    assert variants >= len(t)                                            # most cut and flipped copies still parse
    assert plans == 3 * 3 * streams and nframes == (1 + 3 + 16) * 3 * streams and prog + base == nframes and prog > base > 0
    assert 0 < launches <= 14 * plans
