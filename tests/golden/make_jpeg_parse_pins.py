"""Pins of the JPEG decoder's host code -> tests/golden/jpeg_parse_pins.json: what `whenet_jpeg_parse`, `whenet_jpeg_parse_scans`,
`whenet_jpeg_clip_plan` and `whenet_jpeg_clip_plan_progressive` answer for a sweep of damaged headers and bad arguments, and the
checksums tools/jpeg_dec_host_check.cpp and tools/jpeg_prog_host_check.cpp print of the decode tables and the scan plans.  The
fixture was written ONCE, by the commit before the two parsers, the two clip planners and their callers were folded into one
each; tests/test_jpeg_parse_pins_cpu.py recomputes every pin with the library in hand and compares.  The order in which a parser
checks defects decides which text a stream with two defects gets, and the small refusal tables of the other suites would not
see a changed order: this sweep reaches every header byte.

1. Parsers.  Four base streams (bases()); for each, every single-byte change at every header offset -- from 2 up to the first scan's
   data_offset, and for the progressive bases every byte outside the entropy data of any scan as well -- with the new value drawn
   from {b ^ 0x01, b ^ 0x10, 0x00, 0xFF}, and every truncation to 0 .. data_offset + 40 bytes.  Each input goes through both
   parsers.  The pin of one call is the exception's type and text, or the raw bytes of the info struct (and of the scan records).
   Stored: a SHA-256 (its first 64 bits) per (stream, function, kind, bucket of 16 offsets), so that a mismatch names where to
   look, and the sorted list of the distinct refusal texts reached, with their count (at least 40: digests of a sweep that only
   ever met "a marker is expected" would pin nothing).
2. Clip plans.  The words of both planners for clips of 1, 3 and 16 frames drawn from the bases (baseline ones for the first
   planner, all four for the second), entropy 0 / 1 / 2, seg_bytes 4 / 128 / 4096; and their answers to bad arguments alone and in
   pairs (frames 0 and 17, entropy -1 and 3, seg_bytes 3 and 8192, a negative nbytes, an info whose geometry gives no interval --
   the last one for the first planner only: the second takes streams, and no stream the parser accepts has such a geometry).
3. Decode tables.  The 64-bit FNV-1a checksum the two host-check programs print behind each accepted stream of their case tables
   (built here WITHOUT sanitizers: the checksums are what is compared, the sanitizer runs are the other suites').

    python tests/golden/make_jpeg_parse_pins.py          # writes the fixture: only ever at the commit whose answers are the reference
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
for p in (ROOT, os.path.join(ROOT, "headposeestimation-whenet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import jpeg_decode_cases as DC  # noqa: E402
from tests import jpeg_prog_cases as PC  # noqa: E402
from whenet_hip import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_parse_pins.json")
MIN_TEXTS = 40
DIGEST_HEX = 16      # of a SHA-256: 64 bits name a bucket as surely as the programs' 64-bit checksums name a table


def bases():
    """name -> stream: two baseline and two progressive ones."""
    return {
        "base_420_17x17_dri": DC.pillow_stream(17, 17, subsampling=2, restart_marker_blocks=3, seed=4),
        "base_grey_8x33": DC.pillow_stream(33, 8, mode="L"),
        "prog_420_17x17": PC.pillow_case("pil_420_17x17_q75_blocks3"),
        "prog_" + PC.CONSTRUCTED_NAMES[0]: PC.constructed(PC.CONSTRUCTED_NAMES[0]),
    }


# ---- 1. the parsers ---------------------------------------------------------------------------------------------------------------
def pin_parse(data):
    try:
        return bytes(_lib.jpeg_parse(data))
    except Exception as e:      # noqa: BLE001  (the type is part of the pin)
        return f"{type(e).__name__}: {e}".encode()


def pin_parse_scans(data):
    try:
        info, scans = _lib.jpeg_parse_scans(data)
        return bytes(info) + b"".join(bytes(s) for s in scans)
    except Exception as e:      # noqa: BLE001
        return f"{type(e).__name__}: {e}".encode()


PARSERS = {"jpeg_parse": pin_parse, "jpeg_parse_scans": pin_parse_scans}


def header_offsets(data):
    """(the offsets whose bytes are changed, the largest truncated length)."""
    info, scans = _lib.jpeg_parse_scans(data)
    offs = list(range(2, info.data_offset))
    if scans[0].progressive:
        entropy = set()
        for s in scans:
            entropy.update(range(s.data_offset, s.data_offset + s.data_bytes))
        offs += [o for o in range(info.data_offset, len(data)) if o not in entropy]
    return offs, info.data_offset + 40


def parser_pins():
    """({key: sha256}, the sorted distinct refusal texts)."""
    digests, texts = {}, set()

    def feed(key, pin):
        digests.setdefault(key, hashlib.sha256()).update(len(pin).to_bytes(4, "little") + pin)
        if pin.startswith(b"ValueError: jpeg_parse"):
            texts.add(pin.decode().split(": ", 2)[2])

    for name, data in bases().items():
        offs, longest = header_offsets(data)
        for fn, pin in PARSERS.items():
            for o in offs:
                b = data[o]
                for v in sorted({b ^ 0x01, b ^ 0x10, 0x00, 0xFF} - {b}):
                    m = bytearray(data)
                    m[o] = v
                    feed(f"{name}/{fn}/byte/{o // 16 * 16}", pin(bytes(m)))
            for n in range(0, min(longest, len(data)) + 1):
                feed(f"{name}/{fn}/cut/{n // 16 * 16}", pin(data[:n]))
    return {k: h.hexdigest()[:DIGEST_HEX] for k, h in digests.items()}, sorted(texts)


# ---- 2. the clip planners ---------------------------------------------------------------------------------------------------------
def raw_clip_plan(infos, nbytes, frames, entropy, seg_bytes):
    """whenet_jpeg_clip_plan as it stands: the words' bytes, or the refusal."""
    lib = _lib.load()
    arr = (_lib.JpegInfoC * max(len(infos), 1))(*infos)
    nb = np.ascontiguousarray(list(nbytes) + [0], np.int64)
    out = np.zeros(max(frames, 0) * _lib.JPEG_CLIP_PLAN_FRAME_WORDS + _lib.JPEG_CLIP_PLAN_TOTAL_WORDS, np.int64)
    rc = lib.whenet_jpeg_clip_plan(arr, nb.ctypes.data_as(C.c_void_p), frames, entropy, seg_bytes, out.ctypes.data_as(C.c_void_p))
    return out.tobytes() if rc == _lib.OK else f"{rc}: {lib.whenet_last_error(None).decode()}".encode()


def raw_clip_plan_progressive(datas, sizes, frames, entropy, seg_bytes):
    """whenet_jpeg_clip_plan_progressive as it stands (sizes: what is passed as the streams' sizes)."""
    lib = _lib.load()
    arrs = [np.frombuffer(d, np.uint8) for d in datas]
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    sz = np.ascontiguousarray(list(sizes) + [0], np.int64)
    out = np.zeros(max(frames, 0) * _lib.JPEG_CLIP_PROG_PLAN_FRAME_WORDS + _lib.JPEG_CLIP_PROG_PLAN_TOTAL_WORDS, np.int64)
    rc = lib.whenet_jpeg_clip_plan_progressive(ptrs, sz.ctypes.data_as(C.c_void_p), frames, entropy, seg_bytes, out.ctypes.data_as(C.c_void_p))
    return out.tobytes() if rc == _lib.OK else f"{rc}: {lib.whenet_last_error(None).decode()}".encode()


# the bad arguments, by the argument they spoil: two of one kind cannot be passed together
BAD = {"frames": (0, 17), "entropy": (-1, 3), "seg_bytes": (3, 8192), "nbytes": (-1,), "geometry": (0,)}


def clip_pins():
    """({key: sha256 of the words}, {key: refusal text})."""
    streams = list(bases().values())
    baseline = streams[:2]
    words, refusals = {}, {}
    for frames, entropy, seg_bytes in itertools.product((1, 3, 16), (0, 1, 2), (4, 128, 4096)):
        key = f"{frames}/{entropy}/{seg_bytes}"
        datas = [baseline[f % 2] for f in range(frames)]
        infos = [_lib.jpeg_parse(d) for d in datas]
        pin = raw_clip_plan(infos, [len(d) - i.data_offset for d, i in zip(datas, infos)], frames, entropy, seg_bytes)
        assert len(pin) == 8 * (frames * _lib.JPEG_CLIP_PLAN_FRAME_WORDS + _lib.JPEG_CLIP_PLAN_TOTAL_WORDS), pin[:80]
        words["jpeg_clip_plan/" + key] = hashlib.sha256(pin).hexdigest()[:DIGEST_HEX]
        datas = [streams[f % 4] for f in range(frames)]
        pin = raw_clip_plan_progressive(datas, [len(d) for d in datas], frames, entropy, seg_bytes)
        assert len(pin) == 8 * (frames * _lib.JPEG_CLIP_PROG_PLAN_FRAME_WORDS + _lib.JPEG_CLIP_PROG_PLAN_TOTAL_WORDS), pin[:80]
        words["jpeg_clip_plan_progressive/" + key] = hashlib.sha256(pin).hexdigest()[:DIGEST_HEX]
    singles = [(k, v) for k, vs in BAD.items() for v in vs]
    combos = [(s,) for s in singles] + [c for c in itertools.combinations(singles, 2) if c[0][0] != c[1][0]]
    for combo in combos:
        a = dict(frames=3, entropy=2, seg_bytes=128)
        a.update({k: v for k, v in combo if k in a})
        spoil = {k for k, _ in combo}
        key = ",".join(f"{k}={v}" for k, v in combo)
        n = max(a["frames"], 3)
        datas = [baseline[f % 2] for f in range(n)]
        infos = [_lib.jpeg_parse(d) for d in datas]
        nbytes = [len(d) - i.data_offset for d, i in zip(datas, infos)]
        if "nbytes" in spoil:
            nbytes[1] = -1
        if "geometry" in spoil:
            infos[1].intervals = 0
        refusals["jpeg_clip_plan/" + key] = raw_clip_plan(infos, nbytes, a["frames"], a["entropy"], a["seg_bytes"]).decode()
        if "geometry" in spoil:
            continue
        datas = [streams[f % 4] for f in range(n)]
        sizes = [len(d) for d in datas]
        if "nbytes" in spoil:
            sizes[1] = -1
        refusals["jpeg_clip_plan_progressive/" + key] = raw_clip_plan_progressive(datas, sizes, a["frames"], a["entropy"], a["seg_bytes"]).decode()
    return words, refusals


# ---- 3. the decode tables ---------------------------------------------------------------------------------------------------------
def tool_checksums():
    """{tool/stream: the checksum behind the stream's line}, both programs built without sanitizers and run on their case tables."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "a host C++ compiler (g++ or clang++) is needed"
    tables = {
        "jpeg_dec_host_check": ("tables", {n: DC.case(n) for n in DC.CASE_NAMES if not n.startswith("sample_")}),
        "jpeg_prog_host_check": ("plan", {n: PC.pillow_case(n) if n in PC.PILLOW else PC.constructed(n)
                                          for n in PC.PILLOW_NAMES + PC.CONSTRUCTED_NAMES}),
    }
    tables["jpeg_prog_host_check"][1].update(PC.DAMAGED)
    sums = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tool, (word, streams) in tables.items():
            exe = os.path.join(tmp, tool)
            r = subprocess.run([cxx, "-std=c++17", "-O2", os.path.join(ROOT, "tools", tool + ".cpp"), "-o", exe], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            paths = []
            for name, data in streams.items():
                paths.append(os.path.join(tmp, f"{tool}.{name}.jpg"))
                with open(paths[-1], "wb") as f:
                    f.write(data)
            # (the programs also decode cut and flipped copies of every stream: four processes share the files)
            runs = [subprocess.Popen([exe] + paths[i::4], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for i in range(4)]
            stdout = ""
            for r in runs:
                out, err = r.communicate()
                assert r.returncode == 0, out[-2000:] + err[-2000:]
                stdout += out
            for line in stdout.splitlines():
                if line.startswith("rule1:"):
                    continue
                name, rest = line.split(" ", 1)
                assert f" {word} " in rest, line
                sums[f"{tool}/{name[len(tool) + 1:-4]}"] = rest.rsplit(f" {word} ", 1)[1]
            assert len([k for k in sums if k.startswith(tool)]) == len(streams)
    return sums


def compute():
    digests, texts = parser_pins()
    assert len(texts) >= MIN_TEXTS, f"the sweep reaches {len(texts)} refusal texts"
    words, refusals = clip_pins()
    return {"parser_digests": digests, "refusal_texts": texts, "refusal_text_count": len(texts), "clip_plan_words": words,
            "clip_plan_refusals": refusals, "table_checksums": tool_checksums()}


def main():
    pins = compute()
    with open(OUT, "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{OUT}: {len(pins['parser_digests'])} parser digests, {pins['refusal_text_count']} refusal texts, "
          f"{len(pins['clip_plan_words'])} plans, {len(pins['clip_plan_refusals'])} plan refusals, "
          f"{len(pins['table_checksums'])} table checksums, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
