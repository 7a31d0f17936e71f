"""EXIF orientation: hand-built APP1 segments, the numpy statement of the eight values, and the picture table of the oriented-decode tests.

A test stream is a Pillow stream (tests/jpeg_prog_cases.pillow_stream: the progressive one, or its baseline twin with the same quantised
coefficients) with a hand-built APP1 spliced in behind SOI or behind APP0.  The segments are built with `struct`, byte by byte, and share
no code with csrc/jpeg_dec_host.h (jpeg_exif_orientation); Pillow itself only writes big-endian EXIF.

    tiff(value, ...) -> bytes           # a TIFF header + IFD0 (+ IFD1) that holds the orientation entry in the form asked for
    exif_app1(tiff_bytes) / xmp_app1()  # the marker segments
    splice(stream, segment, where)      # behind SOI ("soi") or behind the stream's first segment ("app0")
    transform(u, value)                 # the oriented frame of the upright frame u: the EXIF standard's table
    SEGMENTS: name -> (list of segments, where, the value jpeg_exif_orientation must return)
    PICTURES: name -> (h, w, sub, pillow keywords)
"""
import functools
import struct

import numpy as np

from tests import jpeg_prog_cases as PC

ORIENTATION = 0x0112


def transform(u, value):
    """with t = u.transpose(1, 0, 2): the table of include/whenet_hip.h (JPEG DECODER, ORIENTATION)"""
    t = u.transpose(1, 0, 2)
    return np.ascontiguousarray({1: u, 2: u[:, ::-1], 3: u[::-1, ::-1], 4: u[::-1], 5: t, 6: t[:, ::-1], 7: t[::-1, ::-1], 8: t[::-1]}[value])


def _entry(e, tag, typ, count, value):
    """a 12-byte IFD entry whose value lies in the value field: type 1 BYTE, 3 SHORT, 4 LONG"""
    if typ == 3:
        field = struct.pack(e + "HH", value, value if count > 1 else 0)
    elif typ == 4:
        field = struct.pack(e + "I", value)
    else:
        field = bytes([value & 255, 0, 0, 0])
    return struct.pack(e + "HHI", tag, typ, count) + field


def tiff(value, order="MM", typ=3, count=1, position=0, magic=42, ifd_offset=8, pad=None, claimed=None, in_ifd1=False):
    """The TIFF block behind "Exif\\0\\0".  The orientation entry is entry `position` of IFD0 (ImageWidth / ImageLength entries in
    front of it), or, in_ifd1, the only entry of IFD1 behind an IFD0 without it.  ifd_offset / pad: where the header says IFD0 lies
    and how many bytes really lie between the header and it (None: ifd_offset - 8).  claimed: the entry count IFD0 states."""
    e = "<" if order == "II" else ">"
    out = (b"II" if order == "II" else b"MM") + struct.pack(e + "HI", magic, ifd_offset)
    out += b"\0" * (ifd_offset - 8 if pad is None else pad)
    fill = [_entry(e, 0x0100 + k, 3, 1, 16 + k) for k in range(position)]
    if in_ifd1:
        ifd0 = [_entry(e, 0x0100, 3, 1, 16)]
        next_ifd = len(out) + 2 + 12 * len(ifd0) + 4
        out += struct.pack(e + "H", len(ifd0)) + b"".join(ifd0) + struct.pack(e + "I", next_ifd)
        return out + struct.pack(e + "H", 1) + _entry(e, ORIENTATION, typ, count, value) + struct.pack(e + "I", 0)
    entries = fill + [_entry(e, ORIENTATION, typ, count, value)]
    return out + struct.pack(e + "H", len(entries) if claimed is None else claimed) + b"".join(entries) + struct.pack(e + "I", 0)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def exif_app1(tiff_bytes):
    return _segment(0xE1, b"Exif\0\0" + tiff_bytes)


def xmp_app1():
    return _segment(0xE1, b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta xmlns:x='adobe:ns:meta/'/>")


def splice(stream, segments, where="app0"):
    """the stream with the segments behind SOI, or behind its first segment (Pillow writes APP0 there)"""
    stream = bytes(stream)
    assert stream[:2] == b"\xff\xd8" and stream[2] == 0xFF
    at = 2
    if where == "app0":
        assert stream[3] == 0xE0
        at = 4 + ((stream[4] << 8) | stream[5])
    return stream[:at] + b"".join(segments) + stream[at:]


def oriented(stream, value, where="app0", **kw):
    """the stream with a well-formed Exif APP1 of that value"""
    return splice(stream, [exif_app1(tiff(value, **kw))], where)


def _segments():
    """name -> (segments, where, expected).  The first block is the list the oriented frame was compared with Pillow on (section 1 of
    the feature's statement); the second block is malformed or out of scope and yields 1."""
    t = {}
    for v in range(10):
        t[f"mm_short_{v}"] = ([exif_app1(tiff(v))], "app0", v if 1 <= v <= 8 else 1)
    for v in (1, 3, 6, 8):
        t[f"ii_short_{v}"] = ([exif_app1(tiff(v, order="II"))], "app0", v)
        t[f"mm_long_{v}"] = ([exif_app1(tiff(v, typ=4))], "app0", v)
        t[f"ii_long_{v}"] = ([exif_app1(tiff(v, order="II", typ=4))], "app0", v)
    t["third_entry_6"] = ([exif_app1(tiff(6, position=2))], "app0", 6)
    t["third_entry_ii_5"] = ([exif_app1(tiff(5, position=2, order="II"))], "app0", 5)
    t["in_front_of_app0_8"] = ([exif_app1(tiff(8))], "soi", 8)
    t["xmp_in_front_3"] = ([xmp_app1(), exif_app1(tiff(3))], "app0", 3)
    t["two_exif_first_wins_6"] = ([exif_app1(tiff(6)), exif_app1(tiff(3))], "app0", 6)
    t["two_exif_first_is_1"] = ([exif_app1(tiff(1)), exif_app1(tiff(6))], "app0", 1)
    t["ifd0_behind_a_gap_7"] = ([exif_app1(tiff(7, ifd_offset=20))], "app0", 7)
    t["long_value_above_8"] = ([exif_app1(tiff(0x00060000, typ=4))], "app0", 1)
    well = dict(t)
    # ---- all of these give 1 ----
    t["no_app1"] = ([], "app0", 1)
    t["xmp_only"] = ([xmp_app1()], "app0", 1)
    t["count_2"] = ([exif_app1(tiff(6, count=2))], "app0", 1)
    t["type_byte"] = ([exif_app1(tiff(6, typ=1))], "app0", 1)
    t["bad_magic"] = ([exif_app1(tiff(6, magic=43))], "app0", 1)
    t["bad_byte_order"] = ([exif_app1(b"IM" + tiff(6)[2:])], "app0", 1)
    t["ifd_offset_outside"] = ([exif_app1(tiff(6, ifd_offset=1000, pad=0))], "app0", 1)
    t["ifd_offset_at_the_end"] = ([exif_app1(tiff(6)[:8])], "app0", 1)
    t["entry_count_overruns"] = ([exif_app1(tiff(6, claimed=200))], "app0", 1)
    t["cut_inside_the_entry"] = ([exif_app1(tiff(6)[:8 + 2 + 9])], "app0", 1)
    t["cut_inside_the_header"] = ([exif_app1(tiff(6)[:5])], "app0", 1)
    t["only_in_ifd1"] = ([exif_app1(tiff(6, in_ifd1=True))], "app0", 1)
    t["exif_without_tiff"] = ([_segment(0xE1, b"Exif\0\0")], "app0", 1)
    t["short_app1"] = ([_segment(0xE1, b"Exi")], "app0", 1)
    return t, list(well)


SEGMENTS, WELL_FORMED = _segments()
MALFORMED = [n for n in SEGMENTS if n not in WELL_FORMED]

# ---- pictures: (h, w, sub, pillow keywords); names say w x h as the rest of the tests do ----
_SIZES = [(1, 1), (7, 1), (1, 7), (7, 9), (35, 17), (65, 33), (48, 64)]      # (h, w): 1x1, 1x7, 7x1, 9x7, 17x35, 33x65, 64x48


def _pictures():
    t = {}
    for h, w in _SIZES:
        for sn, sub in PC.SUBS.items():
            t[f"{sn}_{w}x{h}"] = (h, w, sub, {})
    t["422_35x50_blocks3"] = (50, 35, 1, {"restart_marker_blocks": 3})
    t["420_4x9_cw2"] = (9, 4, 2, {})       # chroma width 2: rule 1's replication branch (with the w = 1 pictures, whose chroma width is 1)
    t["422_3x5_cw2"] = (5, 3, 1, {})
    t["420_48x64"] = (64, 48, 2, {})       # 64 x 48 after a quarter turn
    return t


PICTURES = _pictures()
PICTURE_NAMES = list(PICTURES)
VALUES = list(range(1, 9))


@functools.lru_cache(maxsize=None)
def stream(name, progressive=False):
    """the untagged Pillow stream of a picture at quality 75: baseline (optimize=True), or its progressive twin"""
    h, w, sub, kw = PICTURES[name]
    return PC.pillow_stream(h, w, sub, 75, progressive=progressive, **kw)


def tagged(name, value, progressive=False, **kw):
    return oriented(stream(name, progressive), value, **kw)


def baseline_cut(name="422_35x50_blocks3"):
    """a baseline stream cut in the middle of its entropy data (a damaged stream: the intervals behind the cut are bad)"""
    d = stream(name)
    sos = d.index(b"\xff\xda")
    return d[:(sos + len(d)) // 2]
