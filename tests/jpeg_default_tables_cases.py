"""Streams for the default-Huffman-table tests: Pillow (libjpeg-turbo) streams and the library's own, their copies with DHT
segments cut out as a UVC camera or an AVI writer leaves them out, and a marker walk in Python that shares no code with the library.

The Annex K tables are taken from executed libjpeg, not restated: a non-optimised Pillow stream carries exactly libjpeg's
std_huff_tables in its DHT segments (DC 0, AC 0, DC 1, AC 1), which is what `annex_k()` reads."""
import functools
import io

import numpy as np

SLOTS = ((0, 0), (1, 0), (0, 1), (1, 1))       # (class, id) in the order DC 0, AC 0, DC 1, AC 1


def picture(h, w, seed=5):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + seed), 128 + 90 * np.cos(yy / 5.0), (xx * 5 + yy * 3) % 256], axis=2)
    return np.clip(base + rng.normal(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pillow_stream(h, w, sub, dri=0, progressive=False, optimize=False, quality=85):
    """sub: 0 (4:4:4), 1 (4:2:2), 2 (4:2:0) or 'grey'; dri: restart interval in MCU rows (0: none)"""
    from PIL import Image
    im = Image.fromarray(picture(h, w))
    kw = dict(quality=quality, progressive=progressive, optimize=optimize)
    if dri:
        kw["restart_marker_rows"] = dri
    if sub == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = sub
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def segments(data):
    """[(marker, start, end)] of the marker segments from SOI up to and including the first SOS header (start: the 0xFF)."""
    assert data[:2] == b"\xff\xd8"
    out, p = [], 2
    while True:
        assert data[p] == 0xFF and data[p + 1] not in (0x00, 0xFF)
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, p + 2 + n))
        p += 2 + n
        if m == 0xDA:
            return out


def dht_tables(payload):
    """{(class, id): the table's bytes (its Tc/Th byte, 16 counts, symbols)} of one DHT segment's payload."""
    out, i = {}, 0
    while i < len(payload):
        n = 17 + sum(payload[i + 1:i + 17])
        out[(payload[i] >> 4, payload[i] & 15)] = bytes(payload[i:i + n])
        i += n
    assert i == len(payload)
    return out


def tables_before_sos(data):
    """{(class, id): bytes} of every table a DHT in front of the first SOS defines."""
    out = {}
    for m, a, b in segments(data):
        if m == 0xC4:
            out.update(dht_tables(data[a + 4:b]))
    return out


def strip(data, drop):
    """The stream without the tables `drop` ((class, id) pairs) in front of the first SOS: a DHT segment that loses every table is
    cut out whole, one that keeps some is rewritten with those."""
    out, last = [data[:2]], 2
    for m, a, b in segments(data):
        out.append(data[last:a])
        seg = data[a:b]
        if m == 0xC4:
            kept = b"".join(t for k, t in dht_tables(data[a + 4:b]).items() if k not in drop)
            seg = b"" if not kept else b"\xff\xc4" + (len(kept) + 2).to_bytes(2, "big") + kept
        out.append(seg)
        last = b
    out.append(data[last:])
    return b"".join(out)


STRIPS = {"all": frozenset(SLOTS), "ac": frozenset({(1, 0), (1, 1)}), "id1": frozenset({(0, 1), (1, 1)})}


@functools.lru_cache(maxsize=None)
def annex_k():
    """{(class, id): bytes}: libjpeg's std_huff_tables as a non-optimised Pillow stream carries them."""
    t = tables_before_sos(pillow_stream(16, 16, 2))
    assert set(t) == set(SLOTS) and [len(t[k]) for k in SLOTS] == [29, 179, 29, 179]
    return t


def annex_k_segment(missing):
    """The one DHT segment that holds the Annex K tables of the `missing` slots, in the order DC 0, AC 0, DC 1, AC 1."""
    body = b"".join(annex_k()[k] for k in SLOTS if k in missing)
    return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body


def sos_at(data):
    return segments(data)[-1][1]


# name -> (stream, SOF2?)
@functools.lru_cache(maxsize=None)
def sources():
    from whenet_hip import jpeg
    out = {}
    for sname, sub in (("444", 0), ("422", 1), ("420", 2), ("grey", "grey")):
        for dri in (0, 1):
            out[f"pil_{sname}_35x50" + ("_dri" if dri else "")] = (pillow_stream(35, 50, sub, dri), False)
    out["pil_420_64x48"] = (pillow_stream(64, 48, 2), False)
    out["pil_prog_420_35x50"] = (pillow_stream(35, 50, 2, progressive=True), True)
    out["pil_prog_444_64x48"] = (pillow_stream(64, 48, 0, progressive=True), True)
    for sampling in ("4:2:0", "4:2:2", "4:4:4"):
        out["own_" + sampling.replace(":", "") + "_35x50"] = (jpeg.encode_host(picture(35, 50)[..., ::-1].copy(), 90, sampling=sampling), False)
    return out
