"""The MJPG / AVI writer: three frames written by `MJPGWriter` are walked back chunk by chunk by a RIFF reader of the test's own and
decoded by executed Pillow.  That OpenCV or a player opens the file is unpinned: neither runs next to this code."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_cases as JC
from whenet_hip import jpeg
from whenet_hip.mjpeg import MJPGWriter

H, W = 40, 48


def riff_chunks(data, start, end):
    """[(fourcc, list type or None, payload offset, payload size)] of the chunks between start and end; every chunk starts on a word"""
    out, pos = [], start
    while pos < end:
        fourcc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        assert pos + 8 + size <= end, f"chunk {fourcc} runs past its parent"
        kind = data[pos + 8:pos + 12] if fourcc in (b"RIFF", b"LIST") else None
        out.append((fourcc, kind, pos + 8, size))
        pos += 8 + size + (size & 1)
    assert pos == end or pos == end + 1
    return out


@pytest.fixture(scope="module")
def frames():
    # three streams of different lengths, at least one of them odd
    out = [jpeg.encode_host(JC.smooth(H, W, seed), quality) for seed, quality in ((1, 95), (2, 50), (3, 75), (4, 60))]
    odd = [f for f in out if len(f) & 1]
    even = [f for f in out if not len(f) & 1]
    assert odd and even, "the fixture needs an odd and an even stream length"
    return [odd[0], even[0], (odd + even)[-1]]


def test_avi_file_walks_back_and_decodes(tmp_path, frames):
    path = tmp_path / "out.avi"
    with MJPGWriter(str(path), 30, (W, H)) as out:
        for f in frames:
            out.write(f)
        assert out.frames == 3
    data = path.read_bytes()
    (riff, kind, at, size), = riff_chunks(data, 0, len(data))
    assert riff == b"RIFF" and kind == b"AVI " and size == len(data) - 8
    top = riff_chunks(data, at + 4, at + size)
    assert [(c[0], c[1]) for c in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    # hdrl: avih + one strl (strh vids / MJPG, strf BITMAPINFOHEADER with biCompression MJPG)
    hdrl = riff_chunks(data, top[0][2] + 4, top[0][2] + top[0][3])
    assert [(c[0], c[1]) for c in hdrl] == [(b"avih", None), (b"LIST", b"strl")]
    avih = struct.unpack("<14I", data[hdrl[0][2]:hdrl[0][2] + hdrl[0][3]])
    assert avih[0] == 33333 and avih[3] & 0x10 and avih[4] == 3 and avih[6] == 1 and avih[7] == max(map(len, frames))
    assert (avih[8], avih[9]) == (W, H)
    strl = riff_chunks(data, hdrl[1][2] + 4, hdrl[1][2] + hdrl[1][3])
    assert [c[0] for c in strl] == [b"strh", b"strf"] and strl[0][3] == 56 and strl[1][3] == 40
    strh = struct.unpack("<4s4sIHHIIIIIIII4H", data[strl[0][2]:strl[0][2] + 56])
    assert strh[0] == b"vids" and strh[1] == b"MJPG" and strh[7] / strh[6] == 30 and strh[9] == 3 and strh[-2:] == (W, H)
    strf = struct.unpack("<IiiHH4sIiiII", data[strl[1][2]:strl[1][2] + 40])
    assert strf[:6] == (40, W, H, 1, 24, b"MJPG")
    # movi: one 00dc chunk per frame, word aligned, the odd one padded with a byte that its size does not count
    movi_fourcc = top[1][2]
    movi = riff_chunks(data, movi_fourcc + 4, movi_fourcc + top[1][3])
    assert [c[0] for c in movi] == [b"00dc"] * 3
    for (_, _, off, size), want in zip(movi, frames):
        assert off % 2 == 0 and data[off:off + size] == want
        if size & 1:
            assert data[off + size] == 0
        im = Image.open(io.BytesIO(data[off:off + size]))
        im.load()
        assert im.format == "JPEG" and im.size == (W, H)
    assert any(c[3] & 1 for c in movi)
    # idx1: an entry per frame, its offset counted from the 'movi' fourcc and pointing at the chunk's header
    idx = data[top[2][2]:top[2][2] + top[2][3]]
    assert len(idx) == 16 * 3
    for i, (_, _, off, size) in enumerate(movi):
        ckid, flags, rel, n = struct.unpack("<4sIII", idx[16 * i:16 * i + 16])
        assert ckid == b"00dc" and flags & 0x10 and n == size and movi_fourcc + rel == off - 8
        assert data[movi_fourcc + rel:movi_fourcc + rel + 4] == b"00dc"


def test_writer_rules(tmp_path, frames):
    out = MJPGWriter(str(tmp_path / "a.avi"), 29.97, (W, H))
    with pytest.raises(ValueError):
        out.write(b"not a jpeg")
    out.write(frames[0])
    out.close()
    out.close()                                  # a second close is nothing
    with pytest.raises(ValueError):
        out.write(frames[0])
    data = (tmp_path / "a.avi").read_bytes()
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    at = data.index(b"strh") + 8
    scale, rate = struct.unpack("<II", data[at + 20:at + 28])
    assert abs(rate / scale - 29.97) < 1e-9
    with pytest.raises(ValueError):
        MJPGWriter(str(tmp_path / "b.avi"), 30, (0, H))
    with pytest.raises(ValueError):
        MJPGWriter(str(tmp_path / "b.avi"), 0, (W, H))
