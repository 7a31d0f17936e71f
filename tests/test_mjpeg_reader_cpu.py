"""The MJPG / AVI reader: `MJPGReader` returns, in count and bytes, the frames `MJPGWriter` wrote, the library's decoder opens each of
them, and anything that is not a complete MJPG AVI is refused.  That it opens files OpenCV wrote is unpinned: OpenCV does not run next
to this code."""
import struct

import numpy as np
import pytest

from tests import jpeg_decode_cases as DC
from whenet_hip import jpeg
from whenet_hip.mjpeg import MJPGReader, MJPGWriter

H, W = 40, 48


@pytest.fixture(scope="module")
def frames():
    # streams of different lengths, odd and even ones (an odd chunk is followed by a pad byte)
    out = [DC.own_stream(H, W, quality, seed) for seed, quality in ((1, 95), (2, 50), (3, 75), (4, 60), (5, 30))]
    assert {len(f) & 1 for f in out} == {0, 1}, "the fixture needs an odd and an even stream length"
    return out


@pytest.fixture()
def avi(tmp_path, frames):
    path = tmp_path / "clip.avi"
    with MJPGWriter(str(path), 25, (W, H)) as out:
        for f in frames:
            out.write(f)
    return path


def test_reader_returns_what_the_writer_wrote(avi, frames):
    with MJPGReader(str(avi)) as src:
        assert len(src) == len(frames) and (src.width, src.height) == (W, H) and src.fps == 25
        got = list(src)
        assert got == frames                                   # count and bytes
        assert src[2] == frames[2] and src[-1] == frames[-1]
    with pytest.raises(ValueError, match="closed"):
        src[0]
    for data in got:                                           # ... and the decoder opens them
        frame = jpeg.decode_host(data)
        assert frame.shape == (H, W, 3) and np.array_equal(frame, DC.frame(DC.decode(data)))


def test_reader_finds_frames_inside_rec_lists_and_skips_other_chunks(tmp_path, frames):
    def chunk(fourcc, payload):
        return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")

    path = tmp_path / "plain.avi"
    with MJPGWriter(str(path), 30, (W, H)) as out:
        out.write(frames[0])
    data = path.read_bytes()
    movi_at = data.find(b"movi") - 8
    movi = b"movi" + chunk(b"JUNK", b"abc") + chunk(b"LIST", b"rec " + chunk(b"00dc", frames[1]) + chunk(b"01wb", b"\1\2\3\4")) + \
        chunk(b"01dc", frames[2]) + chunk(b"00dc", frames[0]) + chunk(b"00dc", b"")      # (01dc: another stream's frame, not this one's)
    body = data[12:movi_at] + chunk(b"LIST", movi)
    path.write_bytes(b"RIFF" + struct.pack("<I", 4 + len(body)) + b"AVI " + body)
    with MJPGReader(str(path)) as src:
        assert list(src) == [frames[1], frames[0]]              # an empty chunk is a dropped frame: no stream


def test_reader_refuses_what_is_no_mjpg_avi(tmp_path, avi):
    data = avi.read_bytes()
    cases = {
        "truncated": data[:len(data) // 2],
        "truncated_by_one": data[:-1],
        "short": data[:10],
        "not_riff": b"RIFX" + data[4:],
        "wave": data[:8] + b"WAVE" + data[12:],
        "other_codec": data.replace(b"MJPG", b"XVID"),
        "no_movi": data.replace(b"movi", b"mova"),
        "jpeg_file": DC.case("pil_420_17x17"),
    }
    for name, blob in cases.items():
        p = tmp_path / f"{name}.avi"
        p.write_bytes(blob)
        with pytest.raises(ValueError):
            MJPGReader(str(p))
    with pytest.raises(OSError):
        MJPGReader(str(tmp_path / "missing.avi"))
    with pytest.raises(ValueError, match="Motion-JPEG"):
        (tmp_path / "c.avi").write_bytes(cases["other_codec"])
        MJPGReader(str(tmp_path / "c.avi"))
