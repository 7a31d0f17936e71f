"""A Motion-JPEG AVI writer in pure Python: the file the reference's video loop produces through OpenCV.

demo_video.py:46-47 opens `cv2.VideoWriter(args.output, cv2.VideoWriter_fourcc(*'MJPG'), 30, (frame_width, frame_height))` and
demo_video.py:60 hands it every annotated frame.  With the library's JPEG encoder (`whenet_hip.jpeg`, `FramePipeline`) the frame is
compressed where it lies; what is left of the writer is the container:

    with MJPGWriter("out.avi", 30, (w, h)) as out:
        out.write(jpeg_bytes)            # one complete JPEG stream per frame

THE FILE.  RIFF 'AVI ' with
    LIST 'hdrl':  'avih' (MainAVIHeader, 56 bytes: microseconds per frame, AVIF_HASINDEX, frame count, one stream, width, height)
                  LIST 'strl':  'strh' (AVIStreamHeader, 56 bytes: 'vids' / 'MJPG', scale and rate = the frame rate, length)
                                'strf' (BITMAPINFOHEADER, 40 bytes: 24 bits, biCompression 'MJPG')
    LIST 'movi':  one '00dc' chunk per frame, padded to an even length (the pad byte is not part of the chunk's size)
    'idx1':       one 16-byte entry per frame: '00dc', AVIIF_KEYFRAME, the chunk's offset from the 'movi' fourcc, its size
Sizes and counts are patched on close(); all integers little-endian.  Files are limited to the 4 GiB of a RIFF size field.

PINNED: the test suite walks the file chunk by chunk and Pillow decodes every frame.  UNPINNED: that OpenCV or a player opens the
file -- neither has run next to this code -- and no claim is made to reproduce the bytes OpenCV's own MJPG writer emits.
"""
from __future__ import annotations

import struct
from fractions import Fraction

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10


class MJPGWriter:
    """`MJPGWriter(path, fps, (w, h))`: `write(jpeg_bytes)` appends a frame, `close()` writes the index and patches the sizes."""

    def __init__(self, path, fps, size):
        w, h = int(size[0]), int(size[1])
        if w < 1 or h < 1:
            raise ValueError(f"frame size must be positive, got {w} x {h}")
        rate = Fraction(fps).limit_denominator(100000)
        if rate <= 0:
            raise ValueError(f"fps must be positive, got {fps}")
        self.width, self.height = w, h
        self._rate, self._scale = rate.numerator, rate.denominator
        self._index = []          # (offset from the 'movi' fourcc, size) of every chunk
        self._largest = 0
        self._f = open(path, "wb")
        self._f.write(self._headers(with_index=False))
        self._movi = self._f.tell() - 4      # where the 'movi' fourcc stands

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def frames(self) -> int:
        return len(self._index)

    def _headers(self, with_index: bool) -> bytes:
        n, w, h = len(self._index), self.width, self.height
        usec = round(1_000_000 * self._scale / self._rate)
        avih = struct.pack("<14I", usec, 0, 0, AVIF_HASINDEX, n, 0, 1, self._largest, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self._scale, self._rate, 0, n, self._largest, 0xFFFFFFFF, 0,
                           0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
        hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", strl)
        movi_bytes = 4 + sum(8 + size + (size & 1) for _, size in self._index)
        riff_bytes = 4 + 8 + len(hdrl) + 8 + movi_bytes + (8 + 16 * n if with_index else 0)
        return b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + _chunk(b"LIST", hdrl) + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"

    def write(self, jpeg_bytes) -> None:
        data = bytes(jpeg_bytes)
        if self._f is None:
            raise ValueError("write() on a closed MJPGWriter")
        if data[:2] != b"\xff\xd8" or data[-2:] != b"\xff\xd9":
            raise ValueError("a frame must be one complete JPEG stream (SOI .. EOI)")
        off = self._f.tell() - self._movi
        if self._f.tell() + 8 + len(data) + 1 + 8 + 16 * (len(self._index) + 1) > 0xFFFFFFFF:
            raise ValueError("the file would pass the 4 GiB of a RIFF size field")
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b""))
        self._index.append((off, len(data)))
        self._largest = max(self._largest, len(data))

    def close(self) -> None:
        if self._f is None:
            return
        f, self._f = self._f, None
        try:
            idx = b"".join(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, size) for off, size in self._index)
            f.write(_chunk(b"idx1", idx))
            f.seek(0)
            f.write(self._headers(with_index=True))
        finally:
            f.close()


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
