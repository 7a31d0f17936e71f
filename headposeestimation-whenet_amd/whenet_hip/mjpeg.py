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

`MJPGReader(path)` is the other direction: it walks the same tree and yields every '00dc' chunk's bytes (demo_video.py:49-53,
`cap.read()` of such a file), for `FramePipeline.begin_jpeg` or `whenet_hip.jpeg.decode`.

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


class MJPGReader:
    """`MJPGReader(path)`: the frames of a Motion-JPEG AVI as bytes, one complete JPEG stream each -- what `cap.read()`
    (demo_video.py:49-53) decodes on the host, ready for `FramePipeline.begin_jpeg` / `whenet_hip.jpeg.decode`.

        with MJPGReader("in.avi") as src:
            for data in src: fp.begin_jpeg(data); ...

    Pure Python: it walks the RIFF tree ('RIFF' 'AVI ' > LIST 'hdrl' > 'avih', LIST 'strl' > 'strh' / 'strf'; LIST 'movi' > the 'NNdc'
    chunks of the first video stream, also inside 'rec ' lists) and keeps every video chunk's position; `width`, `height`, `fps`, `len()`, indexing and
    iteration read from those.  The index chunk is not needed.  ValueError for anything that is not an MJPG AVI: no RIFF / 'AVI '
    header, a video stream whose handler and compression are not MJPG, no 'movi' list, a chunk that passes the end of the file
    (a truncated file).

    `MJPGReader(path, default_tables=True)`: UVC cameras and many AVI writers leave the DHT segment out of every frame (the tables
    are T.81's Annex K ones); indexing, iteration and `clips()` then return every frame completed by
    `whenet_hip.jpeg.add_default_tables`.  The default returns the chunks' bytes as they are.

    `MJPGReader(path, layouts=True)`: the file's frames may be 4:1:1 / 4:1:0 / 4:4:0 streams (DV-derived cameras, grabbers, old
    webcams).  The bytes are returned as they are; `layouts` is what `info(i)` passes to `whenet_hip.jpeg.info` and what a caller
    passes on to `jpeg.decode` / `FramePipeline.begin_jpeg` / `begin_clip_jpeg` (`reader.layouts`)."""

    def __init__(self, path, default_tables: bool = False, layouts: bool = False):
        self._default_tables = bool(default_tables)
        self.layouts = bool(layouts)
        self._f = open(path, "rb")
        try:
            self._f.seek(0, 2)
            self._size = self._f.tell()
            self._frames = []          # (offset, size) of every '00dc' payload
            self.width = self.height = 0
            self.fps = 0.0
            self._handler = self._compression = None
            self._streams, self._video = 0, None      # 'strh' chunks seen; the number of the first video stream: its chunks are 'NNdc'
            self._movi = False
            head = self._read(0, 12)
            if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
                raise ValueError("not an AVI file (no RIFF 'AVI ' header)")
            riff_end = 8 + struct.unpack("<I", head[4:8])[0]
            if riff_end > self._size:
                raise ValueError(f"truncated file: the RIFF chunk says {riff_end} bytes, the file has {self._size}")
            self._walk(12, riff_end)
            if not self._movi:
                raise ValueError("no 'movi' list: not a complete AVI file")
            if self._handler is None or self._compression is None:
                raise ValueError("no video stream header ('strh' / 'strf')")
            if self._handler.upper() != b"MJPG" or self._compression.upper() != b"MJPG":
                raise ValueError(f"not a Motion-JPEG AVI: the video stream is {self._handler!r} / {self._compression!r}, not b'MJPG'")
        except Exception:
            self._f.close()
            self._f = None
            raise

    def _read(self, at: int, n: int) -> bytes:
        self._f.seek(at)
        return self._f.read(n)

    def _walk(self, at: int, end: int) -> None:
        while at + 8 <= end:
            fourcc, size = struct.unpack("<4sI", self._read(at, 8))
            body = at + 8
            if body + size > end:
                raise ValueError(f"truncated file: chunk {fourcc!r} at {at} has {size} bytes, its parent ends at {end}")
            if fourcc == b"LIST":
                if size < 4:
                    raise ValueError(f"a LIST chunk of {size} bytes at {at}")
                kind = self._read(body, 4)
                if kind == b"movi":
                    self._movi = True
                if kind in (b"hdrl", b"strl", b"movi", b"rec "):
                    self._walk(body + 4, body + size)
            elif fourcc == b"avih" and size >= 40:
                v = struct.unpack("<10I", self._read(body, 40))
                self.width, self.height = v[8], v[9]
                if v[0]:
                    self.fps = 1_000_000 / v[0]
            elif fourcc == b"strh" and size >= 32:
                v = struct.unpack("<4s4sIHHIII", self._read(body, 28))
                self._streams += 1
                if v[0] == b"vids" and self._handler is None:
                    self._handler, self._video = v[1], self._streams - 1
                    if v[6]:
                        self.fps = v[7] / v[6]
            elif fourcc == b"strf" and size >= 40 and self._handler is not None and self._compression is None:
                v = struct.unpack("<IiiHH4s", self._read(body, 20))
                self._compression = v[5]
                self.width, self.height = v[1], abs(v[2])
            elif fourcc[2:] in (b"dc", b"db") and fourcc[:2].isdigit() and int(fourcc[:2]) == self._video:
                if size > 0:                 # (the chunks of that one stream: another video stream's frames are not mixed in)
                    self._frames.append((body, size))
            at = body + size + (size & 1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __len__(self) -> int:
        return len(self._frames)

    def __getitem__(self, i: int) -> bytes:
        if self._f is None:
            raise ValueError("read from a closed MJPGReader")
        at, size = self._frames[i]
        data = self._read(at, size)
        if len(data) != size:
            raise ValueError(f"truncated file: frame {i} has {len(data)} of {size} bytes")
        if self._default_tables:
            from . import _lib
            data = _lib.jpeg_add_default_tables(data)
        return data

    def info(self, i: int) -> dict:
        """`whenet_hip.jpeg.info` of frame i, with the reader's `layouts`."""
        from . import jpeg
        return jpeg.info(self[i], layouts=self.layouts)

    def __iter__(self):
        for i in range(len(self._frames)):
            yield self[i]

    def clips(self, n: int):
        """Lists of up to `n` consecutive frames' bytes, ready for `FramePipeline.begin_clip_jpeg`: every list but the last has n
        entries, none is empty."""
        if int(n) < 1:
            raise ValueError("clips(n): n must be at least 1")
        for first in range(0, len(self._frames), int(n)):
            yield [self[i] for i in range(first, min(first + int(n), len(self._frames)))]


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
