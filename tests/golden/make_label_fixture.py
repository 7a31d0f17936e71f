"""Records what the reference's own `process_detection` (demo_video.py:11-35) hands to `cv2.putText` with `--display full`
-> tests/golden/reference_labels.npz, and draws the contact sheet of the labels' font -> profiles/overlay_font_contact_sheet.png
(8x, for the eye; a picture, so it stays out of git) and profiles/overlay_font_contact_sheet.txt (the same glyphs as text, committed).

demo_video.py is EXECUTED as it stands under tests/refharness.py (its `cv2` is the recording stand-in) with a stand-in model that
returns designed float32 angles (tests/label_cases.fixture_angles: +-0, +-0.3, +-0.5, +-1.5, +-2.5, 3.5, 99.49999, -179.6, 177,
9999.4, 9999.5 and a seeded spread over [-180, 180]) on boxes of the committed tests/golden/reference_rects.npz set.

Stored (data only: strings and integers): boxes float32 [n,4], frame_hw int32 [n,2], ypr float32 [n,3], window int32 [n,4] =
(y0, x0, y1, x1) of the `cv2.rectangle` call, text S24 [n,3], origin int32 [n,3,2] as (x, y), font int32 [n,3], scale float64 [n,3],
colour int32 [n,3,3], thickness int32 [n,3] -- the arguments of the three putText calls in order.

    python tests/golden/make_label_fixture.py            # the fixture (needs the reference tree) and the contact sheet
    python tests/golden/make_label_fixture.py --sheet    # the contact sheet alone
"""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

from tests import label_cases as LC  # noqa: E402
from tests import refharness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_labels.npz")
RECTS = os.path.join(ROOT, "tests", "golden", "reference_rects.npz")
SHEET = os.path.join(ROOT, "profiles", "overlay_font_contact_sheet.png")
SHEET_TXT = os.path.join(ROOT, "profiles", "overlay_font_contact_sheet.txt")


def cases():
    """(boxes float32 [n,4], frame_hw int32 [n,2], ypr float32 [n,3]): head i takes box 11 i of the rects fixture."""
    ypr = LC.fixture_angles()
    with np.load(RECTS) as z:
        idx = (np.arange(len(ypr)) * 11) % len(z["boxes"])
        return z["boxes"][idx], z["frame_hw"][idx], ypr


def run_reference(boxes, frame_hw, ypr):
    """process_detection executed for every head -> dict of what it passed to cv2.rectangle and cv2.putText."""
    n = len(boxes)
    out = dict(window=np.zeros((n, 4), np.int32), text=np.zeros((n, 3), "S24"), origin=np.zeros((n, 3, 2), np.int32),
               font=np.zeros((n, 3), np.int32), scale=np.zeros((n, 3), np.float64), colour=np.zeros((n, 3, 3), np.int32),
               thickness=np.zeros((n, 3), np.int32))

    class Args:
        display = "full"

    class Model:
        def __init__(self, angles):
            self.angles = angles

        def get_angle(self, img):
            return tuple(np.array([a], np.float32) for a in self.angles)

    with refharness.reference() as R:
        dv = R.load("demo_video")
        for i in range(n):
            frame = refharness.RecordingFrame(int(frame_hw[i][0]), int(frame_hw[i][1]))
            del R.cv2.calls[:]
            dv.process_detection(Model(ypr[i]), frame, boxes[i], Args)
            (_, p, q, _, _), = [c for c in R.cv2.calls if c[0] == "rectangle"]
            out["window"][i] = (p[1], p[0], q[1], q[0])
            calls = [c for c in R.cv2.calls if c[0] == "putText"]
            assert len(calls) == 3, calls
            for j, (_, text, origin, font, scale, colour, thickness) in enumerate(calls):
                out["text"][i, j] = text.encode()
                out["origin"][i, j] = origin
                out["font"][i, j], out["scale"][i, j], out["colour"][i, j], out["thickness"][i, j] = font, scale, colour, thickness
    return out


def contact_sheet(path=SHEET, zoom=8):
    """The 25 glyphs at 8x, one row, each in its 7-pixel cell with the baseline marked: for the eye, not for a test."""
    from PIL import Image
    top, rows = LC.BOX_Y[0] - 1, LC.BOX_Y[1] - LC.BOX_Y[0] + 3
    img = np.full((rows, LC.ADVANCE * len(LC.GLYPHS) + 1, 3), 255, np.uint8)
    img[-top, :] = (215, 215, 255)                                # the baseline
    img[:, ::LC.ADVANCE] = (225, 225, 225)                        # the cells
    for i, ch in enumerate(LC.GLYPHS):
        for x, y in LC.glyph_pixels(ch, margin=0):
            img[y - top, 1 + LC.ADVANCE * i + x] = (0, 0, 0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(img.repeat(zoom, axis=0).repeat(zoom, axis=1)).save(path, optimize=True)
    return path


def contact_sheet_text(path=SHEET_TXT, per_row=9):
    """The same glyphs as text: '#' painted, '.' not, one 6 x 13 box per character, the baseline row marked with '_'."""
    lines = ["The labels' font (include/whenet_hip.h, WHENET_OVERLAY_FONT) under the thin rule: 6 x 13 boxes, rows y = -9 .. 3,",
             "'_' marks unpainted pixels of the baseline row y = 0.  Written by tests/golden/make_label_fixture.py.", ""]
    for i in range(0, len(LC.GLYPHS), per_row):
        chunk = LC.GLYPHS[i:i + per_row]
        lines.append("   ".join(f"'{c}'   " for c in chunk).rstrip())
        for y in range(LC.BOX_Y[0], LC.BOX_Y[1] + 1):
            cells = ["".join("#" if (x, y) in LC.glyph_pixels(c, margin=0) else ("_" if y == 0 else ".")
                             for x in range(LC.BOX_X[0], LC.BOX_X[1] + 1)) for c in chunk]
            lines.append("   ".join(cells))
        lines.append("")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return path


def main():
    if "--sheet" not in sys.argv:
        boxes, frame_hw, ypr = cases()
        out = run_reference(boxes, frame_hw, ypr)
        np.savez_compressed(OUT, boxes=boxes, frame_hw=frame_hw, ypr=ypr, **out)
        print(f"{OUT}: {len(boxes)} heads, {os.path.getsize(OUT)} bytes; e.g. {[t.decode() for t in out['text'][len(LC.DESIGNED_ANGLES)]]}")
    print(f"{contact_sheet()}: {os.path.getsize(SHEET)} bytes; {contact_sheet_text()}")


if __name__ == "__main__":
    main()
