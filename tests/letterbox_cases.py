"""The cases of the detector-input letterbox tests (tests/test_letterbox.py) and of the fixture
tests/golden/reference_letterbox.npz (tests/golden/make_letterbox_fixture.py).

A case is a frame RECIPE (so that any machine rebuilds the same bytes from a seed), a frame size and a
box size (h, w) as the reference's `model_image_size`.  Only the results of the reference's
`letterbox_image` on these frames are committed.  Frames are RGB as `letterbox_image` sees them; the
channel order of the caller's array is a matter of the GPU tests alone.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Tuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "reference_letterbox.npz")
SAMPLE_FRAMES = os.path.join(GOLDEN, "sample_frames.npz")


class Case(NamedTuple):
    name: str
    recipe: str                 # "noise" | "gradient" | "sample0" | "sample1"
    seed: int
    frame_hw: Tuple[int, int]
    box_hw: Tuple[int, int]     # (h, w), as YOLO.model_image_size
    full: bool                  # the fixture holds the whole canvas, not only hash + subsample
    fails: bool = False         # the reference raises (a resized side of zero pixels)


# the 11 frame sizes x 3 box sizes of the feasibility check: up-scaling, identity, a 9.2x shrink
FRAME_SIZES = [(33, 47), (97, 1031), (100, 100), (224, 528), (226, 548), (300, 200), (416, 416), (480, 640),
               (720, 1280), (1080, 1920), (2160, 3840)]
BOX_SIZES = [(416, 416), (608, 608), (320, 416)]


def _cases():
    out = []
    i = 0
    for fhw in FRAME_SIZES:
        for bhw in BOX_SIZES:
            recipe = "noise" if i % 3 != 1 else "gradient"
            out.append(Case(f"{recipe}_{fhw[0]}x{fhw[1]}_to_{bhw[0]}x{bhw[1]}", recipe, 1000 + i, fhw, bhw, False))
            i += 1
    # small boxes with the whole canvas stored (<= 160 x 160)
    for fhw, bhw, recipe in [((720, 1280), (160, 160), "noise"), ((97, 131), (128, 96), "gradient"),
                             ((61, 45), (160, 128), "noise"), ((1080, 1920), (96, 160), "gradient")]:
        out.append(Case(f"{recipe}_{fhw[0]}x{fhw[1]}_to_{bhw[0]}x{bhw[1]}", recipe, 1000 + i, fhw, bhw, True))
        i += 1
    # a box that is neither square nor a multiple of 32 (the C entry point does not ask for one)
    out.append(Case("noise_480x640_to_250x333", "noise", 1000 + i, (480, 640), (250, 333), False))
    i += 1
    # the two frames of sample_frames.npz (crops of the reference's Sample/ images), whole canvas stored
    out.append(Case("sample0_224x528_to_416x416", "sample0", 0, (224, 528), (416, 416), True))
    out.append(Case("sample1_226x548_to_320x416", "sample1", 0, (226, 548), (320, 416), True))
    # a 1-pixel-high strip: nh = int(1 * 0.416) = 0, Pillow raises
    out.append(Case("noise_1x1000_to_416x416_fails", "noise", 1000 + i, (1, 1000), (416, 416), False, True))
    return out


CASES = _cases()
GOOD_CASES = [c for c in CASES if not c.fails]
BAD_CASES = [c for c in CASES if c.fails]


def make_frame(case: Case) -> np.ndarray:
    """uint8 RGB [h, w, 3], the same bytes on every machine."""
    h, w = case.frame_hw
    if case.recipe.startswith("sample"):
        f = np.load(SAMPLE_FRAMES)["frame" + case.recipe[-1]]
        assert f.shape == (h, w, 3)
        return np.ascontiguousarray(f[:, :, ::-1])          # stored BGR, as cv2.imread returns them
    rng = np.random.default_rng(case.seed)
    if case.recipe == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if case.recipe == "gradient":
        # integer arithmetic only: a diagonal ramp per channel plus +-12 levels of noise
        yy = np.arange(h, dtype=np.int64)[:, None, None]
        xx = np.arange(w, dtype=np.int64)[None, :, None]
        cc = np.arange(3, dtype=np.int64)[None, None, :]
        ramp = (yy * 255 * (cc + 1)) // (3 * max(h - 1, 1)) + (xx * 255 * (3 - cc)) // (3 * max(w - 1, 1))
        noise = rng.integers(-12, 13, (h, w, 3), dtype=np.int64)
        return np.clip(ramp // 2 + noise, 0, 255).astype(np.uint8)
    raise ValueError(case.recipe)
