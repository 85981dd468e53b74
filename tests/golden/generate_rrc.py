#!/usr/bin/env python3
"""Golden vectors of the RandomResizedCrop resample (runs where Pillow is installed, never on the GPU box).

Each case is a seeded uint8 source (HWC; c = 3 "RGB" or c = 1 "L"), a crop box (top, left, bh, bw), an output side s, and what
Pillow itself gives for  Image.fromarray(src).crop((left, top, left + bw, top + bh)).resize((s, s), Image.BICUBIC)  -- the calls
torchvision's RandomResizedCrop makes on a PIL image.  Written to rrc_tiny.npz next to this script (plain arrays, no pickle).

Before anything is written the restated rule (tests/rrc_yardstick.py: resize) must equal Pillow on EVERY case: the fixture can never
hold a case the rule does not explain, and no case is dropped to make that so.

Usage:  python tests/golden/generate_rrc.py        (a second; the arrays of rrc_tiny.npz are the same each run)
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rrc_yardstick as R  # noqa: E402

OUT = os.path.join(HERE, "rrc_tiny.npz")

#: (h, w, c, (top, left, bh, bw) or None for the whole image, s, kind); kind: "noise" | "checker" (0 / 255 squares of `kind[1]`
#: pixels: the cubic's negative lobes saturate at both ends) | "binary" (0 / 255 noise)
CASES = [
    # crop side 1, the smallest sources
    (1, 1, 3, None, 4, "noise"),
    (1, 7, 3, (0, 2, 1, 3), 8, "noise"),
    (5, 1, 3, None, 4, "noise"),
    (25, 25, 3, (5, 5, 1, 1), 4, "noise"),
    (30, 30, 3, (29, 0, 1, 30), 16, "noise"),
    (2, 2, 3, None, 32, "noise"),
    # boxes touching each corner of a 48 x 48 source; the last one is exactly 8 x down on both axes
    (48, 48, 3, None, 16, "noise"),
    (48, 48, 3, (0, 0, 30, 40), 32, "noise"),
    (48, 48, 3, (0, 28, 25, 20), 16, "noise"),
    (48, 48, 3, (15, 0, 33, 17), 8, "noise"),
    (48, 48, 3, (16, 16, 32, 32), 4, "noise"),
    # 8 x down on one axis, 5 x on the other; 7.75 x and 7.25 x
    (40, 36, 3, (3, 2, 32, 20), 4, "noise"),
    (31, 29, 3, None, 4, "noise"),
    # a crop side equal to s on one axis only (that pass is skipped), and on both
    (20, 44, 3, (1, 5, 16, 32), 16, "noise"),
    (44, 20, 3, (4, 2, 32, 8), 8, "noise"),
    (33, 48, 3, (0, 3, 33, 40), 40, "noise"),
    (16, 16, 3, None, 16, "noise"),
    # upscales; s = 40 is two tiles per axis, the second one ragged
    (12, 9, 3, None, 32, "noise"),
    (3, 5, 3, None, 40, "noise"),
    (47, 45, 3, (2, 1, 43, 41), 40, "noise"),
    (48, 6, 3, (0, 0, 48, 5), 8, "noise"),
    # an interior box: the taps clamp at the edge of the CROP, not of the image
    (7, 7, 3, (2, 2, 3, 3), 4, "noise"),
    (21, 34, 3, (6, 9, 9, 16), 8, "noise"),
    # saturating images
    (24, 24, 3, None, 16, ("checker", 3)),
    (10, 10, 3, None, 32, ("checker", 1)),
    (48, 48, 3, (1, 1, 46, 46), 8, ("checker", 1)),
    (17, 31, 3, (2, 3, 13, 25), 8, "binary"),
    (9, 9, 3, None, 40, "binary"),
    # mixed
    (37, 23, 3, (4, 0, 30, 23), 16, "noise"),
    (23, 37, 3, (0, 6, 23, 29), 32, "noise"),
    (45, 48, 3, (5, 7, 39, 36), 40, "noise"),
    (13, 11, 3, None, 8, "noise"),
    (8, 40, 3, None, 8, "noise"),
    (19, 19, 3, (3, 3, 13, 13), 4, "noise"),
    # output sides that are no multiple of 4: rows of the batch that are not whole 16-byte pieces
    (14, 17, 3, (1, 2, 11, 13), 6, "noise"),
    (9, 30, 3, (0, 4, 9, 24), 5, "binary"),
    # one channel ("L")
    (1, 1, 1, None, 4, "noise"),
    (48, 48, 1, (7, 9, 40, 32), 16, "noise"),
    (9, 13, 1, None, 32, "noise"),
    (16, 16, 1, None, 8, ("checker", 1)),
    (37, 41, 1, (0, 1, 37, 40), 40, "noise"),
    (11, 15, 1, (2, 2, 9, 12), 6, "binary"),
]


def source(k, h, w, c, kind):
    rng = np.random.default_rng(1000 + k)
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, size=(h, w, c)) * 255).astype(np.uint8)
    q = kind[1]
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat(((((yy // q) + (xx // q)) & 1) * 255).astype(np.uint8)[:, :, None], c, axis=2)


def pil_crop_resize(src, box, s):
    top, left, bh, bw = box
    img = Image.fromarray(src[:, :, 0], "L") if src.shape[2] == 1 else Image.fromarray(src, "RGB")
    out = np.asarray(img.crop((left, top, left + bw, top + bh)).resize((s, s), Image.BICUBIC))
    return out.reshape(s, s, src.shape[2])


def main():
    arrays = {"n_cases": np.array(len(CASES))}
    for k, (h, w, c, box, s, kind) in enumerate(CASES):
        box = (0, 0, h, w) if box is None else box
        top, left, bh, bw = box
        assert 0 <= top and 0 <= left and bh >= 1 and bw >= 1 and top + bh <= h and left + bw <= w, (k, box)
        assert max(bh, bw) <= 8 * s, (k, "a crop side is at most 8 s")
        src = source(k, h, w, c, kind)
        want = pil_crop_resize(src, box, s)
        got = R.resize(src[top:top + bh, left:left + bw], s)
        assert want.dtype == np.uint8 and want.shape == (s, s, c)
        assert np.array_equal(got, want), f"case {k} {CASES[k]}: the restated rule differs from Pillow on {(got != want).sum()} elements"
        arrays[f"src_{k}"], arrays[f"box_{k}"], arrays[f"out_{k}"] = src, np.array(box, dtype=np.int32), want
    np.savez(OUT, **arrays)
    print(f"{len(CASES)} cases, {os.path.getsize(OUT)} bytes -> {OUT}")


if __name__ == "__main__":
    main()
