#!/usr/bin/env python3
"""Writes tests/golden/import_pillow.npz: a few small byte planes and what Pillow's Image.resize(..., Image.BILINEAR)
makes of them (mode "L"), the independent yardstick of tests/test_import_model.py for machines without Pillow.  The
fixture records the Pillow version that made it."""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
# (source width, source height, destination width, destination height, content)
CASES = [(64, 48, 32, 16, "noise"), (33, 77, 48, 40, "noise"), (100, 50, 96, 32, "two"), (2, 2, 16, 16, "noise"),
         (40, 400, 20, 16, "noise"), (57, 31, 56, 30, "smooth"), (16, 16, 16, 16, "noise"), (640, 20, 20, 18, "two")]


def plane(w, h, kind, rng):
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "two":
        return (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return ((np.sin(x / 7.0) + np.cos(y / 5.0) + 2) * 63.75).astype(np.uint8)


def main():
    rng = np.random.default_rng(20260101)
    out = {"pillow_version": np.array(PIL.__version__)}
    for i, (w, h, dw, dh, kind) in enumerate(CASES):
        p = plane(w, h, kind, rng)
        out[f"src{i}"] = p
        out[f"dst{i}"] = np.asarray(Image.fromarray(p).resize((dw, dh), Image.BILINEAR))
    np.savez_compressed(os.path.join(HERE, "import_pillow.npz"), **out)


if __name__ == "__main__":
    main()
