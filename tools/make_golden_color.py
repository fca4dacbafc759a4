#!/usr/bin/env python
"""Generates tests/golden/color_aug.pt with PIL: the expected uint8 results of the colour pass (crop + resize + flip, then
ImageEnhance.Brightness / Contrast / Color in a given order, then the reference's Lighting) and of Resize + CenterCrop -- parameters
and expected bytes only; the source images are regenerated from their seeds (tests/color_ref.py `image`) by the tests.

    python tools/make_golden_color.py
"""
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import color_ref as cr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "color_aug.pt")
B, C, S = "brightness", "contrast", "saturation"


def color_specs():
    """(H, W, seed, box, size, flip, ops, inc)"""
    specs = []
    factors = {B: (0.6, 1.4, 0.83, 1.27, 1.0, 0.97), C: (1.4, 0.6, 1.31, 0.72, 1.05, 1.0), S: (0.6, 1.4, 1.19, 0.66, 0.999, 1.38)}
    incs = [(3.25, -1.5, 0.75), (-20.125, -7.3, -0.01), (17.9, 30.2, 9.6), (260.0, -270.5, 0.4), None, (-0.99, 0.99, 254.5)]
    # all six orders (brightness in front of and behind the contrast: the mean differs), output 64, every image kind, flip on and off
    for q, order in enumerate(itertools.permutations((B, C, S))):
        ops = tuple((name, factors[name][q]) for name in order)
        specs.append((90 + 7 * q, 120 - 5 * q, 20 + q, (3 + q, 2 * q, 70, 80), 64, q % 2 == 1, ops, incs[q]))
    # factors at and around 1.0 (PIL switches from truncation to clamping above 1), and at the ends of the jitter range
    around = [((B, 1.0), (C, 1.0), (S, 1.0)), ((C, 1.0000001), (B, 0.9999999), (S, 1.0000001)), ((S, 0.999), (C, 1.001), (B, 1.001)),
              ((B, 1.4), (S, 1.4), (C, 1.4)), ((C, 0.6), (S, 0.6), (B, 0.6))]
    for q, ops in enumerate(around):
        specs.append((80, 100, 40 + q, (0, 0, 80, 100), 50, q % 2 == 0, ops, (0.5, -0.5, 0.0) if q % 2 else None))   # 50: not a multiple of 64
    # an odd output side, fewer than three ops, Lighting alone
    specs.append((61, 77, 50, (1, 2, 55, 70), 45, True, ((C, 1.3),), (40.0, -40.0, 300.0)))
    specs.append((61, 77, 51, (0, 0, 61, 77), 45, False, (), (-300.0, 12.5, 1e-9)))
    specs.append((61, 77, 52, (5, 5, 50, 50), 45, True, ((S, 0.7), (B, 1.2)), None))
    # the training geometry
    specs.append((375, 500, 60, (30, 41, 300, 410), 224, True, ((B, 1.23), (C, 0.71), (S, 1.36)), (12.7, -9.1, 4.4)))
    specs.append((333, 500, 61, (0, 100, 333, 400), 224, False, ((S, 0.64), (C, 1.39), (B, 0.93)), (-31.0, 2.2, 15.5)))
    return specs


def window_specs():
    """(H, W, seed, resize, crop, flip, filters)"""
    return [(375, 500, 70, 256, 224, False, ("bilinear", "bicubic")),      # landscape, the evaluation geometry
            (500, 333, 71, 64, 56, False, ("bilinear", "bicubic")),        # portrait
            (300, 300, 72, 64, 56, True, ("bilinear", "bicubic")),         # square
            (40, 57, 73, 64, 56, False, ("bilinear", "bicubic")),          # short side below the resize: up-scaling
            (149, 33, 74, 64, 56, False, ("bilinear", "bicubic")),
            (700, 660, 75, 64, 56, False, ("bilinear", "bicubic")),        # scale 10.3: beyond the one-pass tap budget
            (2400, 2600, 76, 256, 224, False, ("bilinear",))]              # scale 9.4 at the evaluation geometry


def main():
    import PIL
    color = []
    for (H, W, seed, box, size, flip, ops, inc) in color_specs():
        img = cr.image(H, W, seed)
        resized = cr.pil_crop_resize_flip(img, box, size, flip)
        want = cr.pil_color_chain(resized, ops, inc)
        assert np.array_equal(want, cr.color_chain(resized, ops, inc)), (H, W, seed)   # the restatement agrees
        color.append(dict(H=H, W=W, seed=seed, box=box, size=size, flip=flip, ops=ops, inc=inc, expected=torch.from_numpy(want)))
    window = []
    for (H, W, seed, resize, crop, flip, filters) in window_specs():
        img = cr.image(H, W, seed)
        c = dict(H=H, W=W, seed=seed, resize=resize, crop=crop, flip=flip)
        for filt in filters:
            c[filt] = torch.from_numpy(cr.pil_resize_center_crop(img, resize, crop, filt, flip))
        window.append(c)
    torch.save(dict(color=color, window=window, pil_version=PIL.__version__), OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes, PIL", PIL.__version__)


if __name__ == "__main__":
    main()
