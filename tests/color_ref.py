"""TEST HELPER -- numpy restatement of the colour ops of 'imagenet1k_mobile' / 'imagenet1k_inception' (PIL.ImageEnhance.Brightness /
Contrast / Color behind torchvision's ColorJitter, the reference's Lighting, utils/transforms.py:21-51) and of Resize + CenterCrop
(through oracle/pil_resize.py), plus the seeded source images shared by tools/make_golden_color.py and the tests.  Pinned against PIL
itself in tests/test_color_transforms.py.  The product (atomnas_amd/) never imports this file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pil_resize as pr  # noqa: E402


def image(H, W, seed, kind=None):
    """uint8 HWC test image from a seed: 0 uniform noise, 1 low contrast around a grey level, 2 smooth with saturated ends"""
    rng = np.random.RandomState(seed)
    kind = seed % 3 if kind is None else kind
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == 0:
        return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == 1:
        return (100 + seed % 60 + rng.randint(-12, 13, (H, W, 3))).clip(0, 255).astype(np.uint8)
    base = np.stack([np.clip(yy * 400 // max(H - 1, 1) - 70, 0, 255), (xx * 3 + yy) % 256, np.clip(300 - (yy + xx), 0, 255)], 2)
    return (base + rng.randint(-9, 10, (H, W, 3))).clip(0, 255).astype(np.uint8)


def grey(img):
    """PIL's RGB -> L: (19595 R + 38470 G + 7471 B + 0x8000) >> 16"""
    p = img.astype(np.int64)
    return (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 0x8000) >> 16


def blend(d, p, f):
    """PIL's Image.blend(degenerate, image, f) on uint8 arrays: fp32 product, fp32 sum; 0 <= f <= 1: truncation; otherwise clamp to
    [0, 255], then truncation"""
    f = np.float32(f)
    d32, p32 = d.astype(np.float32), p.astype(np.float32)
    prod = (f * (p32 - d32)).astype(np.float32)
    t = (d32 + prod).astype(np.float32)
    if not (0.0 <= float(f) <= 1.0):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.uint8)   # truncation (the values are in range)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f):
    L = grey(img)
    m = int(int(L.sum()) / L.size + 0.5)
    return blend(np.full_like(img, m), img, f)


def saturation(img, f):
    return blend(np.repeat(grey(img)[..., None], 3, axis=2).astype(np.uint8), img, f)


OPS = {"brightness": brightness, "contrast": contrast, "saturation": saturation}


def lighting(img, inc):
    """utils/transforms.py:44-47: float64 add, clip, astype(uint8)"""
    return np.clip(np.add(img, np.asarray(inc, dtype=np.float64)), 0, 255).astype(np.uint8)


def color_chain(img, ops, inc):
    """ops: ((name, factor), ...) in the order applied; inc: Lighting's increment or None"""
    for name, f in (ops or ()):
        img = OPS[name](img, f)
    return lighting(img, inc) if inc is not None else img


def resize_size(W, H, size):
    """transforms.Resize(size) -> (oh, ow)"""
    ow, oh = (size, int(size * H / W)) if W <= H else (int(size * W / H), size)
    return oh, ow


def resize_center_crop(img, resize, crop, filt="bilinear", flip=False):
    """transforms.Resize(resize) + CenterCrop(crop) on a uint8 HWC array -> (uint8 [crop, crop, 3], (oh, ow), (top, left))"""
    H, W = img.shape[:2]
    oh, ow = resize_size(W, H, resize)
    top, left = int(round((oh - crop) / 2.)), int(round((ow - crop) / 2.))
    r = pr.resize_u8(img, oh, ow, filt)[top:top + crop, left:left + crop]
    return (r[:, ::-1].copy() if flip else r), (oh, ow), (top, left)


# ---- PIL itself (the fixtures of tests/golden/color_aug.pt are made with these; skipped where PIL is absent)
def pil_color_chain(img, ops, inc):
    from PIL import Image, ImageEnhance
    enh = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}
    im = Image.fromarray(img)
    for name, f in (ops or ()):
        im = enh[name](im).enhance(f)
    arr = np.asarray(im)
    return lighting(arr, inc) if inc is not None else arr.copy()


def pil_crop_resize_flip(img, box, S, flip, filt="bilinear"):
    from PIL import Image
    i, j, h, w = box
    r = Image.fromarray(img).crop((j, i, j + w, i + h)).resize((S, S), Image.BILINEAR if filt == "bilinear" else Image.BICUBIC)
    if flip:
        r = r.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(r).copy()


def pil_resize_center_crop(img, resize, crop, filt="bilinear", flip=False):
    from PIL import Image
    H, W = img.shape[:2]
    oh, ow = resize_size(W, H, resize)
    top, left = int(round((oh - crop) / 2.)), int(round((ow - crop) / 2.))
    r = Image.fromarray(img).resize((ow, oh), Image.BILINEAR if filt == "bilinear" else Image.BICUBIC).crop((left, top, left + crop, top + crop))
    if flip:
        r = r.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(r).copy()
