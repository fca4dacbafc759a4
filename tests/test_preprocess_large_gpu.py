"""Crop boxes beyond the one-pass kernel's tap budget (atomnas_image_preprocess_large, csrc/preprocess.hip) and DevicePrefetcher's
early close.  Images are generated from fixed seeds; the reference bytes come from oracle/pil_resize.py, which tests/test_eval_entry.py
pins against PIL itself at these scales."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kutil  # noqa: E402
import pil_resize as pr  # noqa: E402

pytestmark = pytest.mark.gpu
S = 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _image(H, W, seed):
    """smooth content plus noise (a resampler that reads the wrong taps shows), uint8 HWC"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = 127 + 60 * np.sin(x / (7 + seed % 5))[..., None] * np.cos(y / 11)[..., None] * np.array([1.0, -0.7, 0.4], np.float32)
    return np.clip(base + rng.randint(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)


def _center(H, W):
    c = int(0.875 * min(H, W))
    return ((H - c) // 2, (W - c) // 2, c, c)


# (H, W, box, flip): the centre crops of val images with a shorter side above 2304 px, boxes just below / at / above 9 S, a ragged box
CASES = [(3000, 2400, None, False), (4000, 6000, None, True), (2400, 700, (100, 20, 2300, 600), False),
         (2100, 2100, (5, 7, 2015, 2016), True), (2100, 2100, (0, 0, 2017, 2017), False), (2100, 2100, (30, 40, 2040, 300), True)]


def _batch(cases, seed0=5):
    imgs, boxes, flips = [], [], []
    for q, (H, W, box, fl) in enumerate(cases):
        imgs.append(torch.from_numpy(_image(H, W, seed0 + q)))
        boxes.append(box or _center(H, W))
        flips.append(fl)
    return imgs, boxes, flips


def _launch(imgs, boxes, flips, out_mode, filt, large=True):
    """both launches the way DevicePrefetcher issues them"""
    from atomnas_amd.utils import dataflow as DF
    n = len(imgs)
    pool, desc, _, sel = kutil.feed_upload(imgs, boxes, flips, S)
    out = kutil.feed_out(n, S, out_mode)
    DF.preprocess(pool, desc, n, S, MEAN, STD, out, out_mode, filter=filt)
    if large and sel:
        rows = max(boxes[q][2] for q in sel)
        ws = torch.empty(len(sel) * rows * S * 3, dtype=torch.uint8, device="cuda")
        DF.preprocess_large(pool, desc, torch.tensor(sel, dtype=torch.int32, device="cuda"), len(sel), rows, S, MEAN, STD, out, ws, out_mode,
                            filter=filt)
    torch.cuda.synchronize()
    return out, sel


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
def test_large_boxes_are_pil_exact(gpu_lib, filt):
    imgs, boxes, flips = _batch(CASES)
    got, sel = _launch(imgs, boxes, flips, 2, filt)
    assert sel == [0, 1, 2, 4, 5]   # 2015 x 2016 is within 9 S
    fails = []
    for q, (im, box, fl) in enumerate(zip(imgs, boxes, flips)):
        want = pr.crop_resize_flip(im.numpy(), box, S, fl, filt)
        g = got[q].cpu().numpy()
        if not np.array_equal(g, want):
            fails.append((q, box, int((g != want).sum())))
    assert not fails, fails


def test_large_boxes_to_tensor_normalize_exact(gpu_lib):
    """out_mode 0 (fp32 NCHW) and 1 (bf16 NHWC, pitch 8) equal to_tensor_normalize of the PIL bytes"""
    imgs, boxes, flips = _batch(CASES[:3])
    f32, _ = _launch(imgs, boxes, flips, 0, "bicubic")
    b16, _ = _launch(imgs, boxes, flips, 1, "bicubic")
    for q, (im, box, fl) in enumerate(zip(imgs, boxes, flips)):
        want = torch.from_numpy(pr.to_tensor_normalize(pr.crop_resize_flip(im.numpy(), box, S, fl, "bicubic"), MEAN, STD))
        assert torch.equal(f32[q].cpu(), want), q
        g = b16[q].cpu()
        assert torch.equal(g[..., :3], want.permute(1, 2, 0).to(torch.bfloat16)), q
        assert torch.equal(g[..., 3:], torch.zeros_like(g[..., 3:])), q


def test_mixed_batch_keeps_the_in_range_bytes(gpu_lib):
    """ImageNet-sized images next to oversize ones: the in-range slots are exactly what the one-pass kernel alone writes"""
    rng = np.random.RandomState(2)
    small = [(375, 500, (10, 20, 300, 400), True), (500, 375, (0, 0, 500, 375), False), (224, 224, (0, 0, 224, 224), False)]
    cases = [small[0], CASES[1], small[1], CASES[0], small[2]]
    imgs, boxes, flips = _batch(cases, seed0=int(rng.randint(100)))
    mixed, sel = _launch(imgs, boxes, flips, 2, "bicubic")
    alone, _ = _launch(imgs, boxes, flips, 2, "bicubic", large=False)
    assert sel == [1, 3]
    for q in (0, 2, 4):
        assert torch.equal(mixed[q], alone[q]), q
        assert np.array_equal(mixed[q].cpu().numpy(), pr.crop_resize_flip(imgs[q].numpy(), boxes[q], S, flips[q], "bicubic")), q
    for q in sel:
        assert np.array_equal(mixed[q].cpu().numpy(), pr.crop_resize_flip(imgs[q].numpy(), boxes[q], S, flips[q], "bicubic")), q


class _Batches(object):
    """a loader of `steps` batches (images, boxes, flips, targets) drawn from a fixed list of images"""

    def __init__(self, cases, batch, steps, seed=0):
        self.imgs, self.boxes, self.flips = _batch(cases, seed0=seed)
        self.imgs = [im.pin_memory() for im in self.imgs]
        self.batch, self.steps = batch, steps

    def __len__(self):
        return self.steps

    def __iter__(self):
        for k in range(self.steps):
            idx = [(k * self.batch + i) % len(self.imgs) for i in range(self.batch)]
            yield ([self.imgs[i] for i in idx], [self.boxes[i] for i in idx], [self.flips[i] for i in idx],
                   torch.tensor(idx, dtype=torch.int64).pin_memory())


@pytest.mark.parametrize("threaded", [True, False])
def test_prefetcher_routes_oversize_images(gpu_lib, threaded):
    """DevicePrefetcher launches the two-pass path for the oversize images of a batch and grows its pool for multi-megapixel images"""
    from atomnas_amd.utils import dataflow as DF
    cases = [(375, 500, (10, 20, 300, 400), True), CASES[1], CASES[2], (500, 500, (0, 0, 500, 500), False)]
    loader = _Batches(cases, batch=3, steps=3, seed=40)
    pf = DF.DevicePrefetcher(loader, image_size=S, filter="bicubic", threaded=threaded)
    got = [(x.clone(), y.clone()) for x, y in pf]
    pf.close()
    assert len(got) == 3
    for x, y in got:
        for q, i in enumerate(y.tolist()):
            want = pr.to_tensor_normalize(pr.crop_resize_flip(loader.imgs[i].numpy(), loader.boxes[i], S, loader.flips[i], "bicubic"), MEAN, STD)
            assert torch.equal(x[q].cpu(), torch.from_numpy(want)), (q, i)


@pytest.mark.parametrize("threaded", [True, False])
def test_prefetcher_close_after_an_early_exit(gpu_lib, threaded):
    """broken off after k < len batches (BN calibration's early exit): after close() the worker thread is dead and the side stream has
    completed; close() is idempotent"""
    from atomnas_amd.utils import dataflow as DF
    loader = DF.SyntheticDecodedImages(batch=16, steps=12, num_classes=10, image_size=64, pool_size=8, seed=3)
    pf = DF.DevicePrefetcher(loader, image_size=64, threaded=threaded)
    for k, (x, y) in enumerate(pf):
        x.sum()
        if k == 2:
            break
    if threaded:
        worker = pf._thread
        assert worker.is_alive()
    ev = torch.cuda.Event()
    ev.record(pf.stream)   # behind everything queued on the side stream so far (the worker may queue more until it is joined)
    pf.close()
    assert ev.query()
    if threaded:
        assert not worker.is_alive()
        assert all(t.name != "atomnas-prefetch" or t is not worker for t in threading.enumerate())
    pf.close()
    torch.cuda.synchronize()
