"""'imagenet1k_mobile' / 'imagenet1k_inception', CPU side: the host deciders of atomnas_amd/utils/transforms.py (torchvision's
RandomResizedCrop / ColorJitter / Resize / CenterCrop and the reference's Lighting, utils/transforms.py:21-51) against a transcription
of their formulas written out here, independent of the product module; the tests' numpy restatement of the colour ops and of
Resize + CenterCrop (tests/color_ref.py, which the GPU fixtures are checked with) against PIL itself; the loader plumbing."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_ref as cr  # noqa: E402

from atomnas_amd.utils import dataflow as DF  # noqa: E402
from atomnas_amd.utils import transforms as T  # noqa: E402


class _Flags(dict):
    __getattr__ = dict.__getitem__


def _flags(**kw):
    f = _Flags(data_transforms="imagenet1k_mobile", dataset="imagenet1k_decoded_fake", data_loader="imagenet1k_basic", image_size=224,
               use_distributed=False, test_only=False, bn_calibration=True, fake_train_size=40, fake_val_size=11, random_seed=3,
               _loader_batch_size=8, _loader_batch_size_calib=4, data_loader_workers=0)
    f.update(kw)
    return f


def test_data_transforms_accepts_mobile_and_inception():
    for name, scale, mean, std in (("imagenet1k_mobile", 0.25, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
                                   ("imagenet1k_inception", 0.08, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))):
        tr, va, te = DF.data_transforms(_flags(data_transforms=name))
        assert va is te and isinstance(tr, DF.DeviceTransform)
        for t in (tr, va):
            assert t.size == 224 and t.mean == mean and t.std == std and t.filter == "bilinear"
        assert isinstance(tr.crop, T.RandomResizedCrop) and tr.crop.scale == (scale, 1.0) and tr.crop.ratio == (3. / 4., 4. / 3.)
        assert tr.jitter.ranges == [("brightness", 0.6, 1.4), ("contrast", 0.6, 1.4), ("saturation", 0.6, 1.4)]
        assert tr.lighting.alphastd == 0.1 and tr.flip.p == 0.5 and tr.resize is None
        assert va.resize.size == 256 and va.crop.size == 224 and va.flip is None and va.jitter is None and va.lighting is None
    tr, va, _ = DF.data_transforms(_flags(image_size=192))
    assert tr.size == 192 and va.crop.size == 192 and va.resize.size == 256   # image_size sets the crop, the resize side stays 256
    with pytest.raises(NotImplementedError, match="follow-up"):
        DF.data_transforms(_flags(data_transforms="imagenet1k_basic"))
    with pytest.raises(NotImplementedError):
        T.ColorJitter(0.4, 0.4, 0.4, hue=0.1)
    assert tuple(T.IMAGENET_PCA['eigval']) == (0.2175, 0.0188, 0.0045)
    assert T.IMAGENET_PCA['eigvec'].tolist() == [[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]]


# ---- the formulas, transcribed (torchvision's transforms of the reference's era; utils/transforms.py:21-51 for Lighting)
def ref_train_sample(W, H, scale, ratio=(3. / 4., 4. / 3.), b=0.4, c=0.4, s=0.4, alphastd=0.1):
    """one training sample's decisions from the module-level `random` and numpy's global generator, in Compose order"""
    area = W * H
    box = None
    for _ in range(10):
        target_area = random.uniform(scale[0], scale[1]) * area
        aspect_ratio = math.exp(random.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            i = random.randint(0, H - h)
            j = random.randint(0, W - w)
            box = (i, j, h, w)
            break
    branch = "drawn"
    if box is None:
        in_ratio = W / H
        if in_ratio < min(ratio):
            w = W
            h = int(round(w / min(ratio)))
            branch = "tall"
        elif in_ratio > max(ratio):
            h = H
            w = int(round(h * max(ratio)))
            branch = "wide"
        else:
            w, h = W, H
            branch = "whole"
        box = ((H - h) // 2, (W - w) // 2, h, w)
    fb = random.uniform(1 - b, 1 + b)
    fc = random.uniform(1 - c, 1 + c)
    fs = random.uniform(1 - s, 1 + s)
    ops = [("brightness", fb), ("contrast", fc), ("saturation", fs)]
    random.shuffle(ops)
    rnd = (np.random.randn(3) * alphastd).astype('float32')
    v = (rnd * np.asarray([0.2175, 0.0188, 0.0045])).reshape((3, 1))
    eigvec = np.asarray([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]])
    inc = np.dot(eigvec, v).reshape((3,))
    flip = random.random() < 0.5
    return box, tuple(ops), tuple(float(x) for x in inc), flip, branch


def _train_transform(scale, ratio=(3. / 4., 4. / 3.)):
    return DF.ColorDeviceTransform(T.RandomResizedCrop(224, scale=scale, ratio=ratio), T.RandomHorizontalFlip(), 224, T.IMAGENET_MEAN,
                                   T.IMAGENET_STD, jitter=T.ColorJitter(0.4, 0.4, 0.4), lighting=T.Lighting(0.1))


def test_train_decisions_follow_the_transcribed_formulas_and_draw_order():
    """box, (op, factor) x 3, inc and flip per sample, and both generators' states afterwards (nothing extra drawn, nothing skipped)"""
    # landscape, portrait, square, and images so elongated that all ten attempts fail; (0.9, 1.0) with a narrow ratio range fails on
    # moderately elongated images too and reaches the `whole`-image fall-back when the ratio range is wide
    settings = [((0.25, 1.0), (3. / 4., 4. / 3.), [(500, 375), (375, 500), (224, 224), (2000, 30), (30, 2000), (640, 480)]),
                ((0.08, 1.0), (3. / 4., 4. / 3.), [(500, 375), (333, 500), (3000, 20)]),
                ((0.999, 1.0), (0.5, 2.0), [(300, 200), (200, 300), (100, 100)])]
    branches = set()
    for scale, ratio, sizes in settings:
        t = _train_transform(scale, ratio)
        for seed in range(12):
            for (W, H) in sizes:
                random.seed(seed * 11 + W)
                np.random.seed(seed * 13 + H)
                want = ref_train_sample(W, H, scale, ratio)
                want_state, want_np = random.getstate(), np.random.get_state()
                random.seed(seed * 11 + W)
                np.random.seed(seed * 13 + H)
                box, flip, aug = t((W, H))
                assert (box, aug.ops, aug.inc, flip) == want[:4], (seed, W, H, (box, aug, flip), want)
                assert aug.resize is None
                assert random.getstate() == want_state
                got_np = np.random.get_state()
                assert got_np[0] == want_np[0] and np.array_equal(got_np[1], want_np[1]) and got_np[2:] == want_np[2:]
                i, j, h, w = box
                assert h > 0 and w > 0 and 0 <= i and 0 <= j and i + h <= H and j + w <= W
                branches.add(want[4])
    assert branches == {"drawn", "tall", "wide", "whole"}, branches
    # known answers by hand: a 2000 x 30 image can never hold a box of ratio <= 4/3 and a quarter of the area -> h = H, w = round(30 * 4/3)
    random.seed(0)
    assert T.RandomResizedCrop(224, scale=(0.25, 1.0))((2000, 30)) == (0, 980, 30, 40)
    assert T.RandomResizedCrop(224, scale=(0.25, 1.0))((30, 2000)) == (980, 0, 40, 30)
    assert T.Lighting(0.).get_inc() is None


def test_eval_decisions():
    """Resize(256) + CenterCrop(224): ow, oh = (256, int(256 H / W)) if W <= H else (int(256 W / H), 256); window rounded half-even"""
    _, va, _ = DF.data_transforms(_flags())
    state, np_state = random.getstate(), np.random.get_state()
    for (W, H) in [(500, 375), (375, 500), (300, 300), (57, 40), (2600, 2400), (333, 500), (1001, 999)]:
        ow, oh = (256, int(256 * H / W)) if W <= H else (int(256 * W / H), 256)
        box, flip, aug = va((W, H))
        assert aug == T.Aug(None, None, (oh, ow)) and flip is False
        assert box == (int(round((oh - 224) / 2.)), int(round((ow - 224) / 2.)), 224, 224)
        assert cr.resize_size(W, H, 256) == (oh, ow)
    assert va((500, 375))[0] == (16, 58, 224, 224) and va((500, 375))[2].resize == (256, 341)   # by hand: (341 - 224) / 2 = 58.5 -> 58
    assert random.getstate() == state and np.array_equal(np.random.get_state()[1], np_state[1])   # evaluation draws nothing
    assert DF.check_window(2304, 2304, (256, 256)) is False and DF.check_window(2305, 2400, (256, 266)) is True
    a = np.zeros(1, dtype=DF.AUG_DTYPE)
    assert DF.AUG_DTYPE.itemsize == 72
    with pytest.raises(ValueError):
        DF.fill_aug(a[0], T.Aug(None, None, (256, 341)), (40, 58, 224, 224), 224)    # the window leaves the resized image
    with pytest.raises(ValueError):
        DF.fill_aug(a[0], T.Aug((("contrast", 1.1), ("contrast", 0.9)), None, None))
    DF.fill_aug(a[0], T.Aug((("saturation", 1.25), ("contrast", 0.5)), (1.5, -2.0, 0.25), None))
    assert a[0]["op"].tolist() == [3, 2, 0] and a[0]["factor"].tolist() == [1.25, 0.5, 1.0] and a[0]["inc"].tolist() == [1.5, -2.0, 0.25]


def test_color_restatement_is_bit_identical_to_pil():
    pytest.importorskip("PIL")
    rng = np.random.RandomState(8)
    names = ["brightness", "contrast", "saturation"]
    n = 0
    for t in range(60):
        H, W = int(rng.randint(5, 70)), int(rng.randint(5, 70))
        img = cr.image(H, W, t)
        order = [names[i] for i in rng.permutation(3)]
        f = rng.uniform(0.6, 1.4, 3)
        if t % 7 == 0:
            f[t % 3] = 1.0
        ops = tuple((o, float(x)) for o, x in zip(order, f))
        inc = tuple(float(x) for x in rng.randn(3) * (40 if t % 5 == 0 else 3))
        assert np.array_equal(cr.color_chain(img, ops, inc), cr.pil_color_chain(img, ops, inc)), (t, ops)
        for o, x in ops:   # every op on its own as well
            assert np.array_equal(cr.OPS[o](img, x), cr.pil_color_chain(img, ((o, x),), None)), (t, o, x)
        n += 1
    assert n == 60


def test_resize_center_crop_restatement_is_bit_identical_to_pil():
    pytest.importorskip("PIL")
    for q, (H, W, resize, crop) in enumerate([(75, 100, 32, 28), (100, 75, 32, 28), (64, 64, 32, 32), (20, 31, 32, 28), (310, 330, 32, 28),
                                               (120, 90, 64, 56)]):
        img = cr.image(H, W, 100 + q)
        for filt in ("bilinear", "bicubic"):
            got, (oh, ow), (top, left) = cr.resize_center_crop(img, resize, crop, filt, flip=q % 2 == 1)
            assert got.shape == (crop, crop, 3) and min(oh, ow) == resize and top >= 0 and left >= 0
            assert np.array_equal(got, cr.pil_resize_center_crop(img, resize, crop, filt, flip=q % 2 == 1)), (H, W, filt)


def test_restatement_matches_the_committed_fixture():
    g = torch.load(os.path.join(ROOT, "tests", "golden", "color_aug.pt"), weights_only=False)
    assert len(g["color"]) >= 16 and len(g["window"]) >= 6
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "color_aug.pt")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "input_pipeline.pt"))
    for c in g["color"]:
        img = cr.image(c["H"], c["W"], c["seed"])
        resized = cr.pr.crop_resize_flip(img, c["box"], c["size"], c["flip"])
        assert np.array_equal(cr.color_chain(resized, c["ops"], c["inc"]), c["expected"].numpy()), (c["seed"], c["ops"])
    for c in g["window"]:
        if c["H"] > 1000:
            continue   # (the numpy restatement of a 6-megapixel resize takes a while; the GPU test covers it against PIL's bytes)
        img = cr.image(c["H"], c["W"], c["seed"])
        for filt in ("bilinear", "bicubic"):
            got = cr.resize_center_crop(img, c["resize"], c["crop"], filt, c["flip"])[0]
            assert np.array_equal(got, c[filt].numpy()), (c["seed"], filt)


def _same_batches(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) == 5
        assert all(torch.equal(p, q) for p, q in zip(x[0], y[0])) and x[1] == y[1] and x[2] == y[2] and torch.equal(x[3], y[3]) and x[4] == y[4]


def test_loader_plumbing_with_the_color_transforms():
    F = _flags()
    tr, va, te = DF.data_transforms(F)
    train_set, val_set, _ = DF.dataset(tr, va, te, F)
    assert len(train_set[0]) == 5 and isinstance(train_set[0][3], T.Aug)
    runs = []
    for workers in (0, 0, 3):
        loader = DF.DecodedLoader(train_set, 8, True, seed=3, workers=workers)
        random.seed(21)
        np.random.seed(22)
        runs.append(list(loader))
    _same_batches(runs[0], runs[1])   # reproducible for a fixed seed ...
    _same_batches(runs[0], runs[2])   # ... with several decode threads as well
    images, boxes, flips, target, augs = runs[0][0]
    assert len(images) == len(boxes) == len(flips) == len(augs) == 8 and target.dtype == torch.int64
    a = np.zeros(8, dtype=DF.AUG_DTYPE)
    for q, (im, box, aug) in enumerate(zip(images, boxes, augs)):   # what the prefetcher does with a batch, host side
        assert DF.check_box(im.shape[0], im.shape[1], box, 224) is False
        assert sorted(o for o, _ in aug.ops) == ["brightness", "contrast", "saturation"] and all(0.6 <= f <= 1.4 for _, f in aug.ops)
        assert len(aug.inc) == 3 and aug.resize is None
        DF.fill_aug(a[q], aug, box, 224)
    assert sorted(a[0]["op"].tolist()) == [1, 2, 3]
    assert len({b[4][0].ops for b in runs[0]}) == len(runs[0])   # different draws per batch
    vb = list(DF.DecodedLoader(val_set, 8, False))
    assert [len(b[0]) for b in vb] == [8, 3] and all(len(b) == 5 for b in vb)
    for im, box, fl, aug in zip(vb[0][0], vb[0][1], vb[0][2], vb[0][4]):
        assert aug.resize == cr.resize_size(im.shape[1], im.shape[0], 256) and box[2:] == (224, 224) and fl is False and aug.ops is None
        DF.fill_aug(a[0], aug, box, 224)
    # the synthetic source of bench-style runs takes the transform too, with streams of its own
    s1 = list(DF.SyntheticDecodedImages(batch=4, steps=3, image_size=224, pool_size=6, seed=2, transform=tr))
    st, nst = random.getstate(), np.random.get_state()
    s2 = list(DF.SyntheticDecodedImages(batch=4, steps=3, image_size=224, pool_size=6, seed=2, transform=tr))
    _same_batches(s1, s2)
    assert random.getstate() == st and np.array_equal(np.random.get_state()[1], nst[1])   # the caller's generators are left alone
    # the MnasNet transforms keep the four-element protocol
    m = DF.data_transforms(_flags(data_transforms="imagenet1k_mnas_bilinear"))
    assert all(len(b) == 4 for b in DF.DecodedLoader(DF.DecodedFakeData(9, m[0]), 4, False))


def test_tiny_mobile_config_resolves_on_cpu(tmp_path):
    os.environ["ATOMNAS_E2E_DIR"] = str(tmp_path)
    os.environ.setdefault("ARNOLD_OUTPUT", str(tmp_path))
    os.environ.setdefault("DATA_LMDB", "/tmp/none")
    from atomnas_amd.utils import config
    flags = config.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_mobile.yml")])
    assert flags.data_transforms == "imagenet1k_mobile" and flags.dataset == "imagenet1k_decoded_fake" and flags.optimizer == "sgd"
    tr, va, _ = DF.data_transforms(flags)
    assert isinstance(tr, DF.ColorDeviceTransform) and tr.size == flags.image_size
