"""'imagenet1k_mobile' / 'imagenet1k_inception' on the GPU: atomnas_image_color (ColorJitter + Lighting) and the window mode of the resize
(Resize + CenterCrop, atomnas_image_resize_window[_large]) against PIL's bytes (tests/golden/color_aug.pt, tools/make_golden_color.py;
the source images are regenerated from their seeds), DevicePrefetcher end to end against the per-sample restatement
(tests/color_ref.py, pinned against PIL in tests/test_color_transforms.py), and train.py / val.py with tests/data/tiny_mobile.yml.
All comparisons are exact: the results are integers, and ToTensor / Normalize is required bit for bit as in
tests/test_input_pipeline_gpu.py."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_ref as cr  # noqa: E402
import kutil  # noqa: E402

pr = cr.pr
pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _fixture():
    return torch.load(os.path.join(ROOT, "tests", "golden", "color_aug.pt"), weights_only=False)


_out = kutil.feed_out


def _check_modes(u8, f32, b16, q, tag):
    """out_mode 0 and 1 are ((u8 / 255 - mean) / std) in fp32 of the out_mode 2 bytes, bit for bit"""
    want = torch.from_numpy(pr.to_tensor_normalize(u8[q].numpy(), MEAN, STD))
    assert torch.equal(f32[q], want), (tag, q, float((f32[q] - want).abs().max()))
    assert torch.equal(b16[q, :, :, :3].permute(2, 0, 1), want.bfloat16()) and float(b16[q, :, :, 3:].abs().max()) == 0.0, (tag, q)


def _forms(S):
    return ["auto", "two_launch"] + (["lds"] if S % 2 == 0 and S * S * 3 <= 160 * 1024 - 256 else [])


def test_color_pass_matches_pil_fixture_exactly(gpu_lib):
    from atomnas_amd.utils import dataflow as DF, transforms as T
    g = _fixture()
    by_size = {}
    for c in g["color"]:
        by_size.setdefault(c["size"], []).append(c)
    assert sorted(by_size) == [45, 50, 64, 224]
    for S, cases in by_size.items():
        order = list(range(len(cases)))
        random.Random(S).shuffle(order)   # batch positions shuffled: a per-image table indexed wrongly shows
        cases = [cases[i] for i in order]
        n = len(cases)
        images = [cr.image(c["H"], c["W"], c["seed"]) for c in cases]
        boxes = [c["box"] for c in cases]
        pool, desc, aug, _ = kutil.feed_upload(images, boxes, [c["flip"] for c in cases], S, [T.Aug(c["ops"] or None, c["inc"], None) for c in cases])
        stage = _out(n, S, 2)
        DF.preprocess(pool, desc, n, S, MEAN, STD, stage, 2)
        means = torch.empty(n, dtype=torch.int32, device="cuda")
        for form in _forms(S):
            outs = []
            for mode in (2, 0, 1):
                o = _out(n, S, mode)
                DF.color(stage, aug, n, S, MEAN, STD, o, means, mode, form=form)
                torch.cuda.synchronize()
                outs.append(o.cpu())
            u8, f32, b16 = outs
            bad = [(q, c["seed"], c["ops"], int((u8[q] != c["expected"]).sum())) for q, c in enumerate(cases) if not torch.equal(u8[q], c["expected"])]
            assert not bad, (S, form, bad)
            for q in range(n):
                _check_modes(u8, f32, b16, q, (S, form))


def _window_batch(cases):
    from atomnas_amd.utils import dataflow as DF, transforms as T
    images = [cr.image(c["H"], c["W"], c["seed"]) for c in cases]
    crop = cases[0]["crop"]
    augs, boxes, sel = [], [], []
    for q, c in enumerate(cases):
        oh, ow = cr.resize_size(c["W"], c["H"], c["resize"])
        boxes.append((int(round((oh - crop) / 2.)), int(round((ow - crop) / 2.)), crop, crop))
        augs.append(T.Aug(None, None, (oh, ow)))
        if DF.check_window(c["H"], c["W"], (oh, ow)):
            sel.append(q)
    return images, boxes, augs, sel


def _run_window(images, boxes, flips, augs, sel, crop, mode, filt):
    from atomnas_amd.utils import dataflow as DF
    pool, desc, aug, large = kutil.feed_upload(images, boxes, flips, crop, augs)   # (a window batch: the records describe whole images)
    assert large == sel
    o = _out(len(images), crop, mode)
    DF.resize_window(pool, desc, aug, len(images), crop, MEAN, STD, o, mode, filter=filt)
    if sel:
        rows = max(images[q].shape[0] for q in sel)
        ws = torch.empty(len(sel) * rows * crop * 3, dtype=torch.uint8, device="cuda")
        DF.resize_window_large(pool, desc, aug, torch.tensor(sel, dtype=torch.int32, device="cuda"), len(sel), rows, crop, MEAN, STD, o, ws,
                               mode, filter=filt)
    torch.cuda.synchronize()
    return o.cpu()


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
def test_window_mode_matches_pil_fixture_exactly(gpu_lib, filt):
    g = _fixture()
    groups = {}
    for c in g["window"]:
        if filt in c:
            groups.setdefault((c["resize"], c["crop"]), []).append(c)
    assert (256, 224) in groups and (64, 56) in groups
    n_two_pass = 0
    for (resize, crop), cases in groups.items():
        cases = cases[::-1]
        images, boxes, augs, sel = _window_batch(cases)
        n_two_pass += len(sel)
        flips = [c["flip"] for c in cases]
        u8, f32, b16 = [_run_window(images, boxes, flips, augs, sel, crop, mode, filt) for mode in (2, 0, 1)]
        bad = [(q, c["H"], c["W"], int((u8[q] != c[filt]).sum())) for q, c in enumerate(cases) if not torch.equal(u8[q], c[filt])]
        assert not bad, (filt, resize, crop, bad)
        for q in range(len(cases)):
            _check_modes(u8, f32, b16, q, (filt, resize, crop))
    assert n_two_pass >= 1   # 700 x 660 at Resize(64) (and 2400 x 2600 at Resize(256) for bilinear) are beyond the tap budget


def _expected_sample(im, box, flip, aug, S, mean, std, filt="bilinear"):
    im = im.numpy()
    if aug is not None and aug.resize is not None:
        oh, ow = aug.resize
        r = pr.resize_u8(im, oh, ow, filt)[box[0]:box[0] + S, box[1]:box[1] + S]
        r = r[:, ::-1].copy() if flip else r
    else:
        r = pr.crop_resize_flip(im, box, S, flip, filt)
    if aug is not None:
        r = cr.color_chain(r, aug.ops, aug.inc)
    return torch.from_numpy(pr.to_tensor_normalize(r, mean, std))


def _flags(**kw):
    class _F(dict):
        __getattr__ = dict.__getitem__
    f = _F(data_transforms="imagenet1k_mobile", dataset="imagenet1k_decoded_fake", data_loader="imagenet1k_basic", image_size=64,
           use_distributed=False, test_only=False, bn_calibration=False, fake_train_size=20, fake_val_size=9, random_seed=4,
           _loader_batch_size=6, data_loader_workers=2)
    f.update(kw)
    return f


@pytest.mark.parametrize("name", ["imagenet1k_mobile", "imagenet1k_inception"])
def test_prefetcher_end_to_end_with_the_color_transforms(gpu_lib, name):
    from atomnas_amd.utils import dataflow as DF
    F = _flags(data_transforms=name)
    tr, va, te = DF.data_transforms(F)
    sets = DF.dataset(tr, va, te, F)
    runs = []
    for rep in range(2):
        got = []
        for split, loader in zip(("train", "val"), (DF.data_loader(*sets, F)[0], DF.data_loader(*sets, F)[2])):
            random.seed(31)
            np.random.seed(32)
            want = [b for b in loader]   # the loader is deterministic for these seeds: the same batches again below
            random.seed(31)
            np.random.seed(32)
            loader.epoch = 0             # (the same shuffle as the pass above)
            tf = loader.dset.transform
            pf = DF.DevicePrefetcher(loader, image_size=64, mean=tf.mean, std=tf.std, filter=tf.filter, threaded=False)
            batches = [(x.clone().cpu(), y.clone().cpu()) for x, y in pf]
            pf.close()
            assert len(batches) == len(want) == (4 if split == "train" else 2)
            if rep == 0:
                for (x, y), (images, boxes, flips, target, augs) in zip(batches, want):
                    assert torch.equal(y, target) and tuple(x.shape) == (len(images), 3, 64, 64)
                    for q in range(len(images)):
                        e = _expected_sample(images[q], boxes[q], flips[q], augs[q], 64, tf.mean, tf.std)
                        assert torch.equal(x[q], e), (name, split, q, augs[q], float((x[q] - e).abs().max()))
            got.append(batches)
        runs.append(got)
    for a, b in zip(runs[0], runs[1]):   # two runs with one seed are identical
        assert all(torch.equal(x, u) and torch.equal(y, v) for (x, y), (u, v) in zip(a, b))


class _Fixed(object):
    """a loader over fixed five-element batches"""

    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


@pytest.mark.parametrize("threaded", [True, False])
def test_prefetcher_mixes_oversize_and_ordinary_images(gpu_lib, threaded):
    """colour batches whose crop boxes are partly beyond the tap budget, and evaluation batches whose images are: every slot is right;
    a four-element batch in between takes the plain path"""
    from atomnas_amd.utils import dataflow as DF, transforms as T
    S = 224
    small = [torch.from_numpy(cr.image(375, 500, 81)), torch.from_numpy(cr.image(300, 260, 82))]
    big = torch.from_numpy(cr.image(2100, 2300, 83))
    ops = (("contrast", 1.3), ("brightness", 0.8), ("saturation", 1.2))
    train = ([small[0], big, small[1]], [(10, 20, 300, 400), (0, 0, 2017, 2200), (0, 0, 300, 260)], [True, False, True],
             torch.tensor([1, 2, 3]), [T.Aug(ops, (5.5, -3.25, 1.0), None), T.Aug(ops[::-1], None, None), None])
    plain = ([small[1], small[0]], [(5, 5, 200, 200), (0, 0, 375, 500)], [False, True], torch.tensor([4, 5]))
    big2 = torch.from_numpy(cr.image(2400, 2500, 84))
    imgs = [big2, small[0], small[1]]
    wins = [cr.resize_size(im.shape[1], im.shape[0], 256) for im in imgs]
    val = (imgs, [T.center_crop_box(ow, oh, S, S) for oh, ow in wins], [False, False, False], torch.tensor([6, 7, 8]),
           [T.Aug(None, None, w) for w in wins])
    assert DF.check_box(2100, 2300, train[1][1], S) and DF.check_window(2400, 2500, wins[0]) and not DF.check_window(375, 500, wins[1])
    batches = [train, plain, val, train]
    pf = DF.DevicePrefetcher(_Fixed(batches), image_size=S, threaded=threaded)
    got = [(x.clone().cpu(), y.clone().cpu()) for x, y in pf]
    pf.close()
    assert len(got) == 4
    for (x, y), b in zip(got, batches):
        augs = b[4] if len(b) > 4 else [None] * len(b[0])
        assert torch.equal(y, b[3])
        for q in range(len(b[0])):
            e = _expected_sample(b[0][q], b[1][q], b[2][q], augs[q], S, MEAN, STD)
            assert torch.equal(x[q], e), (q, augs[q], float((x[q] - e).abs().max()))
    with pytest.raises(ValueError):
        p2 = DF.DevicePrefetcher(_Fixed([(val[0], val[1], val[2], val[3], [val[4][0], None, None])]), image_size=S, threaded=False)
        p2.close()


def test_plain_batches_allocate_nothing_new(gpu_lib):
    """the MnasNet path: no aug table, no staging buffer, and the bytes of atomnas_image_preprocess alone"""
    from atomnas_amd.utils import dataflow as DF, transforms as T
    loader = DF.SyntheticDecodedImages(batch=5, steps=3, num_classes=10, image_size=64, pool_size=6, seed=1)
    want = [b for b in loader]
    pf = DF.DevicePrefetcher(DF.SyntheticDecodedImages(batch=5, steps=3, num_classes=10, image_size=64, pool_size=6, seed=1), image_size=64,
                             threaded=False)
    for (x, y), (imgs, boxes, flips, target) in zip(pf, want):
        for q in range(5):
            e = torch.from_numpy(pr.to_tensor_normalize(pr.crop_resize_flip(imgs[q].numpy(), boxes[q], 64, flips[q]), T.IMAGENET_MEAN, T.IMAGENET_STD))
            assert torch.equal(x[q].cpu(), e)
    assert len(pf.slots) == 2 and all(s.out is not None and s.aug is None and s.stage is None and s.ws is None for s in pf.slots)
    pf.close()


def test_train_and_val_entries_with_tiny_mobile(gpu_lib, tmp_path):
    """`train.py app:tests/data/tiny_mobile.yml` in a fresh child process under its own time limit: the shortened search on
    colour-augmented batches, loss finite; then val.py scores its checkpoint with the 'imagenet1k_mobile' val transform"""
    run = str(tmp_path / "search")
    env = dict(os.environ, ATOMNAS_E2E_DIR=run, ARNOLD_OUTPUT=str(tmp_path / "out"))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train.py"),
                        "app:" + os.path.join(ROOT, "tests", "data", "tiny_mobile.yml")], cwd=ROOT, env=env, capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert out.count(" val: ") >= 2 and "Prune threshold" in out, out[-4000:]
    steps = re.findall(r"Epoch (\d+)/2 step (\d+) loss (\S+) ", out)
    assert len(steps) == 6, out[-4000:]
    assert all(np.isfinite(float(s[2])) and float(s[2]) > 0 for s in steps), steps
    ckpt = "best_model" if os.path.exists(os.path.join(run, "best_model.yml")) else "latest_checkpoint"
    assert os.path.exists(os.path.join(run, ckpt + ".pt"))
    app = os.path.join(str(tmp_path), "eval_mobile.yml")
    with open(app, "w") as f:
        f.write("_default: !include %s\n" % os.path.join(ROOT, "apps", "eval", "eval_shrink.yml"))
        f.write("dataset: imagenet1k_decoded_fake\ndata_transforms: imagenet1k_mobile\nfake_train_size: 32\nfake_val_size: 10\n"
                "use_distributed: False\nallreduce_bn: False\nper_gpu_batch_size: 4\nbn_calibration_steps: 2\n"
                "bn_calibration_per_gpu_batch_size: 8\ndata_loader_workers: 2\nnum_epochs: 2\n")
    env.update(FILE=run, CHECKPOINT=ckpt)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "val.py"), "app:" + app], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert re.search(r"Epoch 0/2 test: loss: [0-9.]+, top1_error: [0-9.]+, top5_error: [0-9.]+", out), out[-3000:]
    m = re.search(r"Epoch 0/\d+ test samples: (\d+)", out)
    assert m and int(m.group(1)) == 10, out[-3000:]
