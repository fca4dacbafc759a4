"""Feeding the preprocessing kernels from a decoded image store (atomnas_amd/utils/image_store.py): host mode
(DevicePrefetcher(staging=True): one staged copy per batch, only the crop box's rows) and resident mode (offsets into device memory,
no pixel copy) give exactly the batches of the image-folder path; pool offsets beyond 4 GiB; the memory budget; train.py in both modes."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import kutil
from test_image_store import build_both, flags  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 32
# (data_transforms, split): the mnas training crop (the 330 x 300 image can draw a box above the 9 S tap budget), the colour pass, and
# Resize + CenterCrop in window mode
CASES = {"mnas_train": ("imagenet1k_mnas_bicubic", 0), "mobile_train": ("imagenet1k_mobile", 0), "mobile_eval": ("imagenet1k_mobile", 2)}


class _Epochs(object):
    """two epochs of a loader as one, so that one prefetcher reuses both slots several times; keeps what passed through"""

    def __init__(self, loader):
        self.loader, self.dset, self.seen = loader, loader.dset, []

    def __len__(self):
        return 2 * len(self.loader)

    def __iter__(self):
        for _ in range(2):
            for batch in self.loader:
                self.seen.append((batch[0], batch[1]))
                yield batch


def _run(F, case, staging):
    """every (input, target) of two epochs of the case's loader through a DevicePrefetcher -> (batches, what the loader handed over)"""
    from atomnas_amd.utils import dataflow as DF
    name, which = CASES[case]
    F = flags(**dict(F, data_transforms=name))
    tfs = DF.data_transforms(F)
    loader = _Epochs(DF.data_loader(*DF.dataset(*tfs, F), F)[which])
    tf = loader.dset.transform
    random.seed(9)   # (under this seed the oversize image draws boxes above 9 S: asserted where the reference is computed)
    np.random.seed(29)
    pf = DF.DevicePrefetcher(loader, image_size=S, mean=tf.mean, std=tf.std, filter=tf.filter, staging=staging)
    try:
        got = [(x.clone(), y.clone()) for x, y in pf]
    finally:
        pf.close()
    torch.cuda.synchronize()
    return got, loader.seen


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    return build_both(tmp_path_factory.mktemp("image_store_gpu"), workers=3, shard_bytes=256 << 10)


@pytest.fixture(scope="module")
def reference(gpu_lib, roots):
    """the batches of the image-folder path (PIL decode per epoch, one copy per image), computed once"""
    ref = {}
    for case in CASES:
        ref[case], seen = _run(dict(dataset="imagenet1k", dataset_dir=roots[0], data_loader_workers=2), case, False)
        assert len(ref[case]) == (10 if CASES[case][1] == 0 else 6) and ref[case][0][0].shape == (4, 3, S, S)
        if case == "mnas_train":   # the oversize image drew a box for the two-pass path at least once
            assert any(DF_check(im, box) for images, boxes in seen for im, box in zip(images, boxes))
    return ref


def DF_check(im, box):
    from atomnas_amd.utils import dataflow as DF
    return DF.check_box(int(im.shape[0]), int(im.shape[1]), box, S)


def _assert_same(got, want):
    assert len(got) == len(want)
    for (x, y), (rx, ry) in zip(got, want):
        assert x.dtype == torch.float32 and torch.equal(x, rx) and torch.equal(y, ry)


@pytest.mark.parametrize("case", sorted(CASES))
def test_host_mode_batches_equal_the_image_folders(reference, roots, case):
    from atomnas_amd.utils import image_store as IS
    got, seen = _run(dict(dataset_dir=roots[1]), case, True)
    assert all(isinstance(im, torch.Tensor) and not im.is_pinned() for images, _ in seen for im in images)
    assert isinstance(seen[0][0][0], torch.Tensor) and len(seen) == len(got)
    _assert_same(got, reference[case])
    assert IS.DecodedStore(os.path.join(roots[1], "train"), None).shard_bytes[1:]   # (several shards were in play)


@pytest.mark.parametrize("case", sorted(CASES))
def test_resident_mode_batches_equal_the_image_folders_without_image_copies(reference, roots, case):
    from atomnas_amd.utils import dataflow as DF
    got, seen = _run(dict(dataset_dir=roots[1], dataset_resident=True, dataset_resident_reserve_gb=1), case, False)
    pools = set()
    for images, _ in seen:   # the batch form carries offsets into ONE device tensor and no image tensor
        assert isinstance(images, DF.ResidentImages) and images.pool.is_cuda and images.pool.dtype == torch.uint8
        assert sorted(vars(images)) == ["offs", "pool", "sizes"] and all(isinstance(o, int) and o % 16 == 0 for o in images.offs)
        assert all(isinstance(h, int) and isinstance(w, int) for h, w in images.sizes)
        pools.add(images.pool.data_ptr())
    assert len(pools) == 1 and len(seen) == len(got)
    _assert_same(got, reference[case])


def test_resident_train_and_calibration_loaders_share_one_upload(gpu_lib, roots):
    from atomnas_amd.utils import dataflow as DF
    F = flags(dataset_dir=roots[1], dataset_resident=True, dataset_resident_reserve_gb=1, bn_calibration=True, _loader_batch_size_calib=3)
    train, calib, val, test = DF.data_loader(*DF.dataset(*DF.data_transforms(F), F), F)
    assert train.resident is calib.resident and val.resident is not train.resident and test is val
    a, b = next(iter(train)), next(iter(calib))
    assert a[0].pool.data_ptr() == b[0].pool.data_ptr() and len(a[0]) == 4 and len(b[0]) == 3


def test_budget_refusal_names_both_sizes(gpu_lib, roots):
    from atomnas_amd.utils import image_store as IS
    store = IS.DecodedStore(os.path.join(roots[1], "train"), None)
    res = IS.ResidentStore(store, reserve_gb=1 << 20)   # a reserve no card has
    total, free = res.plan()[2], torch.cuda.mem_get_info()[0]
    with pytest.raises(ValueError) as e:
        res.ensure()
    msg = str(e.value)
    assert "%d bytes" % total in msg and "%d bytes" % (total + (1 << 50)) in msg and "--max-side" in msg and "host mode" in msg
    free_named = int(re.search(r"and (\d+) bytes", msg).group(1))
    assert abs(free_named - free) <= 1 << 30 and res.pool is None   # (the free figure is the device's at that moment)


def test_offsets_beyond_4_gib(gpu_lib):
    """atomnas_img_desc.off is 64-bit all the way: images placed past the 4 GiB mark of a 5 GiB pool (never touched elsewhere, so
    cheap) resize to the bytes they give at offset 0 -- crop-box mode with its two-pass form, and window mode"""
    from atomnas_amd.utils import dataflow as DF
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("less than 8 GiB of device memory free")
    g = torch.Generator().manual_seed(4)
    images = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g) for H, W in ((330, 300), (57, 91), (120, 96))]
    boxes = [(3, 5, 320, 290), (10, 7, 40, 60), (0, 0, 120, 96)]   # the first: above 9 S = 288, rewritten by the two-pass form
    n = len(images)
    far = torch.empty(5 << 30, dtype=torch.uint8, device="cuda")
    near = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    flips = [i & 1 for i in range(n)]
    aug = kutil.feed_tables(images, [(7, 9, S, S)] * n, flips, S, [DF.T.Aug(None, None, (2 * S, 2 * S))] * n)[2]
    aug_dev = torch.from_numpy(aug.view(np.uint8)).cuda()
    outs = []
    for pool, base in ((near, 0), (far, (4 << 30) + 4096)):
        _, desc_dev, _, large = kutil.feed_upload(images, boxes, flips, S, pool=pool, base=base)
        assert large == [0] and (base == 0 or np.frombuffer(desc_dev.cpu().numpy(), dtype=DF.DESC_DTYPE)["off"].min() > 1 << 32)
        sel = torch.zeros(1, dtype=torch.int32, device="cuda")
        box_out = torch.zeros(n, 3, S, S, device="cuda")
        win_out = torch.zeros(n, 3, S, S, device="cuda")
        ws = torch.empty(320 * S * 3, dtype=torch.uint8, device="cuda")
        DF.preprocess(pool, desc_dev, n, S, DF.T.IMAGENET_MEAN, DF.T.IMAGENET_STD, box_out, filter="bicubic")
        DF.preprocess_large(pool, desc_dev, sel, 1, 320, S, DF.T.IMAGENET_MEAN, DF.T.IMAGENET_STD, box_out, ws, filter="bicubic")
        DF.resize_window(pool, desc_dev, aug_dev, n, S, DF.T.IMAGENET_MEAN, DF.T.IMAGENET_STD, win_out, filter="bilinear")
        torch.cuda.synchronize()
        outs.append((box_out, win_out))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][0].abs().sum() > 0 and outs[0][1].abs().sum() > 0 and torch.isfinite(outs[0][0]).all()


def _losses(out):
    return re.findall(r"step \d+ loss \S+ l2 \S+ l1 \S+ lr \S+", out)


def test_train_entry_from_the_store_logs_the_image_folders_losses(gpu_lib, roots, tmp_path):
    """train.py from the store in host and in resident mode: the logged losses are, digit for digit, those of the image-folder run"""
    logs = {}
    for mode, yml, extra in (("folder", "tiny_search_decoded.yml", ["--dataset", "imagenet1k", "--dataset_dir", roots[0], "--data_loader_workers", "4"]),
                             ("host", "tiny_store.yml", ["--dataset_dir", roots[1]]),
                             ("resident", "tiny_store_resident.yml", ["--dataset_dir", roots[1]])):
        out = str(tmp_path / mode)
        env = dict(os.environ, ATOMNAS_E2E_DIR=out, ARNOLD_OUTPUT=out)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "app:" + os.path.join(ROOT, "tests", "data", yml)] + extra,
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        o = r.stdout + r.stderr
        assert r.returncode == 0, o[-4000:]
        assert o.count(" val: ") >= 2, o[-4000:]
        logs[mode] = _losses(o)
        print(mode, logs[mode])
    assert len(logs["folder"]) >= 4
    assert logs["host"] == logs["folder"] and logs["resident"] == logs["folder"]
