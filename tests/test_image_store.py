"""The decoded image store (atomnas_amd/utils/image_store.py, tools/make_image_store.py): an image folder decoded once into flat uint8
shards -- format, builder, reader, the `imagenet1k_store` factory and the resident sampler.  Host logic, no GPU; every store is built
in tmp_path from a folder written here with PIL."""
import importlib.util
import json
import os
import random
import shutil

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["n03", "n01", "n02"]          # written out of order: the class index is the sorted position
TRAIN, VAL = (7, 6, 6), (4, 4, 3)        # files per class: 19 train, 11 val
OVERSIZE = (330, 300)                    # at S = 32 a crop box of this image can exceed the 9 S tap budget (two-pass path)


def make_folder(root, seed=0):
    """root/{train,val}/<class>/<file>: 40 x 56 up to 120 x 96 and one 330 x 300 image, smooth content plus noise, JPEG and PNG, one
    grayscale, one RGBA and one CMYK file in each split"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    for split, counts in (("train", TRAIN), ("val", VAL)):
        k = 0
        for c, cnt in zip(CLASSES, counts):
            d = os.path.join(str(root), split, c)
            os.makedirs(d)
            for f in range(cnt):
                H, W = [(40, 56), (120, 96)][k] if k < 2 else (int(rng.randint(40, 121)), int(rng.randint(56, 97)))
                if split == "train" and k == 9:
                    H, W = OVERSIZE
                yy, xx = np.mgrid[0:H, 0:W]
                smooth = np.stack([yy * 255.0 / H, xx * 255.0 / W, (yy + xx) * 255.0 / (H + W)], axis=2)
                arr = np.clip(smooth + rng.randint(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)
                img, ext = Image.fromarray(arr), ("png" if k % 3 == 0 else "jpg")
                if k == 3:
                    img, ext = img.convert("L"), "png"
                elif k == 4:
                    img, ext = img.convert("RGBA"), "png"
                    img.putalpha(128)
                elif k == 5:
                    img, ext = img.convert("CMYK"), "jpg"
                img.save(os.path.join(d, "%02d.%s" % (f, ext)), quality=90)
                k += 1
    return str(root)


class _Flags(dict):
    __getattr__ = dict.__getitem__

    def __setattr__(self, k, v):
        self[k] = v


def flags(**kw):
    f = _Flags(data_transforms="imagenet1k_mnas_bicubic", dataset="imagenet1k_store", data_loader="imagenet1k_basic", image_size=32,
               use_distributed=False, test_only=False, bn_calibration=False, random_seed=3, _loader_batch_size=4, data_loader_workers=0)
    f.update(kw)
    return f


def build_both(tmp_path, **kw):
    """-> (image-folder root, store root) with the splits train and val"""
    from atomnas_amd.utils import image_store as IS
    src = make_folder(tmp_path / "folder")
    for split in ("train", "val"):
        IS.build_store(os.path.join(src, split), str(tmp_path / "store" / split), **kw)
    return src, str(tmp_path / "store")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return build_both(tmp_path_factory.mktemp("image_store"), workers=3, shard_bytes=64 << 10)


def test_store_is_the_image_folder_byte_for_byte(built):
    from atomnas_amd.utils import dataflow as DF
    from atomnas_amd.utils import image_store as IS
    src, dst = built
    for split, n in (("train", 19), ("val", 11)):
        folder = DF.ImageFolderDecoded(os.path.join(src, split), None)
        store = IS.DecodedStore(os.path.join(dst, split), None)
        assert len(store) == len(folder) == n and store.classes == folder.classes == sorted(CLASSES) and store.max_side is None
        assert store.class_to_idx == folder.class_to_idx
        for i in range(n):
            a, la = store.load(i)
            b, lb = folder.load(i)
            assert a.dtype == torch.uint8 and a.shape == b.shape and torch.equal(a, b) and la == lb and store.size_of(i) == tuple(b.shape[:2])
            shard = store.shards[int(store.index["shard"][i])]
            assert not a.is_pinned() and a.untyped_storage().data_ptr() == shard.untyped_storage().data_ptr()   # a view of the map
        assert isinstance(store.maps[0], np.memmap) and not store.maps[0].flags.writeable
    assert OVERSIZE in [IS.DecodedStore(os.path.join(dst, "train"), None).size_of(i) for i in range(19)]


def test_shards_hold_whole_images_at_multiples_of_16(built):
    from atomnas_amd.utils import image_store as IS
    root = os.path.join(built[1], "train")
    with open(os.path.join(root, "meta.json")) as f:
        meta = json.load(f)
    index = np.load(os.path.join(root, "index.npy"))
    assert meta["version"] == IS.VERSION and meta["count"] == 19 and meta["max_side"] is None and index.dtype == IS.INDEX_DTYPE
    assert len(meta["shard_bytes"]) > 3 and sorted(os.listdir(root)) == sorted(
        ["meta.json", "index.npy"] + [IS.shard_name(k) for k in range(len(meta["shard_bytes"]))])
    end = {}
    for r in index:
        nbytes = 3 * int(r["H"]) * int(r["W"])
        assert r["off"] % 16 == 0 and r["off"] + nbytes <= meta["shard_bytes"][r["shard"]]      # inside ONE shard
        assert r["off"] >= end.get(int(r["shard"]), 0)                                          # no overlap
        end[int(r["shard"])] = int(r["off"]) + nbytes
        assert r["off"] == 0 or r["off"] + nbytes <= 64 << 10                                   # only a lone image may exceed the cap
    assert [os.path.getsize(os.path.join(root, IS.shard_name(k))) for k in range(len(end))] == meta["shard_bytes"]


def test_builder_refuses_an_existing_store_and_a_killed_build_leaves_only_partial(tmp_path):
    from atomnas_amd.utils import dataflow as DF
    from atomnas_amd.utils import image_store as IS
    src = os.path.join(make_folder(tmp_path / "folder"), "val")
    out = str(tmp_path / "store")
    spec = importlib.util.spec_from_file_location("make_image_store", os.path.join(ROOT, "tools", "make_image_store.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main([src, out, "--workers", "2", "--shard-bytes", "40000"])
    assert len(IS.DecodedStore(out, None)) == 11 and not os.path.exists(out + ".partial")
    before = sorted(os.listdir(out))
    with pytest.raises(FileExistsError, match="exists"):
        IS.build_store(src, out)
    assert sorted(os.listdir(out)) == before

    class Dies(DF.ImageFolderDecoded):
        def load(self, index):
            if index == 6:
                raise KeyboardInterrupt("killed")
            return DF.ImageFolderDecoded.load(self, index)

    out2 = str(tmp_path / "store2")
    with pytest.raises(KeyboardInterrupt):
        IS.build_store(src, out2, workers=1, folder=Dies(src, None))
    assert not os.path.exists(out2) and os.path.isdir(out2 + ".partial")
    assert IS.build_store(src, out2, workers=1) == 11 and not os.path.exists(out2 + ".partial")   # a rerun clears the leftover


def test_reader_names_the_file_that_is_wrong(built, tmp_path):
    from atomnas_amd.utils import image_store as IS
    good = os.path.join(built[1], "val")

    def broken(name):
        d = str(tmp_path / name)
        shutil.copytree(good, d)
        return d

    d = broken("version")
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    meta["version"] = 99
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError, match=r"meta\.json.*version 99"):
        IS.DecodedStore(d, None)
    d = broken("truncated")
    with open(os.path.join(d, IS.shard_name(1)), "r+b") as f:
        f.truncate(100)
    with pytest.raises(ValueError, match=r"pixels-00001\.bin"):
        IS.DecodedStore(d, None)
    d = broken("missing")
    os.remove(os.path.join(d, IS.shard_name(0)))
    with pytest.raises(ValueError, match=r"pixels-00000\.bin.*missing"):
        IS.DecodedStore(d, None)
    d = broken("past")
    index = np.load(os.path.join(d, "index.npy"))
    index["off"][2] += 1 << 20
    np.save(os.path.join(d, "index.npy"), index)
    with pytest.raises(ValueError, match=r"index\.npy.*sample 2"):
        IS.DecodedStore(d, None)


def test_max_side_store_is_pils_bicubic_resize(tmp_path):
    from PIL import Image
    from atomnas_amd.utils import dataflow as DF
    from atomnas_amd.utils import image_store as IS
    from atomnas_amd.utils import transforms as T
    src = os.path.join(make_folder(tmp_path / "folder"), "train")
    IS.build_store(src, str(tmp_path / "store"), workers=2, max_side=64)
    folder, store = DF.ImageFolderDecoded(src, None), IS.DecodedStore(str(tmp_path / "store"), None)
    with open(str(tmp_path / "store" / "meta.json")) as f:
        assert json.load(f)["max_side"] == 64 and store.max_side == 64
    resized = 0
    for i in range(len(folder)):
        want = folder.load(i)[0].numpy()
        H, W = want.shape[:2]
        if min(H, W) > 64:
            oh, ow = T.Resize(64).get_size((W, H))   # torchvision's rule: shorter side 64, the other int(64 * long / short)
            assert min(oh, ow) == 64 and max(oh, ow) == int(64 * max(H, W) / min(H, W))
            want = np.asarray(Image.fromarray(want).resize((ow, oh), Image.BICUBIC))
            resized += 1
        got, label = store.load(i)
        assert got.shape == want.shape and np.array_equal(got.numpy(), want) and label == folder.samples[i][1]
    assert 0 < resized < len(folder)


def _same_batches(a, b):
    assert len(a) == len(b) and len(a[0]) == len(b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1] and a[2] == b[2] and torch.equal(a[3], b[3])
    if len(a) > 4:
        for x, y in zip(a[4], b[4]):
            if x is None or y is None:
                assert x is None and y is None
                continue
            assert x.ops == y.ops and x.resize == y.resize and (x.inc is None) == (y.inc is None)
            assert x.inc is None or np.array_equal(np.asarray(x.inc), np.asarray(y.inc))


@pytest.mark.parametrize("transforms", ["imagenet1k_mnas_bicubic", "imagenet1k_mobile"])
def test_factory_and_loader_give_the_image_folders_batches(built, transforms):
    from atomnas_amd.utils import dataflow as DF
    from atomnas_amd.utils import image_store as IS
    src, dst = built
    Fs = flags(dataset_dir=dst, data_transforms=transforms, bn_calibration=True, _loader_batch_size_calib=3)
    Ff = flags(dataset_dir=src, data_transforms=transforms, dataset="imagenet1k", bn_calibration=True, _loader_batch_size_calib=3)
    stores = DF.dataset(*DF.data_transforms(Fs), Fs)
    folders = DF.dataset(*DF.data_transforms(Ff), Ff)
    assert isinstance(stores[0], IS.DecodedStore) and isinstance(stores[1], IS.DecodedStore) and stores[2] is None
    assert (len(stores[0]), len(stores[1])) == (19, 11)
    only_val = DF.dataset(*DF.data_transforms(Fs), flags(dataset_dir=dst, test_only=True))   # the train split only where it is used
    assert only_val[0] is None and len(only_val[1]) == 11
    assert DF.dataset(*DF.data_transforms(Fs), flags(dataset_dir=dst, test_only=True, bn_calibration=True))[0] is not None
    ls, lf = DF.data_loader(*stores, Fs), DF.data_loader(*folders, Ff)
    assert isinstance(ls[0], DF.DecodedLoader) and ls[3] is ls[2]
    for which in (0, 1, 2):
        for epoch in range(2):
            got = []
            for loader in (ls[which], lf[which]):
                random.seed(11 + epoch)
                np.random.seed(5 + epoch)
                got.append(list(loader))
            assert len(got[0]) == len(got[1]) == len(ls[which])
            for a, b in zip(*got):
                _same_batches(a, b)


def test_resident_sampler_is_the_loaders_order_on_one_rank_and_a_fixed_share_on_many(built):
    from atomnas_amd.utils import dataflow as DF
    from atomnas_amd.utils import image_store as IS
    store = IS.DecodedStore(os.path.join(built[1], "train"), None)
    for shuffle in (True, False):
        ref = DF.DecodedLoader(store, 4, shuffle, seed=7)
        res = IS.ResidentLoader(IS.ResidentStore(store, 0, 1, seed=7), 4, shuffle, seed=7)
        assert len(res) == len(ref) == 5
        for epoch in range(3):
            ref.epoch = res.epoch = epoch
            assert res._indices() == ref._indices()
    shares, orders = [], []
    for rank in range(3):
        rs = IS.ResidentStore(store, rank, 3, seed=7)
        ld = IS.ResidentLoader(rs, 4, True, drop_last=True, seed=7)
        per_epoch = []
        for epoch in range(3):
            ld.epoch = epoch
            per_epoch.append(ld._indices())
        assert len(rs.share) == 7 and len(ld) == 1 and all(len(o) == 7 for o in per_epoch)           # the same count on every rank
        assert all(sorted(o) == sorted(rs.share) for o in per_epoch)                                  # the share never changes
        assert per_epoch[0] != per_epoch[1] and per_epoch[1] != per_epoch[2]                          # its order does
        runs, offsets, total = rs.plan()
        assert sorted(offsets) == sorted(set(rs.share)) and all(o % 16 == 0 for o in offsets.values())
        assert total >= sum(int(store.nbytes[i]) for i in set(rs.share)) and sum(r[2] for r in runs) <= total
        shares.append(rs.share)
        orders.append(per_epoch)
    assert sorted(set(sum(shares, []))) == list(range(19)) and len(sum(shares, [])) == 21             # together: the set, 2 wrapped
    # the shares are DecodedLoader's split of the seed's permutation
    assert shares == [DF.DecodedLoader(store, 4, True, rank=r, world=3, seed=7)._indices() for r in range(3)]
    with pytest.raises(ValueError, match="imagenet1k_store"):
        DF.data_loader(DF.DecodedFakeData(8, None), DF.DecodedFakeData(8, None), None, flags(dataset_resident=True))
