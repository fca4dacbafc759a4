"""Decoded image store: an image-folder split decoded ONCE into flat files of uint8 pixels, so that an epoch costs no JPEG decode.

    <root>/meta.json        {"version", "classes" (class-index order), "count", "shard_bytes" (size of every pixels file), "max_side"}
    <root>/index.npy        one INDEX_DTYPE record per sample, in ImageFolderDecoded's sample order
    <root>/pixels-%05d.bin  packed HWC uint8 RGB, row pitch 3 W; every image starts at a multiple of 16 and lies inside one shard

build_store writes one (tools/make_image_store.py is its command line).  DecodedStore reads one with ImageFolderDecoded's interface:
`load(i)` is a zero-copy view of a read-only memory map, so a batch costs the page cache -> pinned staging copy of
DevicePrefetcher(staging=True) and nothing else on the host (host mode, `dataset: imagenet1k_store`).  ResidentStore keeps a rank's
share of a store in device memory and ResidentLoader hands DevicePrefetcher batches of offsets into it (resident mode,
`dataset_resident: True`): per step only the descriptor table crosses PCIe.  Every pixel is what PIL decoded (max_side = null) -- the
resize kernels read the store exactly as they read a freshly decoded image."""
import json
import os
import warnings

import numpy as np
import torch

from . import dataflow

VERSION = 1
ALIGN = 16   # DevicePrefetcher's pool alignment: a stored offset is usable as atomnas_img_desc.off as it stands
INDEX_DTYPE = np.dtype([("shard", "<i4"), ("off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("label", "<i4")])
DEFAULT_SHARD_BYTES = 1 << 30
BOUNCE_BYTES = 64 << 20   # pinned bounce buffer of the resident upload


def shard_name(k):
    return "pixels-%05d.bin" % k


def capped_size(H, W, max_side):
    """(H, W) after --max-side: an image whose shorter side exceeds the cap gets it as its shorter side, the other side
    int(cap * long / short) (torchvision.transforms.Resize's rounding)"""
    if max_side is None or min(H, W) <= max_side:
        return H, W
    return (int(max_side * H / W), max_side) if W <= H else (max_side, int(max_side * W / H))


def build_store(src, out, workers=8, shard_bytes=DEFAULT_SHARD_BYTES, max_side=None, folder=None):
    """decodes the image-folder split `src` into the store `out`: ImageFolderDecoded's sample list and decoder (at most 16 threads),
    written to `out`.partial and renamed when complete; an existing `out` is refused.  An image larger than `shard_bytes` gets a shard
    of its own.  max_side: a LOSSY store -- images whose shorter side exceeds it are resized to it with PIL's BICUBIC.  -> sample count"""
    import concurrent.futures
    import shutil
    out = os.path.normpath(str(out))
    if os.path.lexists(out):
        raise FileExistsError("image store %s exists already: refusing to overwrite it" % out)
    shard_bytes, workers = int(shard_bytes), max(1, min(16, int(workers)))
    if shard_bytes <= 0 or (max_side is not None and int(max_side) <= 0):
        raise ValueError("build_store: shard_bytes and max_side must be positive")
    max_side = None if max_side is None else int(max_side)
    folder = folder if folder is not None else dataflow.ImageFolderDecoded(str(src), None)
    folder.pin = False   # decoded images go to a file, not to the GPU

    def decode(i):
        im, label = folder.load(i)
        arr = im.numpy()
        H, W = capped_size(arr.shape[0], arr.shape[1], max_side)
        if (H, W) != arr.shape[:2]:
            from PIL import Image
            arr = np.asarray(Image.fromarray(arr).resize((W, H), Image.BICUBIC))
        return np.ascontiguousarray(arr), label

    partial = out + ".partial"
    if os.path.isdir(partial):
        shutil.rmtree(partial)   # what a killed build left behind
    os.makedirs(partial)
    n = len(folder)
    index = np.zeros(n, dtype=INDEX_DTYPE)
    sizes, f, pos = [], None, 0
    try:
        with concurrent.futures.ThreadPoolExecutor(max_workers=workers, thread_name_prefix="atomnas-store") as pool:
            for lo in range(0, n, 4 * workers):   # bounded: at most 4 decoded images per thread wait for the writer
                for i, (arr, label) in zip(range(lo, n), pool.map(decode, range(lo, min(n, lo + 4 * workers)))):
                    start = (pos + ALIGN - 1) // ALIGN * ALIGN
                    if f is None or (start > 0 and start + arr.nbytes > shard_bytes):
                        if f is not None:
                            f.close()
                            sizes.append(pos)
                        f, pos, start = open(os.path.join(partial, shard_name(len(sizes))), "wb"), 0, 0
                    f.write(b"\0" * (start - pos))
                    f.write(arr.data)
                    index[i] = (len(sizes), start, arr.shape[0], arr.shape[1], label)
                    pos = start + arr.nbytes
    finally:
        if f is not None:
            f.close()
            sizes.append(pos)
    np.save(os.path.join(partial, "index.npy"), index)
    with open(os.path.join(partial, "meta.json"), "w") as m:
        json.dump({"version": VERSION, "classes": list(folder.classes), "count": n, "shard_bytes": sizes, "max_side": max_side}, m, indent=1)
    os.rename(partial, out)
    return n


class DecodedStore(object):
    """A store with ImageFolderDecoded's interface: `classes`, len(), `load(i)` -> (uint8 HWC tensor, label), `__getitem__` adds the
    split's DeviceTransform decisions.  The tensor is a view of a read-only memory map of its shard: not pinned, not copied, and not to
    be written.  A store that does not match its own meta.json raises ValueError naming the file."""

    def __init__(self, root, transform):
        self.root, self.transform = str(root), transform
        meta_path, index_path = os.path.join(self.root, "meta.json"), os.path.join(self.root, "index.npy")
        try:
            with open(meta_path) as f:
                meta = json.load(f)
            index = np.load(index_path)
        except (OSError, ValueError) as e:
            raise ValueError("image store %s: cannot read meta.json / index.npy (%s)" % (self.root, e))
        if meta.get("version") != VERSION:
            raise ValueError("%s: store format version %r, this reader handles version %d" % (meta_path, meta.get("version"), VERSION))
        if index.dtype != INDEX_DTYPE or index.ndim != 1 or len(index) != meta["count"]:
            raise ValueError("%s: %d records of %s, meta.json promises %d of %s" % (index_path, len(index), index.dtype, meta["count"], INDEX_DTYPE))
        self.classes, self.max_side = list(meta["classes"]), meta["max_side"]
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.index = index
        self.nbytes = 3 * index["H"].astype(np.int64) * index["W"]
        sizes = np.asarray(meta["shard_bytes"], dtype=np.int64)
        if len(index) and not (index["shard"].min() >= 0 and index["shard"].max() < len(sizes) and index["off"].min() >= 0
                               and (index["H"] > 0).all() and (index["W"] > 0).all()):
            raise ValueError("%s: a record names a shard outside 0..%d, a negative offset or an empty image" % (index_path, len(sizes) - 1))
        self.shard_bytes = [int(s) for s in sizes]
        self.maps, self.shards = [], []
        for k, size in enumerate(self.shard_bytes):
            path = os.path.join(self.root, shard_name(k))
            if not os.path.isfile(path):
                raise ValueError("%s: shard missing (meta.json lists %d shards)" % (path, len(sizes)))
            if os.path.getsize(path) != size:
                raise ValueError("%s: %d bytes, meta.json promises %d" % (path, os.path.getsize(path), size))
            past = (index["shard"] == k) & (index["off"] + self.nbytes > size)
            if past.any():
                i = int(np.flatnonzero(past)[0])
                raise ValueError("%s: sample %d ends at byte %d of %s, which holds %d" %
                                 (index_path, i, int(index["off"][i] + self.nbytes[i]), path, size))
            mm = np.memmap(path, dtype=np.uint8, mode="r")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")   # torch warns about the read-only map once per tensor: nothing here writes
                self.shards.append(torch.from_numpy(mm))
            self.maps.append(mm)
        self._rec = [(int(r["shard"]), int(r["off"]), int(r["H"]), int(r["W"]), int(r["label"])) for r in index]

    def __len__(self):
        return len(self._rec)

    def size_of(self, index):
        """(H, W) of sample `index` without touching its pixels"""
        return self._rec[index][2], self._rec[index][3]

    def load(self, index):
        s, off, H, W, label = self._rec[index]
        return self.shards[s][off:off + 3 * H * W].view(H, W, 3), label

    def __getitem__(self, index):
        im, target = self.load(index)
        return (im,) + tuple(self.transform(im)) + (target,)   # (image, box, flip[, aug], target)


def rank_share(n, rank, world, seed):
    """the samples a rank keeps resident for the whole run: randperm(n, seed)[rank::world], the list padded by wrapping around as
    DecodedLoader._indices pads it (every rank the same count)"""
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
    per_rank = (n + world - 1) // world
    idx += idx[:per_rank * world - n]
    return idx[rank:per_rank * world:world]


class ResidentStore(object):
    """A rank's share of a DecodedStore in device memory: one uint8 tensor (`pool`) and a device offset per sample (`offset`).  The
    upload runs on first use (`ensure()`), in runs of adjacent samples through one pinned bounce buffer of 64 MB.  The share plus
    `reserve_gb` must fit into the free device memory at that moment; otherwise ValueError -- nothing falls back to host mode."""

    def __init__(self, store, rank=0, world=1, seed=0, reserve_gb=32):
        self.store, self.rank, self.world, self.seed, self.reserve_gb = store, int(rank), int(world), int(seed), float(reserve_gb)
        self.share = rank_share(len(store), self.rank, self.world, self.seed)
        self.count = np.bincount(np.asarray(self.share, dtype=np.int64), minlength=len(store))   # (a wrapped sample can count twice)
        self.pool, self.offset = None, None

    def plan(self):
        """-> (runs, offsets, total): runs of store bytes that are adjacent in a shard [(shard, first byte, bytes, device offset)],
        the device offset of every sample of the share (dict), the pool size"""
        idx, nb = self.store.index, self.store.nbytes
        runs, offsets, total = [], {}, 0
        for i in np.flatnonzero(self.count).tolist():
            s, off, n = int(idx["shard"][i]), int(idx["off"][i]), int(nb[i])
            if runs and runs[-1][0] == s and runs[-1][1] + (runs[-1][2] + ALIGN - 1) // ALIGN * ALIGN == off:
                r = runs[-1]
                offsets[i] = r[3] + (off - r[1])
                runs[-1] = (s, r[1], off - r[1] + n, r[3])
            else:
                start = (total + ALIGN - 1) // ALIGN * ALIGN
                offsets[i] = start
                runs.append((s, off, n, start))
            total = runs[-1][3] + runs[-1][2]
        return runs, offsets, total

    def ensure(self):
        if self.pool is not None:
            return self
        runs, offsets, total = self.plan()
        free = torch.cuda.mem_get_info()[0]
        reserve = int(self.reserve_gb * (1 << 30))
        if total + reserve > free:
            raise ValueError("resident image store %s: the share of rank %d / %d is %d bytes (%.2f GiB), with the reserve of %d bytes "
                             "(dataset_resident_reserve_gb) %d bytes are needed and %d bytes (%.2f GiB) of device memory are free -- build a "
                             "smaller store (tools/make_image_store.py --max-side) or train in host mode (dataset_resident: False)"
                             % (self.store.root, self.rank, self.world, total, total / 2.0 ** 30, reserve, total + reserve, free, free / 2.0 ** 30))
        pool = torch.empty(max(total, ALIGN), dtype=torch.uint8, device="cuda")
        bounce = torch.empty(min(BOUNCE_BYTES, max(total, ALIGN)), dtype=torch.uint8).pin_memory()
        host, cap, r = bounce.numpy(), bounce.numel(), 0
        for base in range(0, total, cap):   # the pool in windows of the bounce buffer; runs are in device order
            end = min(base + cap, total)
            while r < len(runs) and runs[r][3] < end:
                s, first, nbytes, dev = runs[r]
                lo, hi = max(dev, base), min(dev + nbytes, end)   # (between two runs: alignment padding, never read)
                host[lo - base:hi - base] = self.store.maps[s][first + lo - dev:first + hi - dev]
                if dev + nbytes > end:
                    break   # the rest of this run belongs to the next window
                r += 1
            pool[base:end].copy_(bounce[:end - base], non_blocking=True)
            torch.cuda.current_stream().synchronize()   # the one bounce buffer is rewritten next
        del bounce
        self.pool, self.offset = pool, offsets
        return self


class ResidentLoader(object):
    """DecodedLoader's role over a ResidentStore: batches (ResidentImages, boxes, flips, targets[, augs]) -- offsets instead of
    images.  The rank's share is fixed; an epoch visits it in the order in which randperm(n, seed + epoch) meets its samples
    (shuffle=False: index order), so with world == 1 the sample order, and with it every random decision of the transform, is
    DecodedLoader's.  With world > 1 this is a fixed-shard sampler, not DistributedSampler: a rank never sees another rank's share."""

    def __init__(self, resident, batch_size, shuffle, drop_last=False, seed=0):
        self.resident, self.dset = resident, resident.store   # `dset`: where train.py finds the split's transform
        self.batch_size, self.shuffle, self.drop_last, self.seed = int(batch_size), bool(shuffle), bool(drop_last), int(seed)
        self.epoch = 0
        self.per_rank = len(resident.share)

    def __len__(self):
        return self.per_rank // self.batch_size if self.drop_last else (self.per_rank + self.batch_size - 1) // self.batch_size

    def set_epoch(self, epoch):
        """as DecodedLoader.set_epoch: the next pass is pass `epoch` of a fresh loader"""
        self.epoch = int(epoch)

    def _indices(self):
        n = len(self.dset)
        if self.shuffle:
            order = torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + self.epoch)).numpy()
        else:
            order = np.arange(n)
        return np.repeat(order, self.resident.count[order]).tolist()

    def __iter__(self):
        idx = self._indices()
        self.epoch += 1
        res = self.resident.ensure()
        store, tf = self.dset, self.dset.transform
        for b in range(len(self)):
            chunk = idx[b * self.batch_size:(b + 1) * self.batch_size]
            sizes = [store.size_of(i) for i in chunk]
            dec = [tuple(tf((W, H))) for H, W in sizes]   # the deciders need the size only; drawn in sample order
            target = torch.tensor([store._rec[i][4] for i in chunk], dtype=torch.int64).pin_memory()
            extra = ([d[2] if len(d) > 2 else None for d in dec],) if any(len(d) > 2 for d in dec) else ()
            images = dataflow.ResidentImages(res.pool, [res.offset[i] for i in chunk], sizes)
            yield (images, [d[0] for d in dec], [d[1] for d in dec], target) + extra
