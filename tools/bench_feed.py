#!/usr/bin/env python
"""The AtomNAS-C supernet step at batch 256 fed with real files: what an image folder, a decoded image store in host mode and the
same store resident in device memory deliver per second.

    python tools/bench_feed.py --make-folder DIR                 2,048 synthetic JPEGs (quality 90, smooth content plus noise, the
                                                                 SyntheticDecodedImages.SIZES sizes) as DIR/<class>/<file>
    python tools/bench_feed.py --folder DIR --store STORE_DIR    builds the store if STORE_DIR does not exist, then times the sources
        [--sources folder,host,resident] [--steps 100] [--warmup 20] [--transforms imagenet1k_mnas_bilinear]

Per source: the factories' loader (dataflow.data_loader: 16 decode threads for the folder) -> DevicePrefetcher as train.py builds it
-> TrainStep.set_batch + step, `warmup` steps and then `steps` timed ones; one JSON line each with images/s, ms per step and the
milliseconds per batch the prefetcher's host thread spent drawing the batch, waiting for the device to release the slot's pinned
buffers (idle: the device is the bottleneck then), writing the tables, staging and queueing.  The 2,048 files
are cycled (8 batches per pass, the loader reshuffles each pass) through ONE prefetcher; train.py starts one per epoch.  The transform
defaults to the bilinear one of `bench.py --input-pipeline uint8`, so that the resident line runs the kernel of that figure.  JPEG
decode speed depends on the content: the folder line is indicative only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES, FILES = 16, 2048


def make_folder(root, seed=0):
    import numpy as np
    from PIL import Image
    from atomnas_amd.utils.dataflow import SyntheticDecodedImages
    import concurrent.futures
    for c in range(CLASSES):
        os.makedirs(os.path.join(root, "n%04d" % c))

    def write(k):
        rng = np.random.RandomState(seed * FILES + k)
        H, W = SyntheticDecodedImages.SIZES[k % len(SyntheticDecodedImages.SIZES)]
        d = os.path.join(root, "n%04d" % (k % CLASSES))
        yy, xx = np.mgrid[0:H, 0:W]
        fy, fx, ph = rng.uniform(1, 6, 3), rng.uniform(1, 6, 3), rng.uniform(0, 6.28, 3)
        smooth = np.stack([127 + 100 * np.sin(fy[c] * yy / H + fx[c] * xx / W + ph[c]) for c in range(3)], axis=2)
        arr = np.clip(smooth + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(arr).save(os.path.join(d, "%05d.JPEG" % k), quality=90)

    with concurrent.futures.ThreadPoolExecutor(max_workers=16) as pool:
        list(pool.map(write, range(FILES)))


class Cycle(object):
    """a loader's epochs back to back, `batches` batches in all"""

    def __init__(self, loader, batches):
        self.loader, self.dset, self.batches = loader, loader.dset, batches

    def __len__(self):
        return self.batches

    def __iter__(self):
        k = 0
        while k < self.batches:
            for batch in self.loader:
                if k == self.batches:
                    return
                k += 1
                yield batch


class Flags(dict):
    __getattr__ = dict.__getitem__


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--make-folder", metavar="DIR")
    ap.add_argument("--folder")
    ap.add_argument("--store")
    ap.add_argument("--sources", default="folder,host,resident")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--transforms", default="imagenet1k_mnas_bilinear")
    ap.add_argument("--reserve-gb", type=float, default=32)
    args = ap.parse_args()
    if args.make_folder:
        t0 = time.time()
        make_folder(args.make_folder)
        print("wrote %d JPEGs under %s in %.1f s" % (FILES, args.make_folder, time.time() - t0))
        return
    import torch
    import bench
    from atomnas_amd.utils import dataflow as DF
    from atomnas_amd.utils import image_store as IS
    if not os.path.exists(args.store):
        t0 = time.time()
        n = IS.build_store(args.folder, args.store, workers=16)
        print("built %s: %d samples in %.1f s" % (args.store, n, time.time() - t0), flush=True)
    model, ts, hp, opt, ema, pinfo = bench.build("atomnas_c_supernet", torch.bfloat16, args.batch, seed=1995)
    ts.use_graph = True
    total = args.warmup + args.steps
    for source in args.sources.split(","):
        F = Flags(data_transforms=args.transforms, data_loader="imagenet1k_basic", image_size=hp['image_size'], use_distributed=False,
                  test_only=False, bn_calibration=False, random_seed=1995, drop_last=True, _loader_batch_size=args.batch,
                  data_loader_workers=16 if source == "folder" else 0, dataset_resident=source == "resident",
                  dataset_resident_reserve_gb=args.reserve_gb)
        tf = DF.data_transforms(F)[0]
        dset = DF.ImageFolderDecoded(args.folder, tf) if source == "folder" else IS.DecodedStore(args.store, tf)
        loader = DF.data_loader(dset, dset, None, F)[0]
        pre = DF.DevicePrefetcher(Cycle(loader, total + 1), image_size=hp['image_size'], filter=tf.filter, mean=tf.mean, std=tf.std,
                                  staging=isinstance(dset, IS.DecodedStore))
        try:
            for k in range(total):
                if k == args.warmup:
                    torch.cuda.synchronize()
                    host0, t0 = dict(pre.host_seconds), time.perf_counter()
                x, y = next(pre)
                ts.set_batch(x, y)
                ts.step(lr=hp['base_lr'], rho=1e-4)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            host = {k: round((v - host0[k]) / args.steps * 1e3, 3) for k, v in pre.host_seconds.items()}
        finally:
            pre.close()
        loss = ts.loss.tolist()
        if not all(v == v and abs(v) < 1e6 for v in loss):
            raise SystemExit("bench_feed.py: the timed steps did not train (loss %s)" % loss)
        print(json.dumps(dict(source=source, transforms=args.transforms, images_per_sec=round(args.batch * args.steps / dt, 1),
                              ms_per_step=round(dt / args.steps * 1e3, 3), steps=args.steps, warmup=args.warmup, batch=args.batch,
                              prefetch_host_ms_per_batch=host, store_bytes=sum(dset.shard_bytes) if source != "folder" else None)), flush=True)


if __name__ == "__main__":
    main()
