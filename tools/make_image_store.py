#!/usr/bin/env python
"""Decode one image-folder split into a decoded image store (atomnas_amd/utils/image_store.py):

    python tools/make_image_store.py SRC_SPLIT_DIR OUT_DIR [--workers N] [--shard-bytes B] [--max-side S]

SRC_SPLIT_DIR is what `dataset: imagenet1k` reads (`<class>/<file>`, e.g. $DATA/train); OUT_DIR is what `dataset: imagenet1k_store`
reads (dataset_dir/train, dataset_dir/val).  Same class order, file order and decoder as ImageFolderDecoded, so the store's samples
are byte for byte what the image-folder path feeds.  Written to OUT_DIR.partial and renamed when complete; an existing OUT_DIR is
refused.  --max-side S makes a LOSSY store (recorded in meta.json): an image whose shorter side exceeds S is resized with PIL's
BICUBIC so that it is S -- what lets one card hold a whole train split in resident mode."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    from atomnas_amd.utils import image_store
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src")
    ap.add_argument("out")
    ap.add_argument("--workers", type=int, default=8, help="decode threads (at most 16)")
    ap.add_argument("--shard-bytes", type=int, default=image_store.DEFAULT_SHARD_BYTES, help="cap of one pixels file (default 1 GiB)")
    ap.add_argument("--max-side", type=int, default=None, help="lossy: cap the shorter side of every image")
    args = ap.parse_args(argv)
    t0 = time.time()
    n = image_store.build_store(args.src, args.out, workers=args.workers, shard_bytes=args.shard_bytes, max_side=args.max_side)
    store = image_store.DecodedStore(args.out, None)
    print("%s: %d samples, %d classes, %d shards, %.3f GB, max_side %s, %.1f s" % (
        args.out, n, len(store.classes), len(store.shard_bytes), sum(store.shard_bytes) / 1e9, store.max_side, time.time() - t0))


if __name__ == "__main__":
    main()
