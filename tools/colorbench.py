"""Times the colour pass of 'imagenet1k_mobile' (atomnas_image_color) and the resize in front of it on a training-sized batch:

    python tools/colorbench.py [--batch 256] [--size 224] [--reps 200] [--out FILE.json]

 (a) the colour pass alone, in both forms (two launches: per-image reduction + per-pixel chain; one launch: image in LDS), against
     its algorithmic bytes -- the uint8 image read twice / once, the fp32 batch written once -- and the share of 8 TB/s HBM peak;
 (b) resize (uint8) + colour pass against atomnas_image_preprocess writing the fp32 batch directly (what a batch without colour
     decisions costs).
Device events around `reps` back-to-back launches on one stream (the stream is busy: no launch waits for the host), alternating the
variants over three rounds; prints one JSON line per figure."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from atomnas_amd.utils import dataflow as DF
    if not torch.cuda.is_available():
        raise SystemExit("colorbench needs the GPU")
    n, S = args.batch, args.size
    F = dict(data_transforms="imagenet1k_mobile", image_size=S)

    class _F(dict):
        __getattr__ = dict.__getitem__
    tr = DF.data_transforms(_F(F))[0]
    random.seed(7)
    np.random.seed(7)
    imgs, boxes, flips, _, augs = next(iter(DF.SyntheticDecodedImages(n, 1, image_size=S, seed=7, transform=tr)))
    plan = DF.batch_plan([(int(im.shape[0]), int(im.shape[1])) for im in imgs], boxes, flips, augs, S)
    pool = torch.zeros(plan.total, dtype=torch.uint8, device="cuda")
    d, a = np.zeros(n, dtype=DF.DESC_DTYPE), np.zeros(n, dtype=DF.AUG_DTYPE)
    plan.write(d, a, np.zeros(n, dtype=np.int32))
    for im, off, nb in zip(imgs, plan.offs, plan.nbytes):
        pool[off:off + nb] = im.reshape(-1).cuda()
    desc = torch.from_numpy(d.view(np.uint8).copy()).cuda()
    aug_dev = torch.from_numpy(a.view(np.uint8).copy()).cuda()
    stage = torch.empty(n, S, S, 3, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, 3, S, S, dtype=torch.float32, device="cuda")
    means = torch.empty(n, dtype=torch.int32, device="cuda")
    mean, std = tr.mean, tr.std
    forms = ["two_launch"] + (["lds"] if S % 2 == 0 and S * S * 3 <= 160 * 1024 - 256 else [])
    DF.preprocess(pool, desc, n, S, mean, std, stage, 2)

    variants = {}
    for form in forms:
        variants["color_" + form] = (lambda form=form: DF.color(stage, aug_dev, n, S, mean, std, out, means, 0, form=form))

        def chain(form=form):
            DF.preprocess(pool, desc, n, S, mean, std, stage, 2)
            DF.color(stage, aug_dev, n, S, mean, std, out, means, 0, form=form)
        variants["resize_u8+color_" + form] = chain
    variants["resize_fp32 (no colour)"] = lambda: DF.preprocess(pool, desc, n, S, mean, std, out, 0)
    variants["resize_u8"] = lambda: DF.preprocess(pool, desc, n, S, mean, std, stage, 2)

    # the forms agree bit for bit before anything is timed
    ref = None
    for form in forms:
        out.fill_(float("nan"))
        variants["color_" + form]()
        torch.cuda.synchronize()
        if ref is None:
            ref = out.clone()
        elif not torch.equal(ref, out):
            raise SystemExit("the forms of atomnas_image_color disagree")

    times = {k: [] for k in variants}
    for rnd in range(4):   # round 0 is warm-up
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            e1.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.reps)
    img_b, out_b = S * S * 3, S * S * 3 * 4
    bytes_of = {"color_two_launch": n * (2 * img_b + out_b), "color_lds": n * (img_b + out_b)}
    lines = []
    for name, t in times.items():
        r = dict(name=name, batch=n, size=S, us=round(sorted(t)[len(t) // 2], 2), us_rounds=[round(x, 2) for x in t])
        if name in bytes_of:
            r["algorithmic_bytes"] = bytes_of[name]
            r["tb_per_s"] = round(bytes_of[name] / (r["us"] * 1e-6) / 1e12, 3)
            r["share_of_hbm_peak"] = round(bytes_of[name] / (r["us"] * 1e-6) / HBM_PEAK, 3)
        lines.append(r)
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
