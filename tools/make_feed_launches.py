#!/usr/bin/env python
"""Writes tests/golden/feed_launches.json: what DevicePrefetcher (atomnas_amd/utils/dataflow.py) launches, batch by batch, with which
descriptor / augmentation tables, and what it hands out.

Every case iterates one DevicePrefetcher(threaded=False) over a fixed loader with the five module-level launch wrappers of dataflow
(preprocess, preprocess_large, resize_window, resize_window_large, color) replaced by recorders.  A recorder synchronises the stream it
is given, reads the device tables back and calls through to the real wrapper.  Recorded per case:
  "calls"     per launch: entry name, n (or m), size, out_mode, filter, max_rows, the selected slots, and the SHA-1 of the first n
              descriptor records and of the first n augmentation records (None where the launch takes no such table),
  "outputs"   the SHA-1 of every (x, y) handed out,
  "error"     for a refused batch: [exception type, text].
The kernels are integer resamplers followed by a fixed fp32 normalise: equal tables on equal pixels give equal bytes, so the digests
are an equality.  tests/test_feed_launches_gpu.py asserts the code under test against the table and tests/test_feed_plan.py restates
its tables on the CPU, so the table PINS the feed path: generate it from the dataflow.py whose behaviour is to be kept, never from the
code under change.  Only interfaces that a restructuring of dataflow.py leaves alone are used: the wrappers' names and signatures,
DESC_DTYPE / AUG_DTYPE, ResidentImages, SyntheticDecodedImages and DevicePrefetcher's constructor and iterator protocol.  Every run
happens in a child interpreter whose environment has every ATOMNAS_* variable stripped except ATOMNAS_HIP_LIB.

    python tools/make_feed_launches.py [out.json]      (GPU box; runs the cases twice and writes the file only if both runs agree)
    python tools/make_feed_launches.py --emit          (what a child prints: one JSON line)
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = 32   # the output side of every case: a GPU run of the whole table takes seconds
ENTRIES = ("image_preprocess", "image_preprocess_large", "image_resize_window", "image_resize_window_large", "image_color")


def cases():
    """the case list, in table order"""
    out = []
    for staging in (False, True):
        sfx = "_staged" if staging else ""
        for filt in ("bilinear", "bicubic"):
            out.append(dict(name="synthetic_%s%s" % (filt, sfx), kind="synthetic", filter=filt, staging=staging))
        out.append(dict(name="fixed%s" % sfx, kind="fixed", filter="bilinear", staging=staging))
    out.append(dict(name="resident", kind="resident", filter="bilinear", staging=False))
    for k in ("mixed", "outside", "four_ops", "two_contrasts"):
        out.append(dict(name="refused_" + k, kind="refused", refusal=k, filter="bilinear", staging=False))
    return out


class Fixed(object):
    """a loader over fixed batches"""

    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def _images(shapes, seed, pin):
    import torch
    g = torch.Generator().manual_seed(seed)
    ims = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g) for H, W in shapes]
    return [im.pin_memory() for im in ims] if pin else ims


def _window(ims, short):
    """(boxes, augs) of Resize(short) + CenterCrop(SIZE), the way ColorDeviceTransform decides them"""
    from atomnas_amd.utils import transforms as T
    wins = [T.Resize(short).get_size(im) for im in ims]
    return [T.CenterCrop(SIZE).get_box((ow, oh)) for oh, ow in wins], [T.Aug(None, None, w) for w in wins]


def fixed_batches(pin):
    """the four fixed batches of case (b): a colour batch with one oversize crop box and one aug of None, a four-element batch, a
    window batch with one oversize image, and the first batch again"""
    import torch
    from atomnas_amd.utils import transforms as T
    a = _images([(300, 310), (41, 37), (64, 48)], 21, pin)
    ops = ((T.CONTRAST, 1.25), (T.BRIGHTNESS, 0.75), (T.SATURATION, 1.5))
    colour = (a, [(2, 3, 295, 200), (1, 2, 37, 33), (0, 0, 64, 48)], [True, False, True], torch.tensor([1, 2, 3]),
              [T.Aug(ops, (5.5, -3.25, 1.0), None), None, T.Aug(ops[1:], None, None)])
    b = _images([(37, 41), (50, 33), (64, 64), (33, 35)], 22, pin)
    plain = (b, [(3, 5, 33, 34), (0, 0, 50, 33), (10, 12, 40, 41), (1, 1, 32, 32)], [False, True, True, False], torch.tensor([4, 5, 6, 7]))
    c = _images([(330, 340), (50, 60), (75, 40)], 23, pin)
    boxes, augs = _window(c, 36)
    window = (c, boxes, [False, True, False], torch.tensor([8, 9, 10]), augs)
    return [colour, plain, window, colour]


def refused_batch(kind):
    import torch
    from atomnas_amd.utils import transforms as T
    ims = _images([(50, 60), (75, 40)], 24, False)
    boxes, flips, tgt = [(0, 0, 40, 40), (5, 5, 35, 33)], [False, True], torch.tensor([0, 1])
    if kind == "mixed":
        wb, wa = _window(ims, 36)
        return (ims, wb, flips, tgt, [wa[0], None])
    if kind == "outside":
        return (ims, [boxes[0], (50, 5, 30, 30)], flips, tgt)
    if kind == "four_ops":
        ops = ((T.BRIGHTNESS, 1.1), (T.SATURATION, 0.9), (T.CONTRAST, 1.2), (T.BRIGHTNESS, 0.8))
    else:
        ops = ((T.CONTRAST, 1.1), (T.CONTRAST, 0.9))
    return (ims, boxes, flips, tgt, [None, T.Aug(ops, None, None)])


def resident_parts():
    """(pool bytes as a uint8 CPU tensor, offs, sizes, boxes, flips, targets) of case (d): three images at 16-byte-aligned offsets"""
    import torch
    ims = _images([(45, 50), (300, 40), (33, 64)], 25, False)
    offs, off = [], 32
    for im in ims:
        offs.append(off)
        off += (im.numel() + 15) // 16 * 16 + 16
    pool = torch.zeros(off, dtype=torch.uint8)
    for im, o in zip(ims, offs):
        pool[o:o + im.numel()] = im.reshape(-1)
    order = [2, 0, 1, 0]
    boxes = [(0, 2, 33, 60), (0, 0, 45, 50), (3, 4, 292, 33), (5, 6, 35, 40)]
    return (pool, [offs[i] for i in order], [tuple(ims[i].shape[:2]) for i in order], boxes, [False, True, False, True],
            torch.tensor([3, 2, 1, 0]))


def loader_of(c, gpu):
    """the loader of a case.  gpu=False builds the same batches without touching the device (tests/test_feed_plan.py); the resident
    case then carries (offs, sizes) instead of a ResidentImages"""
    import torch
    from atomnas_amd.utils import dataflow as DF
    if c["kind"] == "synthetic":
        loader = DF.SyntheticDecodedImages(batch=5, steps=3, image_size=SIZE, pool_size=6, seed=1)
        if c["staging"]:
            loader.images = [im.clone() for im in loader.images]   # (a decoded store hands out unpinned views)
        return loader
    if c["kind"] == "fixed":
        return Fixed(fixed_batches(gpu and not c["staging"]))
    if c["kind"] == "refused":
        return Fixed([refused_batch(c["refusal"])])
    pool, offs, sizes, boxes, flips, tgt = resident_parts()
    images = DF.ResidentImages(pool.cuda(), offs, sizes) if gpu else (offs, sizes)
    return Fixed([(images, boxes, flips, tgt)])


def sha(t):
    import torch
    return hashlib.sha1(t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


class Recorders(object):
    """replaces the five launch wrappers of dataflow by recorders that call through; restore() puts the wrappers back"""

    def __init__(self, DF):
        import numpy as np
        self.DF, self.np, self.calls, self.n = DF, np, [], 0
        self.real = {k: getattr(DF, k) for k in ("preprocess", "preprocess_large", "resize_window", "resize_window_large", "color")}
        rec, real = self._rec, self.real

        def preprocess(pool_dev, desc_dev, n, size, mean, std, out, out_mode=0, stream=None, filter="bilinear"):
            rec(ENTRIES[0], stream, n, size, out_mode, filter, desc=desc_dev)
            real["preprocess"](pool_dev, desc_dev, n, size, mean, std, out, out_mode, stream, filter)

        def preprocess_large(pool_dev, desc_dev, sel_dev, m, max_rows, size, mean, std, out, workspace, out_mode=0, stream=None,
                             filter="bilinear"):
            rec(ENTRIES[1], stream, m, size, out_mode, filter, max_rows, sel_dev, desc=desc_dev)
            real["preprocess_large"](pool_dev, desc_dev, sel_dev, m, max_rows, size, mean, std, out, workspace, out_mode, stream, filter)

        def resize_window(pool_dev, desc_dev, aug_dev, n, size, mean, std, out, out_mode=0, stream=None, filter="bilinear"):
            rec(ENTRIES[2], stream, n, size, out_mode, filter, desc=desc_dev, aug=aug_dev)
            real["resize_window"](pool_dev, desc_dev, aug_dev, n, size, mean, std, out, out_mode, stream, filter)

        def resize_window_large(pool_dev, desc_dev, aug_dev, sel_dev, m, max_rows, size, mean, std, out, workspace, out_mode=0, stream=None,
                                filter="bilinear"):
            rec(ENTRIES[3], stream, m, size, out_mode, filter, max_rows, sel_dev, desc=desc_dev, aug=aug_dev)
            real["resize_window_large"](pool_dev, desc_dev, aug_dev, sel_dev, m, max_rows, size, mean, std, out, workspace, out_mode, stream,
                                        filter)

        def color(src, aug_dev, n, size, mean, std, out, means, out_mode=0, stream=None, form="auto"):
            rec(ENTRIES[4], stream, n, size, out_mode, None, aug=aug_dev)
            real["color"](src, aug_dev, n, size, mean, std, out, means, out_mode, stream, form)

        for f in (preprocess, preprocess_large, resize_window, resize_window_large, color):
            setattr(DF, f.__name__, f)

    def _rec(self, entry, stream, count, size, out_mode, filt, max_rows=None, sel_dev=None, desc=None, aug=None):
        import torch
        np, DF = self.np, self.DF
        (stream or torch.cuda.current_stream()).synchronize()
        if sel_dev is None:
            self.n = int(count)   # (the n of a batch: its two-pass and colour launches digest the same records)
        n = self.n
        row = dict(entry=entry, count=int(count), size=int(size), out_mode=int(out_mode), filter=filt, max_rows=max_rows, sel=None, desc=None,
                   aug=None)
        if sel_dev is not None:
            row["max_rows"] = int(max_rows)
            row["sel"] = np.frombuffer(sel_dev.cpu().numpy().tobytes(), dtype=np.int32, count=int(count)).tolist()
        if desc is not None:
            row["desc"] = hashlib.sha1(desc.cpu().numpy().tobytes()[:n * DF.DESC_DTYPE.itemsize]).hexdigest()
        if aug is not None:
            row["aug"] = hashlib.sha1(aug.cpu().numpy().tobytes()[:n * DF.AUG_DTYPE.itemsize]).hexdigest()
        self.calls.append(row)

    def restore(self):
        for k, f in self.real.items():
            setattr(self.DF, k, f)


def run_case(c):
    from atomnas_amd.utils import dataflow as DF
    rec = Recorders(DF)
    out = dict(name=c["name"], calls=rec.calls, outputs=[], error=None)
    pf = None
    try:
        pf = DF.DevicePrefetcher(loader_of(c, True), image_size=SIZE, threaded=False, filter=c["filter"], staging=c["staging"])
        for x, y in pf:
            out["outputs"].append([sha(x), sha(y)])
    except (ValueError, NotImplementedError) as e:
        out["error"] = [type(e).__name__, str(e)]
    finally:
        if pf is not None:
            pf.close()
        rec.restore()
    return out


def check(table):
    """what a table must show before it may be written or trusted: every case, and every launch form where the case list says it is"""
    by = {r["name"]: r for r in table}
    assert [r["name"] for r in table] == [c["name"] for c in cases()], "the table's cases are not the generator's"
    ent = lambda n: [r["entry"] for r in by[n]["calls"]]
    for sfx in ("", "_staged"):
        assert ent("fixed" + sfx) == [ENTRIES[0], ENTRIES[1], ENTRIES[4], ENTRIES[0], ENTRIES[2], ENTRIES[3], ENTRIES[0], ENTRIES[1], ENTRIES[4]]
        calls = by["fixed" + sfx]["calls"]
        assert calls[1]["sel"] == [0] and calls[1]["max_rows"] == 295 and calls[5]["sel"] == [0] and calls[5]["max_rows"] == 330
        assert [r["out_mode"] for r in calls] == [2, 2, 0, 0, 0, 0, 2, 2, 0]
        assert calls[0]["desc"] == calls[6]["desc"] and calls[2]["aug"] == calls[8]["aug"] and calls[3]["aug"] is None
        assert len(by["fixed" + sfx]["outputs"]) == 4 and by["fixed" + sfx]["outputs"][0] == by["fixed" + sfx]["outputs"][3]
        for filt in ("bilinear", "bicubic"):
            r = by["synthetic_%s%s" % (filt, sfx)]
            assert len(r["outputs"]) == 3 and set(e["entry"] for e in r["calls"]) <= set(ENTRIES[:2]) and all(e["filter"] == filt for e in r["calls"])
    assert by["fixed"]["outputs"] == by["fixed_staged"]["outputs"] and by["fixed"]["calls"][0]["desc"] != by["fixed_staged"]["calls"][0]["desc"]
    assert by["synthetic_bicubic"]["outputs"] == by["synthetic_bicubic_staged"]["outputs"] != by["synthetic_bilinear"]["outputs"]
    assert ent("resident") == [ENTRIES[0], ENTRIES[1]] and by["resident"]["calls"][1]["sel"] == [2] and len(by["resident"]["outputs"]) == 1
    for r in table:
        assert (r["error"] is not None) == r["name"].startswith("refused_") and (r["error"] is None or not r["outputs"]), r["name"]
    assert by["refused_mixed"]["error"] == ["ValueError", "a batch mixes resize-window and crop-box samples"]
    assert by["refused_outside"]["error"][1].startswith("crop box (50, 5, 30, 30) outside")
    assert all(by["refused_" + k]["error"][1].startswith("colour decision") for k in ("four_ops", "two_contrasts"))


def emit():
    import torch
    prop = torch.cuda.get_device_properties(0)
    return dict(header=dict(device=prop.name, size=SIZE), cases=[run_case(c) for c in cases()])


def in_child(timeout=300):
    """emit() of a fresh interpreter with every ATOMNAS_* variable of the caller stripped except the library override"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ATOMNAS_") or k == "ATOMNAS_HIP_LIB"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit"], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def load(path=os.path.join(ROOT, "tests", "golden", "feed_launches.json")):
    """(header, [case]) of a written table: the header line, then one compact line per case"""
    lines = [json.loads(l) for l in open(path) if l.strip()]
    return lines[0], lines[1:]


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--emit":
        print(json.dumps(emit()))
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "feed_launches.json")
    a, b = in_child(), in_child()
    assert a == b, "two runs disagree: %s" % [x["name"] for x, y in zip(a["cases"], b["cases"]) if x != y]
    check(a["cases"])
    with open(out, "w") as f:
        f.write(json.dumps(a["header"], sort_keys=True) + "\n")
        for r in a["cases"]:
            f.write(json.dumps(r, sort_keys=True, separators=(",", ":")) + "\n")
    print("%d cases, %d calls, %d batches on %s -> %s" % (len(a["cases"]), sum(len(r["calls"]) for r in a["cases"]),
                                                          sum(len(r["outputs"]) for r in a["cases"]), a["header"]["device"], out))


if __name__ == "__main__":
    main()
