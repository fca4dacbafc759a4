"""Input pipeline on the GPU: the reference's DataPrefetcher (utils/dataflow.py:13-58) with the per-sample pixel work
moved into a HIP kernel.

    reference:  DataLoader workers: PIL decode -> crop -> resize -> flip -> ToTensor -> Normalize (CPU)  -> prefetcher: H2D of fp32 batches
    here:       loader: decoded uint8 HWC images + (box, flip) decisions (atomnas_amd/utils/transforms.py) -> prefetcher: H2D of the
                uint8 pixels on a side stream (a quarter of the fp32 bytes), atomnas_image_preprocess on that stream -> fp32 NCHW batch

Same iterator protocol as the reference's DataPrefetcher (__iter__ / __next__ / __len__, batch k + 1 in flight while batch k trains,
`torch.cuda.current_stream().wait_stream(side)` at hand-over).  Decoding stays on the host, as in the reference: `dataset: imagenet1k`
(image folders) decodes JPEG / PNG with PIL on loader threads (ImageFolderDecoded); LMDB records cannot be read here (no lmdb module).
Loaders hand over decoded uint8 arrays, e.g. SyntheticDecodedImages below (bench.py --input-pipeline uint8).  `dataset: imagenet1k_store`
(image_store.py) reads image folders that were decoded ONCE into flat uint8 shards: no decode per epoch, one staged copy per batch
(DevicePrefetcher(staging=True)), or no pixel copy at all with the store resident in device memory (`dataset_resident: True`).
"""
import concurrent.futures
import ctypes
import importlib
import os
import queue
import random
import threading
import time

import numpy as np
import torch

from .. import _lib
from . import transforms as T

DESC_DTYPE = np.dtype([("off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("bi", "<i4"), ("bj", "<i4"), ("bh", "<i4"), ("bw", "<i4"), ("flip", "<i4"),
                       ("pad", "<i4")])   # struct atomnas_img_desc (include/atomnas_hip.h), 40 bytes
AUG_DTYPE = np.dtype([("oh", "<i4"), ("ow", "<i4"), ("top", "<i4"), ("left", "<i4"), ("op", "<i4", (3,)), ("pad", "<i4"), ("factor", "<f4", (3,)),
                      ("pad2", "<f4"), ("inc", "<f8", (3,))])   # struct atomnas_img_aug (include/atomnas_hip.h), 72 bytes
COLOR_OPS = {T.BRIGHTNESS: 1, T.CONTRAST: 2, T.SATURATION: 3}   # atomnas_img_aug.op
COLOR_FORMS = {"auto": 0, "two_launch": 1, "lds": 2}            # the `form` argument of atomnas_image_color
MAX_SCALE = 9.0   # the one-pass kernel's tap budget: a crop side above 9x the output side goes through atomnas_image_preprocess_large
FILTERS = {"bilinear": 0, "bicubic": 1}   # the `filter` argument of atomnas_image_preprocess: PIL's BILINEAR / BICUBIC resamplers


def _launch(entry, before, mean, std, out, out_mode, filter, after, stream):
    """the one call behind the five wrappers below.  Every atomnas_image_* entry takes `before`, mean, std, out, out_mode, the filter
    code (none for the colour pass), `after` and the stream, in that order; a tensor goes as its pointer, anything else as an int"""
    arg = lambda v: ctypes.c_void_p(v.data_ptr()) if torch.is_tensor(v) else int(v)
    m, s = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    code = () if filter is None else (FILTERS[filter],)
    _lib.call(entry, *[arg(v) for v in before], ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), arg(out), int(out_mode),
              *code, *[arg(v) for v in after], ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream))


def preprocess(pool_dev, desc_dev, n, size, mean, std, out, out_mode=0, stream=None, filter="bilinear"):
    """launches atomnas_image_preprocess: pool_dev uint8 device tensor, desc_dev uint8 device tensor holding n DESC_DTYPE records"""
    _launch("atomnas_image_preprocess", (pool_dev, desc_dev, n, size), mean, std, out, out_mode, filter, (), stream)


def preprocess_large(pool_dev, desc_dev, sel_dev, m, max_rows, size, mean, std, out, workspace, out_mode=0, stream=None, filter="bilinear"):
    """launches atomnas_image_preprocess_large after preprocess() on the same stream: rewrites the m batch slots listed in sel_dev
    (int32 device tensor) through the two-pass form; workspace: uint8 device tensor of at least m * max_rows * size * 3 bytes"""
    _launch("atomnas_image_preprocess_large", (pool_dev, desc_dev, sel_dev, m, max_rows, size), mean, std, out, out_mode, filter,
            (workspace, workspace.numel()), stream)


def resize_window(pool_dev, desc_dev, aug_dev, n, size, mean, std, out, out_mode=0, stream=None, filter="bilinear"):
    """launches atomnas_image_resize_window (Resize + CenterCrop): aug_dev uint8 device tensor holding n AUG_DTYPE records"""
    _launch("atomnas_image_resize_window", (pool_dev, desc_dev, aug_dev, n, size), mean, std, out, out_mode, filter, (), stream)


def resize_window_large(pool_dev, desc_dev, aug_dev, sel_dev, m, max_rows, size, mean, std, out, workspace, out_mode=0, stream=None,
                        filter="bilinear"):
    """launches atomnas_image_resize_window_large after resize_window() on the same stream (max_rows: the tallest selected IMAGE)"""
    _launch("atomnas_image_resize_window_large", (pool_dev, desc_dev, aug_dev, sel_dev, m, max_rows, size), mean, std, out, out_mode, filter,
            (workspace, workspace.numel()), stream)


def color(src, aug_dev, n, size, mean, std, out, means, out_mode=0, stream=None, form="auto"):
    """launches atomnas_image_color: src uint8 [n, size, size, 3] device tensor (out_mode 2 of the resize), aug_dev as above, means an
    int32 device tensor of at least n elements (scratch)"""
    if src.numel() < n * size * size * 3 or means.numel() < n:
        raise ValueError("atomnas_image_color: source or scratch buffer too small")
    _launch("atomnas_image_color", (src, aug_dev, n, size), mean, std, out, out_mode, None, (means, COLOR_FORMS[form]), stream)


def _check_aug(aug, box, size):
    """refuses the transforms.Aug that an AUG_DTYPE record cannot hold"""
    if aug is not None and aug.ops:
        if len(aug.ops) > 3 or sum(1 for name, _ in aug.ops if name == T.CONTRAST) > 1:
            raise ValueError("colour decision %r: at most three ops, at most one contrast" % (aug.ops,))
        for name, _ in aug.ops:
            if name not in COLOR_OPS:
                raise NotImplementedError("colour op %r (atomnas_image_color: %s)" % (name, ", ".join(COLOR_OPS)))
    if aug is not None and aug.resize is not None:
        oh, ow = aug.resize
        top, left, h, w = box
        if not (oh > 0 and ow > 0 and h == size and w == size and 0 <= top and 0 <= left and top + h <= oh and left + w <= ow):
            raise ValueError("window %s of side %d outside a resized image of %d x %d" % (box, size, oh, ow))


def fill_aug(rec, aug, box=None, size=None):
    """writes one AUG_DTYPE record from a transforms.Aug (None: nothing to do); `box` / `size`: the window of a resize decision"""
    _check_aug(aug, box, size)
    _write_aug(rec, aug, box)


def _write_aug(rec, aug, box):   # (fill_aug behind its checks: BatchPlan.write writes what batch_plan has checked already)
    rec["op"], rec["factor"], rec["inc"] = 0, 1.0, 0.0
    rec["oh"] = rec["ow"] = rec["top"] = rec["left"] = rec["pad"] = 0
    rec["pad2"] = 0.0
    if aug is None:
        return
    for k, (name, f) in enumerate(aug.ops or ()):
        rec["op"][k], rec["factor"][k] = COLOR_OPS[name], f
    if aug.inc is not None:
        rec["inc"] = aug.inc
    if aug.resize is not None:
        rec["oh"], rec["ow"], rec["top"], rec["left"] = aug.resize[0], aug.resize[1], box[0], box[1]


def check_window(H, W, resize):
    """-> True when resizing the whole H x W image to `resize` = (oh, ow) needs the two-pass path: check_box's rule on the scale"""
    oh, ow = resize
    return H > MAX_SCALE * oh or W > MAX_SCALE * ow


def check_box(H, W, box, size):
    """rejects a crop box outside the image; -> True when the box needs the two-pass path (a side above MAX_SCALE x the output)"""
    i, j, h, w = box
    if not (0 <= i and 0 <= j and h > 0 and w > 0 and i + h <= H and j + w <= W):
        raise ValueError("crop box %s outside a %d x %d image" % (box, H, W))
    return h > MAX_SCALE * size or w > MAX_SCALE * size


class BatchPlan(object):
    """What batch_plan decides, as plain data: n; window / colour (a resize-window batch / one with a colour pass); augs (None: no aug
    table travels); rows (staged crop-box batch: (first row, row count) per image, else None); nbytes / offs / total (the bytes of every
    image that travel, their 16-byte-aligned pool offsets -- resident: the resident offsets -- and the pool bytes needed); large /
    max_rows (the ordered oversize slots, the tallest in image rows (window) or box rows); entries (the launches' names in order)."""

    def write(self, desc, aug, sel):
        """fills numpy views of the tables: n DESC_DTYPE records, n AUG_DTYPE records (not read without augs), int32 slot list"""
        for i, ((H, W), box, fl) in enumerate(zip(self.hw, self.boxes, self.flips)):
            bi, bj, bh, bw = (0, 0, H, W) if self.window else box   # (the window mode does not read the box)
            if self.rows is not None:   # only the box's rows travel: an image of height bh whose box starts at row 0
                H, bi = self.rows[i][1], 0
            desc[i] = (self.offs[i], H, W, bi, bj, bh, bw, 1 if fl else 0, 0)
            if self.augs is not None:
                _write_aug(aug[i], self.augs[i], box)   # (batch_plan has checked it)
        sel[:len(self.large)] = self.large


def batch_plan(hw, boxes, flips, augs, size, staging=False, resident_offs=None):
    """What DevicePrefetcher does with a batch, decided from the (H, W) of its images, their boxes, flips and augs (None, or per sample
    a transforms.Aug or None) -> BatchPlan.  Pure: no torch.cuda, no library.  Refuses a box outside its image (in a staged batch
    before anything is sized), a batch that mixes window and crop-box samples, and what fill_aug refuses.  staging: only the rows
    [bi, bi + bh) of a crop box travel, described as an image of height bh with bi = 0 -- k_image_preprocess and k_image_resize_h
    (csrc/preprocess.hip) clamp their taps to the crop box, as PIL crops before it resizes, so no other row is ever read -- and whole
    images in a window batch; resident_offs: the images are in device memory at these offsets and nothing travels."""
    p = BatchPlan()
    if augs is not None and all(a is None for a in augs):
        augs = None
    p.n, p.size, p.hw, p.boxes, p.flips, p.augs = len(hw), size, hw, boxes, flips, augs
    p.window = augs is not None and any(a is not None and a.resize is not None for a in augs)
    p.colour = augs is not None and any(a is not None and (a.ops or a.inc is not None) for a in augs)
    p.rows = None
    if resident_offs is not None:
        p.nbytes, p.offs, p.total = [H * W * 3 for H, W in hw], list(resident_offs), 0
    else:
        if staging and not p.window:
            for (H, W), box in zip(hw, boxes):
                check_box(H, W, box, size)
            p.rows = [(int(box[0]), int(box[2])) for box in boxes]
        p.nbytes = [(H if p.rows is None else p.rows[i][1]) * W * 3 for i, (H, W) in enumerate(hw)]
        p.offs, p.total = [], 0
        for b in p.nbytes:
            p.offs.append(p.total)
            p.total += (b + 15) // 16 * 16
    if p.window and not all(a is not None and a.resize is not None for a in augs):
        raise ValueError("a batch mixes resize-window and crop-box samples")
    p.large = []
    for i, ((H, W), box) in enumerate(zip(hw, boxes)):
        # (the ORIGINAL size decides, also where only the box's rows travel)
        if check_window(H, W, augs[i].resize) if p.window else check_box(H, W, box, size):
            p.large.append(i)
        if augs is not None:
            _check_aug(augs[i], box, size)
    p.max_rows = max((hw[i][0] if p.window else int(boxes[i][2]) for i in p.large), default=0)
    resize = "image_resize_window" if p.window else "image_preprocess"
    p.entries = (resize,) + ((resize + "_large",) if p.large else ()) + (("image_color",) if p.colour else ())
    return p


class ResidentImages(object):
    """The `images` of a batch whose pixels are in device memory already (image_store.ResidentStore): `pool` the uint8 device tensor,
    `offs` the byte offset of every sample in it, `sizes` their (H, W).  DevicePrefetcher copies no pixels for such a batch."""

    def __init__(self, pool, offs, sizes):
        self.pool, self.offs, self.sizes = pool, list(offs), list(sizes)

    def __len__(self):
        return len(self.offs)


class _Slot(object):
    """One of DevicePrefetcher's two buffer sets.  Sized by ensure(): `pool` (the pixels on the device; a resident batch brings its own),
    `desc_dev` / `desc_pin` (n DESC_DTYPE records, then the int32 batch positions of the oversize images, at most n), `out` (fp32
    [n, 3, S, S]).  Created when a batch first needs them: `aug` (device table, pinned table, int32 scratch of the colour pass), `stage`
    (uint8 [n, S, S, 3], the resized batch the colour pass reads), `ws` (two-pass workspace), `pin` (pinned staging buffer, staging=True).
    The host (the worker thread), the side stream and the consumer's stream share a slot.  Who may touch it when:
      1. The host rewrites the pinned memory -- descriptors, aug table, staging buffer -- only after wait_read().  `desc_read` is
         recorded on the side stream behind the last host-to-device copy that reads pinned memory and in front of the launches
         (DevicePrefetcher._queue).  Nothing else orders the host against those copies (the reference's prefetcher never reuses host
         staging memory), and a caller that does not synchronise per step (graph replay) runs several steps ahead of the device.
      2. The side stream waits for `consumed` before it writes the pool or the output: DevicePrefetcher.__next__ records it on the
         consumer's stream behind the use of the slot's previous batch.
      3. The worker acquires `free` before it submits into the slot; __next__ releases it once `consumed` is recorded."""

    def __init__(self, size, max_image_bytes):
        self.size, self.max_image_bytes, self.free = size, max_image_bytes, threading.Semaphore(1)
        self.desc_read = self.consumed = None
        self.drop()

    def drop(self):
        self.pool = self.desc_dev = self.desc_pin = self.out = self.aug = self.stage = self.ws = self.pin = None

    def ensure(self, n, nbytes, aug, pool=True):
        """the buffers every batch of n images and `nbytes` pool bytes needs, and the aug triple when it carries augs -> numpy views
        of the pinned tables for BatchPlan.write: (n descriptors, n aug records or None, the int32 slot list)"""
        if self.out is None or self.pool.numel() < nbytes or self.out.shape[0] != n:
            cap = max(nbytes, n * self.max_image_bytes // 4) if pool else 0
            self.pool = torch.empty(cap, dtype=torch.uint8, device="cuda")
            self.desc_dev = torch.empty(n * (DESC_DTYPE.itemsize + 4), dtype=torch.uint8, device="cuda")
            self.desc_pin = torch.empty(n * (DESC_DTYPE.itemsize + 4), dtype=torch.uint8).pin_memory()
            self.out = torch.empty(n, 3, self.size, self.size, dtype=torch.float32, device="cuda")
        if aug and (self.aug is None or self.aug[1].numel() < n * AUG_DTYPE.itemsize):
            self.aug = (torch.empty(n * AUG_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                        torch.empty(n * AUG_DTYPE.itemsize, dtype=torch.uint8).pin_memory(), torch.empty(n, dtype=torch.int32, device="cuda"))
        host = self.desc_pin.numpy()
        return (np.frombuffer(host, dtype=DESC_DTYPE, count=n), np.frombuffer(self.aug[1].numpy(), dtype=AUG_DTYPE, count=n) if aug else None,
                np.frombuffer(host, dtype=np.int32, count=n, offset=n * DESC_DTYPE.itemsize))

    def ensure_bytes(self, name, numel):
        """the uint8 buffer `name`, allocated when it is missing or smaller than numel: 'stage' and 'ws' on the device (_queue calls
        this under the side stream that uses them), 'pin' in pinned memory"""
        if getattr(self, name) is None or getattr(self, name).numel() < numel:
            buf = torch.empty(numel, dtype=torch.uint8, device="cpu" if name == "pin" else "cuda")
            setattr(self, name, buf.pin_memory() if name == "pin" else buf)
        return getattr(self, name)

    def wait_read(self):
        """rule 1: here is where a worker that runs ahead of the device waits for it -> the seconds that took"""
        t = time.perf_counter()
        if self.desc_read is not None:
            self.desc_read.synchronize()
        return time.perf_counter() - t


class DevicePrefetcher(object):
    """DataPrefetcher (utils/dataflow.py:13-58) for decoded uint8 samples.  `loader` yields batches (images, boxes, flips, targets):
    images = list of uint8 HWC tensors (pinned memory makes the copies asynchronous), boxes = list of (top, left, height, width),
    flips = list of bool, targets = int64 tensor.  Yields (input fp32 [N, 3, S, S] on the GPU, target on the GPU).

    A batch may carry a fifth element, (images, boxes, flips, targets, augs): augs = list of transforms.Aug or None per sample -- what
    the colour and evaluation transforms of 'imagenet1k_mobile' / 'imagenet1k_inception' decide beyond a box and a flip.  Aug.ops /
    Aug.inc: ColorJitter's ops in their order and Lighting's increment; the batch is then resized into a per-slot uint8 staging
    buffer (allocated when the first such batch arrives) and atomnas_image_color writes the fp32 batch from it.  Aug.resize = (oh, ow):
    the whole image is resized to that and `box` is the S x S window of the RESIZED image (Resize + CenterCrop,
    atomnas_image_resize_window); all samples of a batch or none.  A batch of four elements, or one whose augs are all None, takes
    exactly the launches and allocations it always took.  batch_plan decides all of this per batch; _queue is what is queued, in order.

    The host side of a batch -- drawing it from the loader (the crop / flip decisions of 256 samples), the descriptor table, 256 copy
    submissions: ~7 ms of Python -- runs in a worker thread (threaded=True, default), one batch ahead of the hand-over; the training
    thread only waits for an event.  Two slots alternate; _Slot states what they hold and who may touch them when.

    staging=True (host mode of a decoded image store, whose images are unpinned views of the page cache): the images of a batch --
    of a crop-box batch only the rows of the boxes -- are packed into the slot's PINNED staging buffer by `STAGE_THREADS` threads
    (numpy copies release the GIL) and ONE copy moves the packed bytes to the device pool, instead of one pageable copy per image.
    Third batch form: `images` is a ResidentImages (image_store.ResidentLoader) -- the pool is the resident device tensor, desc.off the
    resident offset, and no pixel copy is issued at all; only the tables and the targets travel."""
    STAGE_THREADS = 4

    def __init__(self, loader, image_size=224, mean=T.IMAGENET_MEAN, std=T.IMAGENET_STD, max_image_bytes=3 * 640 * 640, threaded=True,
                 filter="bilinear", staging=False):
        if not torch.cuda.is_available():
            raise _lib.AtomnasHipError("DevicePrefetcher needs the GPU (the preprocessing kernel has no CPU fallback)")
        self.loader_len = len(loader) if hasattr(loader, "__len__") else None
        self.loader = iter(loader)
        self.size, self.mean, self.std = int(image_size), tuple(mean), tuple(std)
        if filter not in FILTERS:
            raise NotImplementedError("resampling filter %r (atomnas_image_preprocess: %s)" % (filter, ", ".join(FILTERS)))
        self.filter, self.stream, self.device = filter, torch.cuda.Stream(), torch.cuda.current_device()
        self.staging = bool(staging)   # (its copies run on a thread pool: threads start when the first batch is staged)
        self._stagers = concurrent.futures.ThreadPoolExecutor(self.STAGE_THREADS, "atomnas-stage") if self.staging else None
        # where _submit's host time went (tools/bench_feed.py): drawing the batch from the loader, waiting for the slot's desc_read event
        # (the device is behind: idle time, not work), writing the tables, packing the staging buffer, queueing copies and launches
        self.host_seconds = {"draw": 0.0, "wait": 0.0, "tables": 0.0, "stage": 0.0, "queue": 0.0}
        self.k = self.handed = 0       # batches submitted (batch k goes into slot k & 1) / handed out
        self._done, self.threaded = False, bool(threaded)   # (_done: close() has run)
        self.slots = [_Slot(self.size, int(max_image_bytes)) for _ in range(2)]
        if self.threaded:
            self._q = queue.Queue(maxsize=1)
            self._closed = False
            self._thread = threading.Thread(target=self._work, name="atomnas-prefetch", daemon=True)
            self._thread.start()
        else:
            self._pending = self._submit()

    def _submit(self):
        """draw, plan, ensure the slot, wait for its desc_read, write, stage, queue -> (input, target, ready event); None: loader ended"""
        t0 = time.perf_counter()
        try:
            batch = next(self.loader)
        except StopIteration:
            return None
        t1 = time.perf_counter()
        images, boxes, flips, target = batch[:4]
        resident = isinstance(images, ResidentImages)
        hw = images.sizes if resident else [(int(im.shape[0]), int(im.shape[1])) for im in images]
        plan = batch_plan(hw, boxes, flips, batch[4] if len(batch) > 4 else None, self.size, self.staging, images.offs if resident else None)
        slot = self.slots[self.k & 1]
        tables = slot.ensure(plan.n, plan.total, plan.augs is not None, pool=not resident)
        tw = slot.wait_read()
        plan.write(*tables)
        t2 = time.perf_counter()
        if self.staging and not resident:
            self._stage(slot, images, plan)
        t3 = time.perf_counter()
        item = self._queue(plan, slot, images, target)
        self.k += 1
        hs, t4 = self.host_seconds, time.perf_counter()
        hs["draw"], hs["wait"], hs["tables"] = hs["draw"] + t1 - t0, hs["wait"] + tw, hs["tables"] + t2 - t1 - tw
        hs["stage"], hs["queue"] = hs["stage"] + t3 - t2, hs["queue"] + t4 - t3
        return item

    def _stage(self, slot, images, plan):
        """packs the batch's images (plan.rows: only those rows of each) into the slot's pinned staging buffer at plan.offs"""
        host = slot.ensure_bytes("pin", slot.pool.numel()).numpy()

        def copy(part):
            for i in range(part, plan.n, self.STAGE_THREADS):
                src = images[i].numpy()
                if plan.rows is not None:
                    src = src[plan.rows[i][0]:plan.rows[i][0] + plan.rows[i][1]]
                np.copyto(host[plan.offs[i]:plan.offs[i] + plan.nbytes[i]], src.reshape(-1))

        list(self._stagers.map(copy, range(self.STAGE_THREADS)))   # (re-raises what a copy raised)

    def _queue(self, plan, slot, images, target):
        """queues a planned batch on the side stream -> (input, target, ready event).  In this order, behind the slot's `consumed`
        event (rule 2 of _Slot): one copy per image, or the one staged copy, or none (resident); the descriptor copy; the aug copy
        when the batch carries augs; the slot's desc_read event (rule 1: behind every copy that reads pinned memory, in front of the
        launches); the resize; the two-pass launch when the batch has an oversize slot; the colour pass when it has one (the resize
        then writes uint8 into slot.stage and the colour pass writes the batch); the target copy; the ready event"""
        n, S, out = plan.n, self.size, slot.out
        resident = isinstance(images, ResidentImages)
        pool = images.pool if resident else slot.pool
        with torch.cuda.stream(self.stream):
            if slot.consumed is not None:
                self.stream.wait_event(slot.consumed)
            if self.staging and not resident:
                pool[:plan.total].copy_(slot.pin[:plan.total], non_blocking=True)
            elif not resident:
                for im, off, nb in zip(images, plan.offs, plan.nbytes):
                    pool[off:off + nb].copy_(im.reshape(-1), non_blocking=True)
            slot.desc_dev.copy_(slot.desc_pin, non_blocking=True)
            aug_dev = means = None
            if plan.augs is not None:
                aug_dev, aug_pin, means = slot.aug
                aug_dev[:n * AUG_DTYPE.itemsize].copy_(aug_pin[:n * AUG_DTYPE.itemsize], non_blocking=True)
            slot.desc_read = slot.desc_read or torch.cuda.Event()
            slot.desc_read.record(self.stream)
            dst, mode = (slot.ensure_bytes("stage", n * S * S * 3), 2) if plan.colour else (out, 0)
            resize, resize_large = (resize_window, resize_window_large) if plan.window else (preprocess, preprocess_large)
            tables = (pool, slot.desc_dev) + ((aug_dev,) if plan.window else ())
            resize(*tables, n, S, self.mean, self.std, dst, mode, self.stream, self.filter)
            if plan.large:   # only batches that hold an oversize crop box or image pay for the second launch
                m, sel = len(plan.large), slot.desc_dev[n * DESC_DTYPE.itemsize:]
                ws = slot.ensure_bytes("ws", m * plan.max_rows * S * 3)
                resize_large(*tables, sel, m, plan.max_rows, S, self.mean, self.std, dst, ws, mode, self.stream, self.filter)
            if plan.colour:
                color(dst, aug_dev, n, S, self.mean, self.std, out, means, 0, self.stream)
            tgt = target.cuda(non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        return out, tgt, ready

    def _work(self):
        torch.cuda.set_device(self.device)
        try:
            while not self._closed:
                self.slots[self.k & 1].free.acquire()   # (rule 3 of _Slot)
                if self._closed:
                    break
                item = self._submit()
                self._q.put(item)
                if item is None:
                    break
        except BaseException as e:   # handed to the consumer, which re-raises it
            self._q.put(e)

    def __next__(self):
        cur = torch.cuda.current_stream()
        if self.handed > 0:
            # (rules 2 and 3 of _Slot) everything the caller has queued so far, the use of the batch handed out last time included
            slot = self.slots[(self.handed - 1) & 1]
            slot.consumed = slot.consumed or torch.cuda.Event()
            slot.consumed.record(cur)
            if self.threaded:
                slot.free.release()
        if self.threaded:
            item = self._q.get()
            if isinstance(item, BaseException):
                raise item
        else:
            item, self._pending = self._pending, None
        if item is None:
            raise StopIteration
        out, tgt, ready = item
        cur.wait_event(ready)
        self.handed += 1
        if not self.threaded:
            # synchronous mode: the next batch goes into the OTHER slot right away, behind that slot's `consumed` of one hand-over ago
            self._pending = self._submit()
        return out, tgt

    def close(self):
        """Safe at any point of the iteration (an evaluation that stops after `bn_calibration_steps` batches): the worker is released,
        its queue drained so that a blocked put returns, the worker joined, and the side stream's queued copies / launches completed
        before the slots go back to the allocator."""
        if getattr(self, "_done", True):
            return
        self._done = True
        if self.threaded:
            self._closed = True
            for s in self.slots:
                s.free.release()
            if self._thread is not threading.current_thread():
                while self._thread.is_alive():
                    try:
                        self._q.get(timeout=0.01)
                    except queue.Empty:
                        pass
                self._thread.join()
        self._pending = None
        self.stream.synchronize()
        for s in self.slots:
            s.drop()
        if self._stagers is not None:
            self._stagers.shutdown()
            self._stagers = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __iter__(self):
        return self

    def __len__(self):
        return self.loader_len


def _synthetic_pool(pool_size, g, pin):
    """`pool_size` uint8 HWC images of ImageNet-like sizes drawn in order from the generator `g`, in pinned memory when `pin`"""
    sizes = SyntheticDecodedImages.SIZES
    images = [torch.randint(0, 256, sizes[q % len(sizes)] + (3,), dtype=torch.uint8, generator=g) for q in range(pool_size)]
    return [im.pin_memory() for im in images] if pin else images


class SyntheticDecodedImages(object):
    """A stand-in for the decoded ImageNet samples of the reference's loaders (utils/dataflow.py:173-236; JPEG / LMDB are out of scope):
    `pool_size` uint8 HWC images of ImageNet-like sizes in pinned memory, batches of `batch` samples with the boxes and flips of the
    'imagenet1k_mnas_bilinear' training transform (random.seed(seed) fixes them).  transform: a DeviceTransform of data_transforms
    instead; one that decides more than (box, flip) makes the batches five elements long (DevicePrefetcher), and its numpy draws
    (Lighting) come from a stream seeded the same way."""
    SIZES = [(375, 500), (500, 375), (333, 500), (480, 640), (500, 500), (256, 341), (600, 400), (224, 224)]

    def __init__(self, batch, steps, num_classes=1000, image_size=224, pool_size=64, seed=0, train=True, transform=None):
        g = torch.Generator().manual_seed(seed)
        self.pin = torch.cuda.is_available()   # (host logic runs without a GPU)
        self.images = _synthetic_pool(pool_size, g, self.pin)
        self.batch, self.steps, self.num_classes = batch, steps, num_classes
        self.rng_state = random.Random(seed).getstate()
        tr, va = T.mnas_bilinear_transforms(image_size)
        self.crop, self.flip = tr if train else va
        self.transform = transform
        self.np_state = np.random.RandomState(seed).get_state() if transform is not None else None
        self.g = g

    def __len__(self):
        return self.steps

    def __iter__(self):
        saved = random.getstate()
        random.setstate(self.rng_state)
        try:
            for _ in range(self.steps):
                idx = [random.randrange(len(self.images)) for _ in range(self.batch)]
                imgs = [self.images[i] for i in idx]
                if self.transform is not None:
                    np_saved = np.random.get_state()
                    np.random.set_state(self.np_state)
                    try:
                        dec = [self.transform(im) for im in imgs]
                    finally:
                        self.np_state = np.random.get_state()
                        np.random.set_state(np_saved)
                    extra = ([d[2] for d in dec],) if any(len(d) > 2 for d in dec) else ()
                    boxes, flips = [d[0] for d in dec], [d[1] for d in dec]
                else:
                    extra = ()
                    boxes = [self.crop(im) for im in imgs]
                    flips = [bool(self.flip()) if self.flip is not None else False for _ in imgs]
                target = torch.randint(0, self.num_classes, (self.batch,), generator=self.g)
                target = target.pin_memory() if self.pin else target
                self.rng_state = random.getstate()
                random.setstate(saved)
                yield (imgs, boxes, flips, target) + extra
                saved = random.getstate()
                random.setstate(self.rng_state)
        finally:
            random.setstate(saved)


# ---------------------------------------------------------------------------------------------- the reference's factories
# data_transforms / dataset / data_loader (utils/dataflow.py:92-267): same names, signatures and FLAGS keys, so that
# `train.py app:<yml>` reaches the GPU input pipeline from the yaml.  What differs is WHERE the pixel work happens: a transform here
# only decides (crop box, flip) per sample, the dataset hands out decoded uint8 images with those decisions, and DevicePrefetcher
# runs crop / resize / flip / ToTensor / Normalize in one kernel per batch ('imagenet1k_mobile' / 'imagenet1k_inception': a uint8 resize,
# then ColorJitter / Lighting / ToTensor / Normalize in atomnas_image_color; evaluation: Resize + CenterCrop in window mode).  'imagenet1k' decodes image folders with PIL on loader
# threads; 'imagenet1k_lmdb' raises (no lmdb module in this image).
class DeviceTransform(object):
    """What data_transforms returns per split: the deciders of a transform chain whose pixel work is atomnas_image_preprocess.
    transform(img) -> ((top, left, height, width), flip) for a decoded image (HWC array / tensor, PIL image or (width, height))."""

    def __init__(self, crop, flip, size, mean, std, filter="bilinear"):
        self.crop, self.flip, self.size, self.mean, self.std, self.filter = crop, flip, int(size), tuple(mean), tuple(std), filter

    def __call__(self, img):
        box = self.crop(img)   # random draws in the reference's order: the crop's, then the flip's
        return box, (bool(self.flip()) if self.flip is not None else False)

    def __repr__(self):
        return "DeviceTransform({}, {}, size={})".format(self.crop, self.flip, self.size)


class ColorDeviceTransform(DeviceTransform):
    """The deciders of 'imagenet1k_mobile' / 'imagenet1k_inception'.  transform(img) -> (box, flip, transforms.Aug): three elements, so
    datasets and loaders pass the Aug along as the fifth element of a batch.  Training (crop, jitter, lighting, flip): the draws
    come in the reference's Compose order -- RandomResizedCrop, ColorJitter, Lighting (numpy's global generator), flip -- in the
    calling thread.  Evaluation (resize, crop): Resize(256) + CenterCrop(size), the box is a window of the resized image."""

    def __init__(self, crop, flip, size, mean, std, filter="bilinear", jitter=None, lighting=None, resize=None):
        DeviceTransform.__init__(self, crop, flip, size, mean, std, filter)
        self.jitter, self.lighting, self.resize = jitter, lighting, resize

    def __call__(self, img):
        if self.resize is not None:
            oh, ow = self.resize.get_size(img)
            if oh < self.size or ow < self.size:
                raise NotImplementedError("CenterCrop(%d) of an image resized to %d x %d would pad" % (self.size, oh, ow))
            box, win = self.crop((ow, oh)), (oh, ow)
        else:
            box, win = self.crop(img), None
        ops = self.jitter.get_params() if self.jitter is not None else None
        inc = self.lighting.get_inc() if self.lighting is not None else None
        flip = bool(self.flip()) if self.flip is not None else False
        return box, flip, T.Aug(ops or None, inc, win)

    def __repr__(self):
        return "ColorDeviceTransform({}, {}, {}, {}, {}, size={})".format(self.resize, self.crop, self.jitter, self.lighting, self.flip, self.size)


def data_transforms(FLAGS):
    """Get transform of dataset (utils/dataflow.py:92-170) -> (train_transforms, val_transforms, test_transforms)."""
    name = FLAGS.data_transforms
    size = int(FLAGS.get('image_size', 224)) if hasattr(FLAGS, 'get') else 224
    if name in ('imagenet1k_mnas_bilinear', 'imagenet1k_mnas_bicubic'):
        filt = name.rsplit('_', 1)[1]   # Image.BILINEAR / Image.BICUBIC of the reference: the `filter` of atomnas_image_preprocess
        (crop, flip), (vcrop, _) = T.mnas_transforms(size, filt)
        train = DeviceTransform(crop, flip, size, T.IMAGENET_MEAN, T.IMAGENET_STD, filt)
        val = DeviceTransform(vcrop, None, size, T.IMAGENET_MEAN, T.IMAGENET_STD, filt)
        return train, val, val
    if name in ('imagenet1k_inception', 'imagenet1k_mobile'):
        if name == 'imagenet1k_inception':
            mean, std, crop_scale = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 0.08
        else:
            mean, std, crop_scale = T.IMAGENET_MEAN, T.IMAGENET_STD, 0.25
        (crop, jitter, lighting, flip), (resize, vcrop) = T.color_transforms(size, crop_scale, jitter=0.4, lighting=0.1)
        train = ColorDeviceTransform(crop, flip, size, mean, std, "bilinear", jitter=jitter, lighting=lighting)
        val = ColorDeviceTransform(vcrop, None, size, mean, std, "bilinear", resize=resize)
        return train, val, val
    if name == 'imagenet1k_basic':
        raise NotImplementedError("data_transforms 'imagenet1k_basic': the chain of 'imagenet1k_mobile' with crop_scale 0.08, which the kernels "
                                  "cover; the name is still refused because tests/test_input_pipeline.py pins the refusal -- lifting it is "
                                  "left to a follow-up")
    try:
        transforms_lib = importlib.import_module(name)
        return transforms_lib.data_transforms()
    except ImportError:
        raise NotImplementedError('Data transform {} is not yet implemented.'.format(name))


class FakeData(object):
    """utils/dataflow.py:61-89: `size` samples of one all-zero image with label 0 (the reference's smoke data source)."""

    def __init__(self, size=1000, image_size=(3, 224, 224), num_classes=10):
        self.size, self.image_size, self.num_classes = size, image_size, num_classes
        self.img = torch.zeros(image_size)
        self.target = 0

    def __getitem__(self, index):
        if index >= len(self):
            raise IndexError("{} index out of range".format(self.__class__.__name__))
        return self.img, self.target

    def __len__(self):
        return self.size


class DecodedFakeData(object):
    """`size` decoded samples for the GPU input pipeline: a pool of uint8 HWC images of ImageNet-like sizes in pinned memory (sample i
    is image i mod pool) with seeded labels; __getitem__ applies the split's DeviceTransform and returns (image, box, flip, target), or
    (image, box, flip, aug, target) when the transform decides more (ColorDeviceTransform).
    Stand-in for ImageFolder / ImageFolderLMDB + a JPEG decoder, which this image cannot provide."""

    def __init__(self, size, transform, num_classes=1000, pool_size=64, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.images = _synthetic_pool(pool_size, g, torch.cuda.is_available())
        self.labels = torch.randint(0, num_classes, (pool_size * 16,), generator=g).tolist()
        self.size, self.transform, self.num_classes = int(size), transform, num_classes

    def __len__(self):
        return self.size

    def load(self, index):
        if index >= self.size:
            raise IndexError("{} index out of range".format(self.__class__.__name__))
        return self.images[index % len(self.images)], self.labels[index % len(self.labels)]

    def __getitem__(self, index):
        im, target = self.load(index)
        return (im,) + tuple(self.transform(im)) + (target,)   # (image, box, flip[, aug], target)


IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')   # torchvision.datasets.folder


class ImageFolderDecoded(object):
    """torchvision.datasets.ImageFolder's role (utils/dataflow.py:176-184, `dataset: imagenet1k`) for the GPU input pipeline: samples are
    `root/<class>/<file>` with the classes sorted by name (class index = position) and the files of a class sorted by path; `load(i)`
    decodes with PIL (`Image.open(path).convert('RGB')`, what torchvision's default loader does) into a uint8 HWC tensor (pinned when a
    GPU is present) -- the decode releases the GIL, so DecodedLoader runs it on `data_loader_workers` threads --, `__getitem__` adds the
    split's DeviceTransform decisions: (image, box, flip[, aug], target).  The pixel work of the transform stays on the GPU."""

    def __init__(self, root, transform):
        self.root, self.transform = root, transform
        classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
        if not classes:
            raise FileNotFoundError("Couldn't find any class folder in {}.".format(root))
        self.classes = classes
        self.class_to_idx = {c: i for i, c in enumerate(classes)}
        self.samples = []
        for c in classes:
            for base, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for f in sorted(files):
                    if f.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(base, f), self.class_to_idx[c]))
        if not self.samples:
            raise FileNotFoundError("Found no valid file for the classes in {}.".format(root))
        self.pin = torch.cuda.is_available()

    def __len__(self):
        return len(self.samples)

    def load(self, index):
        from PIL import Image
        path, target = self.samples[index]
        with open(path, 'rb') as f:
            arr = np.asarray(Image.open(f).convert('RGB'))
        im = torch.from_numpy(np.ascontiguousarray(arr))
        return (im.pin_memory() if self.pin else im), target

    def __getitem__(self, index):
        im, target = self.load(index)
        return (im,) + tuple(self.transform(im)) + (target,)   # (image, box, flip[, aug], target)


def dataset(train_transforms, val_transforms, test_transforms, FLAGS):
    """Get dataset for classification (utils/dataflow.py:173-211) -> (train_set, val_set, test_set)."""
    name = FLAGS.dataset
    if name == 'imagenet1k_fake':
        shape = (3, FLAGS.image_size, FLAGS.image_size)
        return FakeData(size=1281167, image_size=shape, num_classes=1000), FakeData(size=50000, image_size=shape, num_classes=1000), None
    needs_train = not FLAGS.get('test_only', False) or FLAGS.get('bn_calibration', False)   # (an evaluation run calibrates on the train split)
    if name == 'imagenet1k_decoded_fake':
        ntrain, nval = int(FLAGS.get('fake_train_size', 1281167)), int(FLAGS.get('fake_val_size', 50000))
        seed = int(FLAGS.get('random_seed', 0))
        train_set = DecodedFakeData(ntrain, train_transforms, seed=seed) if needs_train else None
        return train_set, DecodedFakeData(nval, val_transforms, seed=seed + 1), None
    if name == 'imagenet1k':
        train_set = ImageFolderDecoded(os.path.join(FLAGS.dataset_dir, 'train'), train_transforms) if needs_train else None
        return train_set, ImageFolderDecoded(os.path.join(FLAGS.dataset_dir, 'val'), val_transforms), None
    if name == 'imagenet1k_store':   # the image folders of 'imagenet1k', decoded once by tools/make_image_store.py
        from .image_store import DecodedStore
        train_set = DecodedStore(os.path.join(FLAGS.dataset_dir, 'train'), train_transforms) if needs_train else None
        return train_set, DecodedStore(os.path.join(FLAGS.dataset_dir, 'val'), val_transforms), None
    if name == 'imagenet1k_lmdb':
        raise NotImplementedError("dataset 'imagenet1k_lmdb': the lmdb module is not in this image (utils/lmdb_dataset.py:24-71); the same "
                                  "records decode through ImageFolderDecoded's PIL path once they can be read -- use 'imagenet1k' (image folders)")
    try:
        dataset_lib = importlib.import_module(name)
        return dataset_lib.dataset(train_transforms, val_transforms, test_transforms)
    except ImportError:
        raise NotImplementedError('Dataset {} is not yet implemented.'.format(name))


class DecodedLoader(object):
    """torch.utils.data.DataLoader's role for decoded samples (utils/dataflow.py:217-225 `_build_loader`): batches of `batch_size`
    samples (image, box, flip[, aug], target) -> (images, boxes, flips, targets int64 pinned[, augs]), the form DevicePrefetcher takes.  shuffle:
    a fresh seeded permutation per pass; rank / world: the DistributedSampler split (every rank the same number of samples, the
    index list padded by wrapping around); drop_last as torch's.  workers > 0: the samples of a batch are LOADED (decoded) on that many
    threads (PIL's decoder releases the GIL); the transform's random decisions are then drawn in sample order by the iterating thread
    (one stream of Python's `random` -- and of numpy's global generator, which Lighting draws from -- whatever the thread timing)
    -- with DevicePrefetcher that is its worker thread, off the training thread."""

    def __init__(self, dset, batch_size, shuffle, rank=0, world=1, drop_last=False, seed=0, workers=0):
        self.dset, self.batch_size, self.shuffle = dset, int(batch_size), bool(shuffle)
        self.workers = max(0, int(workers))
        self._pool = None
        self.rank, self.world, self.drop_last, self.seed = int(rank), int(world), bool(drop_last), int(seed)
        self.epoch = 0
        n = len(dset)
        self.per_rank = (n + self.world - 1) // self.world

    def __len__(self):
        return self.per_rank // self.batch_size if self.drop_last else (self.per_rank + self.batch_size - 1) // self.batch_size

    def set_epoch(self, epoch):
        """DistributedSampler.set_epoch (the reference's train.py:155): the next pass is pass `epoch` of a fresh loader, and the passes
        after it count on from there.  Without a call the passes are counted from the loader's construction."""
        self.epoch = int(epoch)

    def _indices(self):
        n = len(self.dset)
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            idx = torch.randperm(n, generator=g).tolist()
        else:
            idx = list(range(n))
        total = self.per_rank * self.world
        idx += idx[:total - n]
        return idx[self.rank:total:self.world]

    def __iter__(self):
        idx = self._indices()
        self.epoch += 1
        pin = torch.cuda.is_available()
        for b in range(len(self)):
            chunk = idx[b * self.batch_size:(b + 1) * self.batch_size]
            if self.workers > 0 and hasattr(self.dset, "load") and hasattr(self.dset, "transform"):
                if self._pool is None:
                    self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="atomnas-decode")
                loaded = list(self._pool.map(self.dset.load, chunk))
                samples = []
                for im, tgt in loaded:
                    samples.append((im,) + tuple(self.dset.transform(im)) + (tgt,))
            else:
                samples = [self.dset[i] for i in chunk]
            target = torch.tensor([s[-1] for s in samples], dtype=torch.int64)
            extra = ([s[3] if len(s) > 4 else None for s in samples],) if any(len(s) > 4 for s in samples) else ()
            yield ([s[0] for s in samples], [s[1] for s in samples], [s[2] for s in samples], (target.pin_memory() if pin else target)) + extra


def _resident_loaders(train_set, val_set, FLAGS, rank, world, training, calibrating, seed):
    """data_loader's four loaders for `dataset_resident: True`: every split the run uses is a rank share in device memory
    (image_store.ResidentStore, uploaded when a loader is first iterated); the calibration loader shares the train upload.  The same
    shuffle flags as the host loaders; with world > 1 the shares are fixed for the run (image_store.ResidentLoader)."""
    from .image_store import DecodedStore, ResidentLoader, ResidentStore
    for dset in (train_set if (training or calibrating) else None, val_set):
        if dset is not None and not isinstance(dset, DecodedStore):
            raise ValueError("dataset_resident: True needs a decoded image store (dataset: imagenet1k_store), not %s" % type(dset).__name__)
    reserve = float(FLAGS.get('dataset_resident_reserve_gb', 32))
    drop_last = FLAGS.get('drop_last', False)
    train_res = ResidentStore(train_set, rank, world, seed, reserve) if (training or calibrating) else None
    train_loader = ResidentLoader(train_res, FLAGS._loader_batch_size, True, drop_last, seed) if training else None
    calib_loader = (ResidentLoader(train_res, FLAGS.get('_loader_batch_size_calib', FLAGS._loader_batch_size), True, drop_last, seed)
                    if calibrating else None)
    val_loader = ResidentLoader(ResidentStore(val_set, rank, world, seed, reserve), FLAGS._loader_batch_size,
                                bool(FLAGS.use_distributed), drop_last, seed)
    return train_loader, calib_loader, val_loader, val_loader


def data_loader(train_set, val_set, test_set, FLAGS):
    """Get data loader (utils/dataflow.py:214-267) -> (train_loader, calib_loader, val_loader, test_loader).  `data_loader_workers`:
    decode threads of a loader (at most 16; the reference's worker processes also crop / resize / normalize, which is GPU work here)."""
    if FLAGS.data_loader != 'imagenet1k_basic':
        try:
            data_loader_lib = importlib.import_module(FLAGS.data_loader)
            return data_loader_lib.data_loader(train_set, val_set, test_set)
        except ImportError:
            raise NotImplementedError('Data loader {} is not yet implemented.'.format(FLAGS.data_loader))
    rank = world = None
    if FLAGS.use_distributed:
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
    training = not FLAGS.get('test_only', False)
    calibrating = bool(FLAGS.get('bn_calibration', False))
    seed = int(FLAGS.get('random_seed', 0))
    workers = min(16, int(FLAGS.get('data_loader_workers', 0) or 0))
    if FLAGS.get('dataset_resident', False):
        return _resident_loaders(train_set, val_set, FLAGS, rank or 0, world or 1, training, calibrating, seed)

    def _build_loader(dset, batch_size, shuffle):
        # distributed: the sampler shuffles (DistributedSampler's default) and the loader does not; single process: the loader does
        return DecodedLoader(dset, batch_size, shuffle if world is None else True, rank=rank or 0, world=world or 1,
                             drop_last=FLAGS.get('drop_last', False), seed=seed, workers=workers)

    train_loader = _build_loader(train_set, FLAGS._loader_batch_size, True) if training else None
    calib_loader = _build_loader(train_set, FLAGS.get('_loader_batch_size_calib', FLAGS._loader_batch_size), True) if calibrating else None
    val_loader = _build_loader(val_set, FLAGS._loader_batch_size, False)
    return train_loader, calib_loader, val_loader, val_loader
