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
import ctypes
import importlib
import random
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


def preprocess(pool_dev, desc_dev, n, size, mean, std, out, out_mode=0, stream=None, filter="bilinear"):
    """launches atomnas_image_preprocess: pool_dev uint8 device tensor, desc_dev uint8 device tensor holding n DESC_DTYPE records"""
    st = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    _lib.call("atomnas_image_preprocess", ctypes.c_void_p(pool_dev.data_ptr()), ctypes.c_void_p(desc_dev.data_ptr()), int(n), int(size),
              ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
              ctypes.c_void_p(out.data_ptr()), int(out_mode), FILTERS[filter], st)


def preprocess_large(pool_dev, desc_dev, sel_dev, m, max_rows, size, mean, std, out, workspace, out_mode=0, stream=None, filter="bilinear"):
    """launches atomnas_image_preprocess_large after preprocess() on the same stream: rewrites the m batch slots listed in sel_dev
    (int32 device tensor) through the two-pass form; workspace: uint8 device tensor of at least m * max_rows * size * 3 bytes"""
    st = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    mm = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    _lib.call("atomnas_image_preprocess_large", ctypes.c_void_p(pool_dev.data_ptr()), ctypes.c_void_p(desc_dev.data_ptr()),
              ctypes.c_void_p(sel_dev.data_ptr()), int(m), int(max_rows), int(size), ctypes.cast(mm, ctypes.c_void_p),
              ctypes.cast(s, ctypes.c_void_p), ctypes.c_void_p(out.data_ptr()), int(out_mode), FILTERS[filter],
              ctypes.c_void_p(workspace.data_ptr()), int(workspace.numel()), st)


def resize_window(pool_dev, desc_dev, aug_dev, n, size, mean, std, out, out_mode=0, stream=None, filter="bilinear"):
    """launches atomnas_image_resize_window (Resize + CenterCrop): aug_dev uint8 device tensor holding n AUG_DTYPE records"""
    st = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    _lib.call("atomnas_image_resize_window", ctypes.c_void_p(pool_dev.data_ptr()), ctypes.c_void_p(desc_dev.data_ptr()),
              ctypes.c_void_p(aug_dev.data_ptr()), int(n), int(size), ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
              ctypes.c_void_p(out.data_ptr()), int(out_mode), FILTERS[filter], st)


def resize_window_large(pool_dev, desc_dev, aug_dev, sel_dev, m, max_rows, size, mean, std, out, workspace, out_mode=0, stream=None,
                        filter="bilinear"):
    """launches atomnas_image_resize_window_large after resize_window() on the same stream (max_rows: the tallest selected IMAGE)"""
    st = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    mm = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    _lib.call("atomnas_image_resize_window_large", ctypes.c_void_p(pool_dev.data_ptr()), ctypes.c_void_p(desc_dev.data_ptr()),
              ctypes.c_void_p(aug_dev.data_ptr()), ctypes.c_void_p(sel_dev.data_ptr()), int(m), int(max_rows), int(size),
              ctypes.cast(mm, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), ctypes.c_void_p(out.data_ptr()), int(out_mode),
              FILTERS[filter], ctypes.c_void_p(workspace.data_ptr()), int(workspace.numel()), st)


def color(src, aug_dev, n, size, mean, std, out, means, out_mode=0, stream=None, form="auto"):
    """launches atomnas_image_color: src uint8 [n, size, size, 3] device tensor (out_mode 2 of the resize), aug_dev as above, means an
    int32 device tensor of at least n elements (scratch)"""
    st = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    if src.numel() < n * size * size * 3 or means.numel() < n:
        raise ValueError("atomnas_image_color: source or scratch buffer too small")
    _lib.call("atomnas_image_color", ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(aug_dev.data_ptr()), int(n), int(size),
              ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), ctypes.c_void_p(out.data_ptr()), int(out_mode),
              ctypes.c_void_p(means.data_ptr()), COLOR_FORMS[form], st)


def fill_aug(rec, aug, box=None, size=None):
    """writes one AUG_DTYPE record from a transforms.Aug (None: nothing to do); `box` / `size`: the window of a resize decision"""
    rec["op"], rec["factor"], rec["inc"] = 0, 1.0, 0.0
    rec["oh"] = rec["ow"] = rec["top"] = rec["left"] = rec["pad"] = 0
    rec["pad2"] = 0.0
    if aug is None:
        return
    if aug.ops:
        if len(aug.ops) > 3 or sum(1 for name, _ in aug.ops if name == T.CONTRAST) > 1:
            raise ValueError("colour decision %r: at most three ops, at most one contrast" % (aug.ops,))
        for k, (name, f) in enumerate(aug.ops):
            if name not in COLOR_OPS:
                raise NotImplementedError("colour op %r (atomnas_image_color: %s)" % (name, ", ".join(COLOR_OPS)))
            rec["op"][k], rec["factor"][k] = COLOR_OPS[name], f
    if aug.inc is not None:
        rec["inc"] = aug.inc
    if aug.resize is not None:
        oh, ow = aug.resize
        top, left, h, w = box
        if not (oh > 0 and ow > 0 and h == size and w == size and 0 <= top and 0 <= left and top + h <= oh and left + w <= ow):
            raise ValueError("window %s of side %d outside a resized image of %d x %d" % (box, size, oh, ow))
        rec["oh"], rec["ow"], rec["top"], rec["left"] = oh, ow, top, left


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


class ResidentImages(object):
    """The `images` of a batch whose pixels are in device memory already (image_store.ResidentStore): `pool` the uint8 device tensor,
    `offs` the byte offset of every sample in it, `sizes` their (H, W).  DevicePrefetcher copies no pixels for such a batch."""

    def __init__(self, pool, offs, sizes):
        self.pool, self.offs, self.sizes = pool, list(offs), list(sizes)

    def __len__(self):
        return len(self.offs)


class DevicePrefetcher(object):
    """DataPrefetcher (utils/dataflow.py:13-58) for decoded uint8 samples.  `loader` yields batches (images, boxes, flips, targets):
    images = list of uint8 HWC tensors (pinned memory makes the copies asynchronous), boxes = list of (top, left, height, width),
    flips = list of bool, targets = int64 tensor.  Yields (input fp32 [N, 3, S, S] on the GPU, target on the GPU).

    A batch may carry a fifth element, (images, boxes, flips, targets, augs): augs = list of transforms.Aug or None per sample -- what
    the colour and evaluation transforms of 'imagenet1k_mobile' / 'imagenet1k_inception' decide beyond a box and a flip.  Aug.ops /
    Aug.inc: ColorJitter's ops in their order and Lighting's increment; the batch is then resized into a per-slot uint8 staging
    buffer (allocated when the first such batch arrives) and atomnas_image_color writes the fp32 batch from it.  Aug.resize = (oh, ow):
    the whole image is resized to that and `box` is the S x S window of the RESIZED image (Resize + CenterCrop,
    atomnas_image_resize_window); all samples of a batch or none.  The table of these decisions (atomnas_img_aug) has per-slot pinned
    and device buffers of its own under the same reuse rule as the descriptors.  A batch of four elements, or one whose augs are all
    None, takes exactly the launches and allocations it always took.

    The host side of a batch -- drawing it from the loader (the crop / flip decisions of 256 samples), the descriptor table, 256 copy
    submissions: ~7 ms of Python -- runs in a worker thread (threaded=True, default), one batch ahead of the hand-over; the training
    thread only waits for an event.  Two slots (pixel pool, descriptors, output) alternate; a slot is refilled only after the consumer
    of its previous batch has been ordered behind an event on the consumer's stream.

    staging=True (host mode of a decoded image store, whose images are unpinned views of the page cache): the images of a batch are
    packed into a per-slot PINNED staging buffer by `STAGE_THREADS` threads (numpy copies release the GIL) and ONE copy moves the packed
    bytes to the device pool, instead of one pageable copy per image.  The staging buffer obeys the descriptors' rule: the host
    rewrites it only after the slot's `desc_read` event, which is recorded behind the copy that reads it.  A crop-box batch stages only
    the rows [bi, bi + bh) of every image and describes them as an image of height bh with bi = 0: k_image_preprocess and
    k_image_resize_h (csrc/preprocess.hip) read the rows bi + ymin + y with ymin + y < bh -- pp_coeffs / PpWindow clamp the taps to
    the crop box, as PIL crops before it resizes -- so no other row is ever read; whether a box is oversize is still decided on the
    original size.  A window batch (Resize + CenterCrop reads the whole image) stages whole images.  staging=False (default) takes
    exactly the launches, copies and allocations it always took.

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
        self.filter = filter
        self.stream = torch.cuda.Stream()
        self.device = torch.cuda.current_device()
        self.max_image_bytes = int(max_image_bytes)
        self.slots = [None, None]   # per slot: (device pool, device descriptors, pinned descriptors, output) sized on first use
        self.aug = [None, None]     # per slot: (device table, pinned table, int32 scratch of the colour pass) once a batch carries augs
        self.stage = [None, None]   # per slot: uint8 [N, S, S, 3], the resized batch the colour pass reads
        self.ws = [None, None]      # per slot: workspace of the two-pass path, allocated when a batch first holds an oversize crop box
        self.staging = bool(staging)
        self.pin = [None, None]     # per slot: pinned staging buffer of the packed pixels (staging=True), under the desc_read rule
        self._stagers = None        # thread pool of the staging copies
        # where _submit's host time went (tools/bench_feed.py): drawing the batch from the loader, waiting for the slot's desc_read event
        # (the device is behind: idle time, not work), writing the tables, packing the staging buffer, queueing copies and launches
        self.host_seconds = {"draw": 0.0, "wait": 0.0, "tables": 0.0, "stage": 0.0, "queue": 0.0}
        # per slot: event behind the last host-to-device copy that READ the slot's pinned descriptors.  The host rewrites them for the
        # batch after next; nothing else orders the host against that copy (the reference's prefetcher never reuses host staging
        # memory), and a caller that does not synchronise per step (graph replay) runs several steps ahead of the device.
        self.desc_read = [None, None]
        self.consumed = [None, None]   # per slot: event on the consumer's stream behind the use of the slot's previous batch
        self.k = 0                     # batches submitted
        self._done = False             # close() has run
        self.handed = 0                # batches handed out
        self.threaded = bool(threaded)
        if self.threaded:
            import queue
            import threading
            self._q = queue.Queue(maxsize=1)
            self._free = [threading.Semaphore(1), threading.Semaphore(1)]
            self._closed = False
            self._thread = threading.Thread(target=self._work, name="atomnas-prefetch", daemon=True)
            self._thread.start()
        else:
            self._pending = self._submit()

    def _slot(self, q, n, nbytes, pool=True):
        s = self.slots[q]
        if s is None or s[0].numel() < nbytes or s[3].shape[0] != n:
            cap = max(nbytes, n * self.max_image_bytes // 4) if pool else 0   # (a resident batch brings its pool along)
            # descriptors, then the int32 batch positions of the oversize images (at most n)
            s = (torch.empty(cap, dtype=torch.uint8, device="cuda"), torch.empty(n * (DESC_DTYPE.itemsize + 4), dtype=torch.uint8, device="cuda"),
                 torch.empty(n * (DESC_DTYPE.itemsize + 4), dtype=torch.uint8).pin_memory(),
                 torch.empty(n, 3, self.size, self.size, dtype=torch.float32, device="cuda"))
            self.slots[q] = s
        return s

    def _submit(self):
        """draws the next batch and queues its copies and the preprocessing launch on the side stream -> (input, target, ready event)
        or None at the end of the loader"""
        t0 = time.perf_counter()
        try:
            batch = next(self.loader)
        except StopIteration:
            return None
        t1 = time.perf_counter()
        images, boxes, flips, target = batch[:4]
        augs = batch[4] if len(batch) > 4 else None
        if augs is not None and all(a is None for a in augs):
            augs = None
        q = self.k & 1
        n = len(images)
        window = augs is not None and any(a is not None and a.resize is not None for a in augs)
        colour = augs is not None and any(a is not None and (a.ops or a.inc is not None) for a in augs)
        resident = isinstance(images, ResidentImages)
        rows = None   # staged crop-box batch: (first row, row count) of every image that travels
        if resident:
            hw, offs = images.sizes, images.offs
            pool, (_, desc_dev, desc_pin, out) = images.pool, self._slot(q, n, 0, pool=False)
        else:
            hw = [(int(im.shape[0]), int(im.shape[1])) for im in images]
            sizes = [int(im.numel()) for im in images]
            if self.staging and not window:
                for (H, W), box in zip(hw, boxes):
                    check_box(H, W, box, self.size)   # (a box outside its image is refused before it sizes anything)
                rows = [(int(box[0]), int(box[2])) for box in boxes]
                sizes = [bh * W * 3 for (H, W), (bi, bh) in zip(hw, rows)]
            offs = np.concatenate([[0], np.cumsum([(b + 15) // 16 * 16 for b in sizes])])
            pool, desc_dev, desc_pin, out = self._slot(q, n, int(offs[-1]))
        ev = self.desc_read[q]
        tw = time.perf_counter()
        if ev is not None:
            # the copy queued two batches ago has read desc_pin (and the staging buffer).  A consumer that does not synchronise per step
            # runs ahead of the device, and so does this thread: here is where it waits for the device (host_seconds['wait'])
            ev.synchronize()
        tw = time.perf_counter() - tw
        d = np.frombuffer(desc_pin.numpy(), dtype=DESC_DTYPE, count=n)
        large = []
        if window and not all(a is not None and a.resize is not None for a in augs):
            raise ValueError("a batch mixes resize-window and crop-box samples")
        if augs is not None:
            if self.aug[q] is None or self.aug[q][1].numel() < n * AUG_DTYPE.itemsize:
                self.aug[q] = (torch.empty(n * AUG_DTYPE.itemsize, dtype=torch.uint8, device="cuda"),
                               torch.empty(n * AUG_DTYPE.itemsize, dtype=torch.uint8).pin_memory(),
                               torch.empty(n, dtype=torch.int32, device="cuda"))
            aug_dev, aug_pin, means = self.aug[q]
            a = np.frombuffer(aug_pin.numpy(), dtype=AUG_DTYPE, count=n)
        for i, ((H, W), box, fl) in enumerate(zip(hw, boxes, flips)):
            if window:
                if check_window(H, W, augs[i].resize):
                    large.append(i)
                box_d = (0, 0, H, W)   # (not read by the window mode)
            else:
                if check_box(H, W, box, self.size):   # (the ORIGINAL size decides, also where only the box's rows travel)
                    large.append(i)
                box_d = box
            if rows is not None:
                H, box_d = rows[i][1], (0, box_d[1], box_d[2], box_d[3])
            d[i] = (int(offs[i]), H, W, box_d[0], box_d[1], box_d[2], box_d[3], 1 if fl else 0, 0)
            if augs is not None:
                fill_aug(a[i], augs[i], box, self.size)
        if large:
            np.frombuffer(desc_pin.numpy(), dtype=np.int32, count=len(large), offset=n * DESC_DTYPE.itemsize)[:] = large
            max_rows = max(hw[i][0] if window else int(boxes[i][2]) for i in large)
        t2 = time.perf_counter()
        staged = self.staging and not resident
        if staged:   # behind the desc_read wait above: the copy that read this slot's staging buffer two batches ago is done
            total = int(offs[-1])
            pin = self._stage(q, images, rows, offs, sizes, pool.numel())
        t3 = time.perf_counter()
        with torch.cuda.stream(self.stream):
            if self.consumed[q] is not None:
                self.stream.wait_event(self.consumed[q])   # the slot's previous batch has been consumed (handed out two batches ago)
            if staged:
                pool[:total].copy_(pin[:total], non_blocking=True)   # in front of the desc_read event below
            elif not resident:
                for i, im in enumerate(images):
                    pool[int(offs[i]):int(offs[i]) + sizes[i]].copy_(im.reshape(-1), non_blocking=True)
            desc_dev.copy_(desc_pin, non_blocking=True)
            if augs is not None:
                aug_dev[:n * AUG_DTYPE.itemsize].copy_(aug_pin[:n * AUG_DTYPE.itemsize], non_blocking=True)   # in front of the event below
            ev = self.desc_read[q] = self.desc_read[q] or torch.cuda.Event()
            ev.record(self.stream)
            dst, mode = out, 0
            if colour:   # the resize writes uint8 into the staging buffer, the colour pass the batch
                if self.stage[q] is None or self.stage[q].numel() < n * self.size * self.size * 3:
                    self.stage[q] = torch.empty(n * self.size * self.size * 3, dtype=torch.uint8, device="cuda")
                dst, mode = self.stage[q], 2
            if window:
                resize_window(pool, desc_dev, aug_dev, n, self.size, self.mean, self.std, dst, mode, self.stream, self.filter)
            else:
                preprocess(pool, desc_dev, n, self.size, self.mean, self.std, dst, mode, self.stream, self.filter)
            if large:   # only batches that hold an oversize crop box pay for the second launch
                need = len(large) * max_rows * self.size * 3
                if self.ws[q] is None or self.ws[q].numel() < need:
                    self.ws[q] = torch.empty(need, dtype=torch.uint8, device="cuda")   # allocated on the side stream that uses it
                sel = desc_dev[n * DESC_DTYPE.itemsize:]
                if window:
                    resize_window_large(pool, desc_dev, aug_dev, sel, len(large), max_rows, self.size, self.mean, self.std, dst, self.ws[q],
                                        mode, self.stream, self.filter)
                else:
                    preprocess_large(pool, desc_dev, sel, len(large), max_rows, self.size, self.mean, self.std, dst, self.ws[q], mode,
                                     self.stream, self.filter)
            if colour:
                color(dst, aug_dev, n, self.size, self.mean, self.std, out, means, 0, self.stream)
            tgt = target.cuda(non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        self.k += 1
        hs, t4 = self.host_seconds, time.perf_counter()
        hs["draw"], hs["wait"], hs["tables"] = hs["draw"] + t1 - t0, hs["wait"] + tw, hs["tables"] + t2 - t1 - tw
        hs["stage"], hs["queue"] = hs["stage"] + t3 - t2, hs["queue"] + t4 - t3
        return out, tgt, ready

    def _stage(self, q, images, rows, offs, sizes, capacity):
        """packs the batch's images (`rows`: only those rows of each) into the slot's pinned staging buffer at `offs` -> the buffer"""
        pin = self.pin[q]
        if pin is None or pin.numel() < capacity:
            pin = self.pin[q] = torch.empty(capacity, dtype=torch.uint8).pin_memory()
        if self._stagers is None:
            import concurrent.futures
            self._stagers = concurrent.futures.ThreadPoolExecutor(max_workers=self.STAGE_THREADS, thread_name_prefix="atomnas-stage")
        host = pin.numpy()

        def copy(part):
            for i in range(part, len(images), self.STAGE_THREADS):
                src = images[i].numpy()
                if rows is not None:
                    src = src[rows[i][0]:rows[i][0] + rows[i][1]]
                np.copyto(host[int(offs[i]):int(offs[i]) + sizes[i]], src.reshape(-1))

        list(self._stagers.map(copy, range(self.STAGE_THREADS)))   # (re-raises what a copy raised)
        return pin

    def _work(self):
        torch.cuda.set_device(self.device)
        try:
            while not self._closed:
                self._free[self.k & 1].acquire()
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
            # everything the caller has queued on its stream so far -- the use of the batch handed out last time included -- is in front
            # of this event: the slot of that batch may be refilled behind it
            q = (self.handed - 1) & 1
            ev = self.consumed[q] = self.consumed[q] or torch.cuda.Event()
            ev.record(cur)
            if self.threaded:
                self._free[q].release()
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
            self._pending = self._submit_after_consume()
        return out, tgt

    def _submit_after_consume(self):
        # synchronous mode: the next batch is submitted right away (it fills the OTHER slot; its own slot's consumer event, recorded
        # one hand-over ago, is waited for on the side stream)
        return self._submit()

    def close(self):
        """Safe at any point of the iteration (an evaluation that stops after `bn_calibration_steps` batches): the worker is released,
        its queue drained so that a blocked put returns, the worker joined, and the side stream's queued copies / launches completed
        before the slots go back to the allocator."""
        if getattr(self, "_done", True):
            return
        self._done = True
        if self.threaded:
            import queue
            import threading
            self._closed = True
            for s in self._free:
                s.release()
            if self._thread is not threading.current_thread():
                while self._thread.is_alive():
                    try:
                        self._q.get(timeout=0.01)
                    except queue.Empty:
                        pass
                self._thread.join()
        self._pending = None
        self.stream.synchronize()
        self.slots, self.ws, self.aug, self.stage = [None, None], [None, None], [None, None], [None, None]
        self.pin = [None, None]
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
        self.images = []
        for q in range(pool_size):
            H, W = self.SIZES[q % len(self.SIZES)]
            im = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
            self.images.append(im.pin_memory() if self.pin else im)
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
    if name in ('imagenet1k_mnas_bilinear', 'imagenet1k_mnas_bicubic'):
        size = int(FLAGS.get('image_size', 224)) if hasattr(FLAGS, 'get') else 224
        filt = name.rsplit('_', 1)[1]   # Image.BILINEAR / Image.BICUBIC of the reference: the `filter` of atomnas_image_preprocess
        (crop, flip), (vcrop, _) = T.mnas_transforms(size, filt)
        train = DeviceTransform(crop, flip, size, T.IMAGENET_MEAN, T.IMAGENET_STD, filt)
        val = DeviceTransform(vcrop, None, size, T.IMAGENET_MEAN, T.IMAGENET_STD, filt)
        return train, val, val
    if name in ('imagenet1k_inception', 'imagenet1k_mobile'):
        size = int(FLAGS.get('image_size', 224)) if hasattr(FLAGS, 'get') else 224
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
        pin = torch.cuda.is_available()
        self.images = []
        for q in range(pool_size):
            H, W = SyntheticDecodedImages.SIZES[q % len(SyntheticDecodedImages.SIZES)]
            im = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
            self.images.append(im.pin_memory() if pin else im)
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
        import os
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
    if name == 'imagenet1k_decoded_fake':
        ntrain, nval = int(FLAGS.get('fake_train_size', 1281167)), int(FLAGS.get('fake_val_size', 50000))
        seed = int(FLAGS.get('random_seed', 0))
        train_set = DecodedFakeData(ntrain, train_transforms, seed=seed) if (not FLAGS.get('test_only', False) or FLAGS.get('bn_calibration', False)) else None
        return train_set, DecodedFakeData(nval, val_transforms, seed=seed + 1), None
    if name == 'imagenet1k':
        import os
        train_set = (ImageFolderDecoded(os.path.join(FLAGS.dataset_dir, 'train'), train_transforms)
                     if (not FLAGS.get('test_only', False) or FLAGS.get('bn_calibration', False)) else None)
        return train_set, ImageFolderDecoded(os.path.join(FLAGS.dataset_dir, 'val'), val_transforms), None
    if name == 'imagenet1k_store':   # the image folders of 'imagenet1k', decoded once by tools/make_image_store.py
        import os
        from .image_store import DecodedStore
        train_set = (DecodedStore(os.path.join(FLAGS.dataset_dir, 'train'), train_transforms)
                     if (not FLAGS.get('test_only', False) or FLAGS.get('bn_calibration', False)) else None)
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
                    import concurrent.futures
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
    val_loader = _build_loader(val_set, FLAGS._loader_batch_size, False) if world is None else \
        DecodedLoader(val_set, FLAGS._loader_batch_size, True, rank=rank, world=world, drop_last=FLAGS.get('drop_last', False), seed=seed, workers=workers)
    return train_loader, calib_loader, val_loader, val_loader
