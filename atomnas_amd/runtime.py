"""Device-resident flat storage ("arenas") behind the reference's nn.Module / optimizer / EMA objects.

The reference keeps 497 separate parameter tensors, 302 BN buffers, 2x497 RMSprop state tensors and 799 EMA shadows and
walks them in Python loops every step (utils/optim.py:226-243, utils/rmsprop.py:70-132, utils/optim.py:54-65,
utils/distributed.py:131-139).  Here every one of those tensors is a *view* into a handful of flat fp32 arenas:

    P    parameters            G    gradients (p.grad)       SQ / BUF   square_avg (RMSprop) / momentum_buffer (RMSprop, SGD)
    EMA  EMA shadows of P      S    BN running statistics    SEMA       EMA shadows of S         CNT  int64 BN counters

so that the optimizer tail, gradient all-reduce, broadcast and regularisers are O(1) launches on one pointer, while
`state_dict()` names, shapes and `nn.Parameter` identities stay those of the reference.

Inside an atomic block the three branches are laid out *fused*: expand weights of all branches form one [HT, inp] matrix,
projection weights one [oup, HT] matrix, BN vectors one [HT] vector, where each branch owns a segment whose length is
rounded up to 16 channels, one slab of the slab-major hidden tensors (HT = sum of padded segments).  Padding entries are zeros that belong to no Parameter; they
stay zero under training (their gradients are identically zero) and let every kernel use aligned 16-byte accesses after a
shrink has produced ragged channel counts (13, 139, ...).

Where everything lives is decided by ONE walk of the module tree, arena_layout(model, compute_dtype) -> ArenaLayout: offsets in the
arenas and pack buffers, the bind list, the pack and fold jobs and one description per plan.  It is integer arithmetic on module
attributes, runs on a CPU model and is pinned by tests/golden/arena_layout.json (tools/make_arena_layout.py): a new slot or table is
added in the walker that owns the module kind, and the table shows what moved.  ArenaManager.materialize is then four steps: layout,
allocate, migrate the values (one job-table launch), bind the plans' views.
"""
import collections
import ctypes

import torch
from torch import nn

from . import ops

ALIGN = 256  # arena slots start on 256-element (1 KiB) boundaries


def pad8(c):
    return (c + 7) // 8 * 8


def pads(c):
    """width of a branch segment inside a block's hidden tensor: whole 16-channel slabs (slab-major layout, ops.Slab)"""
    return (c + 15) // 16 * 16


def pad32(c):
    return (c + 31) // 32 * 32


def pad64(c):
    return (c + 63) // 64 * 64


def _align(n, a=ALIGN):
    return (n + a - 1) // a * a


class _Layout:
    """Assigns offsets inside one arena."""

    def __init__(self):
        self.size = 0

    def take(self, numel, align=ALIGN):
        off = self.size
        self.size = _align(off + max(int(numel), 1), align)
        return off


class _PackJob(ctypes.Structure):   # atomnas_pack_weights / atomnas_gather_jobs
    _fields_ = [("src_off", ctypes.c_long), ("dst_off", ctypes.c_long), ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("src_ld", ctypes.c_int), ("dst_ld", ctypes.c_int), ("c_off", ctypes.c_int), ("mode", ctypes.c_int)]


class _FoldJob(ctypes.Structure):   # ops.fold_jobs, csrc/reduce.hip k_fold_jobs
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("src_ld", ctypes.c_long), ("dst_ld", ctypes.c_long),
                ("rows", ctypes.c_int), ("cols", ctypes.c_int), ("blk0", ctypes.c_uint), ("pad_", ctypes.c_int)]


class _RegJob(ctypes.Structure):    # atomnas_reg_value / atomnas_reg_grad
    _fields_ = [("off", ctypes.c_long), ("count", ctypes.c_int), ("coef", ctypes.c_float)]


def _device_table(struct, rows, dev):
    """the rows as an array of `struct` in device memory (a byte tensor)"""
    arr = (struct * len(rows))(*[struct(*r) for r in rows])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(dev)


def _view(arena, off, shape, strides):
    if strides is None:
        n = 1
        for s in shape:
            n *= s
        return arena[off:off + n].view(shape)
    return torch.as_strided(arena, shape, strides, off)


class PwPack:
    """Packed 1x1 weight in both orientations (see atomnas_pack_weights)."""
    __slots__ = ("w", "wt", "n", "k")


class BlockPlan:
    """Everything the executor needs for one InvertedResidualChannels block: views into arenas and pack buffers."""

    def __init__(self):
        self.valid = False

    def __deepcopy__(self, memo):
        return None   # plans point into the owner's arenas: a copied module gets its own at its first use (plan_of)


class SimplePlan:
    def __deepcopy__(self, memo):
        return None


class ArenaLayout:
    """Where everything of one model lives, as plain data (arena_layout): integer arithmetic on module attributes.  The walkers below are
    the one place that hands out a slot; ArenaManager.materialize allocates, migrates and binds what they wrote down."""

    def __init__(self, compute_dtype):
        self.compute_dtype = compute_dtype
        self.lp, self.ls, self.lc = _Layout(), _Layout(), _Layout()      # params / bn stats / counters
        self.lpk, self.lpf, self.lfw = _Layout(), _Layout(), _Layout()   # packed weights (T) / packed depthwise taps (fp32) / fold scratch
        self.binds = []        # (arena name, module, attribute, offset, shape, strides) of every parameter and buffer, in migration order
        self.reg_slots = []    # (kind, offset, numel) of weight slots for the L2 regulariser: dense / dw / fc / fcbias
        self.jobsT, self.jobsF = [], []   # pack jobs into packT / packF: the rows of _PackJob
        self.fold_jobs = []    # fold jobs of the fused blocks: (scratch offset, gradient-arena offset, src_ld, dst_ld, rows, cols)
        self.plans = []        # (module, plan carrying its scalar fields, dict(so=slot offsets, pk=pack offsets, mods=BatchNorms, act=module))

    @property
    def sizes(self):
        """elements of P (= G, SQ, BUF, EMA), S (= SEMA), CNT, packT, packF and the fold scratch FW"""
        return dict(P=max(self.lp.size, ALIGN), S=max(self.ls.size, ALIGN), CNT=max(self.lc.size, 8), packT=max(self.lpk.size, ALIGN),
                    packF=max(self.lpf.size, ALIGN), FW=max(self.lfw.size, ALIGN))

    # ---- slots
    def param(self, mod, attr, off, shape, strides=None):
        self.binds.append(("P", mod, attr, off, tuple(shape), strides))

    def weight(self, kind, numel):
        """a parameter slot that the L2 regulariser covers whole"""
        off = self.lp.take(numel)
        self.reg_slots.append((kind, off, numel))
        return off

    def bn_slots(self, C):
        return dict(g=self.lp.take(C), b=self.lp.take(C), rm=self.ls.take(C), rv=self.ls.take(C))

    def bind_bn(self, bn, slots, seg, c):
        if bn.affine:
            self.param(bn, "weight", slots["g"] + seg, (c,))
            self.param(bn, "bias", slots["b"] + seg, (c,))
        if bn.track_running_stats:
            self.binds.append(("S", bn, "running_mean", slots["rm"] + seg, (c,), None))
            self.binds.append(("S", bn, "running_var", slots["rv"] + seg, (c,), None))
            self.binds.append(("CNT", bn, "num_batches_tracked", self.lc.take(1, 1), (), None))

    def pw_pack(self, rows, cols, pieces):
        """T pack buffers of W[rows][cols] and of its transpose, filled from `pieces` of the master: (src_off, rows, cols, src_ld, first
        row, first column) each.  Returns (offset, padded rows, ld) of both."""
        ldw, ldt = pad32(cols), pad32(rows)
        o_w, o_t = self.lpk.take(pad64(rows) * ldw), self.lpk.take(pad64(cols) * ldt)
        for src, r, c, src_ld, row0, col0 in pieces:
            self.jobsT.append((src, o_w + row0 * ldw, r, c, src_ld, ldw, col0, 0))
            self.jobsT.append((src, o_t + row0, r, c, src_ld, ldt, col0, 1))
        return (o_w, pad64(rows), ldw), (o_t, pad64(cols), ldt)

    def dw_taps(self, src_off, c, kk):
        """fp32 tap-major [kk][c] copy of a depthwise weight [c][kk]"""
        o_f = self.lpf.take(kk * c)
        self.jobsF.append((src_off, o_f, c, kk, kk, c, 0, 2))
        return (o_f, kk, c)

    def _done(self, m, pl, **info):
        pl.g_hi = self.lp.size
        self.plans.append((m, pl, info))

    # ---- walkers
    def block(self, name, m):
        """InvertedResidualChannels and InvertedResidualChannelsFused (models/mobilenet_base.py).  The kernels run both on the same
        padded-segment layout: every branch owns a segment of the hidden tensors, padded to whole slabs (HT = sum of the segments).  Two
        things differ.  The branch block's masters ARE that layout (one padded [HT] matrix / vector that the branches' parameters are
        views of); the fused block has ONE expand conv / BN and ONE projection conv over all `total` hidden channels, CONTIGUOUS masters
        as the reference's state_dict has them, which reach the padded layout through per-segment pack jobs and leave it through
        per-segment fold jobs.  And only the fused block carries SE."""
        from .models import mobilenet_base as mb  # local import: avoids a cycle
        fused = isinstance(m, mb.InvertedResidualChannelsFused)
        pl = BlockPlan()
        pl.g_lo = self.lp.size
        pl.name, pl.module, pl.fused = name, m, fused
        inp, oup = pl.inp, pl.oup = m.input_dim, m.output_dim
        pl.stride, pl.expand, pl.res = m.stride, m.expand, m.use_res_connect
        ks, hid = pl.ks, pl.hid = list(m.kernel_sizes), list(m.channels)
        branches = [list(op.children()) for op in (m.depth_ops if fused else m.ops)]
        pl.nb = len(branches)
        pl.se = fused and isinstance(m.se_op, mb.SqueezeAndExcitation)
        if pl.nb == 0:
            # an all-pruned block keeps only its (unused) pw_bn; give it ordinary slots.  The fused block keeps nothing
            pl.HT = 0
            if not fused:
                self.bind_bn(m.pw_bn, self.bn_slots(oup), 0, oup)
            return self._done(m, pl)
        # expanding blocks keep their hidden tensors slab-major (segments = whole 16-channel slabs); the first block of the network (no
        # expansion: hidden = input, narrow) stays plain with 8-channel padding
        sp = pl.segpad = pads if m.expand else pad8
        pl.seg, start = [], []
        HT = total = 0
        for h in hid:
            pl.seg.append(HT)
            start.append(total)
            HT += sp(h)
            total += h
        pl.HT = HT
        if fused:
            pl.start, pl.total = start, total
        wide = total if fused else HT                                     # width of the expand / projection masters
        segs = list(zip(pl.seg, start if fused else pl.seg, hid))        # (padded offset, offset in the masters, channels)

        so, pk, mods = {}, {}, dict(bne=[], bnd=[])
        depth = 1 if m.expand else 0    # a branch's children: [expand ConvBNReLU | Narrow], depthwise ConvBNReLU[, projection conv]
        if m.expand:
            so["We"] = self.weight("dense", wide * inp)
            so["bne"] = self.bn_slots(wide)
        so["Wd"] = [self.weight("dw", sp(h) * k * k) for h, k in zip(hid, ks)]
        so["bnd"] = self.bn_slots(HT)
        so["Wp"] = self.weight("dense", oup * wide)
        so["bnp"] = self.bn_slots(oup)

        def bind_expand(cbr, at, c):
            conv, bn, _ = cbr.children()
            self.param(conv, "weight", so["We"] + at * inp, (c, inp, 1, 1))
            self.bind_bn(bn, so["bne"], at, c)
            mods["bne"].append(bn)

        if fused and m.expand:
            bind_expand(m.expand_conv, 0, total)
        for ch, (sg, at, h), k, o_d in zip(branches, segs, ks, so["Wd"]):
            if m.expand and not fused:
                bind_expand(ch[0], at, h)
            conv, bn, _ = ch[depth].children()
            self.param(conv, "weight", o_d, (h, 1, k, k))
            self.bind_bn(bn, so["bnd"], sg, h)
            mods["bnd"].append(bn)
            if not fused:
                self.param(ch[-1], "weight", so["Wp"] + at, (oup, h, 1, 1), (HT, 1, 1, 1))
        if fused:
            pconv, out_bn = m.project_conv.children()
            self.param(pconv, "weight", so["Wp"], (oup, total, 1, 1))
        else:
            out_bn = m.pw_bn
        self.bind_bn(out_bn, so["bnp"], 0, oup)
        mods["bnp"] = [out_bn]

        if m.expand:
            pieces = [(so["We"] + at * inp, h, inp, inp, sg, 0) for sg, at, h in segs] if fused else [(so["We"], HT, inp, inp, 0, 0)]
            pk["We"], pk["WeT"] = self.pw_pack(HT, inp, pieces)
        pieces = [(so["Wp"] + at, oup, h, total, 0, sg) for sg, at, h in segs] if fused else [(so["Wp"], oup, HT, HT, 0, 0)]
        pk["Wp"], pk["WpT"] = self.pw_pack(oup, HT, pieces)
        pk["taps"] = [self.dw_taps(o_d, sp(h), k * k) for o_d, h, k in zip(so["Wd"], hid, ks)]

        if pl.se:
            se = m.se_op
            nh = pl.se_hid = se.n_hidden
            for conv, key in ((se.se_reduce, "se1"), (se.se_expand, "se2")):
                so[key + "w"] = self.weight("dense", conv.weight.numel())
                so[key + "b"] = self.lp.take(conv.bias.numel())
                self.param(conv, "weight", so[key + "w"], tuple(conv.weight.shape))
                self.param(conv, "bias", so[key + "b"], tuple(conv.bias.shape))
            # fp32 copies of the gate's dense layers over the padded channel layout, both with the channels contiguous:
            # W1p[j][sg + c] = W1[j][st + c], W2t[j][sg + c] = W2[st + c][j], b2p[sg + c] = b2[st + c] (csrc/se.hip k_se_mlp)
            o1, o2, o3 = pk["se"] = (self.lpf.take(nh * HT), self.lpf.take(nh * HT), self.lpf.take(HT))
            for sg, at, h in segs:
                self.jobsF.append((so["se1w"] + at, o1, nh, h, total, HT, sg, 0))
                self.jobsF.append((so["se2w"] + at * nh, o2, h, nh, nh, HT, sg, 2))
                self.jobsF.append((so["se2b"] + at, o3, 1, h, total, HT, sg, 0))
        if fused:
            # one weight-gradient GEMM per layer into a padded scratch matrix, folded into the contiguous tensors per segment
            pl.fold_first, pl.fold_np, pl.fold_ne = len(self.fold_jobs), pl.nb, pl.nb if m.expand else 0
            o_p = pl.Wp_scratch_off = self.lfw.take(oup * HT)
            self.fold_jobs += [(o_p + sg, so["Wp"] + at, HT, total, oup, h) for sg, at, h in segs]
            if m.expand:
                o_e = pl.We_scratch_off = self.lfw.take(HT * inp)
                self.fold_jobs += [(o_e + sg * inp, so["We"] + at * inp, h * inp, h * inp, 1, h * inp) for sg, at, h in segs]
        self._done(m, pl, so=so, pk=pk, mods=mods, act=branches[0][depth][2])

    def convbn(self, name, m):
        conv, bn, act = m.children()
        pl = SimplePlan()
        pl.g_lo = self.lp.size
        pl.name, pl.module = name, m
        pl.cin, pl.cout, pl.k, pl.stride, pl.groups = conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0], conv.groups
        C, Cp = conv.out_channels, pad8(conv.out_channels)
        kk = conv.kernel_size[0] * conv.kernel_size[1]
        cols = (conv.in_channels // conv.groups) * kk
        so = dict(W=self.lp.take(Cp * cols), bn=self.bn_slots(Cp))
        self.reg_slots.append(("dense" if conv.groups == 1 else "dw", so["W"], C * cols))
        self.param(conv, "weight", so["W"], tuple(conv.weight.shape))
        self.bind_bn(bn, so["bn"], 0, C)
        pk = {}
        if conv.groups == 1:
            pk["W"], pk["WT"] = self.pw_pack(C, cols, [(so["W"], C, cols, cols, 0, 0)])
        elif conv.groups == conv.in_channels == C:
            pk["taps"] = self.dw_taps(so["W"], Cp, kk)
        else:
            raise NotImplementedError("grouped convolution other than depthwise")
        self._done(m, pl, so=so, pk=pk, mods=dict(bn=[bn]), act=act)

    def linear(self, name, m):
        pl = SimplePlan()
        pl.g_lo = self.lp.size
        pl.name, pl.module = name, m
        n, k = pl.cout, pl.cin = m.out_features, m.in_features
        so = dict(W=self.weight("fc", n * k), b=self.lp.take(pad8(n)))
        self.param(m, "weight", so["W"], (n, k))
        if m.bias is not None:
            self.reg_slots.append(("fcbias", so["b"], n))
            self.param(m, "bias", so["b"], (n,))
        pk = {}
        pk["W"], pk["WT"] = self.pw_pack(n, k, [(so["W"], n, k, k, 0, 0)])
        self._done(m, pl, so=so, pk=pk)


def arena_layout(model, compute_dtype):
    """The arena layout of `model` (on any device; nothing is allocated and no library call is made): one walk of the module tree."""
    from .models import mobilenet_base as mb  # local import: avoids a cycle

    lay = ArenaLayout(compute_dtype)
    handled = set()
    for name, m in model.named_modules():
        if isinstance(m, (mb.InvertedResidualChannels, mb.InvertedResidualChannelsFused)):
            walk = lay.block
        elif isinstance(m, mb.ConvBNReLU) and id(m) not in handled:
            walk = lay.convbn
        elif isinstance(m, nn.Linear) and id(m) not in handled:
            walk = lay.linear
        else:
            continue
        handled.update(id(sub) for sub in m.modules())
        walk(name, m)
    # anything else that owns parameters (e.g. SE convs with bias) gets plain slots
    for name, m in model.named_modules():
        if id(m) in handled:
            continue
        for attr, p in list(m._parameters.items()):
            if p is None:
                continue
            lay.param(m, attr, lay.lp.take(p.numel()), tuple(p.shape))
        if isinstance(m, nn.BatchNorm2d):
            raise NotImplementedError("BatchNorm2d outside ConvBNReLU / InvertedResidualChannels: %s" % name)
    return lay


class ArenaManager:
    """Owns the arenas of one model (attached as model._arena)."""

    def __deepcopy__(self, memo):
        return None   # copy.deepcopy(model) must not drag the arenas, optimizers and EMA of the source along (common.get_ema_model)

    def __init__(self, model):
        self.model = model
        self.dirty = True
        self.optimizers = []
        self.emas = []
        self.P = self.G = self.SQ = self.BUF = self.EMA = self.S = self.SEMA = self.CNT = None
        self._stats_ws, self._stats_off, self._stats_need = None, 0, 0
        self.version = 0
        self.step_counter = None   # device int64[1]: the dropout / stochastic-depth counter, one per micro-batch ever drawn
        self._counter_start = 0    # its value at the first materialisation (set_step_counter before the arenas exist: a resumed run)
        self.param_slots = collections.OrderedDict()  # name -> (off, shape, strides) of every nn.Parameter
        self.compute_dtype = getattr(model, "compute_dtype", torch.bfloat16)

    # ------------------------------------------------------------------ registration
    def attach_optimizer(self, opt):
        if not any(o is opt for o in self.optimizers):
            self.optimizers.append(opt)
            self.dirty = True

    def attach_ema(self, ema):
        if not any(e is ema for e in self.emas):
            self.emas.append(ema)
            self.dirty = True

    def mark_dirty(self):
        self.dirty = True

    def set_step_counter(self, value):
        """The dropout counter of a run that continues another one (train.resume_run): the number of micro-batches drawn so far.  Works
        before the first materialisation (the arenas then start from it) and after it (the tensor captured graphs read is kept)."""
        self._counter_start = int(value)
        if self.step_counter is not None:
            self.step_counter.fill_(int(value))

    def ensure(self):
        if self.dirty:
            self.materialize()

    @property
    def device(self):
        return next(self.model.parameters()).device

    # ------------------------------------------------------------------ layout -> allocate -> migrate -> bind
    def materialize(self):
        """(Re)builds all arenas from the current module tree, migrating values, optimizer state and EMA shadows."""
        dev = self.device
        if dev.type != "cuda":
            raise ops._lib.AtomnasHipError("the AtomNAS arenas live in HBM: move the model to the GPU first (model.cuda())")
        self.compute_dtype = getattr(self.model, "compute_dtype", self.compute_dtype)
        lay = arena_layout(self.model, self.compute_dtype)
        new = self._allocate(lay.sizes, dev)
        self._migrate(lay.binds, new, dev)
        for key, arena in new.items():
            setattr(self, key, arena)
        self._bind(lay, dev)

    def _allocate(self, sizes, dev):
        """zeroed arenas; the optimizer and EMA arenas only where an attached optimizer / EMA keeps such state"""
        def zeros(n, wanted=True):
            return torch.zeros(n, dtype=torch.float32, device=dev) if wanted else None

        nP, nS = sizes["P"], sizes["S"]
        square_avg = any(getattr(o, "needs_square_avg", True) for o in self.optimizers)
        momentum = any(g["momentum"] > 0 for o in self.optimizers for g in o.param_groups)
        has_ema = len(self.emas) > 0
        return dict(P=zeros(nP), G=zeros(nP), S=zeros(nS), CNT=torch.zeros(sizes["CNT"], dtype=torch.int64, device=dev),
                    SQ=zeros(nP, square_avg), BUF=zeros(nP, momentum), EMA=zeros(nP, has_ema), SEMA=zeros(nS, has_ema))

    def _migrate(self, binds, new, dev):
        """Moves every value into its slot of the `new` arenas and re-points the modules' tensors, optimizer state and EMA shadows."""
        model = self.model
        name_of = {id(p): n for n, p in model.named_parameters()}
        name_of.update({id(b): n for n, b in model.named_buffers()})
        self.param_slots = collections.OrderedDict()
        self.buffer_slots = collections.OrderedDict()
        # The value migration is ~2,500 small copies per rebuild (every parameter, its RMSprop state, its EMA shadow, every BatchNorm
        # buffer): recorded and run as ONE launch of the shrink's job-table kernel (ops.copy_job -> atomnas_gather_jobs) where the pair
        # is fp32 on this device; anything else (the first build from host tensors, int64 counters) is a torch copy as before.
        def move(dst, src):
            if not ops.copy_job(dst, src):
                dst.copy_(src.to(dev))
        # A rebuild inside a deferral window (a forward, profiling pass or optimizer call between a shrink's gathers and their flush):
        # the pending gathers WRITE the module tensors the migration below READS, and one job-table launch has no order between its
        # workgroups -- run them first.  The migration's own jobs are flushed before anything reads the new arenas, and the deferral
        # state is restored even when the walk raises.
        was_deferring = ops.gather_deferring()
        if was_deferring:
            ops.gather_flush()
        else:
            ops.gather_defer(True)
        try:
            with torch.no_grad():
                for arena_name, mod, attr, off, shape, strides in binds:
                    if arena_name == "P":
                        p = mod._parameters[attr]
                        nm = name_of.get(id(p))
                        newv = _view(new["P"], off, shape, strides)
                        move(newv, p.data)
                        # optimizer state and EMA shadows follow the parameter
                        for opt in self.optimizers:
                            st = opt.state.get(p)
                            if st:
                                for key, arena in (("square_avg", new["SQ"]), ("momentum_buffer", new["BUF"])):
                                    if key in st and arena is not None:
                                        nv = _view(arena, off, shape, strides)
                                        move(nv, st[key])
                                        st[key] = nv
                        for ema in self.emas:
                            if nm is not None and nm in ema._shadow:
                                nv = _view(new["EMA"], off, shape, strides)
                                move(nv, ema._shadow[nm])
                                ema._shadow[nm] = nv
                        p.data = newv
                        p.grad = _view(new["G"], off, shape, strides)
                        p._atomnas_off = off
                        p._atomnas_mgr = self
                        if nm is not None:
                            self.param_slots[nm] = (off, shape, strides)
                    else:
                        b = mod._buffers[attr]
                        nm = name_of.get(id(b))
                        if arena_name == "S":
                            newv = _view(new["S"], off, shape, None)
                            move(newv, b)
                            for ema in self.emas:
                                if nm is not None and nm in ema._shadow:
                                    nv = _view(new["SEMA"], off, shape, None)
                                    move(nv, ema._shadow[nm])
                                    ema._shadow[nm] = nv
                        else:
                            newv = new["CNT"][off:off + 1].view(shape)
                            newv.copy_(b.to(dev))
                        mod._buffers[attr] = newv
                        if nm is not None:
                            self.buffer_slots[nm] = (arena_name, off, shape)

        finally:
            if not was_deferring:
                ops.gather_defer(False)   # the migration runs here (one launch), before anything reads the new arenas
            else:
                ops.gather_flush()

    def _bind(self, lay, dev):
        """Pack buffers, job tables and the plans' views over the arenas just filled; the per-build state of the step."""
        sizes = lay.sizes
        self.nP, self.nS = sizes["P"], sizes["S"]
        self.reg_slots = lay.reg_slots
        self.packT = torch.zeros(sizes["packT"], dtype=self.compute_dtype, device=dev)
        self.packF = torch.zeros(sizes["packF"], dtype=torch.float32, device=dev)
        self.jobsT = _device_table(_PackJob, lay.jobsT, dev) if lay.jobsT else None
        self.jobsF = _device_table(_PackJob, lay.jobsF, dev) if lay.jobsF else None
        self.njobsT, self.njobsF = len(lay.jobsT), len(lay.jobsF)
        self.plans = {}
        for m, pl, info in lay.plans:
            pl.mgr = self
            self._bind_plan(m, pl, info)
            object.__setattr__(m, "_plan", pl)
            self.plans[pl.name] = pl
        # fused blocks: padded scratch matrices of the expand / projection weight gradients and the table that folds them into the
        # contiguous gradient tensors (ops.fold_jobs, csrc/reduce.hip k_fold_jobs)
        self.FW = torch.zeros(sizes["FW"], dtype=torch.float32, device=dev)   # zero once: every fold clears what it read
        self.fold_table, self.fold_blk0, rows = None, [0], []
        for so, do, sld, dld, r, c in lay.fold_jobs:
            rows.append((self.FW.data_ptr() + 4 * so, self.G.data_ptr() + 4 * do, sld, dld, r, c, self.fold_blk0[-1], 0))
            self.fold_blk0.append(self.fold_blk0[-1] + (r * c + 255) // 256)
        if rows:
            self.fold_table = _device_table(_FoldJob, rows, dev)

        for opt in self.optimizers:
            opt._on_materialize(self)
        for ema in self.emas:
            ema._on_materialize(self)
        self.anchor = torch.zeros(1, dtype=torch.float32, device=dev, requires_grad=True)
        # lr, rho, ema decay, grad scale (atomnas_hip.h: the kernels read slots 0..3); slot 4 is the engine's own: the number of
        # ranks the gradients of this step were summed over (multiplier of the per-rank L1 sub-gradient, engine.TrainStep._opt)
        self.hyper = torch.zeros(8, dtype=torch.float32, device=dev)
        self.hyper[3] = 1.0
        self.hyper[4] = 1.0
        self.hyper_host = torch.zeros(8, dtype=torch.float32)
        self.hyper_host[3] = 1.0
        self.hyper_host[4] = 1.0
        self._hyper_ring = torch.zeros(64, 8, dtype=torch.float32).pin_memory()  # staging slots: the host may run ahead
        self._hyper_slot = 0
        # decorrelates dropout masks across iterations.  It counts the micro-batches of the RUN: a rebuild (a shrink) carries it over, so
        # the steps after one do not draw the masks of steps 0, 1, 2, ... again
        old = self.step_counter
        self.step_counter = torch.full((1,), self._counter_start, dtype=torch.int64, device=dev)
        if old is not None:
            self.step_counter.copy_(old)
        self.bn_trained = False
        self._depth = 0
        self.dirty = False
        self.version += 1
        self.pack()

    # gradient-completion hook: every executor calls grad_done(plan) at the end of its backward; engine.TrainStep uses it to
    # all-reduce the finished part of the gradient arena while the rest of backward is still running
    grad_done_cb = None

    def grad_done(self, pl):
        cb = self.grad_done_cb
        if cb is not None:
            cb(pl)

    def _bnv(self, sl, n, mods, C=None, **segmented):
        """The dict the executors take for one BatchNorm slot group: views of `n` elements, C channels of which are the modules'."""
        P, G, S = self.P, self.G, self.S
        return dict(gamma=P[sl["g"]:sl["g"] + n], beta=P[sl["b"]:sl["b"] + n], dgamma=G[sl["g"]:sl["g"] + n],
                    dbeta=G[sl["b"]:sl["b"] + n], rm=S[sl["rm"]:sl["rm"] + n], rv=S[sl["rv"]:sl["rv"] + n],
                    C=n if C is None else C, mods=mods, mgr=self, **segmented)

    @staticmethod
    def _unit_padding_var(bnv, spans):
        """running_var of the padding channels [lo, hi) = 1, so that eval-mode coefficients stay finite there (padding gamma is 0, so
        the value never matters)"""
        with torch.no_grad():
            for lo, hi in spans:
                bnv["rv"][lo:hi] = 1.0

    def _packview(self, t):
        off, rows, ld = t
        return self.packT[off:off + rows * ld].view(rows, ld)

    def _tapview(self, t):
        off, kk, c = t
        return self.packF[off:off + kk * c].view(kk, c)

    def _bind_plan(self, m, pl, info):
        from .functional import act_code
        P, G = self.P, self.G
        if isinstance(pl, BlockPlan):
            pl.valid = True
            if pl.nb == 0:
                return
        so, pk = info["so"], info["pk"]
        if isinstance(m, nn.Linear):
            pl.W_grad = G[so["W"]:so["W"] + pl.cout * pl.cin]
            pl.bias = P[so["b"]:so["b"] + pad8(pl.cout)] if m.bias is not None else None
            pl.bias_grad = G[so["b"]:so["b"] + pl.cout] if m.bias is not None else None
            pl.W_pack, pl.WT_pack = self._packview(pk["W"]), self._packview(pk["WT"])
            return
        pl.act = act_code(info["act"])
        mods = info["mods"]
        if isinstance(pl, SimplePlan):   # ConvBNReLU
            C, Cp = pl.cout, pad8(pl.cout)
            pl.bn = self._bnv(so["bn"], Cp, mods["bn"], C=C)
            pl.W_grad = G[so["W"]:so["W"] + m[0].weight.numel()]
            if "W" in pk:
                pl.W_pack, pl.WT_pack = self._packview(pk["W"]), self._packview(pk["WT"])
            else:
                pl.taps = self._tapview(pk["taps"])
            self._unit_padding_var(pl.bn, [(C, Cp)])
            return
        HT, fused = pl.HT, pl.fused
        wide = pl.total if fused else HT     # contiguous masters (fused) or padded segments (branch), see ArenaLayout.block
        padding = [(s + h, s + pl.segpad(h)) for s, h in zip(pl.seg, pl.hid)]
        segmented = {}
        if fused:
            # padded kernel channel -> index into the module's contiguous [total] vectors, -1 for the padding between branch segments
            cmap = torch.full((HT,), -1, dtype=torch.int32)
            for sg, st, h in zip(pl.seg, pl.start, pl.hid):
                cmap[sg:sg + h] = torch.arange(st, st + h, dtype=torch.int32)
            pl.cmap = cmap.to(P.device)
            segmented = dict(cmap=pl.cmap, Cpad=HT)   # contiguous [total] vectors, padded [HT] kernel layout
        if pl.expand:
            pl.We_grad = G[so["We"]:so["We"] + wide * pl.inp]
            pl.bne = self._bnv(so["bne"], wide, mods["bne"], **segmented)
            pl.We_pack, pl.WeT_pack = self._packview(pk["We"]), self._packview(pk["WeT"])
            if not fused:
                self._unit_padding_var(pl.bne, padding)
        pl.Wd_grad = [G[o:o + pl.segpad(h) * k * k] for o, h, k in zip(so["Wd"], pl.hid, pl.ks)]
        pl.bnd = self._bnv(so["bnd"], HT, mods["bnd"])
        self._unit_padding_var(pl.bnd, padding)
        pl.Wp_grad = G[so["Wp"]:so["Wp"] + pl.oup * wide]
        pl.bnp = self._bnv(so["bnp"], pl.oup, mods["bnp"])
        pl.Wp_pack, pl.WpT_pack = self._packview(pk["Wp"]), self._packview(pk["WpT"])
        pl.taps = [self._tapview(t) for t in pk["taps"]]
        if pl.se:
            total, nh = pl.total, pl.se_hid
            n1, n2 = nh * total, total * nh
            pl.se_w1, pl.se_b1 = P[so["se1w"]:so["se1w"] + n1], P[so["se1b"]:so["se1b"] + nh]
            pl.se_w2, pl.se_b2 = P[so["se2w"]:so["se2w"] + n2], P[so["se2b"]:so["se2b"] + total]
            pl.se_dw1, pl.se_db1 = G[so["se1w"]:so["se1w"] + n1], G[so["se1b"]:so["se1b"] + nh]
            pl.se_dw2, pl.se_db2 = G[so["se2w"]:so["se2w"] + n2], G[so["se2b"]:so["se2b"] + total]
            pl.se_act = act_code(m.se_op.active_fn)
            o1, o2, o3 = pk["se"]
            pl.se_w1p, pl.se_w2t, pl.se_b2p = self.packF[o1:o1 + nh * HT], self.packF[o2:o2 + nh * HT], self.packF[o3:o3 + HT]

    # ------------------------------------------------------------------ regulariser tables
    def reg_table(self, entries):
        """entries: list of (offset, count, coef) -> device table for atomnas_reg_value / atomnas_reg_grad"""
        return _device_table(_RegJob, [(int(o), int(c), float(k)) for o, c, k in entries], self.device), len(entries)

    # ------------------------------------------------------------------ per-step helpers
    def pack(self):
        """Refreshes the packed (kernel-layout, compute-dtype) copies of all weights from the fp32 master arena."""
        if self.njobsT:
            ops.pack_weights(self.P, self.packT, self.jobsT, self.njobsT, self.compute_dtype)
        if self.njobsF:
            ops.pack_weights(self.P, self.packF, self.jobsF, self.njobsF, torch.float32)

    def zero_grad(self):
        ops.zero_(self.G)

    def push_hyper(self):
        """host -> device copy of (lr, rho, EMA decay, grad scale), stream-ordered before the kernels that read them"""
        slot = self._hyper_ring[self._hyper_slot % 64]
        self._hyper_slot += 1
        slot.copy_(self.hyper_host)
        self.hyper.copy_(slot, non_blocking=True)

    # ---- per-step statistics workspace: every BatchNorm use of a step (forward and backward) takes a distinct slice of partial
    # rows.  The producing kernels write every row (include/atomnas_hip.h), so nothing is ever cleared.  A slice is dead as soon
    # as its finalize kernel has run, so re-using the workspace from the next top-level forward on is safe even when a
    # backward is still pending.
    def take_stats(self, n):
        n = (n + 63) // 64 * 64
        off = self._stats_off
        self._stats_off = off + n
        self._stats_need = max(self._stats_need, self._stats_off)
        ws = self._stats_ws
        if ws is None or off + n > ws.numel():
            return None    # first steps: the caller allocates; the workspace is sized at the next top-level forward
        return ws[off:off + n]

    def _reset_stats(self):
        ws = self._stats_ws
        if self._stats_need > (ws.numel() if ws is not None else 0):
            self._stats_ws = torch.empty(int(self._stats_need * 1.25) // 64 * 64 + 64, dtype=torch.float32, device=self.device)
        self._stats_off = 0

    # Outermost module call: refresh packed weights on entry; on exit bump every BN's num_batches_tracked once if any BN
    # ran with batch statistics (all BNs of the model share their mode in the reference's train / calibration phases).
    def enter(self):
        self.ensure()
        if self._depth == 0:
            self.pack()
            self.bn_trained = False
            self._reset_stats()
        self._depth += 1

    # engine.TrainStep sets it around the forward of every micro-batch of an accumulated step but the last: num_batches_tracked
    # advances once per optimizer step, and every micro-batch of a step sees the same counters (cumulative-average BatchNorms)
    hold_counters = False

    def leave(self):
        self._depth -= 1
        if self._depth == 0 and self.bn_trained:
            if not self.hold_counters:
                ops.add_i64(self.CNT, 1)
            self.bn_trained = False


def manager_of(module):
    """The arena manager that owns `module`: the one of the enclosing model once that has been materialised, otherwise a
    private one created on demand (a block or ConvBNReLU used on its own, as the reference's unit tests do)."""
    pl = getattr(module, "_plan", None)
    if pl is not None and getattr(pl, "mgr", None) is not None and pl.mgr.model is not None:
        return pl.mgr
    mgr = getattr(module, "_arena", None)
    if mgr is None:
        mgr = ArenaManager(module)
        object.__setattr__(module, "_arena", mgr)
    return mgr


def plan_of(module):
    """Plan (arena views) of `module`, (re)materialising its arenas if the structure changed since."""
    mgr = manager_of(module)
    mgr.ensure()
    pl = getattr(module, "_plan", None)
    if pl is None or pl.mgr is not mgr:
        mgr.mark_dirty()
        mgr.ensure()
        pl = module._plan
    return pl
