"""The training iteration of the hot path as one replayable hipGraph (train.py:165-236 of the reference, per process).

    zero_grad -> forward -> CE-smooth mean -> backward -> [gradient all-reduce] -> L1 / L2 gradients + RMSprop + EMA

Everything between the barriers is device work issued from Python once, captured with torch.cuda.graph (the HIP kernels
are launched on the capturing stream through the C ABI, so they become graph nodes) and replayed every iteration.  Values
that change per iteration (lr, rho, EMA decay) are staged through a 4-float device vector, inputs through static buffers.

Data parallelism (utils/distributed.py:131-139, 155-161 of the reference: one blocking all-reduce of all gradients after
backward): the gradient arena is summed over the ranks with RCCL.  With the nccl backend the collective is issued from INSIDE
backward, bucket by bucket on a side stream as soon as the blocks that own a bucket have finished (the arena is laid out in
module order, backward runs it from the end), and is captured into the same hipGraph as the kernels ("graph" mode); the 1/world
scale rides in the optimizer kernel.  Other backends (gloo in the tests) and a failed capture use one blocking all-reduce between
two graphs ("host" mode).

Gradient accumulation (accum_steps = A > 1): one optimizer step consumes A static batches, each a "virtual rank" of a W * A rank
data-parallel job with allreduce_bn.  accumulate() runs forward + backward of a micro-batch, step() the last one plus everything
that happens once per optimizer step.  Every micro-batch writes its gradients into the zeroed arena G exactly as a step of its own
would; one fold launch adds G to a second arena in micro-batch order, and the last fold leaves the sum in G (a second arena because
some gradients receive two additions per backward).  The BatchNorm running statistics of every micro-batch start
from the values at the start of the step, and the step leaves their mean.  A = 1 issues exactly what it did without the feature.

Guarded step (clip_norm and / or skip_nonfinite; both off, the default: nothing of it is allocated, captured or launched).  All of it
sits in _opt(), which every step form ends in: after the regulariser launches one fixed-order pass over the gradient arena G gives the
global L2 norm of the averaged gradient (cross entropy + L1; the L2 term is added inside the optimizer kernel and stays outside, as a
torch optimizer's weight_decay stays outside clip_grad_norm_), and a one-workgroup launch turns it into the verdict vector: OK, the
gradient scale hyper[HYP_GRAD_SCALE] * clip coefficient, norm, coefficient, two cumulative counters.  The guarded optimizer launch scales
by it, or, with OK = 0 (non-finite gradients), writes nothing; the BatchNorm running statistics, which the forward pass has already
overwritten, then go back to their values of the start of the step, and their EMA is left alone.  Nothing synchronises with the host.

Knowledge distillation (teacher=; None, the default: nothing of it is allocated, captured or launched).  A frozen second model of this
project runs its eval forward on the step's images in front of the student's forward, inside _fwd_bwd and therefore inside every step
form and every captured graph; its classifier writes into the static buffer teacher_logits, and the loss node computes
(1 - alpha) * CE_smooth + alpha * T^2 * KL(softmax(teacher / T) || softmax(student / T)) and its gradient in one launch
(atomnas_ce_distill).  loss[0] is the mean of that objective, kd the mean of its unweighted soft term.
"""
import os

import torch
import torch.distributed as dist

from . import ops, runtime
from .utils import optim as aopt
from .utils import prune as aprune

_DEFER_REDUCE = bool(int(os.environ.get("ATOMNAS_DEFER_REDUCE", "1")))   # experiment switch: batched weight-gradient reductions


HYP_SUMMED_RANKS = 4   # engine-owned slot of the per-step scalar vector (runtime.ArenaManager.hyper)


def check_clip_norm(clip_norm):
    """TrainStep's clip_norm argument -> the maximal norm as a float, or None for no clipping (None, 0)"""
    if clip_norm is None:
        return None
    if isinstance(clip_norm, bool) or not isinstance(clip_norm, (int, float)):
        raise TypeError("clip_norm must be a number or None, got %r" % (clip_norm,))
    if not clip_norm >= 0:   # NaN included
        raise ValueError("clip_norm must be >= 0 (0 or None: no clipping), got %r" % (clip_norm,))
    return float(clip_norm) if clip_norm else None


def check_teacher(model, teacher, alpha, temperature):
    """TrainStep's distillation arguments -> (alpha, temperature) as floats; ValueError for values outside 0 <= alpha <= 1, 0 < T < inf,
    alpha > 0 without a teacher, a teacher that is the student, one with another class count or on another device"""
    alpha, temperature = aopt.check_distill(alpha, temperature)
    if teacher is None:
        if alpha > 0.0:
            raise ValueError("distill_alpha = %r needs a teacher" % alpha)
        return alpha, temperature
    if teacher is model:
        raise ValueError("the teacher is the student object: distilling a network from itself is not supported")
    ks, kt = getattr(model, "num_classes", None), getattr(teacher, "num_classes", None)
    if ks is None or kt is None or ks != kt:
        raise ValueError("the teacher classifies %r classes, the student %r" % (kt, ks))
    ds, dt = next(model.parameters()).device, next(teacher.parameters()).device
    if ds != dt:
        raise ValueError("the teacher is on %s, the student on %s" % (dt, ds))
    return alpha, temperature


class TrainStep:

    def __init__(self, model, optimizer, ema=None, prune_info=None, weight_decay=1e-5, wd_method='mnas', label_smoothing=0.1,
                 batch_size=256, image_size=224, use_graph=True, process_group=None, world_size=1, allreduce_bn=False, accum_steps=1,
                 clip_norm=None, skip_nonfinite=False, teacher=None, distill_alpha=0.0, distill_temperature=1.0):
        """clip_norm: maximal global L2 norm of the gradient the optimizer consumes (torch.nn.utils.clip_grad_norm_; None or 0: no
        clipping).  skip_nonfinite: a step whose gradient arena holds a NaN or an Inf is dropped on the device (GradScaler-style): P, the
        optimizer state, both EMAs and the BN running statistics keep their values of before the step.  What a dropped step still
        advances, as GradScaler + a scheduler do: global_step, ema.note_updates (the EMA warm-up count), the learning-rate and rho
        schedules of the caller, the dropout counter and num_batches_tracked of every BatchNorm.  guard_state() reads the verdict."""
        self.clip_norm = check_clip_norm(clip_norm)   # first: a bad value is refused before any device work
        self.distill_alpha, self.distill_temperature = check_teacher(model, teacher, distill_alpha, distill_temperature)
        self.teacher = teacher
        self.model, self.optimizer, self.ema, self.prune_info = model, optimizer, ema, prune_info
        self.weight_decay, self.wd_method = weight_decay, wd_method
        self.use_graph = use_graph
        self.world_size = world_size
        self.pg = process_group
        # average the BN running statistics over the ranks every step, BEFORE their EMA (the reference's order: optimizer.step,
        # allreduce_bn, ema -- train.py:213-226); the optimizer does not read them, so they travel with the gradient collectives
        self.allreduce_bn = bool(allreduce_bn)
        dev = next(model.parameters()).device
        self.mgr = runtime.manager_of(model)
        self.mgr.attach_optimizer(optimizer)
        optimizer._mgr = self.mgr
        if ema is not None:
            ema.attach(self.mgr)
        self.mgr.ensure()
        self.label_smoothing = float(label_smoothing)
        self.x = torch.zeros(batch_size, 3, image_size, image_size, dtype=torch.float32, device=dev)
        self.y = torch.zeros(batch_size, dtype=torch.int64, device=dev)
        self._scal = torch.zeros(8, dtype=torch.float32, device=dev)   # per-step scalars, cleared by ONE memset per step
        self.loss = self._scal[0:3]                                    # CE (mean), L2, L1 of the last step
        self.topk = self._scal[4:6].view(torch.int32)                  # top-1 / top-5 hits of the last step (common.py:73-79)
        self.loss_vec = torch.zeros(batch_size, dtype=torch.float32, device=dev)   # per-sample CE of the last step
        # knowledge distillation (teacher None, the default: nothing below is allocated, captured or launched).  The teacher is frozen: eval
        # mode, no gradients, arenas of its own; the optimizer, the EMA, the prune table, a shrink, the collectives and a checkpoint never
        # see it (they are all built from `model`).  With several ranks every rank holds its own copy.
        self.kd = self.kd_vec = self.teacher_logits = self._teacher_out = self._distill = None
        if teacher is not None:
            teacher.eval()
            for p in teacher.parameters():
                p.requires_grad_(False)
            runtime.manager_of(teacher).ensure()   # before any capture
            K = int(model.num_classes)
            self._teacher_out = torch.zeros(batch_size, ops.pad8(K), dtype=torch.float32, device=dev)   # the teacher's classifier writes here
            self.teacher_logits = self._teacher_out[:, :K]
            self.kd = self._scal[3:4]                                              # mean of kd_vec, cleared with the other scalars
            self.kd_vec = torch.zeros(batch_size, dtype=torch.float32, device=dev)   # per-sample T^2 * KL(teacher || student)
            self._distill = (self.teacher_logits, self.distill_alpha, self.distill_temperature, self.kd_vec, self.kd)
        self._tables_version = -1
        self._comm = None          # side stream of the bucketed all-reduce
        self._buckets = []         # (first plan of the bucket, lo, hi) in backward order
        self._fired = 0
        self.comm_mode = None      # decided at the first step: "graph" | "host" | None (no collective)
        self.g_all = None
        self.g_fwd_bwd = self.g_opt = None
        self._version = -1
        self.global_step = 0
        self._seed_grad = None
        self._agree = torch.ones(1, dtype=torch.float32, device=dev)   # capture outcome, MIN-reduced over the ranks
        # gradient accumulation: accum_steps micro-batches per optimizer step (1: nothing below is ever allocated, captured or launched)
        if isinstance(accum_steps, bool) or int(accum_steps) != accum_steps or int(accum_steps) < 1:
            raise ValueError("accum_steps must be a positive integer, got %r" % (accum_steps,))
        self.accum_steps = int(accum_steps)
        self._pending = 0              # micro-batches accumulated since the last step() / reset_accumulation()
        self._group_version = -1       # arena version the current group started on
        self._acc_version = -1
        self._acc = self._sacc = self._sbase = None   # running sums of G (+ the CE mean behind it) and S, S at the start of the step
        self.g_mb = self.g_last = self.g_all_last = None   # graphs of a micro-batch / the last one / the last one with its collectives
        self._pool = None              # private pool shared by the graphs above: they never run concurrently
        self._fold_buckets = False     # the bucket hook folds its slice of G before the collective (last micro-batch, "graph" mode)
        # guarded step
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.clip_norm is not None or self.skip_nonfinite
        self._guard = self._guard_ws = None
        self._sbase_version = -1
        if self.guarded:
            self._guard = torch.zeros(ops.GUARD_WORDS, dtype=torch.float32, device=dev)   # verdict + cumulative counters (int32 bits)
            self._guard_ws = torch.empty(ops.grad_guard_ws_floats(), dtype=torch.float32, device=dev)

    # ---- pieces
    def _prune_weights(self):
        if self.prune_info is None or len(self.prune_info.weight) == 0:
            return [], []
        table = dict(self.model.named_parameters())
        return [table[n] for n in self.prune_info.weight], self.prune_info.penalty

    def _tables(self):
        """Per-arena-version device tables: weight-decay coefficient per 256-element chunk (cal_l2_loss, utils/optim.py:226-243:
        every conv / fc weight and the classifier bias for 'mnas'; dense conv and fc weights for 'slimmable') and the L1 job
        table (offset, count, penalty) of the prunable gammas (utils/prune.py:161-167)."""
        mgr = self.mgr
        if self._tables_version == mgr.version:
            return
        kinds = {'mnas': ('dense', 'dw', 'fc', 'fcbias'), 'slimmable': ('dense', 'fc')}.get(self.wd_method)
        if kinds is None:
            raise ValueError('Unknown weight_decay method: {}'.format(self.wd_method))
        wd = torch.zeros(mgr.nP // runtime.ALIGN, dtype=torch.float32)
        for kind, off, n in mgr.reg_slots:
            if kind in kinds:
                assert off % runtime.ALIGN == 0
                wd[off // runtime.ALIGN:(off + n + runtime.ALIGN - 1) // runtime.ALIGN] = self.weight_decay
        self._wd_chunk = wd.to(mgr.P.device)
        w, pen = self._prune_weights()
        self._l1 = mgr.reg_table([(p._atomnas_off, p.numel(), c) for p, c in zip(w, pen)]) if w else None
        self._ws = torch.empty(4096 + 64 * max(len(w), 1), dtype=torch.float32, device=mgr.P.device)
        self._tables_version = mgr.version

    # ---- gradient all-reduce overlapped with backward
    def _build_buckets(self, target_floats=4 << 20):
        """Cuts the gradient arena into ~16 MiB buckets at plan boundaries, from the end (backward order).  A bucket is complete
        when the plan with the LOWEST offset in it has finished its backward."""
        plans = sorted((p for p in self.mgr.plans.values() if getattr(p, "nb", 1) != 0), key=lambda p: p.g_lo)   # pruned-away blocks never run
        self._buckets = []
        hi = self.mgr.nP
        acc_lo = None
        for pl in reversed(plans):
            acc_lo = pl.g_lo
            if hi - acc_lo >= target_floats:
                self._buckets.append((pl, acc_lo, hi))
                hi = acc_lo
        if hi > 0:
            first = plans[0] if plans else None
            if self._buckets and self._buckets[-1][0] is first:
                pl, lo, bhi = self._buckets.pop()
                self._buckets.append((pl, 0, bhi))
            else:
                self._buckets.append((first, 0, hi))

    def _on_grad_done(self, pl):
        if self._fired < len(self._buckets) and self._buckets[self._fired][0] is pl:
            _, lo, hi = self._buckets[self._fired]
            self._fired += 1
            ops.reduce_flush()   # the bucket's weight gradients are complete only after their recorded reductions
            if self._fold_buckets:   # last micro-batch of an accumulated step: the collective travels the SUM of the micro-batches
                ops.accum_fold(self._acc[lo:hi], self.mgr.G[lo:hi], None, hi - lo, False, True)
            cur = torch.cuda.current_stream()
            self._comm.wait_stream(cur)
            with torch.cuda.stream(self._comm):
                dist.all_reduce(self.mgr.G[lo:hi], group=self.pg)

    def _reduce_bn(self):
        """utils/distributed.py:164-169 on the statistics arena: one collective + one launch (x 1/world from the hyper vector)"""
        mgr = self.mgr
        dist.all_reduce(mgr.S, group=self.pg)
        ops.scale_by(mgr.S, mgr.nS, mgr.hyper, ops.HYP_GRAD_SCALE)

    def _fwd_bwd_overlapped(self, last=None):
        """last=True: the last micro-batch of an accumulated step (every bucket is folded into the running sum before its collective,
        the statistics are folded before theirs); None: the plain step"""
        mgr = self.mgr
        self._fired = 0
        mgr.grad_done_cb = self._on_grad_done
        self._fold_buckets = last is not None
        try:
            self._fwd_bwd(last)
        finally:
            mgr.grad_done_cb = None
            self._fold_buckets = False
        cur = torch.cuda.current_stream()
        if last is not None:
            self._fold_stats(False, True, True)
        while self._fired < len(self._buckets):   # plans that took no part in this backward (none in the networks of this path)
            _, lo, hi = self._buckets[self._fired]
            self._fired += 1
            if last is not None:
                ops.accum_fold(self._acc[lo:hi], mgr.G[lo:hi], None, hi - lo, False, True)
            self._comm.wait_stream(cur)
            with torch.cuda.stream(self._comm):
                dist.all_reduce(mgr.G[lo:hi], group=self.pg)
        if self.allreduce_bn:
            self._comm.wait_stream(cur)
            with torch.cuda.stream(self._comm):
                self._reduce_bn()
        cur.wait_stream(self._comm)

    def _fold_stats(self, first, last, reducing):
        """The BatchNorm running statistics of one micro-batch into their running sum: S goes back to its values at the start of the
        step, or (last) becomes the mean over the micro-batches.  Where _reduce_bn follows it leaves the plain sum: that collective
        multiplies by 1 / (ranks * micro-batches) itself (HYP_GRAD_SCALE), one multiply as over that many real ranks."""
        mgr = self.mgr
        inv = 1.0 if (reducing and self.allreduce_bn) else 1.0 / self.accum_steps
        ops.accum_fold(self._sacc, mgr.S, self._sbase, mgr.nS, first, last, inv)

    def _fwd_bwd(self, last=None):
        """zero_grad -> forward -> label-smoothed CE (mean) -> backward, HIP launches only.  The regularisers do not go through
        autograd here: their gradients are added in _opt (L1: one launch on the gamma job table after the all-reduce; L2: inside
        the optimizer kernel), which is the same arithmetic as the reference's `loss + l2 + l1` backward because both terms are
        identical on every rank (train.py:171-185)."""
        mgr = self.mgr
        mgr.zero_grad()
        if self.guarded and self.accum_steps == 1:
            # the statistics a dropped step goes back to.  A kernel node of the captured step, not a captured copy (csrc/optim.hip k_zero
            # records why memset-like nodes are not trusted on replay).  Accumulated steps already keep this snapshot: accumulate()
            # takes _sbase when a group starts
            ops.guard_restore(self._stat_base(), mgr.S, mgr.nS, None, True)
        # last False / True: a micro-batch of an accumulated step.  Its scalars were cleared when the group started (the hit counts add
        # up over the micro-batches), and the BatchNorm counters advance with the last micro-batch only
        if last is None:
            ops.zero_(self._scal)
        loss_args = (self.y, self.label_smoothing, self.loss_vec, self.topk, self.loss[0:1])
        if self.teacher is not None:
            # the frozen teacher's eval forward on the same images, part of the same graph; it moves nothing of the teacher's state
            if self.teacher.training:
                self.teacher.eval()
            with torch.no_grad():
                self.teacher(self.x, logits_out=self._teacher_out)
            loss_args += (self._distill,)
        mgr.hold_counters = last is False
        try:
            loss = self.model(self.x, loss_args=loss_args)
        finally:
            mgr.hold_counters = False
        if self._seed_grad is None or self._seed_grad.shape != loss.shape:
            self._seed_grad = torch.ones_like(loss)   # allocated once: backward() would fill a fresh ones tensor every step
        # the fixed-order sums of the weight-gradient partials are recorded during backward and run as a few batched launches
        # (csrc/reduce.hip): ~110 graph nodes less per supernet step
        ops.reduce_defer(_DEFER_REDUCE)
        try:
            loss.backward(self._seed_grad)
        finally:
            ops.reduce_defer(False)   # flushes on the current stream
        if last is not None:
            nP = mgr.nP
            if not self._fold_buckets:   # G -> running sum; after the last micro-batch G holds the sum in micro-batch order
                ops.accum_fold(self._acc, mgr.G, None, nP, False, last)
            # CE mean -> running sum behind the gradients'; after the last micro-batch loss[0] is the mean of the micro-batch means
            # distilling: the four leading scalars in the same launch -- kd sits in _scal[3], and _scal[1:3] (L2, L1) are still zero here
            # (_opt writes them after the last fold)
            ops.accum_fold(self._acc[nP:], self._scal if self.teacher is not None else self.loss, None, 4 if self.teacher is not None else 1,
                           False, last, 1.0 / self.accum_steps)
            if not last:
                ops.add_i64(mgr.step_counter, 1)   # every micro-batch draws its own dropout masks (the last one's advance is in _opt)

    def _stat_base(self):
        """buffer of S at the start of the step (guarded step, accum_steps == 1; accumulate() owns it for accumulated steps)"""
        mgr = self.mgr
        if self._sbase is None or self._sbase_version != mgr.version:
            self._sbase = torch.empty(mgr.nS, dtype=torch.float32, device=mgr.P.device)
            self._sbase_version = mgr.version
        return self._sbase

    def _opt(self):
        """[gradients summed over ranks] -> + world * rho * penalty * sign(gamma) -> [guarded step: verdict on G] -> the optimizer's
        fused launch (RMSprop or SGD) on g / world + wd * p (+ EMA of the parameters, L2 value) -> L1 value -> [guarded step: S back to
        its base after a dropped step] -> EMA of the BN statistics."""
        mgr = self.mgr
        rho_ptr = mgr.hyper[ops.HYP_RHO:ops.HYP_RHO + 1]
        if self._l1 is not None:
            table, njobs = self._l1
            ops.reg_value(mgr.P, table, njobs, 1, rho_ptr, 1.0, self.loss[2:3], ws=self._ws[4096:])
            ops.reg_grad(mgr.P, mgr.G, table, njobs, 1, rho_ptr, mgr.hyper[HYP_SUMMED_RANKS:HYP_SUMMED_RANKS + 1])
        ema_arena = mgr.EMA if self.ema is not None else None
        if not self.guarded:
            self.optimizer.launch_fused(mgr, ema_arena, self._wd_chunk, self.loss[1:2], self._ws)
            if self.ema is not None:
                ops.ema_update(mgr.SEMA, mgr.S, mgr.nS, mgr.hyper)
        else:
            # The verdict reads G only, here: after every collective and fold, with the L1 term in.  It never reads the per-rank loss.  G
            # is bit-identical on every rank after the all-reduce and the two launches sum in a fixed order without atomics, so every
            # rank reaches the same verdict, scale and counters without a collective of its own (step(reduce=False) runs on one rank).
            ops.grad_guard(mgr.G, mgr.nP, mgr.hyper, self.clip_norm or 0.0, self.skip_nonfinite, self._guard, self._guard_ws)
            self.optimizer.launch_fused(mgr, ema_arena, self._wd_chunk, self.loss[1:2], self._ws, guard=self._guard)
            ops.guard_restore(mgr.S, self._sbase, mgr.nS, self._guard, False)
            if self.ema is not None:
                ops.ema_update_guarded(mgr.SEMA, mgr.S, mgr.nS, mgr.hyper, self._guard)
        ops.add_i64(mgr.step_counter, 1)

    def guard_state(self):
        """Verdict of the last guarded step and the cumulative counters, as dict(norm=, coef=, ok=, skipped=, clipped=): norm is the
        global L2 norm of the averaged gradient the optimizer consumed, before clipping (may be inf / nan), coef the clip coefficient.
        Synchronises with the device when called; step() never does."""
        if not self.guarded:
            raise RuntimeError("guard_state(): this TrainStep was built without clip_norm and without skip_nonfinite")
        f = self._guard.tolist()
        c = self._guard.view(torch.int32).tolist()
        return dict(norm=f[ops.GUARD_NORM], coef=f[ops.GUARD_COEF], ok=f[ops.GUARD_OK] != 0.0, skipped=c[ops.GUARD_SKIPPED],
                    clipped=c[ops.GUARD_CLIPPED])

    def _capture(self, want_overlapped=False, accum=False):
        """accum: the graphs of an accumulated step instead (a micro-batch, the last micro-batch, the last one with its in-graph
        collectives; they share one private pool, as no two of them ever run at the same time) -- the optimizer graph is the same.
        Captures what is missing: the one-graph form with the in-graph collectives (want_overlapped, comm mode "graph") and / or
        the forward-backward + optimizer pair that runs without a collective or around a blocking one.  Graphs that exist are kept:
        a step(reduce=False) between reducing steps must not drop the overlapped graph."""
        mgr = self.mgr
        mgr.ensure()
        self._tables()
        # warm-up outside capture (allocator pools, lazy initialisation); it must not leave a trace in the training state:
        # BN running statistics / counters are snapshotted and restored, gradients are re-zeroed by the step itself
        keep_s, keep_c = mgr.S.clone(), mgr.CNT.clone()
        keep_scal = self._scal.clone() if accum else None   # a group may be under way: its hit counts live there
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._fwd_bwd()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        mgr.S.copy_(keep_s)
        mgr.CNT.copy_(keep_c)
        if accum:
            self._scal.copy_(keep_scal)
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
        g_over = "g_all_last" if accum else "g_all"
        pool = dict(pool=self._pool) if accum else {}
        # thread_local: the RCCL watchdog thread of a process group polls events while we capture; in the default "global" mode
        # such a call from another thread invalidates the capture
        if want_overlapped and self.comm_mode == "graph" and getattr(self, g_over) is None:
            # one graph: kernels, bucketed RCCL all-reduces on the side stream, optimizer tail
            ok = True
            try:
                # one real collective on the side stream first: communicator set-up / lazy connections must not happen inside capture
                self._comm.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self._comm):
                    dist.all_reduce(self._agree, group=self.pg)
                torch.cuda.current_stream().wait_stream(self._comm)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local", **pool):
                    self._fwd_bwd_overlapped(True if accum else None)
                    self._opt()
                setattr(self, g_over, g)
            except Exception as e:   # a runtime that cannot capture the collective: fall back to the blocking form
                import logging
                logging.warning("capturing the gradient all-reduce failed (%s); using one blocking all-reduce between two graphs", e)
                torch.cuda.synchronize()
                ok = False
            # The mode is a property of the JOB: a rank that replays N bucketed collectives next to a rank that issues one whole-arena
            # collective hangs or corrupts gradients.  Every rank reports, and one failure switches all of them to the blocking form.
            self._agree.fill_(1.0 if ok else 0.0)
            dist.all_reduce(self._agree, op=dist.ReduceOp.MIN, group=self.pg)
            if float(self._agree.item()) < 0.5:
                self.comm_mode = "host"
                self.g_all = self.g_all_last = None
        if accum:
            if self.g_mb is None:
                self.g_mb = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.g_mb, capture_error_mode="thread_local", **pool):
                    self._fwd_bwd(False)
            if self.g_last is None and not (want_overlapped and self.g_all_last is not None):
                self.g_last = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.g_last, capture_error_mode="thread_local", **pool):
                    self._fwd_bwd(True)
                if self.g_opt is None:
                    self.g_opt = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.g_opt, capture_error_mode="thread_local", **pool):
                        self._opt()
        elif self.g_fwd_bwd is None and not (want_overlapped and self.g_all is not None):
            self.g_fwd_bwd = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_fwd_bwd, capture_error_mode="thread_local"):
                self._fwd_bwd()
            self.g_opt = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_opt, capture_error_mode="thread_local"):
                self._opt()
        self._version = mgr.version

    # ---- public
    def set_batch(self, x, y):
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)

    def _wants_reduce(self):
        # the collective can be forced on a single rank to exercise RCCL next to graph replay on a one-GPU box
        return self.world_size > 1 or (bool(os.environ.get("ATOMNAS_FORCE_ALLREDUCE")) and dist.is_initialized())

    def _sync_arenas(self):
        """follows an arena rebuild (a shrink): graphs and buckets of the old arenas are dropped"""
        mgr = self.mgr
        if mgr.dirty or self._version != mgr.version:
            mgr.ensure()
            self.g_fwd_bwd = self.g_opt = self.g_all = None
            self.g_mb = self.g_last = self.g_all_last = None
            self._buckets = []

    # ---- gradient accumulation
    @property
    def pending(self):
        """micro-batches accumulated since the last step() / reset_accumulation()"""
        return self._pending

    def _check_group(self):
        if self._pending and (self.mgr.dirty or self.mgr.version != self._group_version):
            raise RuntimeError("the arenas were rebuilt (a shrink?) inside a group of accumulated micro-batches: the running sums belong "
                               "to the old layout.  Shrink between optimizer steps, or call reset_accumulation() and start the group again")

    def reset_accumulation(self):
        """discards a partial group: the next accumulate() starts from zero.  The running statistics are already back at their values
        of the start of the step (every fold leaves them there); the dropout counter steps back to where the group began (also across an
        arena rebuild: the counter survives one, runtime.ArenaManager._bind)."""
        if self._pending:
            ops.add_i64(self.mgr.step_counter, -self._pending)
        self._pending = 0

    def accumulate(self):
        """Forward and backward of the current static batch into the running sums of an accumulated step (accum_steps > 1); the
        first call after a step() or reset_accumulation() starts them from zero.  The last micro-batch of a group belongs to step()."""
        mgr = self.mgr
        A = self.accum_steps
        if self._pending >= A - 1:
            raise RuntimeError("accumulate() with %d of %d micro-batches pending: the last micro-batch of a group belongs to step()"
                               % (self._pending, A))
        self._check_group()
        if self._pending == 0:
            self._sync_arenas()
            if self._acc_version != mgr.version:   # the sums follow the arenas' layout
                f32 = dict(dtype=torch.float32, device=mgr.P.device)
                self._acc = torch.empty(mgr.nP + runtime.ALIGN, **f32)
                self._sacc, self._sbase = torch.empty(mgr.nS, **f32), torch.empty(mgr.nS, **f32)
                self._acc_version = mgr.version
            self._group_version = mgr.version
            # outside the graphs: two memsets and the snapshot of the statistics every micro-batch of this step starts from
            self._acc.zero_()
            self._scal.zero_()
            self._sbase.copy_(mgr.S)
        if self.use_graph:
            if self.g_mb is None:
                self._tables()
                self._capture(accum=True)
            self.g_mb.replay()
        else:
            self._fwd_bwd(False)
        self._fold_stats(self._pending == 0, False, False)
        self._pending += 1

    def _last_micro_batch(self, do_reduce, overlapped):
        """step() of an accumulated group: the last micro-batch, the collective over the real ranks, the optimizer tail"""
        mgr = self.mgr
        if self.use_graph:
            if overlapped and self.g_all_last is None:
                self._capture(want_overlapped=True, accum=True)   # may agree on "host" over the ranks
                overlapped = do_reduce and self.comm_mode == "graph"
            if overlapped and self.g_all_last is not None:
                self.g_all_last.replay()
                return
            if self.g_last is None or self.g_opt is None:
                self._capture(accum=True)
            self.g_last.replay()
        elif overlapped:
            self._fwd_bwd_overlapped(True)
            self._opt()
            return
        else:
            self._fwd_bwd(True)
        self._fold_stats(False, True, do_reduce)
        if do_reduce:
            dist.all_reduce(mgr.G, group=self.pg)
            if self.allreduce_bn:
                self._reduce_bn()
        if self.use_graph:
            self.g_opt.replay()
        else:
            self._opt()

    def step(self, lr=None, rho=0.0, ema_decay=None, reduce=None):
        """One iteration on the current static batch.  lr defaults to the optimizer's group lr.  reduce: None = all-reduce the
        gradient arena when world_size > 1; False = never (bench.py's single-rank profiling pass: the other ranks wait at a
        barrier, so no collective may be issued).  A guarded step that is dropped on the device still advances everything the host
        keeps (global_step, the EMA warm-up count) and the device counters; see __init__."""
        do_reduce, overlapped = self._step_begin(lr, rho, ema_decay, reduce)
        if self.accum_steps > 1:
            self._last_micro_batch(do_reduce, overlapped)
        else:
            if overlapped and self.use_graph and self.g_all is None:
                self._capture(want_overlapped=True)   # may agree on "host" over the ranks
                overlapped = do_reduce and self.comm_mode == "graph"
            if overlapped and self.use_graph and self.g_all is not None:
                self.g_all.replay()
            elif overlapped and not self.use_graph:
                self._fwd_bwd_overlapped()
                self._opt()
            else:   # the step has a seam: two halves around the blocking collective (or around nothing)
                self._half_fwd_bwd()
                self._half_reduce(do_reduce)
                self._half_opt()
        self._step_end()

    def _half_fwd_bwd(self):
        if self.use_graph:
            if self.g_fwd_bwd is None:
                self._capture()
            self.g_fwd_bwd.replay()
        else:
            self._fwd_bwd()

    def _half_reduce(self, do_reduce):
        if do_reduce:
            dist.all_reduce(self.mgr.G, group=self.pg)
            if self.allreduce_bn:
                self._reduce_bn()

    def _half_opt(self):
        if self.use_graph:
            self.g_opt.replay()
        else:
            self._opt()

    def _step_begin(self, lr, rho, ema_decay, reduce):
        """host side of a step before its launches: checks, comm mode, the per-step scalars -> (do_reduce, overlapped)"""
        mgr = self.mgr
        A = self.accum_steps
        if self._pending != A - 1:
            raise RuntimeError("step() runs the last of %d micro-batches: %d accumulate() calls must come first, %d were made"
                               % (A, A - 1, self._pending))
        self._check_group()
        do_reduce = self._wants_reduce() if reduce is None else bool(reduce)
        self._sync_arenas()
        if do_reduce and self.comm_mode is None:
            backend = dist.get_backend(self.pg) if dist.is_initialized() else None
            # ATOMNAS_OVERLAP_ALLREDUCE: "0" never, "force" with any backend (tests drive the bucketed path eagerly with gloo ranks)
            env = os.environ.get("ATOMNAS_OVERLAP_ALLREDUCE", "1")
            overlap_ok = env == "force" or (backend == "nccl" and env != "0")
            self.comm_mode = "graph" if overlap_ok else "host"
        if do_reduce and self.comm_mode == "graph" and not self._buckets:
            self._comm = self._comm or torch.cuda.Stream()
            self._build_buckets()
        h = mgr.hyper_host
        self._tables()
        h[ops.HYP_LR] = float(self.optimizer.param_groups[0]['lr'] if lr is None else lr)
        h[ops.HYP_RHO] = float(rho)
        # the scales follow what THIS step does: a step without the collective (bench.py's single-rank profile pass) trains on its own
        # gradients, not on gradients shrunk by 1 / world
        eff_world = (float(max(self.world_size, 1)) if do_reduce else 1.0) * A   # micro-batches count as ranks
        h[ops.HYP_GRAD_SCALE] = 1.0 / eff_world
        h[HYP_SUMMED_RANKS] = eff_world
        if self.ema is not None:
            h[ops.HYP_EMA_DECAY] = float(self.ema.momentum_at(self.global_step + 1) if ema_decay is None else ema_decay)
        else:
            h[ops.HYP_EMA_DECAY] = -1.0
        mgr.push_hyper()
        return do_reduce, do_reduce and self.comm_mode == "graph"

    def _step_end(self):
        """host bookkeeping after the launches of a step (a step dropped by the guard advances it too)"""
        h = self.mgr.hyper_host
        # optimizer / regulariser launches outside TrainStep (RMSprop.step(), cal_bn_l1_loss) read the same vector: leave the neutral
        # scales behind (host copy only: the device vector is re-staged by whoever launches next)
        h[ops.HYP_GRAD_SCALE] = 1.0
        h[HYP_SUMMED_RANKS] = 1.0
        self._pending = 0
        self.global_step += 1
        if self.ema is not None:   # bookkeeping the reference keeps per variable (utils/optim.py:62-63); checkpointed
            self.ema.note_updates(1, float(h[ops.HYP_EMA_DECAY]))
