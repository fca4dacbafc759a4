"""Inference path: a searched network or supernet in eval mode with every atomic block that qualifies run as ONE kernel launch.

The training decomposition of a block (functional.block_forward) writes the 6x-wide hidden maps to HBM between its GEMMs and
re-derives the BatchNorm coefficients on every call, because the backward pass and the batch statistics need them.  In evaluation
neither exists: compile_for_inference folds the three BatchNorms of a block into scale / shift vectors ONCE, snapshots the packed
weights, and runs the block through atomnas_block_infer (csrc/block_infer.hip), which keeps the hidden maps on chip.  A block with
Squeeze-and-Excitation goes through atomnas_block_infer_se where one workgroup owns its whole map (stride 1, at most 256 pixels,
expanding): there the squeeze is a reduction inside the workgroup.  Everything else -- the stem, the other SE blocks, shapes outside
the kernel's envelope, the fused tail -- runs the existing HIP path unchanged.  Opt-in: nothing calls this module unless asked to
(`fused_inference` in the yaml / CLI, tools/infer_bench.py).

    net = compile_for_inference(model.eval())          # model: a _HipModel on the GPU, bf16 compute dtype
    logits = net(images)
    net.refresh()                                       # after weights or running statistics changed

The snapshot does NOT follow in-place updates of the fused blocks' weights or BatchNorm statistics: call refresh().  Modules on the
fallback path read the live parameters, as they always did.
"""
import functools

import torch
from torch import nn

from . import functional as AF
from . import ops, runtime


# Which blocks leave the existing path: "measured" -- those the kernel runs AND measured faster for (atomnas_block_infer_supported,
# atomnas_block_infer_se_supported), the default; "all" -- every block the kernel can run (atomnas_block_infer_runs / _se_runs): tests and
# tools/infer_bench.py, which have to run the kernel on the shapes the measured policy keeps away from it.  Read when a model is
# compiled / refreshed.
POLICY = "measured"


def block_shape(pl, act):
    """The shape of a block from its plan, the ONE derivation: the keyword arguments of ops.block_infer_supported /
    block_infer_se_supported behind N, H, W.  Integer arithmetic on the plan's scalar fields: an arena layout's plan will do (its
    activation code comes from the layout's info, a bound plan carries its own)."""
    return dict(inp=pl.inp, oup=pl.oup, seg_off=list(pl.seg), seg_ch=[pl.segpad(h) for h in pl.hid], seg_k=list(pl.ks), stride=pl.stride,
                act=int(act), expand=bool(pl.expand), residual=bool(pl.res), se=bool(pl.se), se_hid=int(pl.se_hid) if pl.se else 0)


def walk_maps(blocks, plan_for, size):
    """(name, module, plan_for(module), H, W) for every (name, module) of `blocks`, H x W the map the block sees: a square of side
    `size` carried through the strides, the ONE walk.  A block without a plan or with every branch pruned (the identity) leaves it as it is."""
    H = W = size
    for name, m in blocks:
        pl = plan_for(m)
        yield name, m, pl, H, W
        if pl is not None and pl.nb:
            H, W = (H - 1) // pl.stride + 1, (W - 1) // pl.stride + 1


class FusedBlock:
    """Snapshot of one block for atomnas_block_infer / atomnas_block_infer_se: its shape (block_shape), packed bf16 weights, fp32 taps,
    folded BatchNorm coefficients and, with Squeeze-and-Excitation, the gate's packed fp32 dense layers."""

    def __init__(self, name, module):
        self.name, self.module = name, module
        self.snapshot()

    def snapshot(self):
        self.pl = pl = runtime.plan_of(self.module)
        dev = pl.Wp_pack.device
        self.shape = block_shape(pl, pl.act)
        self.se, self.se_hid = self.shape["se"], self.shape["se_hid"]
        self.we = pl.We_pack.clone() if pl.expand else None
        self.wp = pl.Wp_pack.clone()
        self.taps = [t.clone() for t in pl.taps]
        be = AF.bn_forward_coeffs(pl.bne, None, 0, dev) if pl.expand else None
        bd, bp = AF.bn_forward_coeffs(pl.bnd, None, 0, dev), AF.bn_forward_coeffs(pl.bnp, None, 0, dev)
        self.coeffs = (be.scale if be else None, be.shift if be else None, bd.scale, bd.shift, bp.scale, bp.shift)
        self.se_tensors = [t.clone() for t in (pl.se_w1p, pl.se_w2t, pl.se_b1, pl.se_b2p)] if self.se else []

    def tensors(self):
        """every snapshot tensor (None where the block has none), in a fixed order: what _rewrite copies in place"""
        return [self.we, self.wp] + self.taps + list(self.coeffs) + self.se_tensors

    def supported(self, N, H, W, profitable=None):
        fn = ops.block_infer_se_supported if self.se else ops.block_infer_supported
        return fn(N=N, H=H, W=W, dtype=torch.bfloat16, profitable=POLICY != "all" if profitable is None else profitable, **self.shape)

    def __call__(self, x):
        x2d, (N, H, W, C) = AF.to_2d(x, torch.bfloat16)
        sh = self.shape
        if C != sh["inp"]:
            raise ValueError("block %s expects %d input channels, got %d" % (self.name, sh["inp"], C))
        s = sh["stride"]
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        out = torch.empty(N * Ho * Wo, sh["oup"], dtype=torch.bfloat16, device=x.device)
        ops.block_infer(x2d, out, self.we, self.wp, self.taps, *self.coeffs, N, H, W, sh["inp"], sh["oup"], sh["seg_off"], sh["seg_ch"], sh["seg_k"],
                        s, sh["act"], sh["expand"], sh["residual"], *self.se_tensors, se_hid=self.se_hid)
        return AF.to_4d(out, N, Ho, Wo, sh["oup"])


def block_shapes(model, batch_size=1, input_size=None):
    """[(block name, shape dict)] for every atomic block of `model` at its input resolution: the arguments of
    ops.block_infer_supported, from the arena layout alone (integer arithmetic on module attributes: works on a CPU model, no library
    call).  Blocks whose branches are all pruned are skipped."""
    lay = runtime.arena_layout(model, getattr(model, "compute_dtype", torch.bfloat16))
    plans = {id(m): pl for m, pl, _ in lay.plans if isinstance(pl, runtime.BlockPlan)}
    acts = {id(m): AF.act_code(info["act"]) for m, _, info in lay.plans if id(m) in plans}
    size = input_size or getattr(model, "input_size", 224)
    walk = walk_maps(list(model.features.named_children())[1:-2], lambda m: plans.get(id(m)), (size - 1) // 2 + 1)   # behind the stride-2 stem
    return [(name, dict(N=batch_size, H=H, W=W, **block_shape(pl, acts[id(m)]))) for name, m, pl, H, W in walk if pl is not None and pl.nb]


def fallback_reason(pl, supported=None):
    """Why a block stays on the existing path, None when nothing keeps it from the fused kernel.  pl: its bound plan (None: the module
    is no atomic block); supported: the block's predicates at the batch and map in question, FusedBlock.supported with N, H, W bound --
    without it only what the plan alone decides is looked at (a block that fails there has no snapshot to ask)."""
    if pl is None:
        return "not an atomic block"
    if pl.nb == 0:
        return "all branches pruned: the block is the identity"
    if pl.se and pl.se_act != pl.act:
        return "squeeze-and-excitation with an activation of its own (the fused kernel applies the block's inside the gate)"
    if supported is None or supported():
        return None
    if not supported(profitable=False):
        if pl.se:
            return ("squeeze-and-excitation is fused only where one workgroup owns the whole map (stride 1, expanding, <= 256 pixels): "
                    "the squeeze needs it (atomnas_block_infer_se_runs)")
        return "outside the kernel's envelope (atomnas_block_infer_runs)"
    if pl.se:
        return ("squeeze-and-excitation: the two-pass kernel did not measure faster than the existing path for shapes of this kind "
                "(atomnas_block_infer_se_supported)")
    return "measured slower than the existing path for shapes of this kind (atomnas_block_infer_supported)"


class InferenceModel(nn.Module):
    """Eval-mode forward of a _HipModel with one fused launch per qualifying block (compile_for_inference)."""

    def __init__(self, model, use_graph=False, batch_size=None):
        super().__init__()
        from .models.mobilenet_base import InvertedResidualChannels, InvertedResidualChannelsFused
        self._block_types = (InvertedResidualChannels, InvertedResidualChannelsFused)
        self._bare = isinstance(model, self._block_types)   # a block on its own (unit tests, block benchmarks): no stem, no tail
        if not self._bare and not (hasattr(model, "features") and hasattr(model, "classifier") and hasattr(model, "compute_dtype")):
            raise TypeError("compile_for_inference takes a supernet or searched network of atomnas_amd.models (or one atomic block), got %s"
                            % type(model).__name__)
        if model.training or any(m.training for m in model.modules() if isinstance(m, nn.BatchNorm2d)):
            raise ValueError("compile_for_inference needs the model in eval() mode: the BatchNorms are folded into constants")
        if getattr(model, "compute_dtype", torch.bfloat16) != torch.bfloat16:
            raise ValueError("the fused inference kernel stores bf16 activations: the model's compute dtype is %s (set_compute_dtype(torch.bfloat16))"
                             % model.compute_dtype)
        if use_graph and (not batch_size or self._bare):
            raise ValueError("use_graph=True captures a whole network over a static input buffer: pass batch_size")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise ops._lib.AtomnasHipError("compile_for_inference runs on the GPU only: the model is on %s (model.cuda())" % dev)
        object.__setattr__(self, "model", model)   # not a submodule: the compiled model owns no parameters
        self.batch_size = batch_size
        self._graph = self._static_in = self._static_out = None
        self.refresh()
        if use_graph:
            self._capture(dev)

    # ------------------------------------------------------------------ snapshot
    def refresh(self):
        """Re-snapshots weights and BatchNorm coefficients of the fused blocks (after an optimizer step, a checkpoint load, a BatchNorm
        calibration ...).  A captured graph keeps replaying: the snapshot tensors are rewritten in place."""
        model = self.model
        mgr = runtime.manager_of(model)
        mgr.ensure()
        mgr.pack()
        old = {fb.name: fb for fb in getattr(self, "_fused", {}).values()}
        self._fused, self._plan = {}, []
        plan_for = lambda m: runtime.plan_of(m) if isinstance(m, self._block_types) else None
        size = 14 if self._bare else (getattr(model, "input_size", 224) - 1) // 2 + 1   # behind the stride-2 stem; a bare block: a nominal map, every call re-checks
        for name, m, pl, H, W in walk_maps(self._blocks(), plan_for, size):
            why = fallback_reason(pl)
            if why is None:
                fb = old.get(name)
                if fb is not None and self._graph is not None:
                    self._rewrite(fb)
                else:
                    fb = FusedBlock(name, m)
                why = fallback_reason(pl, functools.partial(fb.supported, self.batch_size or 1, H, W))
                if why is None:
                    self._fused[id(m)] = fb
            self._plan.append((name, "fallback", why) if why else (name, "fused", ""))
        self._ok = {}

    @staticmethod
    def _rewrite(fb):
        """new values into the tensors a captured graph points at"""
        new = FusedBlock(fb.name, fb.module)
        for dst, src in zip(fb.tensors(), new.tensors()):
            if dst is not None:
                dst.copy_(src)

    def _blocks(self):
        if self._bare:
            return [(getattr(runtime.plan_of(self.model), "name", "") or "block", self.model)]
        return list(self.model.features.named_children())[1:-2]

    def plan(self):
        """[(block name, 'fused' | 'fallback', reason)] at the model's input size"""
        return list(self._plan)

    def block_steps(self):
        """[(name, module, fused runner or None)] in forward order: what tools/infer_bench.py times block by block"""
        return [(name, m, self._fused.get(id(m))) for name, m in self._blocks()]

    # ------------------------------------------------------------------ forward
    def _block(self, blk, y):
        fb = self._fused.get(id(blk))
        if fb is not None:
            key = (id(blk),) + tuple(y.shape)
            ok = self._ok.get(key)
            if ok is None:
                why = fallback_reason(fb.pl, functools.partial(fb.supported, y.shape[0], y.shape[2], y.shape[3]))
                ok = self._ok[key] = why is None
                if self._bare:   # a block on its own was planned at a nominal map: its plan follows the map it is called with
                    self._plan = [(fb.name, "fallback", why) if why else (fb.name, "fused", "")]
            if ok:
                return fb(y)
        return blk(y)   # the existing path: SE blocks, shapes outside the envelope

    def _eager(self, x):
        model = self.model
        mgr = runtime.manager_of(model)
        mgr.enter()
        try:
            if self._bare:
                return self._block(model, x)
            feats = list(model.features.children())
            y = feats[0](x)
            for blk in feats[1:-2]:
                y = self._block(blk, y)
            last = feats[-2]
            drop, fc = list(model.classifier.children())
            return AF.run_tail(runtime.plan_of(last), runtime.plan_of(fc), y, mgr.anchor, drop.p, False, model.dropout_seed, mgr.step_counter)
        finally:
            mgr.leave()

    def _capture(self, dev):
        """one linear, single-stream hipGraph over a static input buffer (engine.TrainStep's pattern: warm up on a side stream, capture)"""
        size = getattr(self.model, "input_size", 224)
        self._static_in = torch.zeros(self.batch_size, 3, size, size, dtype=torch.float32, device=dev)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(2):
                self._eager(self._static_in)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._static_out = self._eager(self._static_in)
        self._graph = g

    def forward(self, x):
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("InferenceModel is forward-only (the hidden maps a backward pass needs are never stored): "
                               "call it on an input that does not require gradients")
        if not x.is_cuda:
            raise ops._lib.AtomnasHipError("InferenceModel runs on the GPU only (input is on %s)" % x.device)
        if self.model.training:
            raise RuntimeError("the compiled model was put back into training mode: call model.eval() (and refresh() if it was trained)")
        with torch.no_grad():
            if self._graph is not None and tuple(x.shape) == tuple(self._static_in.shape):
                self._static_in.copy_(x)
                self._graph.replay()
                return self._static_out.clone()
            return self._eager(x)


def compile_for_inference(model, use_graph=False, batch_size=None):
    """-> InferenceModel for `model` (a supernet or searched network in eval() mode, bf16 compute dtype, on the GPU).  use_graph: replay
    one captured hipGraph for inputs of [batch_size, 3, input_size, input_size]; other shapes run eagerly."""
    return InferenceModel(model, use_graph=use_graph, batch_size=batch_size)
