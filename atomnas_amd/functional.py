"""Forward / backward executors of the hot path: sequences of C-ABI kernel launches over arena views, wrapped in
torch.autograd.Function so that the reference's `loss.backward()` drives them.

Activations cross module boundaries as ordinary torch tensors of logical shape [N, C, H, W] in channels_last memory
format (i.e. NHWC in HBM) and the model's compute dtype; inside a block the 6x-expanded tensors are [M, HT] buffers.
Parameter gradients are written straight into the gradient arena (p.grad views) instead of being returned to autograd.

Reference call sites: InvertedResidualChannels.forward (models/mobilenet_base.py:371-382), ConvBNReLU (:120-142),
MobileNetV2.forward (models/mobilenet_supernet.py:169-173), CrossEntropyLabelSmooth.forward (utils/optim.py:199-207).
"""
import os

import torch
from torch import nn

from . import ops
from .ops import PRO_BNBWD, PRO_BNRELU, PRO_NONE, STAT_SQ, STAT_Z
from .ops import Slab
from .runtime import pad8, pads

ACT_NONE, ACT_RELU, ACT_RELU6, ACT_SWISH = 0, 1, 2, 3   # the integer `relu` / `mask` arguments of the C ABI


def act_code(module):
    """Maps the activation module a ConvBNReLU holds to the kernels' activation flag."""
    if module is None:
        return ACT_NONE
    if isinstance(module, nn.ReLU6):
        return ACT_RELU6
    if isinstance(module, nn.ReLU):
        return ACT_RELU
    if type(module).__name__ == "Swish":   # models/mobilenet_base.py:72-80
        return ACT_SWISH
    raise NotImplementedError("activation %s is not supported by the HIP path (ReLU / ReLU6 / Swish)" % type(module).__name__)


# ---------------------------------------------------------------------------------------------- layout plumbing
def to_2d(x, dtype):
    """[N,C,H,W] tensor -> ([M, C] NHWC view/copy in `dtype`, (N, H, W, C))."""
    if x.dim() != 4:
        raise ValueError("expected a 4-D activation, got shape %s" % (tuple(x.shape),))
    if not x.is_cuda:
        raise ops._lib.AtomnasHipError("atomnas_amd runs on the GPU only: input tensor is on %s" % x.device)
    N, C, H, W = x.shape
    if C % 8 != 0:
        raise ValueError("block input channels must be a multiple of 8, got %d" % C)
    if x.dtype != dtype:
        x = x.to(dtype)
    x = x.contiguous(memory_format=torch.channels_last)
    return x.permute(0, 2, 3, 1).reshape(N * H * W, C), (N, H, W, C)


def to_4d(y2d, N, H, W, C):
    return y2d.view(N, H, W, C).permute(0, 3, 1, 2)


def _f32(n, dev, zero=False):
    t = torch.empty(n, dtype=torch.float32, device=dev)
    return ops.zero_(t) if zero else t


class StatBuf:
    """Partial-row statistics buffer [rows][2][c] (include/atomnas_hip.h): every producer writes all rows of its channel range
    with plain stores, the BatchNorm finalize sums them in a fixed order -- no initialisation, no atomics."""
    __slots__ = ("t", "rows", "c")

    def __init__(self, t, rows, c):
        self.t, self.rows, self.c = t, rows, c

    def at(self, off):
        """buffer pointer advanced to channel `off` (a branch segment of a fused hidden tensor)"""
        return self.t[off:] if off else self.t


def _stats(c, dev, mgr=None):
    """Uninitialised StatBuf for c channels.  With a manager it is a slice of the per-step statistics workspace."""
    rows = ops.stat_rows_for(c)
    n = rows * 2 * c
    if mgr is not None:
        v = mgr.take_stats(n)
        if v is not None:
            return StatBuf(v, rows, c)
    return StatBuf(torch.empty(n, dtype=torch.float32, device=dev), rows, c)


# ---------------------------------------------------------------------------------------------- batch norm helpers
class BNState:
    """Per-call coefficients of one (possibly branch-fused) BatchNorm: scale/shift for the apply, mean/invstd for backward."""
    __slots__ = ("scale", "shift", "mean", "invstd")


def bn_forward_coeffs(bn, stats, count, dev):
    """bn: dict of arena views (gamma, beta, rm, rv, C, mods).  Uses batch statistics when the BN modules are in training
    mode (updating running statistics with their momentum; momentum None = cumulative average), running statistics otherwise."""
    C = bn["C"]
    cmap = bn.get("cmap")   # fused block: contiguous [total] parameter vectors against the padded-segment kernel layout (runtime.py)
    Ck = bn["Cpad"] if cmap is not None else C   # channels of the kernel layout: one launch covers them, padding gets zeros
    Cp = pad8(Ck)
    st = BNState()
    st.scale, st.shift = _f32(Cp, dev), _f32(Cp, dev)
    mod = bn["mods"][0]
    eps = mod.eps
    if mod.training or not mod.track_running_stats:
        st.mean, st.invstd = _f32(Cp, dev), _f32(Cp, dev)
        track = mod.track_running_stats
        ops.bn_finalize_fwd(stats.t, count, bn["gamma"], bn["beta"], eps, mod.momentum, bn["rm"] if track else None,
                            bn["rv"] if track else None, mod.num_batches_tracked if track else None, st.scale, st.shift, st.mean,
                            st.invstd, Ck, stat_rows=stats.rows, stat_ld=stats.c, cmap=cmap)
        if track:
            bn["mgr"].bn_trained = True
    else:
        st.mean = st.invstd = None
        ops.bn_eval_coeffs(bn["gamma"], bn["beta"], bn["rm"], bn["rv"], eps, st.scale, st.shift, Ck, cmap=cmap)
    return st


def bn_uses_batch_stats(bn):
    mod = bn["mods"][0]
    return mod.training or not mod.track_running_stats


def bn_backward_coeffs(bn, st, stats2, count, dev):
    """-> (c1, c2, c3) with dx = c1*g + c2*x + c3; writes dgamma / dbeta into the gradient arena."""
    C = bn["C"]
    cmap = bn.get("cmap")
    Ck = bn["Cpad"] if cmap is not None else C
    Cp = pad8(Ck)
    c1, c2, c3 = _f32(Cp, dev), _f32(Cp, dev), _f32(Cp, dev)
    if st.mean is None:
        raise RuntimeError("backward through a BatchNorm in eval mode is not supported")
    ops.bn_finalize_bwd(stats2.t, count, bn["gamma"], st.mean, st.invstd, None, None, bn["dgamma"], bn["dbeta"], c1, c2, c3, Ck,
                        stat_rows=stats2.rows, stat_ld=stats2.c, cmap=cmap)
    return c1, c2, c3


# ---------------------------------------------------------------------------------------------- atomic block
# fused block (AtomNAS+): one weight-gradient GEMM per layer into a padded scratch + fold jobs (0: one GEMM per kernel-size segment)
_FUSED_WG_BATCH = bool(int(os.environ.get("ATOMNAS_FUSED_WG_BATCH", "1")))
_CHECK_LOSS_SEED = bool(int(os.environ.get("ATOMNAS_CHECK_LOSS_SEED", "0")))   # experiment switch (same-box A/B of the two layouts)
# widest block output that takes the fused projection backward.  The library covers oup <= 96, but the 80/96-wide instances hold 223 VGPR +
# 96 AGPR (one wave per SIMD) and measured slower than the two-GEMM form on the 14x14 stages: 36.53 vs 36.30 ms/step (r03, bs256 bf16)
PROJECT_BWD_FUSED_MAX_OUP = 48
# widest block input that takes the expand backward without the raw expand output E (csrc/xbwd.hip; atomnas_gram itself serves
# inp <= 64).  48 = stages 1-3 with the streaming kernel k_expand_bwd_s (same-box A/Bs: 31.15 -> 30.20 ms for inp <= 24, -> 30.11 with
# the per-segment launches of 40 -> 720; the 31.41 of profiles/r04_expand_bwd_noe_ab.txt for 48 predates that kernel)
EXPAND_BWD_NOE_MAX_INP = 48
DROP_CONNECT_SEED = 1995   # stochastic depth of a block used on its own (no enclosing model with a `dropout_seed`): the models' default seed
TAIL_TAP = None   # set to a list by tests to receive the dropout keep mask of every tail forward
# set to a list by tests to receive, for every activation the forward applies, (kind, plan, raw tensor, scale, shift): the pre-activation
# is raw * scale + shift per channel -- what a test needs to compare ReLU masks with the oracle's (tests/test_block_gpu.py)
ACT_TAP = None


def _tap(kind, pl, raw, st):
    if ACT_TAP is not None and st is not None:
        ACT_TAP.append((kind, pl, raw, st.scale, st.shift))


# set to a list by tests to receive (name, tensor) for every intermediate an executor produces in a step: activations, gradients,
# BatchNorm coefficients ("<plan>.<bn>.invstd" etc.) -- tests/test_bench_shapes_gpu.py checks them for finiteness at the bench's sizes
STEP_TAP = None


def _stap(pl, **tensors):
    if STEP_TAP is not None:
        for what, t in tensors.items():
            if t is None:
                continue
            if isinstance(t, BNState):
                for f in ("scale", "shift", "mean", "invstd"):
                    if getattr(t, f) is not None:
                        STEP_TAP.append(("%s.%s.%s" % (pl.name, what, f), getattr(t, f)))
            elif isinstance(t, (tuple, list)):
                for q, u in enumerate(t):
                    STEP_TAP.append(("%s.%s%d" % (pl.name, what, q + 1), u))
            else:
                STEP_TAP.append(("%s.%s" % (pl.name, what), t))


def _hidden(pl, M, C, T, dev):
    """hidden tensor of a block: slab-major (ops.Slab) for expanding blocks, plain [M, C] for the narrow non-expanding one"""
    return Slab(M, C, T, dev) if pl.expand else torch.empty(M, C, dtype=T, device=dev)


def _seg(t, o):
    return t.seg(o) if isinstance(t, Slab) else (t[:, o:] if o else t)


def _fwd_stats(st, off=0, mode=True):
    """statistics keywords of a forward producer in front of a BatchNorm (st None: running statistics, nothing is written).
    off: branch segment of a fused hidden tensor; mode=False: a producer without a statistics mode (the depthwise forward)"""
    kw = dict(stats=st.at(off), stat_rows=st.rows) if st is not None else dict(stats=None, stat_rows=None)
    if mode:
        kw["stat_mode"] = STAT_SQ if st is not None else 0
    return kw


def _pro(side, t, mode=PRO_NONE, t2=None, coeffs=(), relu=0, off=0):
    """A GEMM operand, described once as the tuple (t, mode, t2, coeffs, relu) -- t as it is, act(c1*t + c2) (PRO_BNRELU) or
    c1*t + c2*t2 + c3 (PRO_BNBWD) -- seen from hidden channel `off` on.  -> its keywords of ops.gemm_nt (side "a") or ops.gemm_tn
    ("u", "v"): <side>, <side>_mode, <side>2, <side>c1..3, <side>_relu"""
    kw = {side: _seg(t, off), side + "_mode": mode, side + "2": None if t2 is None else _seg(t2, off), side + "_relu": relu}
    kw.update(("%sc%d" % (side, q + 1), c[off:]) for q, c in enumerate(coeffs))
    return kw


def _wg_jobs(pl, layer):
    """Launches of a block's "project" ([oup, hidden]) or "expand" ([hidden, inp]) weight gradient -> ([(segment offset, width,
    destination, its pitch)], (first fold job, number of fold jobs) to submit afterwards).  A fused block's weights are contiguous
    over the un-padded branch widths: ONE launch into the layer's padded scratch matrix + folds, or one launch per branch segment."""
    project = layer == "project"
    if not pl.fused:
        return [(0, pl.HT, pl.Wp_grad if project else pl.We_grad, pl.HT if project else pl.inp)], (0, 0)
    if _FUSED_WG_BATCH:
        off, n = (pl.Wp_scratch_off, pl.oup * pl.HT) if project else (pl.We_scratch_off, pl.HT * pl.inp)
        fold = (pl.fold_first, pl.fold_np) if project else (pl.fold_first + pl.fold_np, pl.fold_ne)
        return [(0, pl.HT, pl.mgr.FW[off:off + n], pl.HT if project else pl.inp)], fold
    grad, row, pitch = (pl.Wp_grad, 1, pl.total) if project else (pl.We_grad, pl.inp, pl.inp)
    return [(sg, h, grad[st * row:], pitch) for sg, st, h in zip(pl.seg, pl.start, pl.hid)], (0, 0)


def _se_forward(D, scale, shift, act, S, cmap, w1p, b1, w2t, b2p, se_act, hid, N, HW, HT):
    """SqueezeAndExcitation (models/mobilenet_base.py:109-112) on A = act(scale * D + shift): squeeze -> two tiny dense layers
    (packed over the padded channel layout) -> gate; S = gate * A.  -> what the backward needs: pooled, gate, hpre"""
    dev = S.device
    sv = dict(pooled=_f32(N * HT, dev).view(N, HT), gate=_f32(N * HT, dev).view(N, HT), hpre=_f32(N * hid, dev).view(N, hid))
    parts = ops.se_pool_parts(N, HW, HT)
    pooled_parts = _f32(parts * N * HT, dev).view(parts, N, HT)
    ops.se_squeeze(D, scale, shift, act, pooled_parts, N, HW, HT)
    ops.se_mlp_fwd(pooled_parts, sv["pooled"], cmap, w1p, b1, w2t, b2p, se_act, sv["hpre"], sv["gate"], N, HT, hid)
    ops.se_scale(D, scale, shift, act, sv["gate"], S, N * HW, HW, HT)
    return sv


def _se_backward(dS, D, scale, shift, act, sv, cmap, w1p, w2t, se_act, hid, dw1, db1, dw2, db2, total, g, st2, N, HW, HT):
    """dS = dL/dS -> g = dL/dD' (D' = scale * D + shift) with its BatchNorm-backward statistics in st2: back through the gate
    (dense-layer gradients accumulate into dw1 / db1 / dw2 / db2, contiguous over `total` channels) and the activation"""
    dev = g.device
    dz2, dpooled = (_f32(N * HT, dev).view(N, HT) for _ in range(2))
    parts = ops.se_pool_parts(N, HW, HT)
    dgate = _f32(parts * N * HT, dev).view(parts, N, HT)
    dz1 = _f32(N * hid, dev).view(N, hid)
    ops.se_bwd_gate(dS, D, scale, shift, act, sv["gate"], sv["pooled"], cmap, w1p, w2t, sv["hpre"], dgate, dz2, dz1, dpooled, dw1, db1, dw2,
                    db2, N, HW, HT, total, hid, se_act=se_act)
    ops.se_bwd_apply(dS, D, scale, shift, act, sv["gate"], dpooled, g, st2.t, N * HW, HW, HT, stat_rows=st2.rows)


def block_forward(pl, x2d, N, H, W, need_grad):
    """InvertedResidualChannels.forward on arena views.  Returns (out2d, saved) -- saved is None when need_grad is False."""
    dev, T = x2d.device, x2d.dtype
    HT, s, act = pl.HT, pl.stride, pl.act
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    M, M2 = N * H * W, N * Ho * Wo
    if pl.expand:
        E = _hidden(pl, M, HT, T, dev)
        stE = _stats(HT, dev, pl.bne["mgr"]) if bn_uses_batch_stats(pl.bne) else None
        ops.gemm_nt(x2d, pl.We_pack, E, M, HT, pl.inp, **_fwd_stats(stE))
        bE = bn_forward_coeffs(pl.bne, stE, M, dev)
        _tap("expand", pl, E, bE)
    else:
        E, bE = x2d, None
    D = _hidden(pl, M2, HT, T, dev)
    stD = _stats(HT, dev, pl.bnd["mgr"]) if bn_uses_batch_stats(pl.bnd) else None
    for i in range(pl.nb):
        o, c = pl.seg[i], pl.segpad(pl.hid[i])
        ops.dwconv_fwd(_seg(E, o), bE.scale[o:] if bE else None, bE.shift[o:] if bE else None, act if bE else 0, pl.taps[i], _seg(D, o),
                       stat_ld=HT, N=N, H=H, W=W, C=c, k=pl.ks[i], stride=s, **_fwd_stats(stD, o, mode=False))
    bD = bn_forward_coeffs(pl.bnd, stD, M2, dev)
    _tap("dw", pl, D, bD)
    Pr = torch.empty(M2, pl.oup, dtype=T, device=dev)
    stP = _stats(pl.oup, dev, pl.bnp["mgr"]) if bn_uses_batch_stats(pl.bnp) else None
    # the projection's operand A: the activated depthwise output act(bn(D)) as a prologue of D, or gated by the SE as a tensor S
    se, A = None, (D, PRO_BNRELU, None, (bD.scale, bD.shift), int(act))
    if pl.se:
        A = (_hidden(pl, M2, HT, T, dev),)
        se = _se_forward(D, bD.scale, bD.shift, int(act), A[0], pl.cmap, pl.se_w1p, pl.se_b1, pl.se_w2t, pl.se_b2p, pl.se_act, pl.se_hid,
                         N, Ho * Wo, HT)
    ops.gemm_nt(wp=pl.Wp_pack, c=Pr, M=M2, N=pl.oup, K=HT, **_pro("a", *A), **_fwd_stats(stP))
    bP = bn_forward_coeffs(pl.bnp, stP, M2, dev)
    out = torch.empty(M2, pl.oup, dtype=T, device=dev)
    drop_p, keep = _drop_rate(pl), None
    if drop_p > 0:
        # stochastic depth: the same launch slot, with the branch dropped per image behind the (undropped) block-output BatchNorm
        keep = pl.drop_keep = torch.empty(N, dtype=torch.uint8, device=dev)
        ops.bn_apply_drop(Pr, bP.scale, bP.shift, x2d, out, keep, drop_p, getattr(pl.mgr.model, "dropout_seed", DROP_CONNECT_SEED),
                          pl.mgr.step_counter, pl.module.drop_connect_index, N, Ho * Wo, pl.oup)
    else:
        ops.bn_apply(Pr, bP.scale, bP.shift, False, x2d if pl.res else None, out, M2, pl.oup)
    _stap(pl, E=E if pl.expand else None, bne=bE, D=D, bnd=bD, P=Pr, bnp=bP, out=out)
    if not need_grad:
        return out, None
    return out, dict(x=x2d, E=E, D=D, P=Pr, bE=bE, bD=bD, bP=bP, dims=(N, H, W, Ho, Wo), se=se, A=A, keep=keep, drop_p=drop_p)


def _drop_rate(pl):
    """stochastic-depth rate of this forward: the module's drop_connect_rate for a residual block in training mode, else 0"""
    m = pl.module
    return float(m.drop_connect_rate) if pl.res and m.training else 0.0


def drop_connect_keep(block):
    """uint8 [N] keep decisions (1 = branch kept) of the last training forward of `block` (an InvertedResidualChannels[Fused] module)
    that ran with stochastic depth, None if it never did.  Every forward allocates its own tensor (as the tail dropout does), so
    "last" is the last forward that ran in Python: a captured step's tensor is rewritten by every replay of that graph, and of the two
    graphs of a captured accumulated step this is the one captured last."""
    pl = getattr(block, "_plan", None)
    return getattr(pl, "drop_keep", None) if pl is not None else None


def project_bwd_form(pl, T, M2, G, D, g, stat_rows):
    """-> "fused" | "dp" | "prologue": the form a block's projection backward takes (G, D, g: its tensors, for their layouts)"""
    # "fused": weight and input gradient from ONE pass over D (atomnas_project_bwd on the materialised dP).  Early stages: plain blocks
    # (an SE needs dL/dS between the two gradients, a fused block's weight is not [oup, HT]) up to the widest output at which the
    # fused kernel wins, where the library has an instance for the widths and serves the layouts
    if (pl.expand and not pl.fused and not pl.se and pl.oup <= PROJECT_BWD_FUSED_MAX_OUP and ops.project_bwd_supported(pl.oup, pl.HT, T)
            and ops.project_bwd_dp_supported(M2, pl.oup, pl.HT, G, D, g, stat_rows)):
        return "fused"
    # "dp": dP = p1*G + p2*P + p3 materialised once, two GEMMs read it without a prologue.  Late stages (oup >= 80: every row of dP
    # feeds 23..54 GEMM tiles): dP is a few MB, and the input-gradient GEMM takes the streaming kernel (k_gemm_nt_st), measured
    # 84 / 102 / 74 us against 158 / 198 / 208 us with the prologue (14x14 80 / 96 wide, 7x7).  bf16 rows of a multiple of 8 channels;
    # else (fp32 storage) "prologue": two GEMMs with the BatchNorm backward of (G, P) in every tile
    return "dp" if T == torch.bfloat16 and pl.oup % 8 == 0 else "prologue"


def expand_bwd_form(pl, T, x2d, h):
    """-> "noe_fused" | "noe_segments" | "noe_gemms" | "e": the form a block's expand backward takes (x2d, h: its tensors, for their layouts)"""
    # "e": two GEMMs with the BatchNorm backward of (h, E) as their prologue.  The forms without the raw expand output E serve bf16
    # plain blocks up to the widest input at which they win; atomnas_gram reads rows of a multiple of 8 channels and pitch
    if not (T == torch.bfloat16 and not pl.fused and pl.inp <= EXPAND_BWD_NOE_MAX_INP and pl.inp % 8 == 0 and x2d.stride(0) % 8 == 0):
        return "e"
    if ops.expand_bwd_supported(pl.inp, pl.HT, T):   # both gradients from ONE pass over h: the accumulators of the hidden width fit
        return "noe_fused"
    # 40 -> 720: those of one branch segment (240 channels) do -- the same kernel once per segment; else three GEMMs
    if pl.nb > 1 and isinstance(h, Slab) and all(ops.expand_bwd_supported(pl.inp, pl.segpad(hh), T) for hh in pl.hid):
        return "noe_segments"
    return "noe_gemms"


def block_backward(pl, sv, G):
    """G = dL/d(out) [M2, oup] -> dL/dx [M, inp]; parameter gradients go to the gradient arena."""
    dev, T = G.device, G.dtype
    N, H, W, Ho, Wo = sv["dims"]
    M, M2 = N * H * W, N * Ho * Wo
    HT, s = pl.HT, pl.stride
    x2d, E, D, bE = sv["x"], sv["E"], sv["D"], sv["bE"]
    # pw_bn backward: statistics pass over (G, P), then coefficients
    st2P = _stats(pl.oup, dev, pl.bnp["mgr"])
    if sv["keep"] is not None:
        # stochastic depth: the branch receives Gs = keep[n] / (1 - p) * G (the same launch slot writes it with its statistics); the
        # residual path below keeps G
        Gb = torch.empty(M2, pl.oup, dtype=T, device=dev)
        ops.drop_connect_bwd(G, sv["P"], sv["keep"], sv["drop_p"], Gb, st2P.t, N, Ho * Wo, pl.oup, stat_rows=st2P.rows)
    else:
        Gb = G
        ops.act_bwd_stats(G, sv["P"], None, None, False, None, st2P.t, M2, pl.oup, stat_rows=st2P.rows)
    p = bn_backward_coeffs(pl.bnp, sv["bP"], st2P, M2, dev)
    # projection backward by form: g = gradient wrt the dw_bn output, with the dw_bn backward statistics
    g = _hidden(pl, M2, HT, T, dev)
    st2D = _stats(HT, dev, pl.bnd["mgr"])
    dP = _project_backward(pl, project_bwd_form(pl, T, M2, Gb, D, g, st2D.rows), sv, Gb, p, g, st2D)
    d1, d2, d3 = d = bn_backward_coeffs(pl.bnd, sv["bD"], st2D, M2, dev)
    # depthwise backward per branch
    h = _hidden(pl, M, HT if pl.expand else pl.inp, T, dev)
    if pl.expand:
        st2E = _stats(HT, dev, pl.bne["mgr"])
        for i in range(pl.nb):
            o, c = pl.seg[i], pl.segpad(pl.hid[i])
            ops.dwconv_bwd(_seg(g, o), _seg(D, o), d1[o:], d2[o:], d3[o:], _seg(E, o), bE.scale[o:], bE.shift[o:], pl.act, pl.taps[i],
                           _seg(h, o), pl.Wd_grad[i], st2E.at(o), HT, N, H, W, c, pl.ks[i], s, stat_rows=st2E.rows)
    elif pl.nb > 1:
        raise NotImplementedError("non-expanding block with more than one branch")
    else:
        ops.dwconv_bwd(g, D, d1, d2, d3, E, None, None, 0, pl.taps[0], h, pl.Wd_grad[0], None, 0, N, H, W, pl.segpad(pl.hid[0]), pl.ks[0], s)
    _stap(pl, p=p, dP=dP, g=g, d=d, h=h)
    if not pl.expand:
        return h + G if pl.res else h
    e = bn_backward_coeffs(pl.bne, bE, st2E, M, dev)
    _stap(pl, e=e)
    # expand backward by form (+ residual branch)
    Gx = torch.empty(M, pl.inp, dtype=T, device=dev)
    res = G if pl.res else None
    form = expand_bwd_form(pl, T, x2d, h)
    if form != "e":
        return _expand_backward_noe(pl, form, x2d, h, e, res, Gx, M)
    # dE = e1*h + e2*E + e3 as the GEMMs' prologue.  Weight gradient dWe[n][k] = sum_m dE[m][n] * x[m][k] (written transposed:
    # out[i=k][j=n] -> dWe[n*inp + k]), then the input gradient
    dE = (h, PRO_BNBWD, E, e)
    jobs, fold = _wg_jobs(pl, "expand")
    for sg, nv, out, pitch in jobs:
        ops.gemm_tn(u=x2d, NU=pl.inp, NV=nv, out=out, si=1, sj=pitch, M=M, **_pro("v", *dE, off=sg))
    ops.fold_jobs(pl.mgr, *fold)
    ops.gemm_nt(wp=pl.WeT_pack, c=Gx, M=M, N=pl.inp, K=HT, add=res, **_pro("a", *dE))
    return Gx


def _project_backward(pl, form, sv, G, p, g, st2D):
    """Projection backward in the form project_bwd_form chose: dWp[n][k] = sum_m dP[m][n] * A[m][k] into the gradient arena; g = dP Wp
    back through the SE gate / masked by the depthwise activation, dw_bn backward statistics in st2D.  -> dP tensor of the "dp" form"""
    N, _, _, Ho, Wo = sv["dims"]
    M2, HT, act = N * Ho * Wo, pl.HT, int(pl.act)
    D, Pr, bD, se = sv["D"], sv["P"], sv["bD"], sv["se"]
    if form == "prologue":
        dP, dPop = None, (G, PRO_BNBWD, Pr, p)
    else:   # dP once: a narrow tensor that the kernels below stream without a prologue
        dP = torch.empty(M2, pl.oup, dtype=G.dtype, device=G.device)
        ops.bnbwd_apply(G, Pr, *p, dP, M2, pl.oup)
        dPop = (dP,)
    if form == "fused":
        ops.project_bwd(dP, pl.WpT_pack, D, bD.scale, bD.shift, act, g, st2D.t, pl.Wp_grad, HT, 1, M2, pl.oup, HT, stat_rows=st2D.rows)
        return None
    jobs, fold = _wg_jobs(pl, "project")
    for sg, nv, out, pitch in jobs:
        ops.gemm_tn(NU=pl.oup, NV=nv, out=out, si=pitch, sj=1, M=M2, **_pro("u", *dPop), **_pro("v", *sv["A"], off=sg))
    ops.fold_jobs(pl.mgr, *fold)
    if se is not None:
        # gradient wrt the gated tensor, then back through the gate (models/mobilenet_base.py:109-112) and the activation
        dS = _hidden(pl, M2, HT, G.dtype, G.device)
        ops.gemm_nt(wp=pl.WpT_pack, c=dS, M=M2, N=HT, K=pl.oup, **_pro("a", *dPop))
        _se_backward(dS, D, bD.scale, bD.shift, act, se, pl.cmap, pl.se_w1p, pl.se_w2t, pl.se_act, pl.se_hid, pl.se_dw1, pl.se_db1,
                     pl.se_dw2, pl.se_db2, pl.total, g, st2D, N, Ho * Wo, HT)
    else:
        # projection input gradient, masked by the depthwise activation
        ops.gemm_nt(wp=pl.WpT_pack, c=g, M=M2, N=HT, K=pl.oup, **_pro("a", *dPop), z=D, zscale=bD.scale, zshift=bD.shift, mask=act,
                    stats=st2D.t, stat_mode=STAT_Z, stat_rows=st2D.rows)
    return dP


def _plan_buffer(pl, name, make):
    """small per-plan scratch that survives across steps (created on first use, i.e. in an eager step before any graph capture)"""
    cache = pl.__dict__.setdefault("_scratch", {})
    t = cache.get(name)
    if t is None:
        t = cache[name] = make()
    return t


def _expand_backward_noe(pl, form, x2d, h, e, res, Gx, M):
    """Backward of the expand convolution from ONE hidden stream (models/mobilenet_base.py:316-320 backward).  With the BatchNorm
    backward dE = e1*h + e2*E + e3 and E = x We^T:
        dX  = (e1*h) We + x M + v (+ residual),        M = We^T diag(e2) We,  v = e3^T We
        dWe = (e1*h)^T x + diag(e2) We (X^T X) + e3 (sum x)^T
    The e2 / e3 terms are inp x inp sized (atomnas_gram + atomnas_xb_coeffs); the wide GEMMs read h alone (e1 as their scale
    prologue), where the BNBWD-prologue forms read h and E.  form: "noe_fused" | "noe_segments" | "noe_gemms" (expand_bwd_form)."""
    dev, T, inp, HT = x2d.device, x2d.dtype, pl.inp, pl.HT
    e1, e2, e3 = e
    gram = torch.empty(inp * inp, dtype=torch.float32, device=dev)
    sx = torch.empty(inp, dtype=torch.float32, device=dev)
    ops.gram(x2d, M, inp, gram, sx, ws=_plan_buffer(pl, "gram_ws", lambda: torch.empty(2048 * (inp * inp + inp), dtype=torch.float32, device=dev)))
    # M packed as a gemm_nt weight (padding stays zero: the buffer is created zeroed once and only its inp x inp corner is rewritten)
    mp = _plan_buffer(pl, "xb_mp", lambda: ops.zeros((inp + 63) // 64 * 64, (inp + 31) // 32 * 32, dtype=T, device=dev))
    vb = torch.empty(pad8(inp), dtype=torch.float32, device=dev)
    ops.xb_coeffs(e2, e3, pl.We_pack, gram, sx, inp, HT, mp, vb, pl.We_grad)
    if form == "noe_fused":
        # one pass over h: both gradients, x M + v added inside the kernel
        ops.expand_bwd(h, e1, x2d, pl.WeT_pack, res, Gx, pl.We_grad, M, inp, HT, mp=mp, vb=vb)
    elif form == "noe_segments":
        # one launch of the streaming kernel per segment; the input gradient accumulates through `add` (a launch reads and writes its
        # own rows of Gx only), x M + v rides in the first launch
        for i in range(pl.nb):
            o, c = pl.seg[i], pl.segpad(pl.hid[i])
            ops.expand_bwd(_seg(h, o), e1[o:], x2d, pl.WeT_pack[:, o:], res if i == 0 else Gx, Gx, pl.We_grad[o * inp:], M, inp,
                           c, mp=mp if i == 0 else None, vb=vb if i == 0 else None)
    else:   # "noe_gemms"
        gx1 = torch.empty(M, inp, dtype=T, device=dev)
        ops.gemm_nt(x2d, mp, gx1, M, inp, inp, bias=vb, add=res)
        zeros = _plan_buffer(pl, "xb_zero%d" % e1.numel(), lambda: ops.zeros(e1.numel(), dtype=torch.float32, device=dev))
        e1h = (h, PRO_BNRELU, None, (e1, zeros))
        ops.gemm_tn(u=x2d, NU=inp, NV=HT, out=pl.We_grad, si=1, sj=inp, M=M, **_pro("v", *e1h))
        ops.gemm_nt(wp=pl.WeT_pack, c=Gx, M=M, N=inp, K=HT, add=gx1, **_pro("a", *e1h))
    return Gx


class BlockFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, pl):
        x2d, (N, H, W, C) = to_2d(x, pl.mgr.compute_dtype)
        if C != pl.inp:
            raise ValueError("block %s expects %d input channels, got %d" % (pl.name, pl.inp, C))
        out, sv = block_forward(pl, x2d, N, H, W, True)
        ctx.pl, ctx.sv = pl, sv
        return to_4d(out, N, *sv["dims"][3:], pl.oup)

    @staticmethod
    def backward(ctx, gout):
        pl, sv = ctx.pl, ctx.sv
        G, _ = to_2d(gout, pl.mgr.compute_dtype)
        N, H, W, _, _ = sv["dims"]
        gx = block_backward(pl, sv, G)
        _stap(pl, gx=gx)
        ctx.sv = None
        pl.mgr.grad_done(pl)
        return to_4d(gx, N, H, W, pl.inp), None, None


def run_block(pl, x, anchor):
    if pl.nb == 0:
        return x
    if torch.is_grad_enabled() and (x.requires_grad or anchor.requires_grad):
        return BlockFunction.apply(x, anchor, pl)
    x2d, (N, H, W, C) = to_2d(x, pl.mgr.compute_dtype)
    out, _ = block_forward(pl, x2d, N, H, W, False)
    s = pl.stride
    return to_4d(out, N, (H - 1) // s + 1, (W - 1) // s + 1, pl.oup)


# ---------------------------------------------------------------------------------------------- stand-alone SqueezeAndExcitation
class SEFunction(torch.autograd.Function):
    """SqueezeAndExcitation.forward (models/mobilenet_base.py:109-112) as a module call of its own: sigmoid(W2 act(W1 mean(x) + b1) + b2) * x
    with the SE sequence of the fused block (_se_forward / _se_backward), which runs it on the raw depthwise output with the dw_bn
    coefficients and the plan's packed weights; here on an already activated tensor: identity coefficients, weights packed on the spot."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, se_act, dtype):
        x2d, (N, H, W, C) = to_2d(x, dtype)
        dev = x.device
        hid = w1.shape[0]
        HT = pads(C)
        M = N * H * W
        D = ops.zeros(M, HT, dtype=dtype, device=dev)
        D[:, :C] = x2d
        cmap = torch.full((HT,), -1, dtype=torch.int32, device=dev)
        cmap[:C] = torch.arange(C, dtype=torch.int32, device=dev)
        w1p, w2t, b2p = (ops.zeros(*shape, dtype=torch.float32, device=dev) for shape in ((hid, HT), (hid, HT), (HT,)))
        w1p[:, :C] = w1.detach().reshape(hid, C).float()
        w2t[:, :C] = w2.detach().reshape(C, hid).float().t()
        b2p[:C] = b2.detach().float()
        one, zero = torch.ones(HT, dtype=torch.float32, device=dev), ops.zeros(HT, dtype=torch.float32, device=dev)
        one[C:] = 0
        S = torch.empty(M, HT, dtype=dtype, device=dev)
        sv = _se_forward(D, one, zero, ACT_NONE, S, cmap, w1p, b1.detach().float().contiguous(), w2t, b2p, se_act, hid, N, H * W, HT)
        ctx.save_for_backward(D, one, zero, sv["gate"], sv["pooled"], cmap, w1p, w2t, sv["hpre"])
        ctx.dims = (N, H, W, C, HT, hid, se_act, dtype)
        return to_4d(S[:, :C], N, H, W, C)

    @staticmethod
    def backward(ctx, gout):
        D, one, zero, gate, pooled, cmap, w1p, w2t, hpre = ctx.saved_tensors
        N, H, W, C, HT, hid, se_act, dtype = ctx.dims
        dev = D.device
        M = N * H * W
        g2d, _ = to_2d(gout, dtype)
        dS = ops.zeros(M, HT, dtype=dtype, device=dev)
        dS[:, :C] = g2d
        dw1, db1, dw2, db2 = (_f32(hid * C, dev, zero=True), _f32(hid, dev, zero=True), _f32(C * hid, dev, zero=True), _f32(C, dev, zero=True))
        g = torch.empty(M, HT, dtype=dtype, device=dev)
        _se_backward(dS, D, one, zero, ACT_NONE, dict(gate=gate, pooled=pooled, hpre=hpre), cmap, w1p, w2t, se_act, hid, dw1, db1, dw2, db2,
                     C, g, _stats(HT, dev), N, H * W, HT)
        return (to_4d(g[:, :C], N, H, W, C), dw1.view(hid, C, 1, 1), db1, dw2.view(C, hid, 1, 1), db2, None, None)


def run_se(module, x):
    """stand-alone call of a SqueezeAndExcitation module (NCHW tensor on the GPU, C a multiple of 8)"""
    dtype = x.dtype if x.dtype in (torch.float32, torch.bfloat16) else torch.float32
    return SEFunction.apply(x, module.se_reduce.weight, module.se_reduce.bias, module.se_expand.weight, module.se_expand.bias,
                            act_code(module.active_fn), dtype)


# ---------------------------------------------------------------------------------------------- ConvBNReLU (stem / 1x1 / depthwise)
def convbn_forward(pl, x, need_grad):
    """Stand-alone ConvBNReLU: stem 3x3/s2 on an NCHW fp32 image (im2col + GEMM), 1x1 conv, or depthwise conv."""
    mgr = pl.mgr
    T = mgr.compute_dtype
    dev = x.device
    act = pl.act
    sv = {}
    if pl.groups == 1 and pl.k == 3:
        if pl.cin != 3 or pl.stride != 2:
            raise NotImplementedError("dense 3x3 convolution other than the 3-channel stride-2 stem")
        N, _, H, W = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        M = N * Ho * Wo
        col = torch.empty(M, 32, dtype=T, device=dev)
        ops.im2col_stem(x.float().contiguous(), col, N, H, W)
        a2d, K = col, 27
        sv["kind"] = "stem"
    elif pl.groups == 1 and pl.k == 1:
        a2d, (N, H, W, C) = to_2d(x, T)
        Ho, Wo, M, K = H, W, N * H * W, pl.cin
        sv["kind"] = "pw"
    else:
        a2d, (N, H, W, C) = to_2d(x, T)
        s = pl.stride
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        M = N * Ho * Wo
        sv["kind"] = "dw"
    Cp = pad8(pl.cout)
    Y = torch.empty(M, Cp, dtype=T, device=dev) if sv["kind"] != "dw" else ops.zeros(M, Cp, dtype=T, device=dev)
    st = _stats(pl.cout, dev, pl.bn["mgr"]) if bn_uses_batch_stats(pl.bn) else None
    if sv["kind"] == "dw":
        ops.dwconv_fwd(a2d, None, None, 0, pl.taps, Y, stat_ld=pl.cout, N=N, H=H, W=W, C=pl.cout, k=pl.k, stride=pl.stride,
                       **_fwd_stats(st, mode=False))
    else:
        ops.gemm_nt(a2d, pl.W_pack, Y, M, pl.cout, K, **_fwd_stats(st))
    b = bn_forward_coeffs(pl.bn, st, M, dev)
    if act:
        _tap("convbn", pl, Y, b)
    out = torch.empty(M, Cp, dtype=T, device=dev)
    ops.bn_apply(Y, b.scale, b.shift, int(act), None, out, M, pl.cout)
    _stap(pl, Y=Y, bn=b, out=out)
    if need_grad:
        sv.update(a=a2d, Y=Y, b=b, dims=(N, H, W, Ho, Wo), K=K if sv["kind"] != "dw" else 0)
    return out, (N, Ho, Wo), sv


def convbn_backward(pl, sv, G, need_input_grad):
    dev, T = G.device, G.dtype
    N, H, W, Ho, Wo = sv["dims"]
    M = N * Ho * Wo
    act = pl.act
    Y, b, a2d = sv["Y"], sv["b"], sv["a"]
    g = torch.empty_like(Y)
    st2 = _stats(pl.cout, dev, pl.bn["mgr"])
    ops.act_bwd_stats(G, Y, b.scale if act else None, b.shift if act else None, int(act), g, st2.t, M, pl.cout, stat_rows=st2.rows)
    c1, c2, c3 = bn_backward_coeffs(pl.bn, b, st2, M, dev)
    _stap(pl, g=g, c=(c1, c2, c3))
    if sv["kind"] == "dw":
        h = ops.zeros(N * H * W, pad8(pl.cout), dtype=T, device=dev)
        ops.dwconv_bwd(g, Y, c1, c2, c3, a2d, None, None, 0, pl.taps, h, pl.W_grad, None, 0, N, H, W, pl.cout, pl.k, pl.stride)
        return h
    K = sv["K"]
    # dW[n][k] = sum_m dY[m][n] * a[m][k]
    ops.gemm_tn(a2d, K, g, pl.cout, pl.W_grad, 1, K, M, v_mode=PRO_BNBWD, v2=Y, vc1=c1, vc2=c2, vc3=c3)
    if not need_input_grad or sv["kind"] == "stem":
        return None
    Gx = torch.empty(M, pad8(K), dtype=T, device=dev)
    ops.gemm_nt(g, pl.WT_pack, Gx, M, K, pl.cout, a_mode=PRO_BNBWD, a2=Y, ac1=c1, ac2=c2, ac3=c3)
    return Gx


class ConvBNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, pl):
        out, (N, Ho, Wo), sv = convbn_forward(pl, x, True)
        ctx.pl, ctx.sv = pl, sv
        ctx.x_needs = x.requires_grad
        return to_4d(out[:, :pl.cout] if out.shape[1] != pl.cout else out, N, Ho, Wo, pl.cout)

    @staticmethod
    def backward(ctx, gout):
        pl, sv = ctx.pl, ctx.sv
        G, _ = to_2d(gout, pl.mgr.compute_dtype)
        gx = convbn_backward(pl, sv, G, ctx.x_needs)
        ctx.sv = None
        pl.mgr.grad_done(pl)
        N, H, W, _, _ = sv["dims"]
        if gx is None:
            return None, None, None
        cin = pl.cin
        return to_4d(gx[:, :cin] if gx.shape[1] != cin else gx, N, H, W, cin), None, None


def run_convbn(pl, x, anchor):
    if pl.cout % 8 != 0:
        raise ValueError("ConvBNReLU output channels must be a multiple of 8 on the HIP path, got %d" % pl.cout)
    if torch.is_grad_enabled() and (x.requires_grad or anchor.requires_grad):
        return ConvBNFunction.apply(x, anchor, pl)
    out, (N, Ho, Wo), _ = convbn_forward(pl, x, False)
    return to_4d(out, N, Ho, Wo, pl.cout)


# ---------------------------------------------------------------------------------------------- fused tail: last conv + pool + dropout + fc
def tail_forward(lp, fp, x, drop_p, training, seed, step_ptr, need_grad, logits_out=None):
    """features[-2] (1x1 ConvBNReLU) -> AvgPool2d(H) -> squeeze -> Dropout -> Linear, without materialising the activated map.
    logits_out: fp32 [N, pad8(classes)] buffer of the caller that receives the logits (the static buffer of a frozen teacher)."""
    mgr = lp.mgr
    T = mgr.compute_dtype
    dev = x.device
    a2d, (N, H, W, C) = to_2d(x, T)
    M = N * H * W
    act = lp.act
    L = torch.empty(M, lp.cout, dtype=T, device=dev)
    st = _stats(lp.cout, dev, lp.bn["mgr"]) if bn_uses_batch_stats(lp.bn) else None
    ops.gemm_nt(a2d, lp.W_pack, L, M, lp.cout, lp.cin, **_fwd_stats(st))
    b = bn_forward_coeffs(lp.bn, st, M, dev)
    if act:
        _tap("convbn", lp, L, b)
    pooled = torch.empty(N, lp.cout, dtype=T, device=dev)
    p = float(drop_p) if training else 0.0
    keep = torch.empty(N, lp.cout, dtype=torch.uint8, device=dev) if p > 0 else None
    if TAIL_TAP is not None:   # tests: the dropout keep mask this forward uses (and its backward re-uses)
        TAIL_TAP.append(keep)
    ops.bn_act_pool(L, b.scale, b.shift, int(act), pooled, keep, p, seed, step_ptr, N, H * W, lp.cout)
    Kc = fp.cout
    logits = logits_out
    if logits is None:
        logits = torch.empty(N, pad8(Kc), dtype=torch.float32, device=dev)
    elif tuple(logits.shape) != (N, pad8(Kc)) or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("logits_out must be a contiguous fp32 [%d, %d] tensor" % (N, pad8(Kc)))
    ops.gemm_nt(pooled, fp.W_pack, logits, N, Kc, fp.cin, bias=fp.bias)
    _stap(lp, L=L, bn=b, pooled=pooled, logits=logits[:, :Kc])
    sv = None
    if need_grad:
        sv = dict(a=a2d, L=L, b=b, pooled=pooled, keep=keep, p=p, dims=(N, H, W))
    return logits[:, :Kc], sv


def tail_backward(lp, fp, sv, dlogits, dl_padded=None):
    """dlogits [N, K] (any float dtype) -> gradient wrt the tail input [M, cin].  dl_padded: the same gradient already in the
    compute dtype with the channel padding zeroed (what atomnas_ce_smooth writes), used as is."""
    mgr = lp.mgr
    T = mgr.compute_dtype
    dev = sv["L"].device
    N, H, W = sv["dims"]
    M, HW = N * H * W, H * W
    Kc = fp.cout
    act = lp.act
    if dl_padded is not None:
        dl = dl_padded
    else:
        dl = ops.zeros(N, pad8(Kc), dtype=T, device=dev)
        dl[:, :Kc] = dlogits
    # classifier
    ops.gemm_tn(dl, Kc, sv["pooled"], fp.cin, fp.W_grad, fp.cin, 1, N)
    if fp.bias_grad is not None:
        ops.colsum(dl, fp.bias_grad, N, Kc)
    dpooled = torch.empty(N, fp.cin, dtype=T, device=dev)
    ops.gemm_nt(dl, fp.WT_pack, dpooled, N, fp.cin, Kc)
    # dropout + average pool + ReLU backward, with the last BN's backward statistics
    L, b = sv["L"], sv["b"]
    gL = torch.empty(M, lp.cout, dtype=T, device=dev)
    st2 = _stats(lp.cout, dev, lp.bn["mgr"])
    ops.pool_act_bwd(dpooled, sv["keep"], sv["p"], L, b.scale, b.shift, int(act), gL, st2.t, N, HW, lp.cout, stat_rows=st2.rows)
    c1, c2, c3 = bn_backward_coeffs(lp.bn, b, st2, M, dev)
    ops.gemm_tn(sv["a"], lp.cin, gL, lp.cout, lp.W_grad, 1, lp.cin, M, v_mode=PRO_BNBWD, v2=L, vc1=c1, vc2=c2, vc3=c3)
    Gx = torch.empty(M, lp.cin, dtype=T, device=dev)
    ops.gemm_nt(gL, lp.WT_pack, Gx, M, lp.cin, lp.cout, a_mode=PRO_BNBWD, a2=L, ac1=c1, ac2=c2, ac3=c3)
    _stap(lp, dpooled=dpooled, gL=gL, c=(c1, c2, c3), gx=Gx)
    return Gx


class TailFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, lp, fp, drop_p, training, seed, step_ptr):
        logits, sv = tail_forward(lp, fp, x, drop_p, training, seed, step_ptr, True)
        ctx.lp, ctx.fp, ctx.sv = lp, fp, sv
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        lp, fp, sv = ctx.lp, ctx.fp, ctx.sv
        gx = tail_backward(lp, fp, sv, dlogits)
        ctx.sv = None
        lp.mgr.grad_done(fp)
        lp.mgr.grad_done(lp)
        N, H, W = sv["dims"]
        return to_4d(gx, N, H, W, lp.cin), None, None, None, None, None, None, None


def run_tail(lp, fp, x, anchor, drop_p, training, seed, step_ptr, logits_out=None):
    if torch.is_grad_enabled() and (x.requires_grad or anchor.requires_grad):
        if logits_out is not None:
            raise ValueError("logits_out is for forwards without a gradient (torch.no_grad())")
        return TailFunction.apply(x, anchor, lp, fp, drop_p, training, seed, step_ptr)
    logits, _ = tail_forward(lp, fp, x, drop_p, training, seed, step_ptr, False, logits_out)
    return logits


class TailLossFunction(torch.autograd.Function):
    """Tail (last 1x1 ConvBNReLU -> pool -> dropout -> classifier) + label-smoothed cross entropy, mean over the batch, as ONE
    autograd node for engine.TrainStep: the loss kernel writes d(mean loss)/d(logits) directly in the compute dtype with zeroed
    padding, so no ATen op (mean, its backward, dtype / padding copies) is left between the HIP launches
    (train.py:176-180 `loss = forward_loss(...)`, utils/optim.py:199-207, common.py:67-80).
    Returns the scalar mean loss; loss_vec / topk receive the per-sample losses and the top-1 / top-5 hit counts.
    distill = (teacher_logits, alpha, temperature, kd_vec, kd_out), optional: the loss becomes (1 - alpha) * CE + alpha * T^2 *
    KL(teacher || student) in one launch (atomnas_ce_distill); without it the node issues exactly what it issued before."""

    @staticmethod
    def forward(ctx, x, anchor, lp, fp, drop_p, training, seed, step_ptr, target, eps, loss_vec, topk, loss_out, distill=None):
        logits, sv = tail_forward(lp, fp, x, drop_p, training, seed, step_ptr, True)
        B, K = logits.shape
        T = lp.mgr.compute_dtype
        dl = torch.empty(B, pad8(K), dtype=T, device=x.device)
        if distill is None:
            ops.ce_smooth(logits, target, eps, B, K, loss_vec, dl, 1.0, topk)   # gscale 1: dl = d(mean loss)/d(logits)
            ops.vec_sum(loss_vec, B, 1.0 / B, loss_out)
        else:
            # knowledge distillation: the combined objective (1 - alpha) * CE + alpha * T^2 * KL(teacher || student) is what loss_vec,
            # loss_out and dl carry; kd_vec / kd_out receive the unweighted second term and its mean
            teacher_logits, alpha, temperature, kd_vec, kd_out = distill
            if tuple(teacher_logits.shape) != (B, K):
                raise ValueError("teacher logits are %s, the student's %s" % (tuple(teacher_logits.shape), (B, K)))
            ops.ce_distill(logits, teacher_logits, target, eps, alpha, temperature, B, K, loss_vec, kd_vec, dl, 1.0, topk)
            ops.vec_sum(loss_vec, B, 1.0 / B, loss_out)
            ops.vec_sum(kd_vec, B, 1.0 / B, kd_out)
        ctx.n_in = 13 if distill is None else 14
        ctx.lp, ctx.fp, ctx.sv, ctx.dl = lp, fp, sv, dl
        ctx.logits = logits
        return loss_out[0]

    @staticmethod
    def backward(ctx, gout):
        # contract: the caller differentiates the loss itself (d total / d loss = 1, as train.py:181 `loss.backward()` does);
        # gout is therefore not multiplied in (that would be an elementwise launch per step for a factor of one).  A caller that
        # scales the returned loss would silently get unscaled gradients: ATOMNAS_CHECK_LOSS_SEED=1 verifies the seed (one host
        # synchronisation per step, so not in the default path and never under graph capture).
        if _CHECK_LOSS_SEED and not torch.cuda.is_current_stream_capturing() and float(gout) != 1.0:
            raise RuntimeError("TailLossFunction differentiates d(loss)/d(loss) = 1 only; got a seed of %r (scale the learning "
                               "rate, or use CrossEntropyLabelSmooth for a loss that is combined with other terms)" % float(gout))
        lp, fp, sv = ctx.lp, ctx.fp, ctx.sv
        gx = tail_backward(lp, fp, sv, None, dl_padded=ctx.dl)
        ctx.sv = ctx.dl = None
        lp.mgr.grad_done(fp)
        lp.mgr.grad_done(lp)
        N, H, W = sv["dims"]
        return (to_4d(gx, N, H, W, lp.cin),) + (None,) * (ctx.n_in - 1)


# ---------------------------------------------------------------------------------------------- loss
class CESmoothFunction(torch.autograd.Function):
    """Per-sample label-smoothed cross entropy; also leaves top-1 / top-5 hit counts in `topk` (int32[2], accumulated)."""

    @staticmethod
    def forward(ctx, logits, target, eps, topk):
        if not logits.is_cuda:
            raise ops._lib.AtomnasHipError("CrossEntropyLabelSmooth runs on the GPU only")
        B, K = logits.shape
        lg = logits.float()
        if lg.stride(1) != 1:
            lg = lg.contiguous()
        loss = torch.empty(B, dtype=torch.float32, device=logits.device)
        dl = torch.empty(B, K, dtype=torch.float32, device=logits.device)
        # gscale = B: dl holds d(loss_i)/d(logits_i) (the 1/B of a mean reduction comes in through grad_output)
        ops.ce_smooth(lg, target, eps, B, K, loss, dl, float(B), topk)
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (dl,) = ctx.saved_tensors
        return dl * gout.unsqueeze(1), None, None, None


class CEDistillFunction(torch.autograd.Function):
    """Per-sample (1 - alpha) * label-smoothed CE + alpha * T^2 * KL(softmax(teacher / T) || softmax(logits / T)); leaves the hit counts
    in `topk` as CESmoothFunction does and the unweighted second term in `kd` (fp32 [B]).  The teacher's logits get no gradient."""

    @staticmethod
    def forward(ctx, logits, teacher, target, eps, alpha, temperature, topk, kd):
        if not (logits.is_cuda and teacher.is_cuda):
            raise ops._lib.AtomnasHipError("DistillCrossEntropy runs on the GPU only")
        B, K = logits.shape
        lg, tc = logits.float(), teacher.float()
        if lg.stride(1) != 1:
            lg = lg.contiguous()
        if tc.stride(1) != 1:
            tc = tc.contiguous()
        loss = torch.empty(B, dtype=torch.float32, device=logits.device)
        dl = torch.empty(B, K, dtype=torch.float32, device=logits.device)
        # gscale = B: dl holds d(loss_i)/d(logits_i) (the 1/B of a mean reduction comes in through grad_output)
        ops.ce_distill(lg, tc, target, eps, alpha, temperature, B, K, loss, kd, dl, float(B), topk)
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (dl,) = ctx.saved_tensors
        return (dl * gout.unsqueeze(1),) + (None,) * 7
