"""Float64 references for the kernels BETWEEN the convolutions and GEMMs (csrc/bn.hip, head.hip, optim.hip, shrink.hip): plain torch and
numpy on the CPU, written from what the operations MEAN (torch.nn.functional, autograd, the oracle), not from the kernels' formulas.
tests/test_glue_ref.py checks these references against independent statements of the same operations; the GPU tests
(test_bn_kernels_gpu.py, test_head_kernels_gpu.py, test_optim_kernels_gpu.py, test_shrink_kernels_gpu.py) compare the kernels with them.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import atomnas_oracle as orc   # noqa: E402


def pad8(c):
    return (c + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------------------------ activations
def act_ref(a, act):
    """0 none, 1 ReLU, 2 ReLU6, 3 swish, through torch's own functions: the masks at exactly 0 and 6 are torch's"""
    if act == 0:
        return a
    if act == 1:
        return torch.relu(a)
    if act == 2:
        return F.hardtanh(a, 0.0, 6.0)
    if act == 3:
        return a * torch.sigmoid(a)
    raise ValueError(act)


def act_grad_ref(pre, act, dy):
    """d act(pre) / d pre * dy by autograd (float64)"""
    a = pre.detach().double().clone().requires_grad_(True)
    act_ref(a, act).backward(dy.double())
    return a.grad if a.grad is not None else dy.double().clone()


# ------------------------------------------------------------------------------------------------------------------ BatchNorm
def bn_train_ref(x, gamma, beta, eps, act, dy=None, res=None):
    """y = act(batch_norm(x; training)) (+ res) on x [M, C] in float64 under autograd.  Returns a dict with y, mean, var_b (biased),
    var_u (unbiased, nan for M = 1) and, given dy, dx, dgamma, dbeta (gamma / beta None: affine-free, no such gradient)."""
    x = x.detach().double().clone().requires_grad_(True)
    g = gamma.detach().double().clone().requires_grad_(True) if gamma is not None else None
    b = beta.detach().double().clone().requires_grad_(True) if beta is not None else None
    if x.shape[0] > 1:
        z = F.batch_norm(x, None, None, g, b, True, 0.0, eps)
    else:   # torch refuses a batch of one value per channel: the normalisation written out (mean = x, variance 0)
        z = (x - x.mean(0)) / torch.sqrt(((x - x.mean(0)) ** 2).mean(0) + eps)
        z = (z * g if g is not None else z) + (b if b is not None else 0.0)
    y = act_ref(z, act)
    if res is not None:
        y = y + res.double()
    out = dict(y=y.detach(), mean=x.detach().mean(0), var_b=x.detach().var(0, unbiased=False),
               var_u=x.detach().var(0, unbiased=True) if x.shape[0] > 1 else torch.full((x.shape[1],), float("nan"), dtype=torch.float64))
    if dy is not None:
        y.backward(dy.double())
        out.update(dx=x.grad, dgamma=g.grad if g is not None else None, dbeta=b.grad if b is not None else None)
    return out


# ------------------------------------------------------------------------------------------------------------------ loss
def ce_ref(logits, target, eps, gscale):
    """label-smoothed cross entropy of the oracle (reduction 'none'), d(mean loss)/dlogits * gscale by autograd, and the top-1 / top-5
    hits under the convention rank = #{j : x_j > x_y}, hit_k = rank < k: a logit that TIES with the target's does not outrank it."""
    x = logits.detach().double().clone().requires_grad_(True)
    loss = orc.ce_label_smooth(x, target, eps)
    loss.mean().backward()
    xd = x.detach()
    xy = xd.gather(1, target.view(-1, 1))
    rank = (xd > xy).sum(1)
    return dict(loss=loss.detach(), dlogits=x.grad * gscale, rank=rank, top1=int((rank < 1).sum()), top5=int((rank < 5).sum()))


# ------------------------------------------------------------------------------------------------------------------ dropout
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def dropout_hash_ref(seed, step, N, C):
    """r[n][c] (uint32 in a uint64 array): key = seed ^ step * 0x100000001B3 ^ ((n*C + c) << 20), splitmix64 finaliser, top 32 bits"""
    with np.errstate(over="ignore"):
        e = np.arange(N * C, dtype=np.uint64).reshape(N, C)
        sk = np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
        st = np.array([(int(step) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
        key = sk ^ st ^ (e << np.uint64(20))
        key = key + np.uint64(0x9E3779B97F4A7C15)
        key = (key ^ (key >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        key = (key ^ (key >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        key = key ^ (key >> np.uint64(31))
        return key >> np.uint64(32)


def dropout_keep_ref(seed, step, N, C, p):
    """keep[n][c] (uint8) = float32((r >> 8) * 2^-24) >= float32(p)"""
    r = dropout_hash_ref(seed, step, N, C)
    u = (r >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(p)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ optimizer
def rmsprop_ref(p, g, sq, buf, ema, wd, lr, alpha, eps, momentum, eps_inside_sqrt, gscale=1.0, ema_decay=None):
    """One fused optimizer step in float64: g' = g * gscale + wd * p, the oracle's rmsprop_update on g', the oracle's ema_update of the
    shadow with the new p (ema None or ema_decay None / < 0: no EMA).  wd: per-element tensor or None.  Returns new p, sq, buf, ema and
    the value of the L2 regulariser at the OLD p, 0.5 * sum wd * p^2."""
    p, g, sq = p.double().clone(), g.double().clone(), sq.double().clone()
    buf = buf.double().clone() if buf is not None else None
    wdv = wd.double() if wd is not None else torch.zeros_like(p)
    l2 = 0.5 * float((wdv * p * p).sum())
    gg = g * gscale + wdv * p
    orc.rmsprop_update(p, gg, sq, buf if momentum > 0 else None, lr, alpha, eps, momentum, eps_inside_sqrt)
    e = None
    if ema is not None:
        e = ema.double().clone()
        if ema_decay is not None and ema_decay >= 0:
            orc.ema_update(e, p, ema_decay)
    return dict(p=p, sq=sq, buf=buf, ema=e, l2=l2)


def regularisers_ref(p, g, jobs, use_sign, mult=1.0, go=1.0, post_scale=1.0):
    """jobs: (off, count, coef).  Gradient: g[off:off+count] += coef * mult * go * (sign(p) or p) (torch.sign: sign(0) = 0).
    Value: post_scale * mult * sum_jobs coef * sum (|p| with use_sign, else p^2).  Returns (new g, value), float64."""
    p, g = p.double(), g.double().clone()
    val = 0.0
    for off, count, coef in jobs:
        s = p[off:off + count]
        g[off:off + count] += float(coef) * mult * go * (torch.sign(s) if use_sign else s)
        val += float(coef) * float((s.abs() if use_sign else s * s).sum())
    return g, post_scale * mult * val


def pack_ref(arena, job):
    """job: dict(src_off, dst_off, rows, cols, src_ld, dst_ld, c_off, mode).  Returns (flat destination element indices, values) of the
    logical [rows][cols] matrix: mode 0 to [r][c_off + c], mode 1 transposed to [c_off + c][r], mode 2 (depthwise taps) to [c][c_off + r]."""
    rows, cols = job["rows"], job["cols"]
    src = torch.as_strided(arena, (rows, cols), (job["src_ld"], 1), job["src_off"]).double()
    r = torch.arange(rows).view(-1, 1).expand(rows, cols)
    c = torch.arange(cols).view(1, -1).expand(rows, cols)
    if job["mode"] == 0:
        idx = r * job["dst_ld"] + job["c_off"] + c
    elif job["mode"] == 1:
        idx = (job["c_off"] + c) * job["dst_ld"] + r
    else:
        idx = c * job["dst_ld"] + job["c_off"] + r
    return (idx + job["dst_off"]).reshape(-1), src.reshape(-1)


def alive_ref(p, ema, thr, mode):
    """mask = |gamma| > thr (mode 0), OR the same of the EMA shadow (1), the shadow alone (2); compared in float32, strictly.  Returns
    (mask bool, ascending kept index from torch.nonzero, kept count)."""
    t = torch.tensor(thr, dtype=torch.float32)
    a = p.float().abs() > t
    b = (ema.float().abs() > t) if ema is not None else torch.zeros_like(a)
    m = a if mode == 0 else ((a | b) if mode == 1 else b)
    idx = torch.nonzero(m).flatten()
    return m, idx, int(idx.numel())


def gather_ref(src, mask, dim):
    return src[mask] if dim == 0 else src[:, mask]
