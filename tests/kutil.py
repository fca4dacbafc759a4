"""Helpers shared by the GPU kernel parity tests: NHWC-padded buffers <-> NCHW tensors, tolerances."""
import collections

import torch


def pad8(c):
    return (c + 7) // 8 * 8


def to_act(x_nchw, dtype, ld=None, device="cuda"):
    """NCHW (any float dtype, CPU) -> [N*H*W, ld] buffer on the GPU, padding channels zero."""
    N, C, H, W = x_nchw.shape
    ld = ld or pad8(C)
    buf = torch.zeros(N * H * W, ld, dtype=dtype, device=device)
    buf[:, :C] = x_nchw.permute(0, 2, 3, 1).reshape(-1, C).to(dtype).to(device)
    return buf


def from_act(buf, N, H, W, C):
    """[M, ld] GPU buffer -> NCHW float64 CPU tensor."""
    return buf[:, :C].double().cpu().reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous()


def rounded(x_nchw, dtype):
    """Value of x after storage in `dtype` (so references see exactly what the kernel reads)."""
    return x_nchw.to(dtype).double()


def cvec(v, device="cuda"):
    """per-channel fp32 vector padded to a multiple of 8"""
    C = v.numel()
    out = torch.zeros(pad8(C), dtype=torch.float32, device=device)
    out[:C] = v.float().to(device)
    return out


def tol(dtype):
    # fp32 kernels: accumulation-order noise only.  bf16 storage: one rounding of the output (2^-8 relative).
    return dict(rtol=2e-4, atol=2e-5) if dtype == torch.float32 else dict(rtol=1.2e-2, atol=1e-2)


# ---- depthwise kernel tests (tests/test_dwconv_family_gpu.py)
def fresh(M, C, dtype, poison=7.0, device="cuda"):
    """output buffer as the allocator hands it out: padding channels zero, the valid region poisoned (unwritten elements are caught;
    tests whose references are integers pass a NaN poison, which equals no reference value)"""
    b = torch.zeros(M, pad8(C), dtype=dtype, device=device)
    b[:, :C] = poison
    return b


def taps(w):
    """[C, 1, k, k] -> the tap table [k*k][pad8(C)], fp32 on the GPU"""
    C, _, k, _ = w.shape
    t = torch.zeros(k * k, pad8(C), dtype=torch.float32, device="cuda")
    t[:, :C] = w.reshape(C, k * k).t().float().cuda()
    return t


def act64(pre, mode):
    """the C ABI's activation codes in float64: 0 none, 1 ReLU, 2 ReLU6, 3 Swish"""
    if mode == 0:
        return pre
    if mode == 1:
        return torch.relu(pre)
    if mode == 2:
        return torch.clamp(pre, 0.0, 6.0)
    return pre * torch.sigmoid(pre)


def act_grad64(pre, mode):
    """derivative of act64 at `pre` as the kernels define it (csrc/common.h act_pass, swish_grad): strict inequalities, so it is zero AT
    0 and AT 6 (torch.clamp's autograd passes the gradient at its bounds)"""
    if mode == 0:
        return torch.ones_like(pre)
    if mode == 1:
        return (pre > 0).to(pre.dtype)
    if mode == 2:
        return ((pre > 0) & (pre < 6)).to(pre.dtype)
    s = torch.sigmoid(pre)
    return s * (1 + pre * (1 - s))


def out_hw(H, W, k, stride):
    P = (k - 1) // 2
    return (H + 2 * P - k) // stride + 1, (W + 2 * P - k) // stride + 1


def family(lib, N, H, W, C, k, stride, dtype, dir, slab):
    """The depthwise kernel family (k = 3 / 5 / 7) that atomnas_dwconv_fwd (dir 0) / atomnas_dwconv_bwd (dir 1) run for the shape, in the
    order of csrc/dwconv.hip dw_pick: "mm" (dwconv_mm.hip, or the stride-2 forward of dwconv_mm2.hip), "cw" (dwconv_cw.hip), "tile".
    `slab`: every activation operand slab-major and the tap table padded to whole 8-channel groups; anything else runs the tile kernels."""
    if not slab:
        return "tile"
    q = (N, H, W, C, k, stride, 0 if dtype == torch.float32 else 1, dir)
    if lib.atomnas_dwconv_mm_supported(*q) == 1:
        return "mm"
    return "cw" if lib.atomnas_dwconv_cw_supported(*q) == 1 else "tile"


def assert_close(name, got, ref, rtol, atol, outlier_frac=0.0, rel_l2=None):
    """Element-wise |got-ref| <= atol + rtol*|ref|, except for at most `outlier_frac` of the elements (bf16 activations
    flip a ReLU mask for pre-activations within rounding distance of zero; such elements are individually wrong by a full
    gradient contribution but rare).  rel_l2 additionally bounds ||got-ref|| / ||ref||."""
    got = got.double().cpu()
    ref = ref.double().cpu()
    err = (got - ref).abs()
    if rel_l2 is not None:
        rl = float(err.norm() / max(float(ref.norm()), float(atol) * ref.numel() ** 0.5, 1e-30))   # atol floors the scale
        if rl > rel_l2:
            raise AssertionError("%s: relative L2 error %.4g > %.4g" % (name, rl, rel_l2))
    bound = atol + rtol * ref.abs()
    bad = err > bound
    if float(bad.sum()) > outlier_frac * bad.numel():
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError("%s: %d/%d mismatches, max err %.4g (ref max %.4g), first at %s got %.6g ref %.6g" %
                             (name, int(bad.sum()), bad.numel(), float(err.max()), float(ref.abs().max()), idx,
                              float(got[tuple(idx)]), float(ref[tuple(idx)])))


# ---- Squeeze-and-Excitation kernel tests (tests/test_se_gpu.py, test_se_family_gpu.py, test_se_reference.py)
def se_layout(widths):
    """branch widths -> (HT, total, cmap, segments[(padded offset, real offset, width)]): every branch in a segment of whole 16-channel
    slabs, cmap[padded channel] = column of the reference's SE weights or -1"""
    segs, o, st = [], 0, 0
    for h in widths:
        segs.append((o, st, h))
        o += (h + 15) // 16 * 16
        st += h
    cmap = torch.full((o,), -1, dtype=torch.int32)
    for sg, s0, h in segs:
        cmap[sg:sg + h] = torch.arange(s0, s0 + h, dtype=torch.int32)
    return o, st, cmap, segs


def se_pack(w1, w2, b2, cmap, HT):
    """the gate's dense layers packed over the padded layout: w1p [hid][HT], w2t [hid][HT], b2p [HT], zeros on padding"""
    hid = w1.shape[0]
    valid = cmap >= 0
    idx = cmap[valid].long()
    w1p = torch.zeros(hid, HT, dtype=torch.float32)
    w2t = torch.zeros(hid, HT, dtype=torch.float32)
    b2p = torch.zeros(HT, dtype=torch.float32)
    w1p[:, valid] = w1[:, idx]
    w2t[:, valid] = w2[idx, :].t()
    b2p[valid] = b2[idx]
    return w1p, w2t, b2p


def se_sequence64(c, D, dS):
    """float64 values of the whole SE sequence (csrc/se.hip) on the REAL channels, every derivative written out (act_grad64):
    D, dS [M, total] raw depthwise output and the gradient of S; c carries N, HW, act, se_act, sc, sh (real channels) and w1, b1, w2, b2.
    g is the gradient with respect to the pre-activation a = D sc + sh."""
    import types
    N, HW = c.N, c.HW
    w1, b1, w2, b2 = (t.double() for t in (c.w1, c.b1, c.w2, c.b2))
    r = types.SimpleNamespace()
    r.a = D * c.sc.double() + c.sh.double()
    A = act64(r.a, c.act)
    r.pooled = A.view(N, HW, -1).mean(1)
    r.hpre = r.pooled @ w1.t() + b1
    r.hact = act64(r.hpre, c.se_act)
    r.gate = torch.sigmoid(r.hact @ w2.t() + b2)
    gm = r.gate.repeat_interleave(HW, 0)
    r.S = A * gm
    r.dgate = (dS * A).view(N, HW, -1).sum(1)
    r.dz2 = r.dgate * r.gate * (1 - r.gate)
    r.dz1 = act_grad64(r.hpre, c.se_act) * (r.dz2 @ w2)
    r.dpooled = r.dz1 @ w1
    r.g = act_grad64(r.a, c.act) * (dS * gm + r.dpooled.repeat_interleave(HW, 0) / HW)
    r.dw1, r.db1 = r.dz1.t() @ r.pooled, r.dz1.sum(0)
    r.dw2, r.db2 = r.dz2.t() @ r.hact, r.dz2.sum(0)
    return r


def se_reference(N, HW, widths, hid, act, se_act, dtype, seed=0):
    """Inputs and float64 results of one SE case.  Padded [M, HT] / [HT] tensors (padding zero): D, dS (float64 values exact in `dtype`),
    scale, shift.  Real-channel tensors: w1 [hid, total], b1, w2 [total, hid], b2, the base values `base` of the four gradient
    accumulators, and every result of se_sequence64 plus g_stored (g rounded to `dtype`) and stats = [sum g_stored, sum g_stored D].
    The pre-activations of the block come from glue_util.margin_input (amp 2.5): none within 2^-6 of 0 (or 6 in mode 2), so no mask can
    flip in fp32; a mode-2 case has at least 5 % of them above 6 and 5 % below 0.  With a ReLU gate the hidden pre-activations stay
    1e-4 away from 0 (the seed is advanced until they do).  Shared between tests: never modified."""
    import types
    import glue_util as G
    HT, total, cmap, segs = se_layout(widths)
    M = N * HW
    valid = cmap >= 0
    idx = valid.nonzero().flatten()
    for attempt in range(64):
        gen = torch.Generator().manual_seed(100003 * seed + 8191 * attempt + 131 * N + 17 * HW + HT + 7 * act + 3 * se_act)
        c = types.SimpleNamespace(N=N, HW=HW, M=M, widths=list(widths), hid=hid, act=act, se_act=se_act, dtype=dtype, HT=HT, total=total,
                                  cmap=cmap, valid=valid, idx=idx)
        c.sc = torch.rand(total, generator=gen) + 0.5
        c.sh = torch.randn(total, generator=gen) * 0.3
        z = G.margin_input(gen, M, total, c.sc, c.sh, act, dtype, amp=2.5)
        dSr = torch.randn(M, total, generator=gen).to(dtype).double()
        c.w1 = torch.randn(hid, total, generator=gen) / total ** 0.5
        c.b1 = torch.randn(hid, generator=gen) * 0.1
        c.w2 = torch.randn(total, hid, generator=gen) / hid ** 0.5
        c.b2 = torch.randn(total, generator=gen) * 0.1
        c.base = [torch.randn(hid * total, generator=gen), torch.randn(hid, generator=gen), torch.randn(total * hid, generator=gen),
                  torch.randn(total, generator=gen)]
        c.ref = se_sequence64(c, z, dSr)
        if se_act not in (1, 2) or float(c.ref.hpre.abs().min()) >= 1e-4:
            break
    else:
        raise AssertionError("no seed keeps the hidden pre-activations away from 0")
    if act == 2:
        assert float((c.ref.a > 6).double().mean()) >= 0.05 and float((c.ref.a < 0).double().mean()) >= 0.05, "ReLU6 range not straddled"
    c.D, c.dS = torch.zeros(M, HT, dtype=torch.float64), torch.zeros(M, HT, dtype=torch.float64)
    c.D[:, idx], c.dS[:, idx] = z, dSr
    c.scale, c.shift = torch.zeros(HT), torch.zeros(HT)
    c.scale[idx], c.shift[idx] = c.sc, c.sh
    c.ref.g_stored = c.ref.g.to(dtype).double()
    c.ref.stats = torch.stack([c.ref.g_stored.sum(0), (c.ref.g_stored * z).sum(0)])
    return c


# ---- module-level parity tests (tests/test_block_gpu.py, tests/test_block_infer_gpu.py, tests/test_block_infer_se_gpu.py)
def randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.dim() == 1 and "bias" not in n:      # BN gamma
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            else:
                fan = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) / fan ** 0.5)
        for n, b in module.named_buffers():
            if "running_mean" in n:
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif "running_var" in n:
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)


def sd64(module, prefix=""):
    return collections.OrderedDict((prefix + k, (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()))
                                   for k, v in module.state_dict().items())


def widen_bn(module, factor):
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.dim() == 1 and "bias" not in n:
                p.mul_(factor)


# ---- input-pipeline tables (tests/test_input_pipeline_gpu.py, test_preprocess_large_gpu.py, test_color_aug_gpu.py, test_image_store_gpu.py).
# The second opinion on dataflow.batch_plan (tests/test_feed_plan.py): keep it independent of it.
def feed_tables(images, boxes, flips, size, augs=None, base=0):
    """What DevicePrefetcher tells the kernels about a batch of uint8 HWC images (arrays or tensors) -> (offs, desc, aug, large):
    the 16-byte-aligned pool offsets from `base` (n + 1 of them), the DESC_DTYPE records (a batch whose augs carry a resize is a
    window batch: its records describe whole images and `boxes` are windows of the resized ones), the AUG_DTYPE records (None
    without augs) and the slots that need the two-pass launch.  A crop box outside its image is refused (check_box)."""
    import numpy as np
    from atomnas_amd.utils import dataflow as DF
    hw = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    offs = base + np.concatenate([[0], np.cumsum([(H * W * 3 + 15) // 16 * 16 for H, W in hw])])
    window = augs is not None and any(a is not None and a.resize is not None for a in augs)
    desc = np.zeros(len(hw), dtype=DF.DESC_DTYPE)
    aug = None if augs is None else np.zeros(len(hw), dtype=DF.AUG_DTYPE)
    large = []
    for q, ((H, W), box, fl) in enumerate(zip(hw, boxes, flips)):
        if DF.check_window(H, W, augs[q].resize) if window else DF.check_box(H, W, box, size):
            large.append(q)
        desc[q] = (int(offs[q]), H, W) + ((0, 0, H, W) if window else tuple(box)) + (1 if fl else 0, 0)
        if augs is not None:
            DF.fill_aug(aug[q], augs[q], box, size)
    return offs, desc, aug, large


def feed_upload(images, boxes, flips, size, augs=None, pool=None, base=0):
    """feed_tables on the device -> (pool, desc_dev, aug_dev, large): the images packed into `pool` (a fresh zeroed one by default)"""
    import numpy as np
    offs, desc, aug, large = feed_tables(images, boxes, flips, size, augs, base)
    if pool is None:
        pool = torch.zeros(int(offs[-1]), dtype=torch.uint8, device="cuda")
    for q, im in enumerate(images):
        flat = torch.as_tensor(im).reshape(-1)
        pool[int(offs[q]):int(offs[q]) + flat.numel()].copy_(flat)
    dev = lambda t: None if t is None else torch.from_numpy(t.view(np.uint8).copy()).cuda()
    return pool, dev(desc), dev(aug), large


def feed_out(n, size, out_mode):
    """an output buffer of the resize / colour kernels filled with what none of them writes: fp32 NCHW (0), bf16 NHWC pitch 8 (1), uint8 (2)"""
    if out_mode == 2:
        return torch.full((n, size, size, 3), 77, dtype=torch.uint8, device="cuda")
    if out_mode == 1:
        return torch.full((n, size, size, 8), 7.0, dtype=torch.bfloat16, device="cuda")
    return torch.full((n, 3, size, size), float("nan"), dtype=torch.float32, device="cuda")


# ---- deterministic, RNG-free fills shared with tools/make_golden.py (inputs of the golden fixtures are regenerated, not stored)
def counter_fill(t, seed):
    n = t.numel()
    idx = torch.arange(n, dtype=torch.float64)
    v = torch.sin(idx * 12.9898 + seed * 78.233) * 43758.5453
    v = v - torch.floor(v)   # [0, 1)
    return (v - 0.5).reshape(t.shape)


def randomize_counter(module, seed):
    with torch.no_grad():
        for i, (n, p) in enumerate(module.named_parameters()):
            f = counter_fill(p, seed + i)
            if p.dim() == 1 and "bias" not in n:
                p.copy_(f + 1.0)
            elif p.dim() == 1:
                p.copy_(f * 0.4)
            else:
                p.copy_(f * 2.0 / p[0].numel() ** 0.5)
        for i, (n, b) in enumerate(module.named_buffers()):
            if "running_mean" in n:
                b.copy_(counter_fill(b, seed + 1000 + i) * 0.2)
            elif "running_var" in n:
                b.copy_(counter_fill(b, seed + 2000 + i) + 1.0)


def check_digest(name, t, d, rtol=1e-6, atol=0.0):
    """Compares a tensor with the fingerprint stored in a golden fixture (shape, sum, sum of squares, head, tail).  `atol` is an
    absolute per-element floor for tensors that are rounding noise around zero (a BN bias in front of another BN)."""
    f = t.detach().double().cpu().flatten()
    assert tuple(t.shape) == tuple(d["shape"]), (name, tuple(t.shape), d["shape"])
    scale = max(1.0, abs(d["sum"]), d["sumsq"] ** 0.5)
    assert abs(float(f.sum()) - d["sum"]) <= rtol * scale * max(1.0, f.numel() ** 0.5) + atol * f.numel(), (name, float(f.sum()), d["sum"])
    assert abs(float((f * f).sum()) - d["sumsq"]) <= rtol * max(1.0, d["sumsq"]) * 10 + atol * f.numel(), (name, float((f * f).sum()), d["sumsq"])
    s = max(1e-6, float(d["head"].abs().max()), float(d["tail"].abs().max()))
    assert float((f[:4] - d["head"]).abs().max()) <= rtol * 100 * s + 1e-12 + atol, (name, f[:4], d["head"])
    assert float((f[-4:] - d["tail"]).abs().max()) <= rtol * 100 * s + 1e-12 + atol, (name, f[-4:], d["tail"])


def bf16_storage():
    """The oracle's storage model of the bf16 HIP path on THIS library: Bf16Storage, with the depthwise convolutions restated as
    matrix-core ones (fp16 / bf16 MFMA operands, csrc/dwconv_mm.hip) exactly where the library says it runs those kernels."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import atomnas_oracle as orc
    from atomnas_amd import _lib
    lib = _lib.load()

    def pred(k, stride, N, C, H, W, slab):
        if not slab:
            return False, False
        return (bool(lib.atomnas_dwconv_mm_supported(N, H, W, C, k, stride, 1, 0)), bool(lib.atomnas_dwconv_mm_supported(N, H, W, C, k, stride, 1, 1)))
    return orc.bf16_storage_mm(pred)
