"""Kernel-level parity (GPU) of the depthwise 9 x 9 / 11 x 11 family (csrc/dwconv_big.hip) behind atomnas_dwconv_fwd / atomnas_dwconv_bwd.

Style, helpers and tolerances of tests/test_kernels_gpu.py (test_dwconv_fwd / test_dwconv_bwd), unchanged: inputs are rounded to the
storage type, the reference is torch float64 F.conv2d plus autograd on the CPU, and the kernel must agree to one output rounding (bf16)
or accumulation order (fp32).  The 81- / 121-term sums did not need a wider bound.  Statistics buffers arrive as NaN: every partial row
has to be written.  The shapes: a map smaller than the kernel, ragged channels below and above a slab, a non-square map, several slabs,
several tiles with odd extents under stride 2.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from kutil import assert_close, cvec, from_act, pad8, rounded, to_act, tol

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
SHAPES = [(2, 1, 7, 7), (3, 13, 15, 15), (2, 32, 8, 14), (1, 70, 28, 28), (2, 24, 44, 37)]
KS = list(itertools.product([9, 11], [1, 2]))


def _ops():
    from atomnas_amd import ops
    return ops


def fresh(M, C, dtype):
    """output buffer as the allocator hands it out: padding channels zero, the valid region poisoned"""
    b = torch.zeros(M, pad8(C), dtype=dtype, device="cuda")
    b[:, :C] = 7.0
    return b


def poisoned_stats(rows, C):
    """partial-row statistics buffer as the contract allows it to arrive: uninitialised (here NaN)"""
    return torch.full((rows, 2, C), float("nan"), dtype=torch.float32, device="cuda")


def taps(w):  # [C,1,k,k] -> [k*k][pad8(C)] fp32 on GPU
    C, _, k, _ = w.shape
    t = torch.zeros(k * k, pad8(C), dtype=torch.float32, device="cuda")
    t[:, :C] = w.reshape(C, k * k).t().float().cuda()
    return t


def act64(pre, mode):
    if mode == 0:
        return pre
    if mode == 1:
        return torch.relu(pre)
    if mode == 2:
        return torch.clamp(pre, 0.0, 6.0)
    return pre * torch.sigmoid(pre)


def out_hw(H, W, k, stride):
    P = (k - 1) // 2
    return (H + 2 * P - k) // stride + 1, (W + 2 * P - k) // stride + 1


def fwd_inputs(N, C, H, W, k, stride, gain=1.0):
    g = torch.Generator().manual_seed(1000 * k + 10 * stride + C)
    x = torch.randn(N, C, H, W, generator=g) * gain
    w = torch.randn(C, 1, k, k, generator=g) * 0.3
    sc = torch.rand(C, generator=g) + 0.5
    sh = torch.randn(C, generator=g) * 0.3
    return x, w, sc, sh


def fwd_ref(x, w, sc, sh, dtype, k, stride, mode):
    """mode None: no prologue at all; otherwise act_mode(x * sc + sh)"""
    xr = rounded(x, dtype)
    xa = xr if mode is None else act64(xr * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), mode)
    return F.conv2d(xa, w.double(), None, stride, (k - 1) // 2, 1, x.shape[1])


def run_fwd(x, w, sc, sh, dtype, k, stride, mode, rows=64, slab=False, with_stats=True):
    """-> (y buffer [M, pad] plain, statistics buffer or None)"""
    ops = _ops()
    N, C, H, W = x.shape
    Ho, Wo = out_hw(H, W, k, stride)
    xb, yb = to_act(x, dtype), fresh(N * Ho * Wo, C, dtype)
    if slab:
        xb, yb = ops.Slab.from_plain(xb, C), ops.Slab.from_plain(yb, C)
    stats = poisoned_stats(rows, C) if with_stats else None
    fused = mode is not None
    ops.dwconv_fwd(xb, cvec(sc) if fused else None, cvec(sh) if fused else None, mode if fused else 0, taps(w), yb, stats, C, N, H, W, C, k,
                   stride)
    torch.cuda.synchronize()
    return (yb.to_plain() if slab else yb), stats


def check_fwd(x, w, sc, sh, dtype, k, stride, mode, rows=64):
    N, C, H, W = x.shape
    Ho, Wo = out_hw(H, W, k, stride)
    yref = fwd_ref(x, w, sc, sh, dtype, k, stride, mode)
    yb, stats = run_fwd(x, w, sc, sh, dtype, k, stride, mode, rows)
    y = from_act(yb, N, Ho, Wo, C)
    assert_close("y", y, yref, **tol(dtype))
    assert float(yb[:, C:].abs().max() if pad8(C) > C else 0) == 0.0
    assert bool(torch.isfinite(stats).all()), "a partial row was left unwritten"
    stats = stats.sum(0)
    assert_close("sum", stats[0], y.sum((0, 2, 3)), rtol=1e-4, atol=1e-3)
    assert_close("sumsq", stats[1], (y * y).sum((0, 2, 3)), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,stride", KS)
@pytest.mark.parametrize("N,C,H,W", SHAPES)
def test_dwconv_big_fwd(gpu_lib, dtype, k, stride, N, C, H, W):
    x, w, sc, sh = fwd_inputs(N, C, H, W, k, stride)
    for mode in (None, 1):   # no prologue / fused BatchNorm apply + ReLU
        check_fwd(x, w, sc, sh, dtype, k, stride, mode)


def bwd_inputs(N, C, H, W, k, stride, gain=1.0):
    g = torch.Generator().manual_seed(2000 * k + 10 * stride + C)
    Ho, Wo = out_hw(H, W, k, stride)
    d = dict(x=torch.randn(N, C, H, W, generator=g) * gain, w=torch.randn(C, 1, k, k, generator=g) * 0.3,
             sc=torch.rand(C, generator=g) + 0.5, sh=torch.randn(C, generator=g) * 0.3,
             gup=torch.randn(N, C, Ho, Wo, generator=g), yraw=torch.randn(N, C, Ho, Wo, generator=g),
             c1=torch.rand(C, generator=g) + 0.5, c2=torch.randn(C, generator=g) * 0.1, c3=torch.randn(C, generator=g) * 0.1)
    return d


def bwd_ref(d, dtype, k, stride, mode):
    """-> (h, dw): mode None = no prologue, no BatchNorm backward; otherwise both fused, activation `mode`"""
    v = lambda t: t.double().view(1, -1, 1, 1)
    C = d["x"].shape[1]
    xr = rounded(d["x"], dtype).requires_grad_(True)
    xa = xr if mode is None else act64(xr * v(d["sc"]) + v(d["sh"]), mode)
    wd = d["w"].double().requires_grad_(True)
    y = F.conv2d(xa, wd, None, stride, (k - 1) // 2, 1, C)
    dy = rounded(d["gup"], dtype) if mode is None else v(d["c1"]) * rounded(d["gup"], dtype) + v(d["c2"]) * rounded(d["yraw"], dtype) + v(d["c3"])
    (y * dy).sum().backward()
    # xr.grad = dwconv^T(dY) * act'(pre) * sc: the kernel's h stops in front of the scale
    href = xr.grad if mode is None else xr.grad / v(d["sc"])
    return href, wd.grad


def run_bwd(d, dtype, k, stride, mode, rows=64, slab=False, with_dw=True, with_stats=True, with_yraw=True):
    """-> (h buffer [M, pad] plain, dw [C, k*k] or None, statistics buffer or None)"""
    ops = _ops()
    N, C, H, W = d["x"].shape
    fused = mode is not None
    lay = (lambda t: ops.Slab.from_plain(t, C)) if slab else (lambda t: t)
    bn = fused and with_yraw
    hb = lay(fresh(N * H * W, C, dtype))
    dw = torch.zeros(C, k * k, dtype=torch.float32, device="cuda") if with_dw else None
    stats = poisoned_stats(rows, C) if with_stats else None
    ops.dwconv_bwd(lay(to_act(d["gup"], dtype)), lay(to_act(d["yraw"], dtype)) if bn else None, cvec(d["c1"]) if bn else None,
                   cvec(d["c2"]) if bn else None, cvec(d["c3"]) if bn else None, lay(to_act(d["x"], dtype)), cvec(d["sc"]) if fused else None,
                   cvec(d["sh"]) if fused else None, mode if fused else 0, taps(d["w"]), hb, dw, stats, C, N, H, W, C, k, stride,
                   stat_rows=None if with_stats else rows)
    torch.cuda.synchronize()
    return (hb.to_plain() if slab else hb), dw, stats


def check_bwd(d, dtype, k, stride, mode, rows=64):
    N, C, H, W = d["x"].shape
    href, dwref = bwd_ref(d, dtype, k, stride, mode)
    hb, dw, stats = run_bwd(d, dtype, k, stride, mode, rows)
    h = from_act(hb, N, H, W, C)
    t = tol(dtype)
    assert_close("h", h, href, t["rtol"], t["atol"] * 4)
    assert float(hb[:, C:].abs().max() if pad8(C) > C else 0) == 0.0
    assert_close("dw", dw.reshape(C, 1, k, k), dwref, rtol=2e-3, atol=2e-3 * float(dwref.abs().max()))
    assert bool(torch.isfinite(stats).all()), "a partial row was left unwritten"
    stats = stats.sum(0)
    assert_close("sum_h", stats[0], h.sum((0, 2, 3)), rtol=1e-4, atol=2e-3)
    assert_close("sum_hx", stats[1], (h * rounded(d["x"], dtype)).sum((0, 2, 3)), rtol=1e-4, atol=2e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,stride", KS)
@pytest.mark.parametrize("N,C,H,W", SHAPES)
def test_dwconv_big_bwd(gpu_lib, dtype, k, stride, N, C, H, W):
    d = bwd_inputs(N, C, H, W, k, stride)
    for mode in (None, 1):   # plain / fused prologue (BatchNorm apply + ReLU) and BatchNorm backward
        check_bwd(d, dtype, k, stride, mode)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("k,stride", [(9, 2), (11, 1)])
def test_relu6_and_swish(gpu_lib, dtype, mode, k, stride):
    """activation modes 2 and 3 in the prologue (forward) and as the derivative (backward); inputs wide enough to reach ReLU6's 6"""
    N, C, H, W = 3, 13, 15, 15
    x, w, sc, sh = fwd_inputs(N, C, H, W, k, stride, gain=4.0)
    check_fwd(x, w, sc, sh, dtype, k, stride, mode)
    check_bwd(bwd_inputs(N, C, H, W, k, stride, gain=4.0), dtype, k, stride, mode)


@pytest.mark.parametrize("k,stride", KS)
def test_three_partial_rows(gpu_lib, k, stride):
    """stat_rows = part_rows = 3: three workers per slab walk many tiles each"""
    N, C, H, W = 4, 16, 28, 28
    x, w, sc, sh = fwd_inputs(N, C, H, W, k, stride)
    check_fwd(x, w, sc, sh, torch.bfloat16, k, stride, 1, rows=3)
    check_bwd(bwd_inputs(N, C, H, W, k, stride), torch.bfloat16, k, stride, 1, rows=3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,stride", KS)
def test_slab_major_equals_plain(gpu_lib, dtype, k, stride):
    """the layout changes addresses only: slab-major operands give the bits of plain ones"""
    N, C, H, W = 2, 40, 14, 14
    x, w, sc, sh = fwd_inputs(N, C, H, W, k, stride)
    yp, sp = run_fwd(x, w, sc, sh, dtype, k, stride, 1)
    ys, ss = run_fwd(x, w, sc, sh, dtype, k, stride, 1, slab=True)
    assert torch.equal(yp[:, :C], ys[:, :C]) and torch.equal(sp, ss)
    assert float(ys[:, C:].float().abs().max()) == 0.0
    d = bwd_inputs(N, C, H, W, k, stride)
    hp, dwp, sp = run_bwd(d, dtype, k, stride, 1)
    hs, dws, ss = run_bwd(d, dtype, k, stride, 1, slab=True)
    assert torch.equal(hp[:, :C], hs[:, :C]) and torch.equal(dwp, dws) and torch.equal(sp, ss)


@pytest.mark.parametrize("k,stride", KS)
def test_two_calls_are_bit_identical(gpu_lib, k, stride):
    N, C, H, W = 1, 70, 28, 28
    x, w, sc, sh = fwd_inputs(N, C, H, W, k, stride)
    a, b = run_fwd(x, w, sc, sh, torch.bfloat16, k, stride, 1), run_fwd(x, w, sc, sh, torch.bfloat16, k, stride, 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    d = bwd_inputs(N, C, H, W, k, stride)
    a, b = run_bwd(d, torch.float32, k, stride, 1), run_bwd(d, torch.float32, k, stride, 1)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("k,stride", [(9, 1), (11, 2)])
def test_null_forms(gpu_lib, k, stride):
    """dw, stats and yraw may be absent: the other results do not move"""
    N, C, H, W = 3, 13, 15, 15
    dtype = torch.float32
    d = bwd_inputs(N, C, H, W, k, stride)
    h, dw, st = run_bwd(d, dtype, k, stride, 1)
    h1, dw1, st1 = run_bwd(d, dtype, k, stride, 1, with_dw=False)
    assert dw1 is None and torch.equal(h1, h) and torch.equal(st1, st)
    h2, dw2, st2 = run_bwd(d, dtype, k, stride, 1, with_stats=False)
    assert st2 is None and torch.equal(h2, h) and torch.equal(dw2, dw)
    h3, dw3, st3 = run_bwd(d, dtype, k, stride, 1, with_dw=False, with_stats=False)
    assert torch.equal(h3, h)
    # yraw == NULL: dYraw = g, the prologue of x stays
    h4, dw4, st4 = run_bwd(d, dtype, k, stride, 1, with_yraw=False)
    v = lambda t: t.double().view(1, -1, 1, 1)
    xr = rounded(d["x"], dtype).requires_grad_(True)
    wd = d["w"].double().requires_grad_(True)
    y = F.conv2d(torch.relu(xr * v(d["sc"]) + v(d["sh"])), wd, None, stride, (k - 1) // 2, 1, C)
    (y * rounded(d["gup"], dtype)).sum().backward()
    assert_close("h", from_act(h4, N, H, W, C), xr.grad / v(d["sc"]), tol(dtype)["rtol"], tol(dtype)["atol"] * 4)
    assert_close("dw", dw4.reshape(C, 1, k, k), wd.grad, rtol=2e-3, atol=2e-3 * float(wd.grad.abs().max()))
    assert bool(torch.isfinite(st4).all())
    # forward without statistics
    x, w, sc, sh = fwd_inputs(N, C, H, W, k, stride)
    y0, _ = run_fwd(x, w, sc, sh, dtype, k, stride, 1)
    y1, s1 = run_fwd(x, w, sc, sh, dtype, k, stride, 1, with_stats=False)
    assert s1 is None and torch.equal(y0, y1)


@pytest.mark.parametrize("k", [13, 4])
def test_other_kernel_sizes_still_raise(gpu_lib, k):
    from atomnas_amd._lib import AtomnasHipError
    ops = _ops()
    N, C, H, W = 1, 8, 16, 16
    x = torch.zeros(N * H * W, C, device="cuda")
    y = torch.zeros(N * H * W, C, device="cuda")
    w = torch.zeros(k * k, C, device="cuda")
    with pytest.raises(AtomnasHipError, match="dwconv_fwd: unsupported k=%d" % k):
        ops.dwconv_fwd(x, None, None, 0, w, y, None, C, N, H, W, C, k, 1)
    with pytest.raises(AtomnasHipError, match="dwconv_bwd: unsupported k=%d" % k):
        ops.dwconv_bwd(x, None, None, None, None, x, None, None, 0, w, y, None, None, C, N, H, W, C, k, 1)
