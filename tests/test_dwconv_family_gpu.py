"""Kernel-level parity (GPU) of the depthwise k = 3 / 5 / 7 kernels behind atomnas_dwconv_fwd / atomnas_dwconv_bwd, per kernel family
(csrc/dwconv.hip tile kernels, dwconv_cw.hip channel-pair kernels stride 1 and stride-2 backward, dwconv_mm.hip matrix cores), per
activation instance (none behind a BatchNorm, ReLU, ReLU6, Swish) and per call form, in the manner of tests/test_dwconv_big_gpu.py.

Every case names the family it is written for and asserts it (kutil.family) before it launches: a dispatch change fails the case
instead of letting it check another kernel.  The kernels behind the non-default bits of ATOMNAS_DW_MM (read once per process) run in
child interpreters (test_dw_mm_0_runs_cw, test_dw_mm_255_runs_mm_backward; their cases skip in a process without the switch).

Reference: float64 torch on the CPU from inputs rounded to the storage type.  y = conv2d(act(x sc + sh), w); dy = c1 g + c2 yraw + c3
(g without yraw); h = dwconv^T(dy) act'(pre) = x.grad / sc (x.grad without a prologue); dw from autograd; the statistics against the
sums of the STORED y and h.  x comes from glue_util.margin_input: every pre-activation is at least 2^-6 from 0 (and from 6 in mode 2)
after the rounding, so no element may flip a mask and no outliers are allowed; mode-2 cases assert that at least 5 % of the
pre-activations lie above 6 and 5 % below 0.

Bounds.  y, h and the statistics: kutil.tol(dtype) (atol x 4 for h), rtol 1e-4 with atol 1e-3 (forward) / 2e-3 (backward), as
tests/test_kernels_gpu.py.  dw: with u = 2^-24, n output pixels per channel and S = sum |dy act(pre)| per tap in float64,
    tile, cw, cw2 (either storage type)   |dw - ref| <= (n + 24) u S      glue_util.sum_bound + 8 u per factor (both are computed in
                                                                          fp32 from stored values; storage rounding does not enter)
    mm backward                           + 2 * 2^-9 S                    the two bf16 operand roundings of dwconv_mm.hip
    Swish                                 the 8 u of the activated factor times SWISH_FWD_K (measured, tests/test_bn_kernels_gpu.py)
Largest observed error / bound per family on an MI355X (printed with -s, the children's figures by their parents):
    tile 0.0053    cw 0.0097 (ATOMNAS_DW_MM=0: 0.0016)    cw2 0.0014    mm backward 0.12 (k = 7 ring; ATOMNAS_DW_MM=255, k = 3 / 5 / 7: 0.29)
The fp32 sums stay two orders of magnitude inside the bound (n u S is the worst case of a sum whose error grows like sqrt(n)); the mm
figure is the 2^-9 term, a worst case of two independent roundings per product.

Wrong activations these tests were seen to catch (tried on scratch builds of the library, never committed):
  ReLU6's upper bound 5 in every forward activation (cw_act, cw_clamp16_bounds, the tile kernels' inline clamps)
      -> every mode-2 case of test_parity (the backward-only cw2 rows through dw), every mode-2 case of test_exact_boundaries, both children
  `a < 6` dropped from the ReLU6 mask (cw_act_bwd, the tile backward's inline mask)
      -> every mode-2 case of test_parity, every mode-2 backward case of test_exact_boundaries, both children
  `a < 5` in the same masks
      -> every mode-2 case of test_parity and both children (test_exact_boundaries cannot: none of its values lies in [5, 6))

Exact boundaries (test_exact_boundaries): x in {-1, 0, 0.5, 6, 7}, sc = 1, sh = 0, taps in {+-0.5, +-0.25}, g = 1.  h must be exactly 0
where x <= 0 and, in mode 2, where x >= 6 (torch's convention, tests/glue_ref.py).  Everything else is required EXACTLY as well: every
operand is exact in bf16 and fp16, every product exact in fp32, and every partial sum a multiple of 2^-3 (y), 2^-2 (h), 2^-1 (dw) far
below 2^24 of them, so no summation order can round; h (|h| < 64, multiples of 1/4) is exact in bf16, y is the reference rounded once.
"""
import functools
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import glue_util as G
from glue_util import U
from kutil import act64, assert_close, counter_fill, cvec, family, fresh, from_act, out_hw, taps, to_act, tol
from test_bn_kernels_gpu import SWISH_FWD_K

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DW_MM = os.environ.get("ATOMNAS_DW_MM")
RATIO = {}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if RATIO:
        print("\ndw: largest error / derived bound:", {k: round(v, 4) for k, v in sorted(RATIO.items())})


def _ops():
    from atomnas_amd import ops
    return ops


def _name(dtype):
    return "fp32" if dtype == F32 else "bf16"


def _v(t):
    return t.double().view(1, -1, 1, 1)


def _finish(c):
    """the float64 reference of a case: y, h, dw and the per-tap sums S of |dy act(pre)|"""
    C, k, P = c.C, c.k, (c.k - 1) // 2
    xr = c.x.clone().requires_grad_(True)
    pre = xr * _v(c.sc) + _v(c.sh) if c.prologue else xr
    xa = act64(pre, c.mode)
    xa.retain_grad()
    wd = c.w.double().requires_grad_(True)
    y = F.conv2d(xa, wd, None, c.stride, P, 1, C)
    dy = _v(c.c1) * c.gup + _v(c.c2) * c.yraw + _v(c.c3) if c.bn else c.gup
    (y * dy).sum().backward()
    c.pre, c.yref, c.dwref, c.dxa = pre.detach(), y.detach(), wd.grad, xa.grad
    c.href = xr.grad / _v(c.sc) if c.prologue else xr.grad
    w0 = torch.zeros_like(c.w, dtype=torch.float64).requires_grad_(True)
    (F.conv2d(xa.detach().abs(), w0, None, c.stride, P, 1, C) * dy.abs()).sum().backward()
    c.S = w0.grad
    return c


def _shape(N, C, H, W, k, stride, dtype, mode, prologue, bn):
    Ho, Wo = out_hw(H, W, k, stride)
    return types.SimpleNamespace(N=N, C=C, H=H, W=W, k=k, stride=stride, dtype=dtype, mode=mode, prologue=prologue, bn=bn, Ho=Ho, Wo=Wo)


@functools.lru_cache(maxsize=None)
def case(N, C, H, W, k, stride, dtype, mode, prologue=True, bn=True):
    """inputs (CPU, float64 values exact in `dtype`; taps and per-channel vectors fp32) and reference of one case; shared, never modified"""
    c = _shape(N, C, H, W, k, stride, dtype, mode, prologue, bn)
    gen = torch.Generator().manual_seed(7000 * k + 100 * stride + 10 * mode + C + H + (0 if prologue else 5) + (0 if bn else 3))
    c.w = torch.randn(C, 1, k, k, generator=gen) * 0.3
    c.sc = torch.rand(C, generator=gen) + 0.5 if prologue else torch.ones(C)
    c.sh = torch.randn(C, generator=gen) * 0.3 if prologue else torch.zeros(C)
    z = G.margin_input(gen, N * H * W, C, c.sc, c.sh, mode, dtype, amp=3.0)
    c.x = z.reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous()
    c.gup = torch.randn(N, C, c.Ho, c.Wo, generator=gen).to(dtype).double()
    c.yraw = torch.randn(N, C, c.Ho, c.Wo, generator=gen).to(dtype).double()
    c.c1, c.c2, c.c3 = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.1, torch.randn(C, generator=gen) * 0.1
    return _finish(c)


@functools.lru_cache(maxsize=None)
def edge_case(N, C, H, W, k, stride, dtype, mode):
    """the exact-boundary case of the module docstring"""
    c = _shape(N, C, H, W, k, stride, dtype, mode, True, False)
    vals = torch.tensor([-1.0, 0.0, 0.5, 6.0, 7.0], dtype=torch.float64)
    i = ((counter_fill(torch.empty(N, C, H, W), 11 + k) + 0.5) * 5).long().clamp(0, 4)
    c.x = vals[i]
    assert all(int((i == j).sum()) > 0 for j in range(5))
    tv = torch.tensor([0.5, -0.5, 0.25, -0.25])
    c.w = tv[((counter_fill(torch.empty(C, 1, k, k), 5 + k) + 0.5) * 4).long().clamp(0, 3)]
    c.sc, c.sh = torch.ones(C), torch.zeros(C)
    c.gup = torch.ones(N, C, c.Ho, c.Wo, dtype=torch.float64)
    c.yraw = c.c1 = c.c2 = c.c3 = None
    return _finish(c)


def _lay(slab, C):
    from atomnas_amd.ops import Slab
    return (lambda t: Slab.from_plain(t, C)) if slab else (lambda t: t)


def _stats(rows, C, stat_ld):
    """partial rows [rows][2][stat_ld] as the contract allows them to arrive: uninitialised (here NaN)"""
    return torch.full((rows, 2, stat_ld or C), float("nan"), dtype=torch.float32, device="cuda")


def run_fwd(c, slab, rows=64, with_stats=True, stat_ld=None):
    """-> (y buffer [M, pad] plain, statistics buffer or None)"""
    ops, lay = _ops(), _lay(slab, c.C)
    yb = lay(fresh(c.N * c.Ho * c.Wo, c.C, c.dtype))
    stats = _stats(rows, c.C, stat_ld) if with_stats else None
    ops.dwconv_fwd(lay(to_act(c.x, c.dtype)), cvec(c.sc) if c.prologue else None, cvec(c.sh) if c.prologue else None, c.mode, taps(c.w), yb,
                   stats, stat_ld or c.C, c.N, c.H, c.W, c.C, c.k, c.stride)
    torch.cuda.synchronize()
    return (yb.to_plain() if slab else yb), stats


def run_bwd(c, slab, rows=64, with_dw=True, with_stats=True, stat_ld=None):
    """-> (h buffer [M, pad] plain, dw [C, k*k] or None, statistics buffer or None); without statistics ops.dwconv_bwd sizes the
    weight-gradient partials by ops.stat_rows_for(C), whatever `rows` says"""
    ops, lay = _ops(), _lay(slab, c.C)
    hb = lay(fresh(c.N * c.H * c.W, c.C, c.dtype))
    dw = torch.zeros(c.C, c.k * c.k, dtype=torch.float32, device="cuda") if with_dw else None
    stats = _stats(rows, c.C, stat_ld) if with_stats else None
    ops.dwconv_bwd(lay(to_act(c.gup, c.dtype)), lay(to_act(c.yraw, c.dtype)) if c.bn else None, cvec(c.c1) if c.bn else None,
                   cvec(c.c2) if c.bn else None, cvec(c.c3) if c.bn else None, lay(to_act(c.x, c.dtype)), cvec(c.sc) if c.prologue else None,
                   cvec(c.sh) if c.prologue else None, c.mode, taps(c.w), hb, dw, stats, stat_ld or c.C, c.N, c.H, c.W, c.C, c.k, c.stride)
    torch.cuda.synchronize()
    return (hb.to_plain() if slab else hb), dw, stats


def _spread(c):
    if c.mode == 2:   # the clamp is really exercised on both sides
        assert float((c.pre > 6).double().mean()) >= 0.05 and float((c.pre < 0).double().mean()) >= 0.05


def _padding_is_zero(buf, C):
    assert float(buf[:, C:].float().abs().max() if buf.shape[1] > C else 0) == 0.0, "padding channels are not zero"


def _check_stats(names, stats, C, refs, atol):
    assert bool(torch.isfinite(stats[:, :, :C]).all()), "a partial row was left unwritten"
    if stats.shape[2] > C:
        assert bool(torch.isnan(stats[:, :, C:]).all()), "a write into statistics columns >= C"
    s = stats[:, :, :C].sum(0)
    for i in (0, 1):
        assert_close(names[i], s[i], refs[i], rtol=1e-4, atol=atol)


def assert_family(lib, c, slab, dirn, fam):
    got = family(lib, c.N, c.H, c.W, c.C, c.k, c.stride, c.dtype, dirn, slab)
    assert got == fam, "%s of N%d C%d H%d W%d k%d s%d %s runs the %s kernels, this case is written for %s" % (
        "backward" if dirn else "forward", c.N, c.C, c.H, c.W, c.k, c.stride, _name(c.dtype), got, fam)


def check_fwd(lib, c, slab, fam, rows=64, stat_ld=None):
    assert_family(lib, c, slab, 0, fam)
    _spread(c)
    yb, stats = run_fwd(c, slab, rows, True, stat_ld)
    y = from_act(yb, c.N, c.Ho, c.Wo, c.C)
    assert_close("y", y, c.yref, **tol(c.dtype))
    _padding_is_zero(yb, c.C)
    _check_stats(("sum", "sumsq"), stats, c.C, (y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))), 1e-3)
    return yb, stats


def dw_bound(c, fam):
    """the module docstring's bound of the weight gradient"""
    n = c.N * c.Ho * c.Wo
    b = (n + 8 + 8 + 8 * (SWISH_FWD_K if c.mode == 3 else 1.0)) * U * c.S
    return b + 2 * 2.0 ** -9 * c.S if fam == "mm" else b


def check_dw(c, fam, dw):
    bound = dw_bound(c, fam)
    err = (dw.double().cpu().reshape(c.C, 1, c.k, c.k) - c.dwref).abs()
    ok = bound > 0
    key = "cw2" if fam == "cw" and c.stride == 2 else fam
    RATIO[key] = max(RATIO.get(key, 0.0), float((err[ok] / bound[ok]).max()))
    G.assert_within("dw", dw.reshape(c.C, 1, c.k, c.k), c.dwref, bound + G.TINY)


def check_bwd(lib, c, slab, fam, rows=64, stat_ld=None, with_stats=True):
    assert_family(lib, c, slab, 1, fam)
    _spread(c)
    hb, dw, stats = run_bwd(c, slab, rows, True, with_stats, stat_ld)
    h = from_act(hb, c.N, c.H, c.W, c.C)
    t = tol(c.dtype)
    assert_close("h", h, c.href, t["rtol"], t["atol"] * 4)
    _padding_is_zero(hb, c.C)
    check_dw(c, fam, dw)
    if with_stats:
        _check_stats(("sum_h", "sum_hx"), stats, c.C, (h.sum((0, 2, 3)), (h * c.x).sum((0, 2, 3))), 2e-3)
    return hb, dw, stats


# ---------------------------------------------------------------------------------------------------------------- parity per family
# (label, family forward or None, family backward, slab-major, storage type, (N, C, H, W), k, stride)
def _parity_rows():
    rows = []
    for dt in (F32, BF16):
        for k in (3, 5, 7):
            for s in (1, 2):
                rows.append(("tile", "tile", "tile", False, dt, (3, 13, 15, 15), k, s))
    rows.append(("tile-slab", "tile", "tile", True, BF16, (2, 24, 12, 12), 5, 1))      # W % 7 != 0: neither cw nor mm
    for k in (3, 5, 7):
        rows.append(("cw-whole", "cw", "cw", True, F32, (3, 13, 14, 14), k, 1))       # NI = 2, the last tile half empty
        for dt in (F32, BF16):
            rows.append(("cw-ring", "cw", "cw", True, dt, (2, 16, 44, 28), k, 1))     # odd ring-tile height: mm declines
            rows.append(("cw2-whole", None, "cw", True, dt, (3, 13, 28, 28), k, 2))   # (no stride-2 forward in the cw family)
    rows.append(("cw2-ring", None, "cw", True, BF16, (2, 16, 88, 56), 7, 2))
    for shape in ((3, 24, 7, 7), (3, 13, 14, 14), (2, 13, 21, 21)):                   # 1 / 2 / 3 MFMA groups, whole images
        for k in (5, 7):
            rows.append(("mm-whole", "mm", "cw", True, BF16, shape, k, 1))            # (their backward: cw in bf16, whole images)
    for k in (5, 7):
        rows.append(("mm-ring", "mm", "mm" if k == 7 else "cw", True, BF16, (2, 13, 28, 28), k, 1))   # backward k = 7: MAXG = 2
    return rows


def _row_id(r):
    return "%s-%s-%s-k%ds%d" % (r[0], _name(r[4]), "x".join(map(str, r[5])), r[6], r[7])


PARITY = _parity_rows()


@pytest.mark.parametrize("mode", [0, 2, 3])
@pytest.mark.parametrize("row", PARITY, ids=_row_id)
def test_parity(gpu_lib, row, mode):
    """modes 2 and 3, and mode 0 behind a prologue (instance 0 with in_relu = 0), forward and backward"""
    _, ffam, bfam, slab, dtype, shape, k, stride = row
    c = case(*shape, k, stride, dtype, mode)
    if ffam:
        check_fwd(gpu_lib, c, slab, ffam)
    check_bwd(gpu_lib, c, slab, bfam)


# ---------------------------------------------------------------------------------------------------------------- forms
# one per family at its first shape: (label, directions, family, slab-major, storage type, (N, C, H, W), k, stride)
FORMS = [("tile", "fb", "tile", False, F32, (3, 13, 15, 15), 5, 1), ("tile", "fb", "tile", False, BF16, (3, 13, 15, 15), 3, 2),
         ("cw", "fb", "cw", True, F32, (3, 13, 14, 14), 5, 1), ("cw2", "b", "cw", True, BF16, (3, 13, 28, 28), 3, 2),
         ("mm", "f", "mm", True, BF16, (3, 24, 7, 7), 7, 1), ("mm", "fb", "mm", True, BF16, (2, 13, 28, 28), 7, 1)]
form_cases = pytest.mark.parametrize("form", FORMS, ids=_row_id)
bwd_form_cases = pytest.mark.parametrize("form", [f for f in FORMS if "b" in f[1]], ids=_row_id)


@bwd_form_cases
def test_bwd_of_a_plain_depthwise_layer(gpu_lib, form):
    """yraw and c1..c3 but no input prologue, no statistics, dw present: functional.py's call for a non-expanding block and for a
    depthwise ConvBN layer"""
    _, _, fam, slab, dtype, shape, k, stride = form
    check_bwd(gpu_lib, case(*shape, k, stride, dtype, 0, prologue=False), slab, fam, with_stats=False)


@form_cases
def test_absent_outputs_leave_the_others_bit_identical(gpu_lib, form):
    _, dirs, fam, slab, dtype, shape, k, stride = form
    c = case(*shape, k, stride, dtype, 1)
    if "f" in dirs:
        assert_family(gpu_lib, c, slab, 0, fam)
        y, st = run_fwd(c, slab)
        y1, st1 = run_fwd(c, slab, with_stats=False)
        assert st1 is None and torch.equal(y1, y)
    if "b" in dirs:
        assert_family(gpu_lib, c, slab, 1, fam)
        rows = _ops().stat_rows_for(c.C)   # what ops.dwconv_bwd passes as part_rows when there are no statistics
        h, dw, st = run_bwd(c, slab, rows)
        h1, dw1, st1 = run_bwd(c, slab, rows, with_dw=False)
        assert dw1 is None and torch.equal(h1, h) and torch.equal(st1, st)
        h2, dw2, st2 = run_bwd(c, slab, rows, with_stats=False)
        assert st2 is None and torch.equal(h2, h) and torch.equal(dw2, dw)
        h3, dw3, st3 = run_bwd(c, slab, rows, with_dw=False, with_stats=False)
        assert dw3 is None and st3 is None and torch.equal(h3, h)


@form_cases
def test_statistics_pitch_wider_than_C(gpu_lib, form):
    """stat_ld = pad8(C) + 16 (functional.py passes the pitch of the whole hidden tensor): columns >= C stay untouched"""
    _, dirs, fam, slab, dtype, shape, k, stride = form
    c = case(*shape, k, stride, dtype, 1)
    ld = G.pad8(c.C) + 16
    if "f" in dirs:
        check_fwd(gpu_lib, c, slab, fam, stat_ld=ld)
    if "b" in dirs:
        check_bwd(gpu_lib, c, slab, fam, stat_ld=ld)


@pytest.mark.parametrize("form", [("tile", "fb", "tile", False, F32, (3, 13, 15, 15), 7, 1), ("tile", "fb", "tile", False, BF16, (3, 13, 15, 15), 5, 2),
                                  ("cw", "fb", "cw", True, F32, (2, 16, 44, 28), 5, 1), ("cw2", "b", "cw", True, BF16, (2, 16, 88, 56), 7, 2),
                                  ("mm", "fb", "mm", True, BF16, (2, 13, 28, 28), 7, 1)], ids=_row_id)
def test_three_partial_rows(gpu_lib, form):
    """stat_rows = part_rows = 3: every worker walks several tiles and owns one partial row"""
    _, dirs, fam, slab, dtype, shape, k, stride = form
    c = case(*shape, k, stride, dtype, 1)
    if "f" in dirs:
        check_fwd(gpu_lib, c, slab, fam, rows=3)
    check_bwd(gpu_lib, c, slab, fam, rows=3)


@form_cases
def test_two_launches_are_bit_identical(gpu_lib, form):
    _, dirs, fam, slab, dtype, shape, k, stride = form
    c = case(*shape, k, stride, dtype, 3)
    if "f" in dirs:
        assert_family(gpu_lib, c, slab, 0, fam)
        a, b = run_fwd(c, slab), run_fwd(c, slab)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if "b" in dirs:
        assert_family(gpu_lib, c, slab, 1, fam)
        a, b = run_bwd(c, slab), run_bwd(c, slab)
        assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- exact boundaries
EDGES = [("tile", "fb", "tile", False, F32, (3, 13, 15, 15), 3, 1), ("tile", "fb", "tile", False, F32, (3, 13, 15, 15), 3, 2),
         ("tile", "fb", "tile", False, BF16, (3, 13, 15, 15), 5, 1), ("tile", "fb", "tile", False, BF16, (3, 13, 15, 15), 7, 2),
         ("cw", "fb", "cw", True, F32, (3, 13, 14, 14), 3, 1), ("cw", "fb", "cw", True, F32, (3, 13, 14, 14), 5, 1),
         ("cw", "fb", "cw", True, F32, (3, 13, 14, 14), 7, 1), ("cw2", "b", "cw", True, F32, (3, 13, 28, 28), 3, 2),
         ("cw2", "b", "cw", True, BF16, (3, 13, 28, 28), 5, 2), ("cw2", "b", "cw", True, BF16, (3, 13, 28, 28), 7, 2),
         ("mm", "f", "mm", True, BF16, (3, 24, 7, 7), 5, 1), ("mm", "f", "mm", True, BF16, (3, 24, 7, 7), 7, 1),
         ("mm", "fb", "mm", True, BF16, (2, 13, 28, 28), 7, 1)]


def check_edges(lib, form, mode):
    _, dirs, fam, slab, dtype, shape, k, stride = form
    c = edge_case(*shape, k, stride, dtype, mode)
    if "f" in dirs:
        assert_family(lib, c, slab, 0, fam)
        yb, _ = run_fwd(c, slab)
        y = from_act(yb, c.N, c.Ho, c.Wo, c.C)
        assert torch.equal(y, c.yref.to(dtype).double()), "y differs from the (once rounded) exact result: max |diff| %g" % float((y - c.yref).abs().max())
    if "b" in dirs:
        assert_family(lib, c, slab, 1, fam)
        hb, dw, _ = run_bwd(c, slab)
        h = from_act(hb, c.N, c.H, c.W, c.C)
        dead = (c.x <= 0) | ((c.x >= 6) if mode == 2 else torch.zeros_like(c.x, dtype=torch.bool))
        assert bool((h[dead] == 0).all()), "%d gradients passed a closed activation (x <= 0%s)" % (
            int((h[dead] != 0).sum()), " or x >= 6" if mode == 2 else "")
        href = torch.where(dead, torch.zeros_like(c.dxa), c.dxa)
        assert torch.equal(h, href), "h differs from the exact result: max |diff| %g" % float((h - href).abs().max())
        assert torch.equal(dw.double().cpu().reshape(c.C, 1, k, k), c.dwref), "dw differs from the exact result"


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("form", EDGES, ids=_row_id)
def test_exact_boundaries(gpu_lib, form, mode):
    check_edges(gpu_lib, form, mode)


# ---------------------------------------------------------------------------------------------------------------- non-default switches
def _child(marker, value, passed):
    """the cases whose name carries `marker`, in ONE child interpreter with ATOMNAS_DW_MM = value"""
    env = dict(os.environ, ATOMNAS_DW_MM=value)
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-k", marker]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        pytest.exit("the %s child did not end: nothing else is started on the GPU" % marker, returncode=1)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit("the %s child ended by a signal (%d): nothing else is started on the GPU\n%s" % (marker, r.returncode, (r.stdout + r.stderr)[-3000:]),
                    returncode=1)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "%d passed" % passed in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-1000:]
    for line in r.stdout.splitlines():
        if line.startswith("dw: largest"):
            print("\nATOMNAS_DW_MM=%s %s" % (value, line))


MM0 = [(shape, k, mode) for shape in ((3, 13, 14, 14), (2, 13, 28, 28)) for k in (5, 7) for mode in (1, 2, 3)]
MM255 = [(shape, k, mode) for shape in ((3, 13, 14, 14), (2, 13, 21, 21), (10, 16, 7, 7), (2, 13, 28, 28)) for k in (3, 5, 7) for mode in (1, 2, 3)]
_sw_id = lambda p: "%s-k%d-m%d" % ("x".join(map(str, p[0])), p[1], p[2])


@pytest.mark.skipif(DW_MM != "0", reason="runs in the child of test_dw_mm_0_runs_cw (ATOMNAS_DW_MM=0)")
@pytest.mark.parametrize("p", MM0, ids=_sw_id)
def test_swmm0_cw_takes_the_bf16_shapes(gpu_lib, p):
    """without the matrix-core kernels the slab-major bf16 stride-1 shapes run k_dwf_cw / k_dwb_cw: whole images, ring of even height"""
    shape, k, mode = p
    c = case(*shape, k, 1, BF16, mode)
    check_fwd(gpu_lib, c, True, "cw")
    check_bwd(gpu_lib, c, True, "cw")


@pytest.mark.skipif(DW_MM != "255", reason="runs in the child of test_dw_mm_255_runs_mm_backward (ATOMNAS_DW_MM=255)")
@pytest.mark.parametrize("p", MM255, ids=_sw_id)
def test_swmm255_mm_backward(gpu_lib, p):
    """every bit set: k_dwb_mm at k = 3 / 5 / 7, on whole-image tiles of two groups (14 x 14), of three (21 x 21: the MAXG = MM_MAXG
    instance) and with the backward's NI below the forward's (7 x 7 at N = 10), and on the ring"""
    shape, k, mode = p
    check_bwd(gpu_lib, case(*shape, k, 1, BF16, mode), True, "mm")


@pytest.mark.skipif(DW_MM != "255", reason="runs in the child of test_dw_mm_255_runs_mm_backward (ATOMNAS_DW_MM=255)")
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_swmm255_mm_forward_k3(gpu_lib, mode):
    check_fwd(gpu_lib, case(3, 13, 14, 14, 3, 1, BF16, mode), True, "mm")


def test_dw_mm_0_runs_cw(gpu_lib):
    _child("swmm0_", "0", len(MM0))


def test_dw_mm_255_runs_mm_backward(gpu_lib):
    _child("swmm255_", "255", len(MM255) + 3)
