"""The two stochastic-depth kernels of csrc/bn.hip at kernel level (GPU): atomnas_bn_apply_drop and atomnas_drop_connect_bwd at edge
shapes, in both storage types, against float64 references, every output inside a NaN-filled allocation (tests/glue_util.py).  The keep
mask is compared bit for bit with the numpy transcription of the key and hash (tests/drop_connect_ref.py).

Bounds (u = 2^-24, glue_util).  Forward, kept rows: y = res + s * (x*scale + shift) evaluated in fp32 and rounded once:
8 u * (|res| + s * (|x*scale| + |shift|)), plus 2^-8 |ref| for bf16 storage.  Rows of dropped images are copies: torch.equal.
Backward, kept rows: one fp32 product s * g, rounded to the storage type: u |ref| (fp32), 2^-8 |ref| (bf16); rows of dropped images are
exact zeros.  The statistic rows are fixed-order fp32 sums of the STORED gs (and of gs * z) of at most M terms: (M + 8) u * sum |terms|
against the float64 sums of the gs tensor read back.

Single-line changes to csrc/bn.hip these tests were seen to catch (tried on scratch builds of the library, one change each):
  k_bn_apply_drop     keep decided per pixel (`n = m` in the key) instead of per image       -> test_bn_apply_drop (keep mask, kept rows)
  k_bn_apply_drop     the dropped image multiplied by zero (`v += 0 * a`) instead of selected -> test_bn_apply_drop (NaN in dropped rows)
  k_drop_connect_bwd  keep indexed by pixel (`keep[p % N]`, in bounds) instead of by image    -> test_drop_connect_bwd
  k_drop_connect_bwd  statistics taken before the rounding to the storage type                -> test_drop_connect_bwd[*-bf16]
"""
import numpy as np
import pytest
import torch

import drop_connect_ref as DR
import glue_util as G
from glue_util import U, pad8

pytestmark = pytest.mark.gpu

# (N, HW, C, (ld of x / g, ld of res / z, ld of y / gs))
SHAPES = [(1, 1, 1, None), (5, 49, 13, None), (3, 4, 24, (24, 32, 40)), (9, 196, 40, None)]
SEEDS = (1995, 0xC0FFEE1234567)
STEPS = (None, 7, (1 << 20) + 7)
BLOCKS = (0, 21)


def _ids(s):
    return "N%d-HW%d-C%d" % s[:3]


def _pitches(C, lds):
    return lds if lds is not None else (pad8(C),) * 3


def _poison(act, N, HW, keep):
    """NaN in every row (padding columns too) of the images that are dropped"""
    for n in range(N):
        if not keep[n]:
            act.t[n * HW:(n + 1) * HW] = G.NAN


def _forward(N, HW, C, lds, dtype, p, seed, step, block, gen):
    from atomnas_amd import ops
    M = N * HW
    ldx, ldr, ldy = _pitches(C, lds)
    keep = DR.keep_mask(seed, step, block, N, p)
    x = G.Act(M, C, ldx, dtype, torch.randn(M, C, generator=gen))
    res = G.Act(M, C, ldr, dtype, torch.randn(M, C, generator=gen))
    scale = G.cvec(torch.rand(C, generator=gen) + 0.5)
    shift = G.cvec(torch.randn(C, generator=gen))
    xs = x.stored()
    _poison(x, N, HW, keep)
    y = G.Act(M, C, ldy, dtype)
    kout = G.Vec(N, dtype=torch.uint8)
    step_t = None if step is None else torch.tensor([step], dtype=torch.int64, device="cuda")
    ops.bn_apply_drop(x.t, scale.v, shift.v, res.t, y.t, kout.v, p, seed, step_t, block, N, HW, C)
    torch.cuda.synchronize()
    got_keep = kout.check("keep").cpu().numpy()
    assert np.array_equal(got_keep, keep), (got_keep, keep)
    got = y.read("y")
    r = res.stored()
    assert torch.equal(res.read("res"), r)   # the inputs are untouched
    s = DR.scale_of(p)
    sc, sh = scale.v[:C].double().cpu(), shift.v[:C].double().cpu()
    ref = r + s * (xs * sc + sh)
    terms = r.abs() + s * ((xs * sc).abs() + sh.abs())
    rows = torch.from_numpy(np.repeat(keep.astype(bool), HW))
    assert torch.equal(got[~rows], r[~rows]), "rows of dropped images are not copies of the residual"
    if bool(rows.any()):
        G.assert_within("kept rows", got[rows], ref[rows], G.elem_bound(terms[rows], ref[rows], dtype))
    return keep


@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_bn_apply_drop(gpu_lib, shape, dt, p):
    N, HW, C, lds = shape
    gen = torch.Generator().manual_seed(N * 1009 + HW * 31 + C)
    masks = []
    for seed in SEEDS:
        for step in STEPS:
            for block in BLOCKS:
                masks.append(tuple(_forward(N, HW, C, lds, G.T(dt), p, seed, step, block, gen)))
    if N >= 5:   # the cases draw different masks, with kept and dropped images among them
        assert len(set(masks)) > 1 and any(0 < sum(m) < N for m in masks)


@pytest.mark.parametrize("dt", G.DTYPES)
def test_bn_apply_drop_every_image_dropped(gpu_lib, dt):
    N, HW, C, p, seed, block = 2, 4, 13, 0.9, 1995, 3
    step = DR.find_step(seed, block, N, p, lambda m: int(m.sum()) == 0)
    keep = _forward(N, HW, C, None, G.T(dt), p, seed, step, block, torch.Generator().manual_seed(5))
    assert int(keep.sum()) == 0


def test_bn_apply_drop_refuses_bad_arguments(gpu_lib):
    from atomnas_amd import _lib, ops
    t = torch.zeros(4, 8, device="cuda")
    v = torch.ones(8, device="cuda")
    k = torch.zeros(1, dtype=torch.uint8, device="cuda")
    for p in (0.0, 1.0):
        with pytest.raises(_lib.AtomnasHipError):
            ops.bn_apply_drop(t, v, v, t, t.clone(), k, p, 1, None, 0, 1, 4, 8)
    with pytest.raises(_lib.AtomnasHipError):
        ops.bn_apply_drop(t, v, v, None, t.clone(), k, 0.5, 1, None, 0, 1, 4, 8)


# ---------------------------------------------------------------------------------------------------------------- backward
def _grid_rows(M, C, stat_rows):
    """rows the launch writes sums into (the host code of atomnas_drop_connect_bwd / atomnas_act_bwd_stats); the rest are zeroed"""
    ncg, lcg = (C + 7) // 8, 0
    while (1 << lcg) < ncg and lcg < 5:
        lcg += 1
    pl = 256 >> lcg
    return min((M + pl - 1) // pl, 2048, stat_rows)


def _given_masks(N):
    if N == 1:
        return [np.array([1], np.uint8), np.array([0], np.uint8)]
    a = (np.arange(N) % 3 != 1).astype(np.uint8)          # kept, dropped, kept, kept, dropped ...
    return [a, (1 - a).astype(np.uint8)]


@pytest.mark.parametrize("stat_rows", [1, 8, 1024])
@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_drop_connect_bwd(gpu_lib, shape, dt, stat_rows):
    from atomnas_amd import ops
    N, HW, C, lds = shape
    dtype, M = G.T(dt), N * HW
    ldg, ldz, ldgs = _pitches(C, lds)
    gen = torch.Generator().manual_seed(N * 2003 + HW * 17 + C + stat_rows)
    for p in (0.2, 0.5):
        for keep in _given_masks(N):
            g = G.Act(M, C, ldg, dtype, torch.randn(M, C, generator=gen))
            z = G.Act(M, C, ldz, dtype, torch.randn(M, C, generator=gen) + 0.5)
            gv, zv = g.stored(), z.stored()
            _poison(g, N, HW, keep)
            _poison(z, N, HW, keep)
            gs = G.Act(M, C, ldgs, dtype)
            svec, sview = G.stats_buf(stat_rows, C)
            kt = G.Vec(N, dtype=torch.uint8, fill=torch.from_numpy(keep))
            ops.drop_connect_bwd(g.t, z.t, kt.v, p, gs.t, svec.v, N, HW, C, stat_rows=stat_rows)
            torch.cuda.synchronize()
            got = gs.read("gs")
            assert np.array_equal(kt.check("keep").cpu().numpy(), keep)
            rows = torch.from_numpy(np.repeat(keep.astype(bool), HW))
            assert torch.equal(got[~rows], torch.zeros_like(got[~rows])), "rows of dropped images are not zero"
            ref = gv * DR.scale_of(p)
            if bool(rows.any()):
                G.assert_within("kept rows", got[rows], ref[rows], (U if dtype == torch.float32 else 2.0 ** -8) * ref[rows].abs() + G.TINY)
            total = G.stats_total(svec, sview)
            zk = torch.where(rows[:, None], zv, torch.zeros_like(zv))   # a dropped row contributes nothing (its z is NaN on the device)
            G.assert_within("sum gs", total[0], got.sum(0), G.sum_bound(M, got.abs().sum(0)) + G.TINY)
            G.assert_within("sum gs*z", total[1], (got * zk).sum(0), G.sum_bound(M, (got * zk).abs().sum(0)) + G.TINY)
            used = _grid_rows(M, C, stat_rows)
            assert bool((sview[used:] == 0).all()), "rows beyond the grid are not zero"


def test_drop_connect_bwd_refuses_bad_arguments(gpu_lib):
    from atomnas_amd import _lib, ops
    t = torch.zeros(4, 8, device="cuda")
    k = torch.ones(1, dtype=torch.uint8, device="cuda")
    st = torch.zeros(2 * 8, device="cuda")
    for p in (0.0, 1.0):
        with pytest.raises(_lib.AtomnasHipError):
            ops.drop_connect_bwd(t, t, k, p, t.clone(), st, 1, 4, 8, stat_rows=1)
    with pytest.raises(_lib.AtomnasHipError):
        ops.drop_connect_bwd(t, t, k, 0.5, t.clone(), st, 1, 4, 8, stat_rows=0)
