"""csrc/optim.hip at kernel level (GPU): the fused RMSprop + EMA step as a raw entry point, the small utility kernels, the regularisers
over a job table and the weight packing, against float64 references (tests/glue_ref.py), every output inside a sentinel-filled
allocation (tests/glue_util.py).

Single-line changes to csrc/optim.hip these tests were seen to catch (tried on a scratch build of the library):
  k_rmsprop_ema   sqrt(s + eps) on the eps-outside branch      -> test_rmsprop_raw_entry_point...[*-False]
  k_reg_grad      sign(0) = -1                                  -> test_reg_grad_and_value_over_a_job_table[1-*]
  k_pack          the source row pitch taken as `cols`          -> test_pack_weights_three_modes
(the last one also fails the fused-block tests of tests/test_fused_gpu.py, which pack bands of a wider matrix).
"""
import numpy as np
import pytest
import torch

import glue_ref as R
import glue_util as G
from kutil import assert_close

pytestmark = pytest.mark.gpu

REG_DT = np.dtype([("off", "<i8"), ("count", "<i4"), ("coef", "<f4")])
PACK_DT = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("src_ld", "<i4"), ("dst_ld", "<i4"),
                    ("c_off", "<i4"), ("mode", "<i4")])


def _table(dt, rows):
    tab = np.zeros(len(rows), dtype=dt)
    for i, r in enumerate(rows):
        tab[i] = r
    return torch.from_numpy(tab.view(np.uint8).copy()).cuda()


# ---------------------------------------------------------------------------------------------------------------- RMSprop + EMA
@pytest.mark.parametrize("inside", [True, False])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("n", [1, 255, 257, 1000003])
def test_rmsprop_raw_entry_point_lengths_and_null_arguments(gpu_lib, n, momentum, inside):
    """atomnas_fused_rmsprop_ema on lengths around a 256-element chunk and on 1000003: buf == NULL for momentum 0, eps inside and outside
    the sqrt; first with ema == NULL and wd_chunk == NULL, then with an EMA arena and a decay < 0 (the shadow is left alone), then with
    everything given and the L2 value against the float64 sum.  Everything outside [0, n) is NaN before and after."""
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(n + int(momentum * 10) + int(inside))
    lr, alpha, eps, gs = 0.05, 0.9, 1e-3, 0.5
    hyper = torch.tensor([lr, 0.0, -1.0, gs, 0, 0, 0, 0], dtype=torch.float32).cuda()   # lr, rho, EMA decay (< 0: skip), gradient scale
    p0, g0, b0, e0 = (torch.randn(n, generator=gen) for _ in range(4))
    s0 = torch.rand(n, generator=gen)

    def check(tag, P, S, B, E, ref, e_ref):
        assert_close(tag + " param", P.check(), ref["p"], rtol=1e-5, atol=1e-5 * float(ref["p"].abs().max()))
        assert_close(tag + " sq", S.check(), ref["sq"], rtol=1e-5, atol=1e-5 * float(ref["sq"].abs().max()))
        if momentum > 0:
            assert_close(tag + " buf", B.check(), ref["buf"], rtol=1e-4, atol=1e-6)
        else:
            assert torch.equal(B.check().cpu(), b0)   # not touched (and not passed)
        if E is not None:
            assert_close(tag + " ema", E.check(), e_ref, rtol=1e-5, atol=1e-5 * float(e_ref.abs().max()))

    for with_ema in (False, True):
        P, Gr, S, B = G.Vec(n, fill=p0), G.Vec(n, fill=g0), G.Vec(n, fill=s0), G.Vec(n, fill=b0)
        E = G.Vec(n, fill=e0) if with_ema else None
        ops.fused_rmsprop_ema(P.v, Gr.v, S.v, B.v if momentum > 0 else None, E.v if E else None, None, n, hyper, alpha, eps, inside, momentum)
        torch.cuda.synchronize()
        ref = R.rmsprop_ref(p0, g0, s0, b0, None, None, lr, alpha, eps, momentum, inside, gs)
        check("plain", P, S, B, None, ref, None)
        if E is not None:
            assert torch.equal(E.check().cpu(), e0), "EMA decay < 0 must leave the shadow alone"
    # every optional argument: weight decay per 256-element chunk, EMA, L2 value
    nch = (n + 255) // 256
    wdc = (torch.rand(nch, generator=gen) * 1e-2).float()
    wdc[::3] = 0.0
    if nch > 1:
        wdc[1] = 7e-3
    else:
        wdc[0] = 7e-3
    hyper[2] = 0.9
    P, Gr, S, B, E = G.Vec(n, fill=p0), G.Vec(n, fill=g0), G.Vec(n, fill=s0), G.Vec(n, fill=b0), G.Vec(n, fill=e0)
    l2 = G.Vec(1)
    ws = G.Vec(4096)
    ops.fused_rmsprop_ema(P.v, Gr.v, S.v, B.v if momentum > 0 else None, E.v, wdc.cuda(), n, hyper, alpha, eps, inside, momentum,
                          l2_value=l2.v, ws=ws.v)
    torch.cuda.synchronize()
    wd_el = wdc.double().repeat_interleave(256)[:n]
    ref = R.rmsprop_ref(p0, g0, s0, b0, e0, wd_el, lr, alpha, eps, momentum, inside, gs, 0.9)
    check("full", P, S, B, E, ref, ref["ema"])
    ws.check("workspace")
    got = float(l2.check("l2")[0])
    assert abs(got - ref["l2"]) <= 1e-5 * abs(ref["l2"]), (got, ref["l2"])


# ---------------------------------------------------------------------------------------------------------------- small kernels
@pytest.mark.parametrize("nbytes", [4, 12, 16, 20, 4 * ((1 << 20) + 3)])
def test_zero_tails(gpu_lib, nbytes):
    """16-byte pieces plus a tail of up to three words: exactly [0, bytes) becomes zero"""
    from atomnas_amd import ops
    n = nbytes // 4
    v = G.Vec(n, fill=1.5)
    ops.zero_(v.v)
    torch.cuda.synchronize()
    assert bool((v.check("zero") == 0).all())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_vec_sum(gpu_lib, n):
    """out[0] = scale * sum x (written, not accumulated: the output holds NaN before)"""
    from atomnas_amd import ops
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    xin, out = G.Vec(n, fill=x), G.Vec(1)
    ops.vec_sum(xin.v, n, 0.125, out.v)
    torch.cuda.synchronize()
    # thread t adds at most ceil(n / 256) values, then an 8-level tree, then the scale
    depth = (n + 255) // 256 + 9
    G.assert_within("vec_sum", out.check(), 0.125 * x.double().sum().view(1), G.sum_bound(depth, 0.125 * x.double().abs().sum()))


@pytest.mark.parametrize("n", [1, 257, (1 << 19) + 1])
def test_ema_scale_add(gpu_lib, n):
    """atomnas_ema_update, atomnas_scale_by (each hyper index) and atomnas_add_i64: grid-stride loops with a ragged end"""
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(n)
    hyper = torch.tensor([0.05, 3.0, 0.875, 0.3, 0, 0, 0, 0], dtype=torch.float32).cuda()
    hd = hyper.double().cpu()
    s0, x0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    S, X = G.Vec(n, fill=s0), G.Vec(n, fill=x0)
    ops.ema_update(S.v, X.v, n, hyper)
    torch.cuda.synchronize()
    d = float(hd[2])
    ref = s0.double() * d + (1.0 - d) * x0.double()
    G.assert_within("ema", S.check("ema"), ref, G.elem_bound(s0.double().abs() * d + (1.0 - d) * x0.double().abs()))
    for idx in range(4):
        X = G.Vec(n, fill=x0)
        ops.scale_by(X.v, n, hyper, idx)
        torch.cuda.synchronize()
        ref = x0.double() * float(hd[idx])
        G.assert_within("scale_by[%d]" % idx, X.check("scale_by"), ref, G.elem_bound(ref.abs()))
    c0 = torch.randint(-5, 1 << 40, (n,), generator=gen)
    Cn = G.Vec(n, torch.int64, fill=c0)
    ops.add_i64(Cn.v, 3)
    torch.cuda.synchronize()
    assert torch.equal(Cn.check("add_i64").cpu(), c0 + 3)


# ---------------------------------------------------------------------------------------------------------------- regularisers
REG_COUNTS = (1, 255, 256, 257, 16384, 16385, 40000)   # around one workgroup's stride (256) and the launch's (64 * 256)


def _reg_case():
    gen = torch.Generator().manual_seed(5)
    jobs, off = [], 37
    for i, cnt in enumerate(REG_COUNTS):
        jobs.append((off, cnt, 0.5 + 0.25 * i))
        off += cnt + 11 + 3 * i           # scattered: gaps between the jobs
    n = off + 50
    p = torch.randn(n, generator=gen)
    p[::7] = 0.0                          # sign(0) = 0
    g = torch.randn(n, generator=gen)
    return jobs, n, p, g


@pytest.mark.parametrize("with_go", [False, True])
@pytest.mark.parametrize("with_mult", [False, True])
@pytest.mark.parametrize("use_sign", [0, 1])
def test_reg_grad_and_value_over_a_job_table(gpu_lib, use_sign, with_mult, with_go):
    """g changes only inside the jobs, by coef * mult * go * (sign(p) or p) with sign(0) = 0; the value accumulates onto `out`"""
    from atomnas_amd import ops
    jobs, n, p, g = _reg_case()
    tab = _table(REG_DT, jobs)
    mult = torch.tensor([0.375]).cuda() if with_mult else None
    go = torch.tensor([1.5]).cuda() if with_go else None
    mv, gv = (0.375 if with_mult else 1.0), (1.5 if with_go else 1.0)
    Gv, Pv = G.Vec(n, fill=g), G.Vec(n, fill=p)
    ops.reg_grad(Pv.v, Gv.v, tab, len(jobs), use_sign, mult, go)
    torch.cuda.synchronize()
    got = Gv.check("g").cpu()
    ref, val = R.regularisers_ref(p, g, jobs, bool(use_sign), mv, gv, post_scale=2.0 if with_go else 1.0)
    inside = torch.zeros(n, dtype=torch.bool)
    for off, cnt, _ in jobs:
        inside[off:off + cnt] = True
    assert torch.equal(got[~inside], g[~inside]), "g changed outside the jobs"
    if use_sign:
        # exactly: coef, mult and go are dyadic, their product is exact in fp32 and the sign is 0 or +-1
        assert torch.equal(got[inside], ref.float()[inside])
        assert torch.equal(got[inside & (p == 0)], g[inside & (p == 0)])
    else:
        G.assert_within("g", got, ref, G.elem_bound(g.double().abs() + (ref - g.double()).abs()))
    out, ws = G.Vec(1, fill=0.25), G.Vec(64 * len(jobs))
    ops.reg_value(Pv.v, tab, len(jobs), use_sign, mult, 2.0 if with_go else 1.0, out.v, ws=ws.v)
    torch.cuda.synchronize()
    ws.check("workspace")
    mag = sum(c * float((p[o:o + k].double().abs() if use_sign else p[o:o + k].double() ** 2).sum()) for o, k, c in jobs) * mv * (2.0 if with_go else 1.0)
    # longest chain of additions: 3 per thread, 6 wave levels, 3 wave partials, 2 per thread of the final pass, its 8-level tree, `out`
    G.assert_within("value", out.check("out"), torch.tensor([0.25 + val]), G.sum_bound(32, torch.tensor(0.25 + mag)))


# ---------------------------------------------------------------------------------------------------------------- weight packing
@pytest.mark.parametrize("dt", G.DTYPES)
def test_pack_weights_three_modes(gpu_lib, dt):
    """one table with the three modes (PW, PW transposed, depthwise taps): odd rows / cols, src_ld > cols, c_off > 0, padded dst_ld; modes
    0 and 1 store the storage type, mode 2 always fp32; every element of the pack buffer that no job owns keeps its sentinel"""
    from atomnas_amd import ops
    dtype = G.T(dt)
    es = 4 // dtype.itemsize                     # storage elements per float
    gen = torch.Generator().manual_seed(9)
    arena = torch.randn(6000, generator=gen)
    # the buffer in floats: [0, 4000) holds storage-type matrices (element offsets in storage elements), [4000, 6500) fp32 taps
    jobs = [dict(src_off=5, dst_off=16, rows=13, cols=7, src_ld=7, dst_ld=24, c_off=0, mode=0),
            dict(src_off=200, dst_off=16, rows=13, cols=9, src_ld=11, dst_ld=24, c_off=7, mode=0),       # second segment of the same rows
            dict(src_off=400, dst_off=400, rows=5, cols=300, src_ld=300, dst_ld=8, c_off=3, mode=1),     # -> [3 + c][r], 303 x 8
            dict(src_off=2000, dst_off=4000 + 40, rows=9, cols=37, src_ld=40, dst_ld=56, c_off=0, mode=2),
            dict(src_off=2400, dst_off=4000 + 40, rows=25, cols=37, src_ld=37, dst_ld=56, c_off=9, mode=2),
            dict(src_off=3400, dst_off=3900 * es, rows=1, cols=1, src_ld=1, dst_ld=8, c_off=5, mode=0)]
    want = torch.full((7000,), G.NAN, dtype=torch.float32)
    buf = want.clone().cuda()
    for jb in jobs:
        idx, vals = R.pack_ref(arena, jb)
        if jb["mode"] == 2:
            assert int(idx.min()) >= 4000 and int(idx.max()) < 6500
            want[idx] = vals.float()
        else:
            assert int(idx.max()) < 4000 * es
            want.view(dtype)[idx] = vals.to(dtype)
    tab = _table(PACK_DT, [tuple(jb[k] for k in PACK_DT.names) for jb in jobs])
    ops.pack_weights(arena.cuda(), buf, tab, len(jobs), dtype)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu().view(torch.int32), want.view(torch.int32)), "packed bytes differ (values or a write outside the jobs)"
