"""The kernels of the guarded step through the C ABI (csrc/optim.hip): atomnas_grad_guard (fixed-order global L2 norm of the gradient
arena -> verdict vector), the guarded instances of the fused optimizer kernels, atomnas_ema_update_guarded and atomnas_guard_restore.
Geometry and the norm's error bound: tests/guard_util.py.  Outputs live inside NaN-filled allocations (tests/glue_util.py)."""
import pytest
import torch

import glue_util as G
import guard_util as U

pytestmark = pytest.mark.gpu

GS = 0.3   # hyper[HYP_GRAD_SCALE]: not a power of two, so that every product rounds
NAN, INF = float("nan"), float("inf")


def _hyper(gs=GS, lr=0.05, decay=0.875):
    return torch.tensor([lr, 0.0, decay, gs, 0, 0, 0, 0], dtype=torch.float32).cuda()


def _arena(n, values):
    """the n floats the kernel gets (16-byte aligned), inside an allocation whose bytes behind n are NaN: a read past n flips the
    verdict"""
    full = torch.full((n + 64,), NAN, dtype=torch.float32, device="cuda")
    full[:n] = values.cuda()
    return full[:n]


def _guard():
    """(Vec, view) of a zeroed 8-word guard vector inside a NaN allocation"""
    v = G.Vec(8, fill=0.0)
    return v, v.v


def _run(g, n, hyper, max_norm, skip, guard, ws=None):
    from atomnas_amd import ops
    ws = ws or G.Vec(U.MAX_BLOCKS)
    ops.grad_guard(g, n, hyper, max_norm, skip, guard.v, ws.v)
    torch.cuda.synchronize()
    ws.check("guard workspace")
    out = guard.check("guard vector").clone()
    return out.cpu(), out.view(torch.int32).cpu()


def _formulas(norm32, max_norm, gs32):
    """torch's fp32 evaluation of clip_grad_norm_'s coefficient on the reported norm, and of the scale"""
    coef = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm32 + torch.tensor(1e-6, dtype=torch.float32)), max=1.0)
    return coef, gs32 * coef


# n = one sweep of the capped grid (1024 workgroups x 1024 sixteen-byte pieces) + 3: every thread runs exactly one full sweep, and the
# ragged tail holds three floats
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, U.ONE_SWEEP_FLOATS + 3]


@pytest.mark.parametrize("n", SIZES)
def test_norm_coefficient_scale_and_determinism(gpu_lib, n):
    assert gpu_lib.atomnas_grad_guard_ws_floats() == U.MAX_BLOCKS
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    g = _arena(n, x)
    hyper = _hyper()
    gs32 = hyper[3].cpu()
    ref = float(torch.linalg.vector_norm(x.double())) * float(gs32.double())
    bound = U.norm_rel_bound(n)
    assert bound < 4e-6
    # no clipping (max_norm 0, negative, +inf): coef 1, scale gs, counters untouched
    for mx in (0.0, -1.0, INF):
        guard = _guard()[0]
        f, c = _run(g, n, hyper, mx, True, guard)
        assert f[U.GUARD_OK] == 1.0 and f[U.GUARD_COEF] == 1.0 and torch.equal(f[U.GUARD_SCALE], gs32)
        assert abs(float(f[U.GUARD_NORM]) - ref) <= bound * ref, (float(f[U.GUARD_NORM]), ref, bound)
        assert int(c[U.GUARD_SKIPPED]) == 0 and int(c[U.GUARD_CLIPPED]) == 0
        assert float(f[6]) == 0.0 and float(f[7]) == 0.0
    norm32 = f[U.GUARD_NORM]
    # max_norm above the norm: exactly 1, the clipped counter stays; below: < 1, bit-equal to torch's formulas, counter + 1
    guard = _guard()[0]
    f, c = _run(g, n, hyper, 2.0 * float(norm32), False, guard)
    assert f[U.GUARD_COEF] == 1.0 and torch.equal(f[U.GUARD_SCALE], gs32) and int(c[U.GUARD_CLIPPED]) == 0
    mx = 0.37 * float(norm32)
    f, c = _run(g, n, hyper, mx, False, guard)
    coef, scale = _formulas(norm32, mx, gs32)
    assert float(coef) < 1.0
    assert torch.equal(f[U.GUARD_NORM], norm32), "two launches on the same input differ"
    assert torch.equal(f[U.GUARD_COEF], coef), (float(f[U.GUARD_COEF]), float(coef))
    assert torch.equal(f[U.GUARD_SCALE], scale), (float(f[U.GUARD_SCALE]), float(scale))
    assert f[U.GUARD_OK] == 1.0 and int(c[U.GUARD_CLIPPED]) == 1 and int(c[U.GUARD_SKIPPED]) == 0
    # determinism and accumulation: two more launches, the same bits, the counter at 3
    for k in (2, 3):
        f2, c2 = _run(g, n, hyper, mx, False, guard)
        assert torch.equal(f2[:4].view(torch.int32), f[:4].view(torch.int32))
        assert int(c2[U.GUARD_CLIPPED]) == k and int(c2[U.GUARD_SKIPPED]) == 0


def _nonfinite_cases():
    cases = []
    for n, places in ((1023, (0, 1022, 1020)), (256, (0, 255)), (5, (4,)), (U.SWEEP * 4 * 2 + 2, (U.SWEEP * 4 * 2 + 1, 4100))):
        for bad in (NAN, INF, -INF):
            for at in places:
                cases.append((n, bad, at))
    return cases


@pytest.mark.parametrize("n,bad,at", _nonfinite_cases())
def test_nonfinite_gradients(gpu_lib, n, bad, at):
    """NaN, +Inf and -Inf at index 0, at n - 1 and inside the ragged tail (n = 1023: pieces end at 1020; n = 5: the tail is element 4),
    in the last full piece (n = 256) and in the second workgroup (two workgroups + 2)"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    x[at] = bad
    g = _arena(n, x)
    hyper = _hyper()
    guard = _guard()[0]
    f, c = _run(g, n, hyper, 1e-3, True, guard)   # a max_norm that would clip any finite gradient
    assert f[U.GUARD_OK] == 0.0 and f[U.GUARD_COEF] == 1.0 and torch.equal(f[U.GUARD_SCALE], hyper[3].cpu())
    assert not bool(torch.isfinite(f[U.GUARD_NORM]))
    assert int(c[U.GUARD_SKIPPED]) == 1 and int(c[U.GUARD_CLIPPED]) == 0
    f, c = _run(g, n, hyper, 1e-3, False, guard)  # clip only: what the un-guarded code does on a bad step
    assert f[U.GUARD_OK] == 1.0 and f[U.GUARD_COEF] == 1.0 and int(c[U.GUARD_SKIPPED]) == 1 and int(c[U.GUARD_CLIPPED]) == 0
    for k in (2, 3):   # the skipped counter accumulates
        f, c = _run(g, n, hyper, 0.0, True, guard)
        assert f[U.GUARD_OK] == 0.0 and int(c[U.GUARD_SKIPPED]) == k


@pytest.mark.parametrize("values", [[3e19, 1.0, -2.0], [1e19] * 8 + [1.0]], ids=["square", "sum"])
def test_finite_gradients_whose_squares_overflow_count_as_nonfinite(gpu_lib, values):
    """3e19^2 = 9e38 is beyond fp32; eight squares of 1e19 (1e38 each, finite) overflow in the sum"""
    x = torch.tensor(values, dtype=torch.float32)
    assert bool(torch.isfinite(x).all())
    n = x.numel()
    g = _arena(n, x)
    guard = _guard()[0]
    f, c = _run(g, n, _hyper(), 1.0, True, guard)
    assert f[U.GUARD_OK] == 0.0 and f[U.GUARD_COEF] == 1.0 and int(c[U.GUARD_SKIPPED]) == 1 and int(c[U.GUARD_CLIPPED]) == 0
    f, c = _run(g, n, _hyper(), 1.0, False, guard)
    assert f[U.GUARD_OK] == 1.0 and f[U.GUARD_COEF] == 1.0 and int(c[U.GUARD_SKIPPED]) == 1


# ---------------------------------------------------------------------------------------------------------------- guarded optimizers
def _opt_case(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p0, g0, b0, e0 = (torch.randn(n, generator=gen) for _ in range(4))
    s0 = torch.rand(n, generator=gen)
    nch = (n + 255) // 256
    wdc = (torch.rand(nch, generator=gen) * 1e-2).float()
    wdc[0] = 7e-3
    return p0, g0, s0, b0, e0, wdc.cuda()


def _launch(kind, opt, st, g, wdc, n, hyper, guard):
    """kind "rmsprop": opt = momentum; "sgd": opt = (momentum, nesterov).  st: dict of Vecs p, sq, buf, ema, l2, ws"""
    from atomnas_amd import ops
    if kind == "rmsprop":
        ops.fused_rmsprop_ema(st["p"].v, g, st["sq"].v, st["buf"].v if opt > 0 else None, st["ema"].v, wdc, n, hyper, 0.9, 1e-3, True, opt,
                              l2_value=st["l2"].v, ws=st["ws"].v, guard=guard)
    else:
        ops.fused_sgd_ema(st["p"].v, g, st["buf"].v if opt[0] > 0 else None, st["ema"].v, wdc, n, hyper, opt[0], opt[1],
                          l2_value=st["l2"].v, ws=st["ws"].v, guard=guard)
    torch.cuda.synchronize()
    st["ws"].check("workspace")
    return {k: st[k].check(k).clone() for k in ("p", "sq", "buf", "ema", "l2")}


def _fresh(n, p0, s0, b0, e0):
    return dict(p=G.Vec(n, fill=p0), sq=G.Vec(n, fill=s0), buf=G.Vec(n, fill=b0), ema=G.Vec(n, fill=e0), l2=G.Vec(1), ws=G.Vec(4096))


@pytest.mark.parametrize("kind,opt", [("rmsprop", 0.0), ("rmsprop", 0.9), ("sgd", (0.0, False)), ("sgd", (0.9, False)), ("sgd", (0.9, True))],
                         ids=["rmsprop", "rmsprop-momentum", "sgd-plain", "sgd-momentum", "sgd-nesterov"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_guarded_optimizers(gpu_lib, kind, opt, n):
    """OK = 1 and GUARD_SCALE = s: the bits of the plain entry run with hyper[HYP_GRAD_SCALE] = s (the guarded entry must not read
    hyper[3]: it holds NaN).  OK = 0 and g full of NaN: p, sq, buf and ema keep their bits, the L2 value is the plain entry's."""
    p0, g0, s0, b0, e0, wdc = _opt_case(n, n + 17)
    s = 0.3 * 0.61
    g = G.Vec(n, fill=g0)
    ref = _launch(kind, opt, _fresh(n, p0, s0, b0, e0), g.v, wdc, n, _hyper(gs=s), None)
    assert not torch.equal(ref["p"].cpu(), p0) and not torch.equal(ref["ema"].cpu(), e0)
    guard = torch.tensor([1.0, s, NAN, NAN, 0, 0, 0, 0], dtype=torch.float32).cuda()
    got = _launch(kind, opt, _fresh(n, p0, s0, b0, e0), g.v, wdc, n, _hyper(gs=NAN), guard)
    for k in ref:
        assert torch.equal(got[k], ref[k]), (k, float((got[k] - ref[k]).abs().max()))
    guard = torch.tensor([0.0, s, NAN, 1.0, 0, 0, 0, 0], dtype=torch.float32).cuda()
    gnan = G.Vec(n, fill=NAN)
    got = _launch(kind, opt, _fresh(n, p0, s0, b0, e0), gnan.v, wdc, n, _hyper(gs=NAN), guard)
    for k, v0 in (("p", p0), ("sq", s0), ("buf", b0), ("ema", e0)):
        assert torch.equal(got[k].cpu(), v0), k + " changed in a dropped step"
    assert torch.equal(got["l2"], ref["l2"]) and bool(torch.isfinite(got["l2"]).all())


# ---------------------------------------------------------------------------------------------------------------- ema / restore
@pytest.mark.parametrize("n", [1, 6, 257, 1027, (1 << 19) + 1])
def test_ema_update_guarded_both_branches(gpu_lib, n):
    """OK = 1: the bits of atomnas_ema_update; OK = 0: the shadow keeps its bits.  (1 << 19) + 1: past one sweep of the capped grid."""
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(n)
    s0, x0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    hyper = _hyper()
    X = G.Vec(n, fill=x0)
    ref = G.Vec(n, fill=s0)
    ops.ema_update(ref.v, X.v, n, hyper)
    for ok in (1.0, 0.0):
        S = G.Vec(n, fill=s0)
        guard = torch.tensor([ok, NAN, NAN, NAN, 0, 0, 0, 0], dtype=torch.float32).cuda()
        ops.ema_update_guarded(S.v, X.v, n, hyper, guard)
        torch.cuda.synchronize()
        want = ref.check("ema") if ok else s0.cuda()
        assert torch.equal(S.check("guarded ema"), want), ok
    assert torch.equal(X.check("x").cpu(), x0)


@pytest.mark.parametrize("n", [1, 3, 4, 6, 257, 1027, 2048 * 256 * 4 + 1029])
def test_guard_restore_both_branches(gpu_lib, n):
    """dst = src exactly when `unconditional` or OK == 0; 16-byte pieces with a tail of 1..3 floats (n = 1, 3, 6, 257, 1027), no tail
    (4), and past one sweep of the capped grid (2048 workgroups x 256 pieces) with a tail of 1"""
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(n % 1000)
    d0, s0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    src = G.Vec(n, fill=s0)
    for ok, uncond, copies in ((1.0, False, False), (0.0, False, True), (1.0, True, True), (None, True, True)):
        dst = G.Vec(n, fill=d0)
        guard = None if ok is None else torch.tensor([ok, NAN, NAN, NAN, 0, 0, 0, 0], dtype=torch.float32).cuda()
        ops.guard_restore(dst.v, src.v, n, guard, uncond)
        torch.cuda.synchronize()
        assert torch.equal(dst.check("dst").cpu(), s0 if copies else d0), (ok, uncond)
    assert torch.equal(src.check("src").cpu(), s0)
