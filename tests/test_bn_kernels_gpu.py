"""csrc/bn.hip at kernel level (GPU): the BatchNorm finalize steps, the element-wise apply passes, the pooling head with its dropout mask
and the masked-gradient + statistics passes, at edge shapes, in both storage types, against float64 references (tests/glue_ref.py:
torch's batch_norm under autograd), every output inside a NaN-filled allocation (tests/glue_util.py).

Bounds.  u = 2^-24.  The partial rows are summed by at most 8 additions per thread and 64 in order (72 terms); a result that depends on
such sums gets the propagated error of the sums, written out in fwd_bounds / bwd_bounds; the last expression adds 8 u * sum |terms| and
bf16 storage 2^-8 |ref| (glue_util).  Swish uses __expf, whose error is not derived but MEASURED on the GPU as the largest ratio of the
observed fp32 error to the derived bound of the same element, over the swish cases of this file:
    forward  (swish itself:     bn_apply, bn_act_pool, the chain's y)                  measured ratio 0.074  -> SWISH_FWD_K = 0.30
    backward (swish derivative: act_bwd_stats, pool_act_bwd, the chain's dx / dgamma)  measured ratio 0.43   -> SWISH_BWD_K = 1.72
The bound of a swish result is K = 4 x that ratio times the derived bound, never above the bf16 bound of the element.  (Run with -s:
the module prints the ratios it observed.)

Single-line changes to csrc/bn.hip these tests were seen to catch (tried on a scratch build of the library, one kernel each):
  k_bn_finalize_fwd   `gamma ? gamma[p] : 0.f`                                   -> ..._fwd_variants[*no_affine*]
  k_bn_eval_coeffs    `beta ? beta[p] : 1.f`                                     -> test_bn_eval_coeffs[*no_affine*]
  k_bn_finalize_bwd   sign(0) = -1 in the L1 term                                -> ..._bwd_variants[*l1*]
  k_bn_apply          `cg = C / 8` (the partial channel group left out)          -> the chain at C = 3, 13
  k_bn_act_pool       the dropout counter from the padded index n*pad8(C) + c    -> ..._dropout_mask at C = 13, 1283
  k_pool_act_bwd      keep == NULL still scaled by 1 / (1 - p)                   -> test_pool_act_bwd (keep0 rows1024)
  k_act_bwd_stats     the gradient rounded to bf16 before it is summed           -> test_act_bwd_stats_shapes[*-bf16]
k_bnbwd_apply at odd C in both storage types is also covered by tests/test_kernels_gpu.py::test_bnbwd_apply.
"""
import numpy as np
import pytest
import torch

import glue_ref as R
import glue_util as G
from glue_util import U, pad8

pytestmark = pytest.mark.gpu

EPS = 1e-3
SWISH_FWD_K = 0.30    # 4 x the measured 0.074 (see above)
SWISH_BWD_K = 1.72    # 4 x the measured 0.43
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _report_measurements():
    yield
    if MEASURED:
        print("\nswish: largest fp32 error / derived bound:", {k: round(v, 3) for k, v in MEASURED.items()})


def swish_bound(kind, base, ref, got, dtype):
    """bound of a swish result: K * base, capped by the bf16 bound of the element; records the measured ratio of the fp32 cases"""
    if dtype == torch.float32:
        err = (got.double().cpu() - ref).abs()
        ok = base > 0
        if bool(ok.any()):
            MEASURED[kind] = max(MEASURED.get(kind, 0.0), float((err[ok] / base[ok]).max()))
    cap = base + 2.0 ** -8 * ref.abs()
    b = torch.minimum((SWISH_FWD_K if kind == "fwd" else SWISH_BWD_K) * base, cap)
    return b if dtype == torch.float32 else cap


# ---------------------------------------------------------------------------------------------------------------- error propagation
def fwd_bounds(x, gamma, beta, count, n=72):
    """errors of mean, var, invstd, scale, shift computed in fp32 from partial rows summed as <= n-term fixed-order sums (x: [M, C] fp64)"""
    A1, E2 = x.abs().sum(0) / count, (x * x).sum(0) / count
    mean = x.sum(0) / count
    var = (E2 - mean * mean).clamp(min=0)
    em = (n + 10) * U * A1
    ev = (n + 10) * U * E2 + 2 * mean.abs() * em + 4 * U * (E2 + mean * mean)
    r = (var + EPS) ** -0.5
    er = 0.5 * r ** 3 * ev + 4 * U * r
    s = gamma * r
    es = gamma.abs() * er + 2 * U * s.abs()
    eh = 8 * U * (beta.abs() + (mean * s).abs()) + s.abs() * em + mean.abs() * es
    return dict(mean=em, var=ev, invstd=er, scale=es, shift=eh, r=r, s=s, h=beta - mean * s)


def bwd_bounds(x, g, gamma, mean, r, M, n=72, eg=None, em=0.0, er=0.0):
    """errors of dgamma, dbeta and of the coefficients the backward finalize derives from [sum g, sum g x] summed as <= n-term sums;
    eg: per-element error of the summed g (swish), em / er: errors of the saved mean / invstd the kernel reads"""
    Sg, Sgx = g.abs().sum(0), (g * x).abs().sum(0)
    sg, sgx = g.sum(0), (g * x).sum(0)
    e_sg = (n + 10) * U * Sg + (eg.sum(0) if eg is not None else 0.0)
    e_sgx = (n + 10) * U * Sgx + ((eg * x.abs()).sum(0) if eg is not None else 0.0)
    dg = r * (sgx - mean * sg)
    rel = er / r
    edg = r * (e_sgx + mean.abs() * e_sg + sg.abs() * em) + 8 * U * r * (sgx.abs() + (mean * sg).abs()) + dg.abs() * rel
    ga = gamma.abs()
    c1, c2 = gamma * r, -gamma * r * r * dg / M
    t1, t2 = (ga * r * r * mean * dg).abs() / M, (ga * r * sg).abs() / M
    ec1 = 8 * U * c1.abs() + c1.abs() * rel
    ec2 = ga * r * r * edg / M + 8 * U * c2.abs() + 2 * c2.abs() * rel
    ec3 = ga * r * (mean.abs() * r * edg + e_sg + r * dg.abs() * em) / M + 8 * U * (t1 + t2) + (2 * t1 + t2) * rel
    return dict(dgamma=edg, dbeta=e_sg, c1=ec1, c2=ec2, c3=ec3, vals=(c1, c2))


def split_rows(gen, M, rows):
    """row id of every sample: an uneven split of M samples over `rows` partial rows (many of them empty when rows > M)"""
    cuts = torch.sort(torch.randint(0, M + 1, (rows - 1,), generator=gen)).values if rows > 1 else torch.zeros(0, dtype=torch.int64)
    return torch.searchsorted(cuts, torch.arange(M), right=True)


def partial_rows(rid, rows, ld, a, b, C, hole_cols=()):
    """fp32 statistics [rows][2][ld] on the GPU inside a NaN allocation: plane 0 sums of a, plane 1 sums of b per row; columns C..pad8(C)-1
    and the holes hold finite garbage (read, never used), columns pad8(C)..ld-1 NaN (never to be read)"""
    st = torch.zeros(rows, 2, ld, dtype=torch.float64)
    st[:, 0, :C].index_add_(0, rid, a)
    st[:, 1, :C].index_add_(0, rid, b)
    st[:, :, C:pad8(C)] = 7.0
    for c in hole_cols:
        st[:, :, c] = 5.0
    st[:, :, pad8(C):] = G.NAN
    vec, view = G.stats_buf(rows, ld)
    view.copy_(st.float())
    return vec


def make_cmap(gen, C, holes):
    """(cmap int32 [C] with -1 holes or None, live padded channels, their parameter indices)"""
    if not holes:
        return None, list(range(C)), torch.arange(C)
    live = [c for c in range(C) if c % 3 != 1] if C > 1 else [0]
    perm = torch.randperm(len(live), generator=gen)
    cmap = torch.full((C,), -1, dtype=torch.int32)
    cmap[live] = perm.to(torch.int32)
    return cmap, live, perm


def by_channel(vals_live, live, C, fill=0.0):
    out = torch.full((C,), fill, dtype=torch.float64)
    out[live] = vals_live
    return out


# ---------------------------------------------------------------------------------------------------------------- finalize, forward
def _fwd_case(C, rows, ld, momentum=0.01, nbt0=0, running=True, affine=True, save=True, holes=False, count_one=False, ratio=None):
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(C * 7919 + rows * 31 + ld + int(holes))
    M = 1 if count_one else 300
    cmap, live, pidx = make_cmap(gen, C, holes)
    P = len(live)
    std = torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    mu = torch.randn(C, generator=gen, dtype=torch.float64) if ratio is None else std * ratio
    x = torch.randn(M, C, generator=gen, dtype=torch.float64) * std + mu
    gamma_p = torch.rand(P, generator=gen, dtype=torch.float64) + 0.5
    gamma_p[::3] *= -1
    beta_p = torch.randn(P, generator=gen, dtype=torch.float64)
    if not affine:
        gamma_p, beta_p = torch.ones(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
    rm0, rv0 = torch.randn(P, generator=gen).double(), (torch.rand(P, generator=gen) + 0.5).double()
    holes_c = [c for c in range(C) if c not in live]
    stats = partial_rows(split_rows(gen, M, rows), rows, ld, x, x * x, C, holes_c)
    gam, bet = (G.Vec(P, fill=gamma_p), G.Vec(P, fill=beta_p)) if affine else (None, None)
    rm, rv = (G.Vec(P, fill=rm0), G.Vec(P, fill=rv0)) if running else (None, None)
    nbt = G.Vec(1, torch.int64, fill=nbt0)
    Cp = pad8(C)
    sc, sh = G.Vec(Cp), G.Vec(Cp)
    sm, si = (G.Vec(Cp), G.Vec(Cp)) if save else (None, None)
    cm = G.Vec(C, torch.int32, fill=cmap) if cmap is not None else None
    ops.bn_finalize_fwd(stats.v, float(M), gam.v if gam else None, bet.v if bet else None, EPS, momentum, rm.v if rm else None,
                        rv.v if rv else None, nbt.v if running else None, sc.v, sh.v, sm.v if sm else None, si.v if si else None, C,
                        stat_rows=rows, stat_ld=ld, cmap=cm.v if cm else None)
    torch.cuda.synchronize()
    xl = x[:, live]
    g_c, b_c = gamma_p[pidx], beta_p[pidx]                  # parameters in the order of the live padded channels
    ref = R.bn_train_ref(xl, g_c, b_c, EPS, 0)
    eb = fwd_bounds(xl, g_c, b_c, float(M))
    r = 1.0 / torch.sqrt(ref["var_b"] + EPS)
    tag = "C%d rows%d ld%d" % (C, rows, ld)

    def chk(name, vec, want_live, bound_live):
        got = vec.check(name).cpu()
        assert bool((got[C:] == 0).all()), "%s %s: lanes C..pad8(C)-1 must be zero" % (tag, name)
        assert bool((got[holes_c] == 0).all()), "%s %s: cmap holes must be zero" % (tag, name)
        G.assert_within("%s %s" % (tag, name), got[live], want_live, bound_live)
    chk("scale", sc, g_c * r, eb["scale"])
    chk("shift", sh, b_c - ref["mean"] * g_c * r, eb["shift"])
    if save:
        chk("save_mean", sm, ref["mean"], eb["mean"])
        chk("save_invstd", si, r, eb["invstd"])
        if ratio is not None:
            var_got = 1.0 / si.v.double().cpu()[live] ** 2 - EPS
            G.assert_within("%s variance from invstd" % tag, var_got, ref["var_b"], 256 * U * (ref["mean"] ** 2 + ref["var_b"]))
    assert nbt.check("num_batches_tracked").tolist() == [nbt0], "the counter is the caller's to bump"
    if running:
        m = momentum if momentum is not None else 1.0 / (nbt0 + 1)
        var_run = ref["var_u"] if M > 1 else ref["var_b"]       # one value per channel: no unbiasing (torch refuses that batch)
        unb = M / (M - 1.0) if M > 1 else 1.0
        want_rm, want_rv = rm0.clone(), rv0.clone()
        want_rm[pidx] = (1 - m) * rm0[pidx] + m * ref["mean"]
        want_rv[pidx] = (1 - m) * rv0[pidx] + m * var_run
        b_rm, b_rv = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
        b_rm[pidx] = 8 * U * (((1 - m) * rm0[pidx]).abs() + (m * ref["mean"]).abs()) + m * eb["mean"]
        b_rv[pidx] = 8 * U * (((1 - m) * rv0[pidx]).abs() + m * var_run) + m * unb * eb["var"]
        G.assert_within(tag + " running_mean", rm.check("running_mean"), want_rm, b_rm)
        G.assert_within(tag + " running_var", rv.check("running_var"), want_rv, b_rv)
    stats.check("statistics (input)")


FWD_C = [1, 7, 8, 9, 24, 100, 257]


@pytest.mark.parametrize("C", FWD_C)
def test_bn_finalize_fwd_rows_and_pitches(gpu_lib, C):
    """partial rows of a real x [300, C], split unevenly over 1 / 63 / 64 / 65 / 512 rows, at pitch pad8(C) and pad8(C) + 12: scale, shift,
    saved mean / invstd and the running statistics (momentum 0.01, unbiased variance) against torch's batch_norm in float64"""
    for rows in (1, 63, 64, 65, 512):
        for ld in (pad8(C), pad8(C) + 12):
            _fwd_case(C, rows, ld)


@pytest.mark.parametrize("variant", ["count1", "cumulative0", "cumulative1", "cumulative7", "no_running", "no_affine_no_save", "cmap",
                                     "cmap_no_affine"])
@pytest.mark.parametrize("C", FWD_C)
def test_bn_finalize_fwd_variants(gpu_lib, C, variant):
    """count = 1 (running variance without the count / (count - 1) factor), cumulative momentum at num_batches_tracked 0 / 1 / 7 (m = 1 / (n + 1),
    the counter itself untouched), no running statistics, gamma == beta == save_mean == NULL, and a cmap: a permutation of the parameters
    with -1 holes inside the range -- parameters indexed by cmap[c], coefficients by c, holes written as zero"""
    kw = dict(count1=dict(count_one=True), cumulative0=dict(momentum=None, nbt0=0), cumulative1=dict(momentum=None, nbt0=1),
              cumulative7=dict(momentum=None, nbt0=7), no_running=dict(running=False), no_affine_no_save=dict(affine=False, save=False),
              cmap=dict(holes=True), cmap_no_affine=dict(holes=True, affine=False))[variant]
    for rows, ld in ((1, pad8(C)), (65, pad8(C) + 12)):
        _fwd_case(C, rows, ld, **kw)


@pytest.mark.parametrize("ratio", [0.0, 1.0, 8.0, 64.0])
def test_bn_finalize_fwd_cancellation(gpu_lib, ratio):
    """var = E[x^2] - mean^2 in fp32 at |mean| / std = 0, 1, 8, 64: the variance recovered from save_invstd satisfies
    |var - var_ref| <= 256 u (mean^2 + var) -- two fixed-order sums of at most 72 positive terms and the subtraction, with margin.
    That is the precision of this form: at |mean| = 64 std the bound is 6 % of the variance."""
    for rows in (1, 512):
        _fwd_case(24, rows, 24, ratio=ratio)


@pytest.mark.parametrize("variant", ["plain", "cmap", "no_affine", "cmap_no_affine"])
@pytest.mark.parametrize("C", FWD_C)
def test_bn_eval_coeffs(gpu_lib, C, variant):
    """scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale; parameters by cmap[c], holes and padding lanes zero"""
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(C + len(variant))
    cmap, live, pidx = make_cmap(gen, C, "cmap" in variant)
    P = len(live)
    affine = "no_affine" not in variant
    gamma = (torch.rand(P, generator=gen) + 0.5).double()
    beta = torch.randn(P, generator=gen).double()
    gamma[::3] *= -1
    if not affine:
        gamma, beta = torch.ones(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
    rm, rv = torch.randn(P, generator=gen).double(), (torch.rand(P, generator=gen) + 0.05).double()
    Cp = pad8(C)
    sc, sh = G.Vec(Cp), G.Vec(Cp)
    gv, bv, rmv, rvv = G.Vec(P, fill=gamma), G.Vec(P, fill=beta), G.Vec(P, fill=rm), G.Vec(P, fill=rv)
    cm = G.Vec(C, torch.int32, fill=cmap) if cmap is not None else None
    ops.bn_eval_coeffs(gv.v if affine else None, bv.v if affine else None, rmv.v, rvv.v, EPS, sc.v, sh.v, C, cmap=cm.v if cm else None)
    torch.cuda.synchronize()
    x = torch.randn(4, P, generator=gen, dtype=torch.float64)
    want = torch.nn.functional.batch_norm(x, rm.float().double(), rv.float().double(), gamma.float().double(), beta.float().double(), False, 0.0, EPS)
    s, h = sc.check("scale").double().cpu(), sh.check("shift").double().cpu()
    holes_c = [c for c in range(C) if c not in live]
    for v in (s, h):
        assert bool((v[C:] == 0).all()) and bool((v[holes_c] == 0).all())
    sl, hl = s[live], h[live]
    xs = x[:, pidx]
    rr = (rv[pidx].float().double() + EPS) ** -0.5
    ws = gamma[pidx].float().double() * rr
    wh = beta[pidx].float().double() - rm[pidx].float().double() * ws
    G.assert_within("scale", sl, ws, G.elem_bound(ws.abs()))
    G.assert_within("shift", hl, wh, G.elem_bound(beta[pidx].abs() + (rm[pidx] * ws).abs()) + rm[pidx].abs() * 8 * U * ws.abs())
    # and as what they are for: x * scale + shift is torch's eval-mode batch_norm
    assert torch.allclose(xs * sl + hl, want[:, pidx], rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- finalize, backward
def _bwd_case(C, rows, ld, holes=False, l1=False, null_grads=False, affine=True):
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(C * 104729 + rows * 17 + ld + int(holes) + 2 * int(l1))
    M = 300
    cmap, live, pidx = make_cmap(gen, C, holes)
    P = len(live)
    x = torch.randn(M, C, generator=gen, dtype=torch.float64) * (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5) + torch.randn(C, generator=gen, dtype=torch.float64)
    dy = torch.randn(M, C, generator=gen, dtype=torch.float64)
    gamma_p = (torch.rand(P, generator=gen) + 0.5).double()
    gamma_p[::3] *= -1
    if l1 and P > 1:
        gamma_p[1::4] = 0.0                                 # sign(0) = 0: no L1 sub-gradient at a dead channel
    if not affine:
        gamma_p = torch.ones(P, dtype=torch.float64)
    gamma_p = gamma_p.float().double()
    beta_p = torch.randn(P, generator=gen).double()
    g_c = gamma_p[pidx]
    xl, gl = x[:, live], dy[:, live]
    ref = R.bn_train_ref(xl, g_c, beta_p[pidx], EPS, 0, gl)
    r = 1.0 / torch.sqrt(ref["var_b"] + EPS)
    holes_c = [c for c in range(C) if c not in live]
    stats = partial_rows(split_rows(gen, M, rows), rows, ld, dy, dy * x, C, holes_c)
    Cp = pad8(C)
    smean, sinv = G.Vec(Cp, fill=0.0), G.Vec(Cp, fill=0.0)
    smean.v[:C] = by_channel(ref["mean"], live, C).float().cuda()
    sinv.v[:C] = by_channel(r, live, C).float().cuda()
    gam = G.Vec(P, fill=gamma_p) if affine else None
    rho, pen_p = 0.375, (torch.rand(P, generator=gen) + 0.5).float().double()
    rho_v, pen_v = (G.Vec(1, fill=rho), G.Vec(P, fill=pen_p)) if l1 else (None, None)
    dgam, dbet = (None, None) if null_grads else (G.Vec(P, fill=0.25), G.Vec(P, fill=0.25))
    c1, c2, c3 = G.Vec(Cp), G.Vec(Cp), G.Vec(Cp)
    cm = G.Vec(C, torch.int32, fill=cmap) if cmap is not None else None
    ops.bn_finalize_bwd(stats.v, float(M), gam.v if gam else None, smean.v, sinv.v, rho_v.v if l1 else None, pen_v.v if l1 else None,
                        dgam.v if dgam else None, dbet.v if dbet else None, c1.v, c2.v, c3.v, C, stat_rows=rows, stat_ld=ld,
                        cmap=cm.v if cm else None)
    torch.cuda.synchronize()
    tag = "C%d rows%d ld%d" % (C, rows, ld)
    eb = bwd_bounds(xl, gl, g_c, ref["mean"], r, M)
    co = []
    for name, v in (("c1", c1), ("c2", c2), ("c3", c3)):
        got = v.check(name).double().cpu()
        assert bool((got[C:] == 0).all()) and bool((got[holes_c] == 0).all()), "%s %s: holes and padding lanes must be zero" % (tag, name)
        co.append(got[live])
    # the coefficients as what they are for: c1 * g + c2 * x + c3 is the input gradient of torch's batch_norm
    dx = co[0] * gl + co[1] * xl + co[2]
    G.assert_within(tag + " dx from c1, c2, c3", dx, ref["dx"], gl.abs() * eb["c1"] + xl.abs() * eb["c2"] + eb["c3"])
    if not null_grads:
        sign = torch.sign(g_c)
        l1v = rho * pen_p[pidx] * sign if l1 else torch.zeros(len(live), dtype=torch.float64)
        want_dg, want_db = torch.full((P,), 0.25, dtype=torch.float64), torch.full((P,), 0.25, dtype=torch.float64)
        want_dg[pidx] += ref["dgamma"] + l1v
        want_db[pidx] += ref["dbeta"]
        b_dg, b_db = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
        b_dg[pidx] = eb["dgamma"] + 8 * U * (0.25 + ref["dgamma"].abs() + l1v.abs())
        b_db[pidx] = eb["dbeta"] + 8 * U * (0.25 + ref["dbeta"].abs())
        G.assert_within(tag + " dgamma", dgam.check("dgamma"), want_dg, b_dg)
        G.assert_within(tag + " dbeta", dbet.check("dbeta"), want_db, b_db)
        if l1:   # the L1 term by itself, where dgamma's data part is exactly zero: gamma == 0 gives dgamma = r * sum g (x - mean), no sign term
            assert bool((sign[g_c == 0] == 0).all())


@pytest.mark.parametrize("C", FWD_C)
def test_bn_finalize_bwd_rows_and_pitches(gpu_lib, C):
    """[sum g, sum g x] of a real (x, dy) [300, C] over 1 / 63 / 64 / 65 / 512 rows at both pitches: dgamma and dbeta ACCUMULATE onto 0.25,
    and c1 * g + c2 * x + c3 is autograd's input gradient of batch_norm"""
    for rows in (1, 63, 64, 65, 512):
        for ld in (pad8(C), pad8(C) + 12):
            _bwd_case(C, rows, ld)


@pytest.mark.parametrize("variant", ["null_grads", "l1", "cmap", "cmap_l1", "no_gamma"])
@pytest.mark.parametrize("C", FWD_C)
def test_bn_finalize_bwd_variants(gpu_lib, C, variant):
    """dgamma == dbeta == NULL; the L1 sub-gradient rho * penalty[p] * sign(gamma) with positive, negative and exactly zero gammas (zero at
    zero); a cmap with holes, with and without the L1 term; gamma == NULL"""
    kw = dict(null_grads=dict(null_grads=True), l1=dict(l1=True), cmap=dict(holes=True), cmap_l1=dict(holes=True, l1=True),
              no_gamma=dict(affine=False, null_grads=True))[variant]
    for rows, ld in ((1, pad8(C)), (65, pad8(C) + 12)):
        _bwd_case(C, rows, ld, **kw)


# ---------------------------------------------------------------------------------------------------------------- the chain
def _chain_x(gen, M, C, gamma, beta, act, dtype):
    """x [M, C] as stored in dtype (float64 values) whose normalised pre-activation keeps 2^-6 from 0 (ReLU, ReLU6) and from 6 (ReLU6)"""
    x = (torch.randn(M, C, generator=gen, dtype=torch.float64) * (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
         + torch.randn(C, generator=gen, dtype=torch.float64)).to(dtype).double()
    if act in (0, 3):
        return x
    gap = 2.0 ** -5
    for _ in range(40):
        mean, var = x.mean(0), x.var(0, unbiased=False)
        rg = gamma / torch.sqrt(var + EPS)
        pre = (x - mean) * rg + beta
        near0, near6 = pre.abs() < gap, ((pre - 6).abs() < gap) & (act == 2)
        if not bool((near0 | near6).any()):
            break
        push = torch.where(near6, torch.where(pre >= 6, 0.125, -0.125), torch.where(pre >= 0, 0.125, -0.125)).double()
        x = torch.where(near0 | near6, (x + push / rg).to(dtype).double(), x)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    pre = (x - mean) * gamma / torch.sqrt(var + EPS) + beta
    assert float(pre.abs().min()) >= 2.0 ** -6 and (act != 2 or float((pre - 6).abs().min()) >= 2.0 ** -6)
    return x


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("M,C", [(5, 3), (300, 13), (1000, 264)])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_split_batchnorm_chain(gpu_lib, act, M, C, with_res, dt):
    """The split BatchNorm end to end: statistics of x (summed in torch) -> bn_finalize_fwd -> bn_apply (with and without the residual)
    = act(batch_norm(x)) (+ res); dy -> act_bwd_stats -> bn_finalize_bwd -> bnbwd_apply = autograd's dx, dgamma, dbeta.  A wrong sign or
    a wrong 1 / M anywhere in the chain shows here.  (act_bwd_stats lays its rows out at pitch C, the finalize reads pitch >= pad8(C): the
    step runs them at multiples of 8 where the two agree, so the masked pass runs over the padded width pad8(C) here, whose extra
    channels are zero in every tensor.)"""
    from atomnas_amd import ops
    dtype = G.T(dt)
    gen = torch.Generator().manual_seed(act * 1000 + M + C)
    Cp = pad8(C)
    ld = Cp + 8 if with_res else Cp
    gamma = ((torch.rand(C, generator=gen) + 0.5) * torch.where(torch.rand(C, generator=gen) > 0.3, 1.0, -1.0)).float().double()
    beta = (torch.randn(C, generator=gen) * 1.5 + (2.0 if act == 2 else 0.0)).float().double()
    xs = _chain_x(gen, M, C, gamma, beta, act, dtype)
    X = G.Act(M, C, ld, dtype, xs)
    res = G.Act(M, C, Cp, dtype, torch.randn(M, C, generator=gen)) if with_res else None
    DY = G.Act(M, C, ld, dtype, torch.randn(M, C, generator=gen))
    dys = DY.stored()
    ref = R.bn_train_ref(xs, gamma, beta, EPS, act, dys, res.stored() if res else None)
    # forward
    rows = 3
    stats = partial_rows(torch.arange(M) % rows, rows, Cp, xs, xs * xs, C)
    gam, bet = G.Vec(Cp, fill=0.0), G.Vec(Cp, fill=0.0)
    gam.v[:C], bet.v[:C] = gamma.float().cuda(), beta.float().cuda()
    sc, sh, sm, si = G.Vec(Cp), G.Vec(Cp), G.Vec(Cp), G.Vec(Cp)
    ops.bn_finalize_fwd(stats.v, float(M), gam.v, bet.v, EPS, 0.01, None, None, None, sc.v, sh.v, sm.v, si.v, C, stat_rows=rows, stat_ld=Cp)
    Y = G.Act(M, C, ld, dtype)
    ops.bn_apply(X.t, sc.v, sh.v, act, res.t if res else None, Y.t, M, C)
    torch.cuda.synchronize()
    fb = fwd_bounds(xs, gamma, beta, float(M))
    e_pre = 8 * U * ((xs * fb["s"]).abs() + fb["h"].abs()) + xs.abs() * fb["scale"] + fb["shift"]
    base = e_pre + (8 * U * res.stored().abs() if res else 0.0)
    y = Y.read("y")
    bound = swish_bound("fwd", base, ref["y"], y, dtype) if act == 3 else base + (2.0 ** -8 * ref["y"].abs() if dtype == torch.bfloat16 else 0.0)
    G.assert_within("y", y, ref["y"], bound)
    # backward
    srows = 64
    sv, sview = G.stats_buf(srows, Cp)
    Gt = G.Act(M, C, ld, dtype)
    ops.act_bwd_stats(DY.t, X.t, sc.v, sh.v, act, Gt.t, sview, M, Cp, stat_rows=srows)
    dgam, dbet = G.Vec(C, fill=0.25), G.Vec(C, fill=0.25)
    c1, c2, c3 = G.Vec(Cp), G.Vec(Cp), G.Vec(Cp)
    ops.bn_finalize_bwd(sv.v, float(M), gam.v, sm.v, si.v, None, None, dgam.v, dbet.v, c1.v, c2.v, c3.v, C, stat_rows=srows, stat_ld=Cp)
    DX = G.Act(M, C, ld, dtype)
    ops.bnbwd_apply(Gt.t, X.t, c1.v, c2.v, c3.v, DX.t, M, C)
    torch.cuda.synchronize()
    G.stats_total(sv, sview)
    pre = xs * fb["s"] + fb["h"]
    g_ref = R.act_grad_ref(pre, act, dys)
    eg_sw = None
    if act == 3:      # the derivative of swish: |d^2/da^2| <= 1/2, and the measured factor for __expf
        eg_sw = SWISH_BWD_K * (8 * U * g_ref.abs() + 0.5 * dys.abs() * e_pre)
        eg_sw = torch.minimum(eg_sw, 8 * U * g_ref.abs() + 0.5 * dys.abs() * e_pre + 2.0 ** -8 * g_ref.abs())
    eg_store = (eg_sw if eg_sw is not None else 0.0) + (2.0 ** -8 * g_ref.abs() if (dtype == torch.bfloat16 and act == 3) else 0.0)
    # act_bwd_stats: <= 256 pixel lanes in order after <= ceil(M / 64) per thread, then the finalize's 72
    bb = bwd_bounds(xs, g_ref, gamma, ref["mean"], fb["r"], M, n=72 + 256 + 16, eg=eg_sw, em=fb["mean"], er=fb["invstd"])
    cc1, cc2 = bb["vals"]
    e_dx = (g_ref.abs() * bb["c1"] + xs.abs() * bb["c2"] + bb["c3"] + cc1.abs() * eg_store
            + 8 * U * ((cc1 * g_ref).abs() + (cc2 * xs).abs() + (ref["dx"] - cc1 * g_ref - cc2 * xs).abs()))
    if dtype == torch.bfloat16:
        e_dx = e_dx + 2.0 ** -8 * ref["dx"].abs()
    G.assert_within("g", Gt.read("g"), g_ref, eg_store + 8 * U * g_ref.abs())
    G.assert_within("dx", DX.read("dx"), ref["dx"], e_dx)
    G.assert_within("dgamma", dgam.check("dgamma"), 0.25 + ref["dgamma"], bb["dgamma"] + 8 * U * (0.25 + ref["dgamma"].abs()))
    G.assert_within("dbeta", dbet.check("dbeta"), 0.25 + ref["dbeta"], bb["dbeta"] + 8 * U * (0.25 + ref["dbeta"].abs()))


# ---------------------------------------------------------------------------------------------------------------- act_bwd_stats
def _coeffs(gen, C):
    sc = ((torch.rand(C, generator=gen) + 0.5) * torch.where(torch.rand(C, generator=gen) > 0.3, 1.0, -1.0)).float().double()
    return sc, (torch.randn(C, generator=gen) * 0.5).float().double()


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("C", [1, 8, 9, 17, 40, 100, 257, 264])
def test_act_bwd_stats_shapes(gpu_lib, C, dt):
    """g = dy * act'(z * scale + shift) and the rows [sum g, sum g z] for M in {1, 5, 255, 257, 1000} x stat_rows in {1, 3, 1024} (the grid
    clamped to one workgroup, striding, and with tail rows to clear), the channel counts that select every lane split (lcg 0..5) and a
    second block column; masked with each activation and unmasked (scale == NULL), with g == NULL (statistics only) and with
    stats2 == NULL.  All stat_rows rows are finite afterwards; their sums are the float64 sums of the STORED g.
    Convention written down here: for swish in bf16 the kernel sums the UNROUNDED fp32 gradient (k_pool_act_bwd rounds first, this kernel
    does not), so that case is compared with the sums of the float64 gradient instead; the distance to the stored sums is printed."""
    from atomnas_amd import ops
    dtype = G.T(dt)
    gen = torch.Generator().manual_seed(C)
    Cp = pad8(C)
    k = 0
    for M in (1, 5, 255, 257, 1000):
        for srows in (1, 3, 1024):
            k += 1
            act = (None, 1, 2, 3, 0)[k % 5]                 # None: unmasked (scale == NULL)
            want_g, want_st = (k % 4 != 3), (k % 7 != 5)
            ld = Cp + 8 * (k % 2)
            if act is None:
                sc = sh = None
                zs = torch.randn(M, C, generator=gen).to(dtype).double()
                pre = zs
            else:
                sc, sh = _coeffs(gen, C)
                zs = G.margin_input(gen, M, C, sc, sh, act, dtype) if act in (1, 2) else torch.randn(M, C, generator=gen).to(dtype).double()
                pre = zs * sc + sh
            Z, DY = G.Act(M, C, ld, dtype, zs), G.Act(M, C, Cp, dtype, torch.randn(M, C, generator=gen))
            dys = DY.stored()
            g_ref = R.act_grad_ref(pre, act or 0, dys)
            Gt = G.Act(M, C, ld, dtype) if want_g else None
            sv, sview = G.stats_buf(srows, C) if want_st else (None, None)
            scv, shv = (G.cvec(sc, C), G.cvec(sh, C)) if sc is not None else (None, None)
            ops.act_bwd_stats(DY.t, Z.t, scv.v if scv else None, shv.v if shv else None, act or 0, Gt.t if Gt else None, sview, M, C,
                              stat_rows=srows if want_st else None)
            torch.cuda.synchronize()
            tag = "M%d rows%d act%s" % (M, srows, act)
            base = 8 * U * g_ref.abs()
            if act == 3:
                base = base + 0.5 * dys.abs() * 8 * U * ((zs * sc).abs() + sh.abs())
            g_sum_ref = g_ref
            if want_g:
                got = Gt.read(tag + " g")
                bound = swish_bound("bwd", base, g_ref, got, dtype) if act == 3 else base + (2.0 ** -8 * g_ref.abs() if dtype == torch.bfloat16 else 0.0)
                G.assert_within(tag + " g", got, g_ref, bound)
                if not (act == 3 and dtype == torch.bfloat16):
                    g_sum_ref = got                          # the stored values
            if want_st:
                tot = G.stats_total(sv, sview, tag + " statistics")
                e_el = torch.zeros_like(g_ref) if g_sum_ref is not g_ref or act != 3 else torch.minimum(SWISH_BWD_K * base, base + 2.0 ** -8 * g_ref.abs())
                for pl, terms, name in ((0, g_sum_ref, "sum g"), (1, g_sum_ref * zs, "sum g z")):
                    eterm = e_el if pl == 0 else e_el * zs.abs()
                    G.assert_within("%s %s" % (tag, name), tot[pl], terms.sum(0), G.sum_bound(M, terms.abs().sum(0)) + eterm.sum(0))
                if act == 3 and dtype == torch.bfloat16 and want_g:
                    d_st = float((tot[0] - Gt.stored().sum(0)).abs().max())
                    d_un = float((tot[0] - g_ref.sum(0)).abs().max())
                    print("act_bwd_stats swish bf16 %s C%d: |sum - stored sums| %.3g, |sum - unrounded sums| %.3g" % (tag, C, d_st, d_un))


@pytest.mark.parametrize("dt", G.DTYPES)
def test_masked_kernels_at_the_boundaries(gpu_lib, dt):
    """pre-activations exactly 0 and exactly 6 (scale 1, shift 0; both exact in bf16): the gradient there is 0, as in torch (ReLU'(0) = 0,
    hardtanh' = 0 at both ends) -- act_bwd_stats and pool_act_bwd; forward values through bn_apply and bn_act_pool"""
    from atomnas_amd import ops
    dtype = G.T(dt)
    C, M = 8, 6
    vals = torch.tensor([0.0, 6.0, 3.0, -1.0, 7.0, 0.0]).double()
    zs = vals.view(M, 1).repeat(1, C)
    dys = torch.full((M, C), 0.5, dtype=torch.float64)
    one, zero = G.cvec(torch.ones(C)), G.cvec(torch.zeros(C))
    for act in (1, 2):
        g_ref = R.act_grad_ref(zs, act, dys)
        assert g_ref[:, 0].tolist() == ([0, 0.5, 0.5, 0, 0.5, 0] if act == 1 else [0, 0, 0.5, 0, 0, 0])
        Z, DY, Gt = G.Act(M, C, C, dtype, zs), G.Act(M, C, C, dtype, dys), G.Act(M, C, C, dtype)
        sv, sview = G.stats_buf(2, C)
        ops.act_bwd_stats(DY.t, Z.t, one.v, zero.v, act, Gt.t, sview, M, C, stat_rows=2)
        Y = G.Act(M, C, C, dtype)
        ops.bn_apply(Z.t, one.v, zero.v, act, None, Y.t, M, C)
        # pool_act_bwd: N = M images of one pixel, dpooled = dy
        Gp = G.Act(M, C, C, dtype)
        pv, pview = G.stats_buf(2, C)
        ops.pool_act_bwd(DY.t, None, 0.0, Z.t, one.v, zero.v, act, Gp.t, pview, M, 1, C, stat_rows=2)
        Pl = G.Act(M, C, C, dtype)
        ops.bn_act_pool(Z.t, one.v, zero.v, act, Pl.t, None, 0.0, 1, None, M, 1, C)
        torch.cuda.synchronize()
        assert torch.equal(Gt.read("g"), g_ref) and torch.equal(Gp.read("pool g"), g_ref)
        assert torch.equal(Y.read("y"), R.act_ref(zs, act)) and torch.equal(Pl.read("pooled"), R.act_ref(zs, act))
        for v, view in ((sv, sview), (pv, pview)):
            tot = G.stats_total(v, view)
            assert torch.equal(tot[0], g_ref.sum(0)) and torch.equal(tot[1], (g_ref * zs).sum(0))


# ---------------------------------------------------------------------------------------------------------------- pooling head
POOL_SHAPES = [(1, 1, 1, 0), (5, 49, 13, 3), (37, 4, 1283, 2), (64, 49, 1000, 1)]     # N, HW, C, activation


def _pool_inputs(gen, N, HW, C, act, dtype):
    sc, sh = _coeffs(gen, C)
    M = N * HW
    xs = G.margin_input(gen, M, C, sc, sh, act, dtype) if act in (1, 2) else torch.randn(M, C, generator=gen).to(dtype).double()
    return sc, sh, xs


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("N,HW,C,act", POOL_SHAPES)
def test_bn_act_pool_and_dropout_mask(gpu_lib, N, HW, C, act, dt):
    """pooled[n][c] = mean_hw act(x * scale + shift) * keep / (1 - p); the keep mask equals the numpy transcription of the documented counter
    hash BIT FOR BIT for two seeds and steps 0 (step_ptr == NULL), 7 and 2^20 + 7, at p = 0.2 and 0.5; with p = 0 a given keep buffer is
    left untouched"""
    from atomnas_amd import ops
    dtype = G.T(dt)
    gen = torch.Generator().manual_seed(N * 100 + C)
    sc, sh, xs = _pool_inputs(gen, N, HW, C, act, dtype)
    Cp = pad8(C)
    X = G.Act(N * HW, C, Cp + 8, dtype, xs)
    scv, shv = G.cvec(sc, C), G.cvec(sh, C)
    pre = xs * sc + sh
    a = R.act_ref(pre, act).view(N, HW, C)
    mean = a.mean(1)
    base = G.sum_bound(HW, a.abs().sum(1)) / HW + (8 * U * ((xs * sc).abs() + sh.abs())).view(N, HW, C).mean(1)
    for p in (0.0, 0.2, 0.5):
        for seed in ((1995,) if p == 0 else (1995, 0xDEADBEEFCAFEF00D)):
            for step in ((7,) if p == 0 else (None, 7, (1 << 20) + 7)):
                pooled = G.Act(N, C, Cp + 16 if step == 7 else Cp, dtype)
                keep = G.Vec(N * C, torch.uint8)
                stp = torch.tensor([step], dtype=torch.int64).cuda() if step is not None else None
                ops.bn_act_pool(X.t, scv.v, shv.v, act, pooled.t, keep.v, p, seed, stp, N, HW, C)
                torch.cuda.synchronize()
                kv = keep.check("keep").cpu()
                if p == 0:
                    assert bool((kv == keep.marker).all()), "p = 0 must leave the keep buffer alone"
                    ref = mean
                else:
                    kr = torch.from_numpy(R.dropout_keep_ref(seed, step or 0, N, C, p))
                    assert torch.equal(kv.view(N, C), kr), "keep mask differs from the documented hash (seed %d step %s p %g)" % (seed, step, p)
                    ref = mean * kr.double() / (1 - np.float32(p).astype(np.float64))
                scale = 1.0 / (1.0 - p)
                got = pooled.read("pooled")
                b = base * scale + 8 * U * ref.abs()
                bound = swish_bound("fwd", b, ref, got, dtype) if act == 3 else b + (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0.0)
                G.assert_within("pooled p=%g" % p, got, ref, bound)


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("N,HW,C,act", POOL_SHAPES + [(3, 5, 257, 2)])
def test_pool_act_bwd(gpu_lib, N, HW, C, act, dt):
    """g[n,hw,c] = dpooled[n][c] / HW * keep / (1 - p) * act'(x * scale + shift), rounded to the storage type, and rows [sum g, sum g x] of the
    ROUNDED values, with keep given and keep == NULL, for stat_rows in {1, 8, 1024}; C = 257, 1000, 1283 span several block columns"""
    from atomnas_amd import ops
    dtype = G.T(dt)
    gen = torch.Generator().manual_seed(N * 100 + C + 1)
    sc, sh, xs = _pool_inputs(gen, N, HW, C, act, dtype)
    Cp, M = pad8(C), N * HW
    X = G.Act(M, C, Cp, dtype, xs)
    DP = G.Act(N, C, Cp + 8, dtype, torch.randn(N, C, generator=gen))
    dps = DP.stored()
    scv, shv = G.cvec(sc, C), G.cvec(sh, C)
    pre = xs * sc + sh
    p = 0.2
    keep = (torch.rand(N, C, generator=gen) >= p).to(torch.uint8)
    kd = G.Vec(N * C, torch.uint8, fill=keep.flatten())
    for use_keep, srows in ((True, 1), (True, 8), (False, 1024), (True, 1024)):
        dflat = dps / HW
        if use_keep:
            dflat = dflat * keep.double() / (1.0 - float(np.float32(p)))
        dy = dflat.view(N, 1, C).expand(N, HW, C).reshape(M, C)
        g_ref = R.act_grad_ref(pre, act, dy)
        Gt = G.Act(M, C, Cp + 8, dtype)
        sv, sview = G.stats_buf(srows, C)
        ops.pool_act_bwd(DP.t, kd.v if use_keep else None, p, X.t, scv.v, shv.v, act, Gt.t, sview, N, HW, C, stat_rows=srows)
        torch.cuda.synchronize()
        tag = "keep%d rows%d" % (use_keep, srows)
        got = Gt.read(tag + " g")
        base = 8 * U * g_ref.abs() * 2
        if act == 3:
            base = base + 0.5 * dy.abs() * 8 * U * ((xs * sc).abs() + sh.abs())
        bound = swish_bound("bwd", base, g_ref, got, dtype) if act == 3 else base + (2.0 ** -8 * g_ref.abs() if dtype == torch.bfloat16 else 0.0)
        G.assert_within(tag + " g", got, g_ref, bound)
        tot = G.stats_total(sv, sview, tag + " statistics")
        G.assert_within(tag + " sum g", tot[0], got.sum(0), G.sum_bound(M, got.abs().sum(0)))
        G.assert_within(tag + " sum g x", tot[1], (got * xs).sum(0), G.sum_bound(M, (got * xs).abs().sum(0)))
