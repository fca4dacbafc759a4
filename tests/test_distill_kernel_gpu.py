"""csrc/head.hip k_ce_distill at kernel level (GPU): the label-smoothed cross entropy with a soft-target term from a teacher's logits, at
edge shapes, in both storage types, against the float64 reference tests/distill_ref.py, outputs inside NaN-filled allocations
(tests/glue_util.py).

Bounds (u = 2^-24; s the student's row, t the teacher's, z = x / T, lq_j = zt_j - lse_q, lp_j = zs_j - lse_p, d_j = lq_j - lp_j):
  * a log-probability z_j - lse carries the rounding of z_j (u |z_j|; exact for the T = 1, 4 used here), of lse = mx + log(se)
    (u |lse|, plus the relative error of se: every exp(z_k - mx) inherits u |z_k - mx| from its argument, weighted by its probability,
    and the lane sums add (K / 64 + 6) u) and of the difference: at most about 4 u A with A = max_k |z_k| + |lse|.
  * kd = T^2 sum_j q_j d_j with q_j = exp(lq_j): q_j has the relative error of its argument (4 u A_q) and of expf (2 u), d_j the absolute
    error 4 u (A_q + A_p), the fixed-order sum (K / 64 + 8) u sum_j q_j |d_j|.  With S = sum_j q_j |d_j| and sum_j q_j = 1:
        |kd - ref| <= T^2 * 8 u * [(A_q + A_p) + (A_q + K / 64 + 8) * S]
    (8 for the derived 4: the factor of two the project's bounds carry).  Measured on these inputs against the float64 reference:
    the largest error of kd is 0.055 of this bound and that of the loss 0.055 of its bound (first reached at K = 64); the gradient
    reaches 0.22 of its bound in fp32 at K = 4 and 0.99 in bf16 (the half ulp of the storage type, which the 2^-8 |ref| term is); the
    shape test prints the figures per output and storage type.
  * loss = (1 - alpha) CE + alpha kd: (1 - alpha) times test_head_kernels_gpu's bound of CE, alpha times the bound of kd, and the last
    addition's 8 u (|(1 - alpha) CE| + |alpha kd|).
  * dlogits = [(1 - alpha)(p_j - tgt_j) + alpha T (pT_j - q_j)] gscale / B: every probability exp(x - lse) has the relative error
    u (1 + |x| + |lse|) of its argument, as in test_head_kernels_gpu._ce_check, then the short expression: elem_bound of
        [(1 - alpha)(p (1 + |s| + |lse|) + tgt) + alpha T (pT (1 + |zs| + |lse_p|) + q (1 + |zt| + |lse_q|))] gscale / B.

Single-line changes to k_ce_distill these tests were written to catch: `lq - lp` formed as logf(q) - logf(pT) (NaN where q underflows),
one max subtraction shared by the two tempered soft-maxes (overflow), the T^2 or the T of the gradient dropped, the teacher's row read
at the student's pitch, padding columns read, `wce * ce` folded differently from k_ce_smooth (alpha = 0 bits).
"""
import ctypes

import pytest
import torch

import distill_ref as D
import glue_ref as R
import glue_util as G
from glue_util import U

pytestmark = pytest.mark.gpu

CE_B = (1, 3, 4, 5, 33)
RATIO = {}   # largest error / bound seen in this process per output and storage type (printed by the shape test)


def _inputs(B, K, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, K, generator=gen) * 30).float()   # every soft-max overflows fp32 without its max subtraction
    t = (torch.randn(B, K, generator=gen) * 30).float()   # drawn independently: q underflows to 0 for many classes at T = 1
    y = torch.randint(0, K, (B,), generator=gen)
    return x, t, y


class Launch:
    def __init__(self, ops, x, t, y, eps, alpha, T, gscale, dtype, ldl, ldt, ldd, want=("loss", "kd", "dl", "topk"), topk0=(3, 9)):
        B, K = x.shape
        self.lg = G.Act(B, K, ldl, torch.float32)
        self.lg.t[:, :K] = x.cuda()                          # every padding column of both logit tensors stays NaN
        self.tc = G.Act(B, K, ldt, torch.float32)
        self.tc.t[:, :K] = t.cuda()
        self.loss = G.Vec(B) if "loss" in want else None
        self.kd = G.Vec(B) if "kd" in want else None
        self.dl = G.Act(B, K, ldd, dtype) if "dl" in want else None
        self.topk = G.Vec(2, torch.int32, fill=torch.tensor(topk0)) if "topk" in want else None
        self.topk0 = topk0
        v = lambda o: o.v if o is not None else None
        ops.ce_distill(self.lg.t, self.tc.t, y.cuda(), eps, alpha, T, B, K, v(self.loss), v(self.kd), self.dl.t if self.dl else None, gscale,
                       v(self.topk))
        torch.cuda.synchronize()

    def dl_values(self, K):
        B = self.dl.M
        assert bool(torch.isnan(self.dl.full[:G.GUARD]).all()) and bool(torch.isnan(self.dl.full[G.GUARD + B:]).all()), "dlogits: a write outside the rows"
        got = self.dl.t.double().cpu()
        assert bool((got[:, K:] == 0).all()), "dlogits: the padding K..ldd-1 is not zero"
        return got[:, :K]


def _within(name, got, ref, bound, dtype):
    err = G.assert_within(name, got, ref, bound)
    b = bound.double().cpu()
    key = "%s %s" % (name, "bf16" if dtype == torch.bfloat16 else "fp32")
    RATIO[key] = max(RATIO.get(key, 0.0), float(((got.double().cpu() - ref.double().cpu()).abs() / b).max()))
    return err


def _check(x, t, y, eps, alpha, T, gscale, dtype, L, ref=None):
    B, K = x.shape
    ref = ref or D.distill_ref(x, t, y, eps, alpha, T, gscale)
    xd, td = x.double(), t.double()
    zs, zt = xd / T, td / T
    lse, lse_p, lse_q = torch.logsumexp(xd, 1), torch.logsumexp(zs, 1), torch.logsumexp(zt, 1)
    lq, lp = zt - lse_q.view(-1, 1), zs - lse_p.view(-1, 1)
    q, pT = torch.exp(lq), torch.exp(lp)
    A_q, A_p = zt.abs().max(1).values + lse_q.abs(), zs.abs().max(1).values + lse_p.abs()
    S = (q * (lq - lp).abs()).sum(1)
    kd_bound = T * T * 8 * U * ((A_q + A_p) + (A_q + K / 64 + 8) * S) + G.TINY
    if L.kd is not None:
        _within("kd", L.kd.check("kd"), ref["kd"], kd_bound, torch.float32)
    if L.loss is not None:
        ce = ref["ce"]
        ce_bound = 1e-4 * ce.abs() + 1e-4 * float(ce.pow(2).mean().sqrt()) + 8 * U * (xd.gather(1, y.view(-1, 1)).flatten().abs() + lse.abs())
        bound = (1 - alpha) * ce_bound + alpha * kd_bound + 8 * U * ((1 - alpha) * ce.abs() + alpha * ref["kd"].abs()) + G.TINY
        _within("loss", L.loss.check("loss"), ref["loss"], bound, torch.float32)
    if L.dl is not None:
        p = torch.exp(xd - lse.view(-1, 1))
        tgt = torch.full_like(p, eps / K)
        tgt[torch.arange(B), y] += 1 - eps
        terms = ((1 - alpha) * (p * (1 + xd.abs() + lse.abs().view(-1, 1)) + tgt)
                 + alpha * T * (pT * (1 + zs.abs() + lse_p.abs().view(-1, 1)) + q * (1 + zt.abs() + lse_q.abs().view(-1, 1)))) * (gscale / B)
        _within("dlogits", L.dl_values(K), ref["dlogits"], G.elem_bound(terms, ref["dlogits"], L.dl.dtype), L.dl.dtype)
    if L.topk is not None:
        assert L.topk.check("topk").tolist() == [L.topk0[0] + ref["top1"], L.topk0[1] + ref["top5"]]
    return ref


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("K", [1, 4, 5, 63, 64, 65, 1000, 1001])
def test_ce_distill_shapes(gpu_lib, K, dt):
    """every B in {1, 3, 4, 5, 33} with eps in {0, 0.1} x alpha in {0, 0.3, 1} x T in {1, 4} x gscale in {1, 0.25}; both logit tensors scaled
    by 30 and drawn independently, three different pitches beyond K with NaN in the logits' padding; the counters accumulate onto (3, 9)"""
    from atomnas_amd import ops
    for B in CE_B:
        x, t, y = _inputs(B, K, 100 * K + B)
        ldl, ldt, ldd = G.pad8(K) + 8, G.pad8(K) + 24, G.pad8(K) + 16
        for eps in (0.0, 0.1):
            for alpha in (0.0, 0.3, 1.0):
                for T in (1.0, 4.0):
                    ref = D.distill_ref(x, t, y, eps, alpha, T, 1.0)
                    assert bool(torch.isfinite(ref["kd"]).all())
                    for gscale in (1.0, 0.25):
                        L = Launch(ops, x, t, y, eps, alpha, T, gscale, G.T(dt), ldl, ldt, ldd)
                        _check(x, t, y, eps, alpha, T, gscale, G.T(dt), L, dict(ref, dlogits=ref["dlogits"] * gscale))
        if K >= 63 and B > 1:
            assert int((torch.softmax(t, 1) == 0).sum()) > 0   # q does underflow in fp32 on these inputs
    print("ce_distill K=%d %s: largest error / bound %s" % (K, dt, {k: round(v, 4) for k, v in sorted(RATIO.items())}))


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("K", [1, 5, 64, 65, 1000, 1001])
def test_alpha_zero_has_the_bits_of_ce_smooth(gpu_lib, K, dt):
    """alpha = 0 and a finite teacher: loss_per_sample, dlogits and the counters are bit-identical to atomnas_ce_smooth's on the same
    student inputs, whatever T; kd is still the teacher's term"""
    from atomnas_amd import ops
    for B in (1, 5, 33):
        x, t, y = _inputs(B, K, 7 * K + B)
        for eps, gscale, T in ((0.0, 1.0, 1.0), (0.1, 0.25, 4.0), (0.1, 1.0, 3.0)):
            ld = G.pad8(K) + 8
            L = Launch(ops, x, t, y, eps, 0.0, T, gscale, G.T(dt), ld, ld, ld)
            lg = G.Act(B, K, ld, torch.float32)
            lg.t[:, :K] = x.cuda()
            loss, dl, topk = G.Vec(B), G.Act(B, K, ld, G.T(dt)), G.Vec(2, torch.int32, fill=torch.tensor((3, 9)))
            ops.ce_smooth(lg.t, y.cuda(), eps, B, K, loss.v, dl.t, gscale, topk.v)
            torch.cuda.synchronize()
            assert torch.equal(L.loss.v, loss.v), "loss differs from ce_smooth at alpha = 0"
            assert torch.equal(L.dl.t, dl.t), "dlogits differ from ce_smooth at alpha = 0"
            assert torch.equal(L.topk.v, topk.v)
            assert bool(torch.isfinite(L.kd.v).all())


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("K", [1, 5, 64, 65, 1000, 1001])
def test_teacher_equal_to_student_is_exactly_the_scaled_cross_entropy(gpu_lib, K, dt):
    """teacher == logits bit for bit: kd is exactly 0 at any T, the gradient does not depend on T (its soft part is exactly 0), and with
    alpha = 0.5 -- an exact scaling -- gradient and loss are ce_smooth's: dlogits at twice the gscale, loss at half the value"""
    from atomnas_amd import ops
    for B in (1, 4, 33):
        x, _, y = _inputs(B, K, 11 * K + B)
        ld = G.pad8(K) + 8
        for eps in (0.1,):
            base = None
            for T in (1.0, 4.0, 3.0):
                L = Launch(ops, x, x.clone(), y, eps, 0.3, T, 1.0, G.T(dt), ld, ld + 8, ld)
                assert bool((L.kd.check("kd") == 0).all()), "kd is not exactly zero for teacher == student (T = %g)" % T
                base = base or L
                assert torch.equal(L.dl.t, base.dl.t) and torch.equal(L.loss.v, base.loss.v), "the soft part is not exactly zero at T = %g" % T
            _check(x, x.clone(), y, eps, 0.3, 1.0, 1.0, G.T(dt), base)
            H = Launch(ops, x, x.clone(), y, eps, 0.5, 4.0, 2.0, G.T(dt), ld, ld, ld)
            lg = G.Act(B, K, ld, torch.float32)
            lg.t[:, :K] = x.cuda()
            loss, dl = G.Vec(B), G.Act(B, K, ld, G.T(dt))
            ops.ce_smooth(lg.t, y.cuda(), eps, B, K, loss.v, dl.t, 1.0, None)
            torch.cuda.synchronize()
            assert torch.equal(H.dl.t, dl.t), "alpha = 0.5, gscale 2: not the cross-entropy gradient"
            assert torch.equal(H.loss.v, loss.v * 0.5)


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("absent", ["loss", "kd", "dl", "topk"])
def test_ce_distill_optional_arguments(gpu_lib, absent, dt):
    """each of loss_per_sample, kd_per_sample, dlogits and topk NULL in turn: the others are computed as before; exact pitches"""
    from atomnas_amd import ops
    B, K = 5, 64
    x, t, y = _inputs(B, K, 7)
    want = tuple(w for w in ("loss", "kd", "dl", "topk") if w != absent)
    L = Launch(ops, x, t, y, 0.1, 0.3, 4.0, 0.25, G.T(dt), K, K, K, want=want)
    _check(x, t, y, 0.1, 0.3, 4.0, 0.25, G.T(dt), L)


def test_ce_distill_ties_count_as_hits(gpu_lib):
    """the convention of test_head_kernels_gpu.test_ce_smooth_ties_count_as_hits on the new entry: rank = #{j : s_j > s_y} of the STUDENT's
    logits; a teacher that ranks the classes differently changes nothing"""
    from atomnas_amd import ops
    K = 70
    x = torch.full((4, K), -50.0)
    x[0] = 2.0
    x[1, :8] = torch.tensor([9.0, 8.0, 7.0, 6.0, 1.0, 1.0, 1.0, 0.0])
    x[2] = x[1]
    x[3] = x[1]
    x[3, 69] = 10.0
    y = torch.tensor([37, 6, 64, 5])
    x[2, 64] = 1.0
    t = x.flip(1).contiguous()
    ref = D.distill_ref(x, t, y, 0.1, 0.3, 2.0, 1.0)
    assert ref["rank"].tolist() == [0, 4, 4, 5] and (ref["top1"], ref["top5"]) == (1, 3)
    assert (ref["top1"], ref["top5"]) == (R.ce_ref(x, y, 0.1, 1.0)["top1"], R.ce_ref(x, y, 0.1, 1.0)["top5"])
    L = Launch(ops, x, t, y, 0.1, 0.3, 2.0, 1.0, torch.float32, K + 2, K + 10, K + 2, topk0=(0, 0))
    assert L.topk.check("topk").tolist() == [1, 3]


@pytest.mark.parametrize("dt", G.DTYPES)
def test_ce_distill_is_reproducible_and_row_independent(gpu_lib, dt):
    """two launches of the same inputs are bit-identical; loss and kd of row i of a B = 33 launch are those of the row launched alone"""
    from atomnas_amd import ops
    B, K = 33, 1001
    x, t, y = _inputs(B, K, 5)
    ld = G.pad8(K) + 8
    a = Launch(ops, x, t, y, 0.1, 0.3, 4.0, 1.0, G.T(dt), ld, ld, ld)
    b = Launch(ops, x, t, y, 0.1, 0.3, 4.0, 1.0, G.T(dt), ld, ld, ld)
    for u, v in ((a.loss.v, b.loss.v), (a.kd.v, b.kd.v), (a.dl.t, b.dl.t), (a.topk.v, b.topk.v)):
        assert torch.equal(u, v)
    for i in (0, 3, 4, 17, 32):
        one = Launch(ops, x[i:i + 1], t[i:i + 1], y[i:i + 1], 0.1, 0.3, 4.0, 1.0, G.T(dt), ld, ld, ld)
        assert torch.equal(one.loss.v, a.loss.v[i:i + 1]) and torch.equal(one.kd.v, a.kd.v[i:i + 1]), "row %d depends on its batch" % i


def test_ce_distill_refuses_bad_arguments(gpu_lib):
    """NULL logits / teacher / target, B <= 0, K <= 0, pitches below K, T <= 0 and alpha outside [0, 1] return an error with
    atomnas_last_error set; nothing is launched (the outputs keep their NaN)"""
    from atomnas_amd import _lib
    lib = _lib.load()
    B, K = 4, 16
    x, t, y = _inputs(B, K, 3)
    xs, ts, ys = x.cuda(), t.cuda(), y.cuda()
    loss, kd, dl = G.Vec(B), G.Vec(B), G.Act(B, K, K, torch.float32)
    topk = G.Vec(2, torch.int32, fill=torch.tensor((3, 9)))
    P = lambda z: ctypes.c_void_p(z.data_ptr())
    good = dict(logits=P(xs), ldl=K, teacher=P(ts), ldt=K, target=P(ys), eps=0.1, alpha=0.3, T=2.0, B=B, K=K, ldd=K)
    cases = [dict(logits=None), dict(teacher=None), dict(target=None), dict(B=0), dict(B=-1), dict(K=0), dict(ldl=K - 1), dict(ldt=K - 1),
             dict(ldd=K - 1), dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan"))]
    for c in cases:
        a = dict(good, **c)
        rc = lib.atomnas_ce_distill(a["logits"], a["ldl"], a["teacher"], a["ldt"], a["target"], a["eps"], a["alpha"], a["T"], a["B"], a["K"],
                                    P(loss.v), P(kd.v), P(dl.t), a["ldd"], 1.0, P(topk.v), 0, None)
        assert rc != 0, c
        assert b"ce_distill" in lib.atomnas_last_error(), (c, lib.atomnas_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss.full).all()) and bool(torch.isnan(kd.full).all()) and bool(torch.isnan(dl.full).all())
    assert topk.check("topk").tolist() == [3, 9]
    rc = lib.atomnas_ce_distill(good["logits"], K, good["teacher"], K, good["target"], 0.1, 0.3, 2.0, B, K, P(loss.v), P(kd.v), P(dl.t), K, 1.0,
                                P(topk.v), 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isfinite(loss.v).all())


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_distill_criterion_is_the_kernel_with_autograd_around_it(gpu_lib, reduction):
    """utils.optim.DistillCrossEntropy (eager use outside TrainStep): per-sample values and hit counts are those of a direct launch with
    gscale = B, the gradient through grad_output is that launch's dlogits times d(reduction)/d(loss_i), the teacher's logits get none;
    and the values are the reference's within the bounds of the shape test"""
    from atomnas_amd import ops
    from atomnas_amd.utils import optim
    B, K, eps, alpha, T = 5, 65, 0.1, 0.3, 4.0
    x, t, y = _inputs(B, K, 21)
    crit = optim.DistillCrossEntropy(K, eps, alpha, T, reduction=reduction)
    xs, tc = x.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    out = crit(xs, tc, y.cuda())
    out.sum().backward()
    L = Launch(ops, x, t, y, eps, alpha, T, float(B), torch.float32, G.pad8(K), G.pad8(K), G.pad8(K), topk0=(0, 0))
    _check(x, t, y, eps, alpha, T, float(B), torch.float32, L)
    per = {"none": L.loss.v, "mean": L.loss.v.mean(), "sum": L.loss.v.sum()}[reduction]
    assert torch.equal(out.detach(), per) and torch.equal(crit.kd, L.kd.v) and torch.equal(crit.topk_correct, L.topk.v)
    scale = torch.tensor(1.0 / B if reduction == "mean" else 1.0, device="cuda")
    assert torch.equal(xs.grad, L.dl.t[:, :K] * scale) and tc.grad is None
