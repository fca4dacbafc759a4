"""csrc/head.hip at kernel level (GPU): label-smoothed cross entropy with its top-k counters, the classifier-bias column sum and the
stem's im2col, at edge shapes, in both storage types, against float64 references (tests/glue_ref.py), outputs inside NaN-filled
allocations (tests/glue_util.py).

Single-line changes to csrc/head.hip these tests were seen to catch (tried on a scratch build of the library):
  k_ce_smooth     a logit equal to the target's outranks it (`v >= xy && j != y`)  -> test_ce_smooth_ties_count_as_hits
  k_colsum        `out[c] =` for `out[c] +=`                                        -> test_colsum_accumulates
  k_im2col_stem   columns 32..ld-1 left unwritten (the kernel before this fix)      -> test_im2col_stem[*-40-*]
"""
import pytest
import torch
import torch.nn.functional as F

import glue_ref as R
import glue_util as G
from glue_util import U

pytestmark = pytest.mark.gpu

CE_B = (1, 3, 4, 5, 33)


def _ce_inputs(B, K, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, K, generator=gen) * 30).float()          # exp(x) overflows fp32 without the max subtraction
    y = torch.randint(0, K, (B,), generator=gen)
    return x, y


def _ce_launch(ops, x, y, eps, gscale, dtype, ldl, ldd, want_loss=True, want_dl=True, topk0=(3, 9)):
    B, K = x.shape
    lg = G.Act(B, K, ldl, torch.float32)
    lg.t[:, :K] = x.cuda()                                        # every padding column of the logits stays NaN
    loss = G.Vec(B) if want_loss else None
    dl = G.Act(B, K, ldd, dtype) if want_dl else None
    topk = G.Vec(2, torch.int32, fill=torch.tensor(topk0)) if topk0 is not None else None
    ops.ce_smooth(lg.t, y.cuda(), eps, B, K, loss.v if loss else None, dl.t if dl else None, gscale, topk.v if topk else None)
    torch.cuda.synchronize()
    return loss, dl, topk


def _ce_check(x, y, eps, gscale, dtype, loss, dl, topk, topk0=(3, 9)):
    B, K = x.shape
    ref = R.ce_ref(x, y, eps, gscale)
    xd = x.double()
    lse = torch.logsumexp(xd, 1)
    if loss is not None:
        # the bench sweep's bound (rtol 1e-4 of the value and of the batch's rms) plus the fp32 bound of the last subtraction x_y - lse
        rl = ref["loss"]
        bound = 1e-4 * rl.abs() + 1e-4 * float(rl.pow(2).mean().sqrt()) + 8 * U * (xd.gather(1, y.view(-1, 1)).flatten().abs() + lse.abs())
        G.assert_within("loss", loss.check("loss"), rl, bound)
    if dl is not None:
        # g = (p - t) * gscale / B with p = exp(x_j - lse): the exponent carries the rounding of x_j - lse (relative error of p
        # <= u (|x_j| + |lse|) each for the operands and the difference), then the short expression
        p = torch.exp(xd - lse.view(-1, 1))
        t = (ref["dlogits"] / (gscale / B) - p).abs()
        terms = (p * (1 + xd.abs() + lse.abs().view(-1, 1)) + t) * (gscale / B)
        assert bool(torch.isnan(dl.full[:G.GUARD]).all()) and bool(torch.isnan(dl.full[G.GUARD + B:]).all()), "dlogits: a write outside the rows"
        got = dl.t.double().cpu()
        assert bool((got[:, K:] == 0).all()), "dlogits: the padding K..ldd-1 is not zero"
        G.assert_within("dlogits", got[:, :K], ref["dlogits"], G.elem_bound(terms, ref["dlogits"], dl.dtype))
    if topk is not None:
        assert topk.check("topk").tolist() == [topk0[0] + ref["top1"], topk0[1] + ref["top5"]]
    return ref


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("K", [1, 4, 5, 63, 64, 65, 1000, 1001])
def test_ce_smooth_shapes(gpu_lib, K, dt):
    """every B in {1, 3, 4, 5, 33} (one wave per sample, four per workgroup) with eps in {0, 0.1} x gscale in {1, 0.25}; logits scaled
    by 30, pitches beyond K with NaN in the logits' padding; the counters accumulate onto (3, 9)"""
    from atomnas_amd import ops
    for B in CE_B:
        x, y = _ce_inputs(B, K, 100 * K + B)
        for eps in (0.0, 0.1):
            for gscale in (1.0, 0.25):
                ldl, ldd = G.pad8(K) + 8, G.pad8(K) + 16
                loss, dl, topk = _ce_launch(ops, x, y, eps, gscale, G.T(dt), ldl, ldd)
                ref = _ce_check(x, y, eps, gscale, G.T(dt), loss, dl, topk)
        # tie-free inputs: the convention's hits are torch.topk's
        top = x.topk(min(5, K), 1).indices
        assert ref["top1"] == int((top[:, 0] == y).sum()) and ref["top5"] == int((top == y.view(-1, 1)).any(1).sum())


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("absent", ["loss", "dlogits", "topk"])
def test_ce_smooth_optional_arguments(gpu_lib, absent, dt):
    """each of loss_per_sample, dlogits and topk NULL in turn: the others are computed as before; exact pitches (ldl = K = ldd)"""
    from atomnas_amd import ops
    B, K = 5, 64
    x, y = _ce_inputs(B, K, 7)
    loss, dl, topk = _ce_launch(ops, x, y, 0.1, 0.25, G.T(dt), K, K, want_loss=absent != "loss", want_dl=absent != "dlogits",
                                topk0=None if absent == "topk" else (3, 9))
    _ce_check(x, y, 0.1, 0.25, G.T(dt), loss, dl, topk)


def test_ce_smooth_ties_count_as_hits(gpu_lib):
    """The kernel's convention is rank = #{j : x_j > x_y}, hit_k = rank < k: a logit EQUAL to the target's does not outrank it, so ties
    count as hits.  torch.topk leaves the order of equal values undefined, so this is a convention of this project, pinned here against
    ce_ref: a row of equal logits is a top-1 and a top-5 hit whatever its target; a target tied for fifth place (four larger logits,
    three equal ones) is a top-5 hit; one with five larger logits is not."""
    from atomnas_amd import ops
    K = 70
    x = torch.full((4, K), -50.0)
    x[0] = 2.0
    x[1, :8] = torch.tensor([9.0, 8.0, 7.0, 6.0, 1.0, 1.0, 1.0, 0.0])
    x[2] = x[1]
    x[3] = x[1]
    x[3, 69] = 10.0           # a fifth larger logit, in the second round of the lanes
    y = torch.tensor([37, 6, 64, 5])
    x[2, 64] = 1.0            # the target ties from the second round of the lanes
    ref = R.ce_ref(x, y, 0.1, 1.0)
    assert ref["rank"].tolist() == [0, 4, 4, 5] and (ref["top1"], ref["top5"]) == (1, 3)
    loss, dl, topk = _ce_launch(ops, x, y, 0.1, 1.0, torch.float32, K + 2, K + 2, topk0=(0, 0))
    assert topk.check("topk").tolist() == [1, 3]


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("C", [1, 255, 256, 257, 1000])
def test_colsum_accumulates(gpu_lib, C, dt):
    """out[c] += sum_m x[m][c] for M in {1, 3, 4, 5, 7, 256} (the 4-way unrolled rows and their tail), pitch beyond C: `out` starts at 0.25
    and comes back as 0.25 + the sum -- the entry point ACCUMULATES (into the zeroed gradient arena)"""
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(C)
    for M in (1, 3, 4, 5, 7, 256):
        x = G.Act(M, C, G.pad8(C) + 8, G.T(dt), torch.randn(M, C, generator=gen))
        out = G.Vec(C, fill=0.25)
        ops.colsum(x.t, out.v, M, C)
        torch.cuda.synchronize()
        xs = x.stored()
        G.assert_within("colsum M=%d" % M, out.check("colsum"), 0.25 + xs.sum(0), G.sum_bound(M + 1, 0.25 + xs.abs().sum(0)))


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("ld", [32, 40])
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 5, 7), (3, 8, 6), (2, 33, 17)])
def test_im2col_stem(gpu_lib, N, H, W, ld, dt):
    """3x3 / stride 2 / pad 1 patches of an NCHW fp32 image as rows of 27 values in the storage type, columns 27..ld-1 ZERO for every
    admitted pitch (ld = 40: the kernel used to leave columns 32..39 unwritten), nothing outside the rows"""
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(N * 100 + H)
    img = torch.randn(N, 3, H, W, generator=gen)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    M = N * Ho * Wo
    ref = F.unfold(img, 3, padding=1, stride=2).permute(0, 2, 1).reshape(M, 27).to(G.T(dt)).double()
    full = torch.full((M + 2 * G.GUARD, ld), G.NAN, dtype=G.T(dt), device="cuda")
    col = full[G.GUARD:G.GUARD + M]
    ops.im2col_stem(img.cuda().contiguous(), col, N, H, W)
    torch.cuda.synchronize()
    assert bool(torch.isnan(full[:G.GUARD]).all()) and bool(torch.isnan(full[G.GUARD + M:]).all()), "a write outside the rows"
    got = col.double().cpu()
    assert torch.equal(got[:, :27], ref)
    assert bool((got[:, 27:] == 0).all()), "columns 27..ld-1 must be zero"
