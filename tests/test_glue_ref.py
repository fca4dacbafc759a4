"""Keeps tests/glue_ref.py honest (CPU): each reference against an independent statement of the same operation."""
import numpy as np
import pytest
import torch

import glue_ref as R


# ---------------------------------------------------------------------------------------------------------------- dropout hash
def _z_binom(k, n, q):
    return (k - n * q) / np.sqrt(n * q * (1 - q))


def _lag1_z(keep, axis, q):
    """normalised lag-1 covariance of the centred mask along an axis: N(0, 1) for independent Bernoulli(q) draws"""
    a = keep.astype(np.float64) - q
    prod = (a[1:] * a[:-1]) if axis == 0 else (a[:, 1:] * a[:, :-1])
    if prod.size == 0:
        return 0.0
    return float(prod.sum() / (q * (1 - q)) / np.sqrt(prod.size))


@pytest.mark.parametrize("N,C,p", [(64, 1000, 0.2), (37, 1283, 0.2), (64, 1000, 0.5)])
def test_dropout_keep_ref_statistics(N, C, p):
    """The transcribed counter hash behaves like independent Bernoulli(1 - p) draws: overall, per sample, per channel, between
    neighbours along both axes, and against the masks of the next step and of the next seed (expected agreement p^2 + (1-p)^2).
    Everything within 5 binomial sigma, at fixed inputs."""
    seed, step = 1995, 7
    keep = R.dropout_keep_ref(seed, step, N, C, p)
    assert keep.shape == (N, C) and keep.dtype == np.uint8 and int(keep.max()) <= 1
    q = 1.0 - p
    zs = {"all": _z_binom(float(keep.sum()), N * C, q)}
    zs["sample"] = float(np.abs(_z_binom(keep.sum(1).astype(np.float64), C, q)).max())
    zs["channel"] = float(np.abs(_z_binom(keep.sum(0).astype(np.float64), N, q)).max())
    zs["lag n"] = _lag1_z(keep, 0, q)
    zs["lag c"] = _lag1_z(keep, 1, q)
    agree = p * p + q * q
    zs["step"] = _z_binom(float((keep == R.dropout_keep_ref(seed, step + 1, N, C, p)).sum()), N * C, agree)
    zs["seed"] = _z_binom(float((keep == R.dropout_keep_ref(seed + 1, step, N, C, p)).sum()), N * C, agree)
    print({k: round(float(v), 2) for k, v in zs.items()})
    for k, v in zs.items():
        assert abs(v) <= 5.0, (k, v)


def test_dropout_hash_ref_is_splitmix64_of_the_documented_key():
    """a few elements against the formula in python integers (unbounded, masked to 64 bits)"""
    M = (1 << 64) - 1
    seed, step, N, C = 0xDEADBEEFCAFEF00D, (1 << 20) + 7, 5, 13
    r = R.dropout_hash_ref(seed, step, N, C)
    for n, c in ((0, 0), (0, 12), (4, 12), (3, 5)):
        key = seed ^ ((step * 0x100000001B3) & M) ^ (((n * C + c) << 20) & M)
        key = (key + 0x9E3779B97F4A7C15) & M
        key = ((key ^ (key >> 30)) * 0xBF58476D1CE4E5B9) & M
        key = ((key ^ (key >> 27)) * 0x94D049BB133111EB) & M
        key = key ^ (key >> 31)
        assert int(r[n, c]) == key >> 32
    assert R.dropout_keep_ref(seed, step, N, C, 0.0).all()


# ---------------------------------------------------------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,K", [(1, 1), (3, 5), (33, 1001)])
def test_ce_ref_matches_torch_cross_entropy(B, K, eps):
    g = torch.Generator().manual_seed(B * 1000 + K)
    x = torch.randn(B, K, generator=g, dtype=torch.float64) * 30
    y = torch.randint(0, K, (B,), generator=g)
    out = R.ce_ref(x, y, eps, 0.25)
    xr = x.clone().requires_grad_(True)
    want = torch.nn.CrossEntropyLoss(label_smoothing=eps, reduction="none")(xr, y)
    want.mean().backward()
    assert torch.allclose(out["loss"], want.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(out["dlogits"], xr.grad * 0.25, rtol=1e-12, atol=1e-15)
    top = x.topk(min(5, K), 1).indices                      # tie-free: torch.topk is well defined
    assert out["top1"] == int((top[:, 0] == y).sum())
    assert out["top5"] == int((top == y.view(-1, 1)).any(1).sum())


def test_ce_ref_counts_ties_as_hits():
    x = torch.zeros(2, 8, dtype=torch.float64)
    x[1] = torch.tensor([9.0, 8.0, 7.0, 6.0, 1.0, 1.0, 1.0, 0.0])
    out = R.ce_ref(x, torch.tensor([3, 6]), 0.1, 1.0)
    assert out["rank"].tolist() == [0, 4] and out["top1"] == 1 and out["top5"] == 2


# ---------------------------------------------------------------------------------------------------------------- RMSprop + EMA
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_rmsprop_ref_matches_torch_rmsprop(momentum):
    """eps outside the sqrt, not centered: torch.optim.RMSprop's arithmetic, three steps, weight decay and gradient scale included"""
    g = torch.Generator().manual_seed(3)
    n, lr, alpha, eps, wd, gs = 257, 0.05, 0.9, 1e-3, 1e-2, 0.5
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    tp = p0.clone().requires_grad_(True)
    opt = torch.optim.RMSprop([tp], lr=lr, alpha=alpha, eps=eps, weight_decay=wd, momentum=momentum, centered=False)
    p, sq, buf, ema = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), p0.clone()
    for _ in range(3):
        gr = torch.randn(n, generator=g, dtype=torch.float64)
        tp.grad = gr * gs
        opt.step()
        out = R.rmsprop_ref(p, gr, sq, buf, ema, torch.full((n,), wd, dtype=torch.float64), lr, alpha, eps, momentum, False, gs, 0.75)
        assert abs(out["l2"] - 0.5 * wd * float((p * p).sum())) <= 1e-12
        want_ema = 0.75 * ema + 0.25 * out["p"]
        p, sq, buf, ema = out["p"], out["sq"], out["buf"], out["ema"]
        assert torch.allclose(p, tp.detach(), rtol=1e-12, atol=1e-14)
        assert torch.allclose(ema, want_ema, rtol=1e-12, atol=1e-14)
    assert torch.allclose(sq, opt.state[tp]["square_avg"], rtol=1e-12, atol=1e-14)


def test_rmsprop_ref_eps_inside_sqrt_and_skipped_ema():
    p, gr, sq = torch.tensor([1.5]), torch.tensor([-2.0]), torch.tensor([0.5])
    out = R.rmsprop_ref(p, gr, sq, None, p.clone(), None, 0.1, 0.9, 1e-3, 0.0, True, 1.0, -1.0)
    s = 0.9 * 0.5 + 0.1 * 4.0
    assert abs(float(out["sq"]) - s) < 1e-15 and abs(float(out["p"]) - (1.5 + 0.1 * 2.0 / (s + 1e-3) ** 0.5)) < 1e-15
    assert float(out["ema"]) == 1.5 and out["buf"] is None and out["l2"] == 0.0


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_bn_train_ref_dx_is_the_three_coefficient_form(act):
    """dx = c1*g + c2*x + c3 with g = dy * act'(pre), dgamma = invstd * sum g (x - mean), dbeta = sum g,
    c1 = gamma*invstd, c2 = -gamma*invstd^2*dgamma/M, c3 = gamma*invstd*(mean*invstd*dgamma - dbeta)/M, written out in float64.
    The only place in the tests where that formula is stated."""
    gen = torch.Generator().manual_seed(11 + act)
    M, C, eps = 300, 13, 1e-3
    x = torch.randn(M, C, generator=gen, dtype=torch.float64) * 2 + 3
    gamma = torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    gamma[::4] *= -1
    beta = torch.randn(C, generator=gen, dtype=torch.float64) + 2
    dy = torch.randn(M, C, generator=gen, dtype=torch.float64)
    out = R.bn_train_ref(x, gamma, beta, eps, act, dy)
    mean, var = x.mean(0), ((x - x.mean(0)) ** 2).mean(0)
    assert torch.allclose(out["mean"], mean) and torch.allclose(out["var_b"], var) and torch.allclose(out["var_u"], var * M / (M - 1))
    r = 1.0 / torch.sqrt(var + eps)
    pre = (x - mean) * r * gamma + beta
    if act == 0:
        d = torch.ones_like(pre)
    elif act == 1:
        d = (pre > 0).double()
    elif act == 2:
        d = ((pre > 0) & (pre < 6)).double()
    else:
        s = 1.0 / (1.0 + torch.exp(-pre))
        d = s * (1 + pre * (1 - s))
    g = dy * d
    dg, db = r * (g * (x - mean)).sum(0), g.sum(0)
    c1, c2, c3 = gamma * r, -gamma * r * r * dg / M, gamma * r * (mean * r * dg - db) / M
    assert torch.allclose(out["dgamma"], dg, rtol=1e-10, atol=1e-11) and torch.allclose(out["dbeta"], db, rtol=1e-10, atol=1e-11)
    assert torch.allclose(out["dx"], c1 * g + c2 * x + c3, rtol=1e-9, atol=1e-11)
    assert torch.allclose(R.act_grad_ref(pre, act, dy), g, rtol=1e-12, atol=1e-14)


def test_bn_train_ref_boundary_masks_are_torchs():
    """pre-activations exactly 0 and exactly 6: torch gives gradient 0 at both (ReLU6) and at 0 (ReLU)"""
    pre = torch.tensor([0.0, 6.0, 3.0, -1.0, 7.0], dtype=torch.float64)
    one = torch.ones(5, dtype=torch.float64)
    assert R.act_grad_ref(pre, 1, one).tolist() == [0, 1, 1, 0, 1]
    assert R.act_grad_ref(pre, 2, one).tolist() == [0, 0, 1, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- the small ones
def test_small_references():
    p = torch.tensor([0.5, -0.25, 0.0, 0.25, -2.0])
    m, idx, kept = R.alive_ref(p, None, 0.25, 0)
    assert m.tolist() == [True, False, False, False, True] and idx.tolist() == [0, 4] and kept == 2
    e = torch.tensor([0.0, 1.0, 0.0, 0.0, 0.0])
    assert R.alive_ref(p, e, 0.25, 1)[1].tolist() == [0, 1, 4] and R.alive_ref(p, e, 0.25, 2)[1].tolist() == [1]
    g, val = R.regularisers_ref(p, torch.zeros(5), [(1, 3, 2.0)], True, mult=0.5, go=3.0, post_scale=2.0)
    assert g.tolist() == [0, -3.0, 0.0, 3.0, 0] and val == 2.0 * 0.5 * 2.0 * 0.5
    arena = torch.arange(20.0)
    # the logical matrix src[r][c] = arena[3 + 4 r + c] = [[3, 4], [7, 8]] into a pitch-7 destination at column / row offset 2
    want = {0: {0 * 7 + 2: 3.0, 0 * 7 + 3: 4.0, 1 * 7 + 2: 7.0, 1 * 7 + 3: 8.0},     # dst[r][2 + c]
            1: {2 * 7 + 0: 3.0, 3 * 7 + 0: 4.0, 2 * 7 + 1: 7.0, 3 * 7 + 1: 8.0},     # dst[2 + c][r]
            2: {0 * 7 + 2: 3.0, 1 * 7 + 2: 4.0, 0 * 7 + 3: 7.0, 1 * 7 + 3: 8.0}}     # dst[c][2 + r]
    for mode in (0, 1, 2):
        idx, vals = R.pack_ref(arena, dict(src_off=3, dst_off=100, rows=2, cols=2, src_ld=4, dst_ld=7, c_off=2, mode=mode))
        assert dict(zip((idx - 100).tolist(), vals.tolist())) == want[mode]
