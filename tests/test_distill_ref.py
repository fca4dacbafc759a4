"""tests/distill_ref.py against independent statements of the same loss (CPU)."""
import torch
import torch.nn.functional as F

import distill_ref as D
import glue_ref as R


def _inputs(B=6, K=37, seed=0, scale=3.0):
    gen = torch.Generator().manual_seed(seed)
    s = torch.randn(B, K, generator=gen, dtype=torch.float64) * scale
    t = torch.randn(B, K, generator=gen, dtype=torch.float64) * scale
    y = torch.randint(0, K, (B,), generator=gen)
    return s, t, y


def test_alpha_zero_is_the_label_smoothed_cross_entropy():
    s, t, y = _inputs()
    for eps in (0.0, 0.1):
        got, ref = D.distill_ref(s, t, y, eps, 0.0, 4.0, 0.25), R.ce_ref(s, y, eps, 0.25)
        assert torch.equal(got["loss"], ref["loss"]) and torch.equal(got["dlogits"], ref["dlogits"])
        assert (got["top1"], got["top5"]) == (ref["top1"], ref["top5"]) and torch.equal(got["rank"], ref["rank"])


def test_teacher_equal_to_student_gives_no_soft_term():
    s, _, y = _inputs(seed=1)
    for T in (1.0, 4.0):
        got, ref = D.distill_ref(s, s.clone(), y, 0.1, 0.3, T, 1.0), R.ce_ref(s, y, 0.1, 1.0)
        assert float(got["kd"].abs().max()) <= 1e-14 * T * T
        torch.testing.assert_close(got["dlogits"], 0.7 * ref["dlogits"], rtol=1e-12, atol=1e-15)
        torch.testing.assert_close(got["loss"], 0.7 * ref["loss"], rtol=1e-12, atol=1e-14)


def test_unit_temperature_is_functional_cross_entropy_plus_kl():
    s, t, y = _inputs(seed=2)
    alpha = 0.3
    x = s.clone().requires_grad_(True)
    ce = F.cross_entropy(x, y, reduction="none")
    kl = (F.softmax(t, 1) * (F.log_softmax(t, 1) - F.log_softmax(x, 1))).sum(1)   # the sum written out
    loss = (1 - alpha) * ce + alpha * kl
    loss.mean().backward()
    got = D.distill_ref(s, t, y, 0.0, alpha, 1.0, 1.0)
    torch.testing.assert_close(got["loss"], loss.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(got["kd"], kl.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(got["dlogits"], x.grad, rtol=1e-12, atol=1e-15)
    # and torch's own batch reduction of the same divergence
    assert abs(float(got["kd"].mean()) - float(F.kl_div(F.log_softmax(s, 1), F.softmax(t, 1), reduction="batchmean"))) < 1e-12


def test_underflowing_teacher_classes_contribute_nothing():
    """logits scaled by 30: q underflows to exactly 0 for many classes at T = 1; the term stays finite and non-negative"""
    s, t, y = _inputs(B=5, K=65, seed=3, scale=30.0)
    got = D.distill_ref(s, t, y, 0.1, 1.0, 1.0, 1.0)
    assert bool(torch.isfinite(got["kd"]).all()) and bool((got["kd"] >= 0).all()) and bool(torch.isfinite(got["dlogits"]).all())
    assert int((F.softmax(t.float(), 1) == 0).sum()) > 0   # in fp32, the kernel's format


def test_t_squared_keeps_the_soft_gradient_scale():
    """on small logits softmax(x / T) ~ 1/K + (x - mean) / (K T): the gradient of T^2 KL is (s - t - mean) / (K B) to first order, whatever
    T -- without the T^2 it would shrink as 1 / T^2"""
    s, t, y = _inputs(B=4, K=16, seed=4, scale=1e-3)
    first_order = ((s - s.mean(1, keepdim=True)) - (t - t.mean(1, keepdim=True))) / (16 * 4)
    grads = [D.distill_ref(s, t, y, 0.0, 1.0, T, 1.0)["dlogits"] for T in (1.0, 2.0, 8.0)]
    for g in grads:
        assert float((g - first_order).abs().max()) <= 2e-2 * float(first_order.abs().max())
    assert float((grads[0] - grads[2]).abs().max()) <= 2e-2 * float(grads[0].abs().max())
