"""Float64 reference of the knowledge-distillation loss (csrc/head.hip k_ce_distill), written from what the loss MEANS: the oracle's
label-smoothed cross entropy, torch.nn.functional's log_softmax / kl_div for the soft term, autograd for the gradient.  Not from the
kernel's formulas.  tests/test_distill_ref.py checks it against independent statements; the GPU tests compare the kernel and the
training step with it.

    kd_i   = T^2 * KL(softmax(t_i / T) || softmax(s_i / T))          (Hinton et al. 2015: the T^2 keeps the gradient's scale)
    loss_i = (1 - alpha) * CE_smooth(s_i, y_i) + alpha * kd_i
"""
import torch
import torch.nn.functional as F

import glue_ref as R

orc = R.orc


def kd_term(student, teacher, temperature):
    """per-sample T^2 * KL(teacher || student) at temperature T, float64; differentiable in `student`"""
    T = float(temperature)
    logp = F.log_softmax(student.double() / T, dim=1)
    logq = F.log_softmax(teacher.double() / T, dim=1)
    # log_target=True: classes whose teacher probability underflows contribute exp(-inf..) * finite = 0, never 0 * log 0
    return F.kl_div(logp, logq, reduction="none", log_target=True).sum(1) * (T * T)


def distill_ref(logits, teacher, target, eps, alpha, temperature, gscale):
    """dict(loss, kd: per-sample float64; dlogits: d(mean loss)/d(logits) * gscale by autograd; rank / top1 / top5 of the STUDENT's logits
    against the hard label, under ce_ref's convention (ties are hits))"""
    x = logits.detach().double().clone().requires_grad_(True)
    ce = orc.ce_label_smooth(x, target, eps)
    kd = kd_term(x, teacher.detach(), temperature)
    loss = (1.0 - alpha) * ce + alpha * kd
    loss.mean().backward()
    xd = x.detach()
    rank = (xd > xd.gather(1, target.view(-1, 1))).sum(1)
    return dict(loss=loss.detach(), kd=kd.detach(), ce=ce.detach(), dlogits=x.grad * gscale, rank=rank, top1=int((rank < 1).sum()),
                top5=int((rank < 5).sum()))
