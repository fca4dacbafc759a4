"""kutil.se_reference (the float64 reference of tests/test_se_family_gpu.py, every derivative written out) against torch autograd of the
module formula (SqueezeAndExcitation.forward, models/mobilenet_base.py:109-112, behind act(D scale + shift)) in float64.  On margin
inputs no pre-activation sits on a bound of ReLU / ReLU6, so torch.clamp's convention there does not enter and the two agree to 1e-12:
each vouches for the other.  Runs without a GPU."""
import pytest
import torch

from kutil import act64, act_grad64, se_reference

CASES = [
    # N, HW, branch widths, hidden units, SE activation, storage type
    (3, 7, [5, 19], 3, 1, torch.float32),
    (2, 30, [23], 6, 3, torch.bfloat16),
]


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("case", CASES, ids=["relu_gate_fp32", "swish_gate_bf16"])
def test_se_reference_against_autograd(case, act):
    N, HW, widths, hid, se_act, dtype = case
    c = se_reference(N, HW, widths, hid, act, se_act, dtype)
    r = c.ref
    # the inputs: exact in the storage type, zero on padding, the real channels where cmap says
    assert torch.equal(c.D.to(dtype).double(), c.D) and torch.equal(c.dS.to(dtype).double(), c.dS)
    pad = ~c.valid
    assert pad.any() and not c.D[:, pad].any() and not c.dS[:, pad].any() and not c.scale[pad].any() and not c.shift[pad].any()
    assert torch.equal(c.cmap[c.idx].long(), torch.arange(c.total))
    a = (c.D[:, c.idx] * c.sc.double() + c.sh.double()).requires_grad_(True)
    assert torch.equal(a.detach(), r.a)
    assert float(a.detach().abs().min()) >= 2.0 ** -6 and (act != 2 or float((a.detach() - 6).abs().min()) >= 2.0 ** -6)
    p = [t.double().requires_grad_(True) for t in (c.w1, c.b1, c.w2, c.b2)]
    A = act64(a, act)
    pooled = A.view(N, HW, -1).mean(1)
    hpre = pooled @ p[0].t() + p[1]
    z2 = act64(hpre, se_act) @ p[2].t() + p[3]
    gate = torch.sigmoid(z2)
    S = A * gate.repeat_interleave(HW, 0)
    for t in (pooled, hpre, z2, gate):
        t.retain_grad()
    S.backward(c.dS[:, c.idx])
    for name, got, ref in (("pooled", r.pooled, pooled), ("hpre", r.hpre, hpre), ("gate", r.gate, gate), ("S", r.S, S),
                           ("dgate", r.dgate, gate.grad), ("dz2", r.dz2, z2.grad), ("dz1", r.dz1, hpre.grad),
                           ("dpooled", r.dpooled, pooled.grad), ("g", r.g, a.grad), ("dw1", r.dw1, p[0].grad), ("db1", r.db1, p[1].grad),
                           ("dw2", r.dw2, p[2].grad), ("db2", r.db2, p[3].grad)):
        ref = ref.detach()
        assert got.shape == ref.shape, name
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), name
    assert torch.equal(r.g_stored, r.g.to(dtype).double())
    assert float((r.stats[0] - r.g_stored.sum(0)).abs().max()) == 0 and float((r.stats[1] - (r.g_stored * c.D[:, c.idx]).sum(0)).abs().max()) == 0


def test_act_grad_is_zero_on_the_bounds():
    """the convention the kernels use (csrc/common.h act_pass): strict inequalities; torch.clamp's autograd passes 1 at 0 and at 6"""
    x = torch.tensor([-1.0, 0.0, 0.5, 5.5, 6.0, 6.5], dtype=torch.float64)
    assert act_grad64(x, 0).tolist() == [1, 1, 1, 1, 1, 1]
    assert act_grad64(x, 1).tolist() == [0, 0, 1, 1, 1, 1]
    assert act_grad64(x, 2).tolist() == [0, 0, 1, 1, 0, 0]
    xr = x.clone().requires_grad_(True)
    act64(xr, 3).sum().backward()
    assert float((act_grad64(x, 3) - xr.grad).abs().max()) <= 1e-15
