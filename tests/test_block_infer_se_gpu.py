"""Inference path on the GPU for blocks WITH Squeeze-and-Excitation: atomnas_block_infer_se (csrc/block_infer.hip, template parameter SE)
and atomnas_amd.inference against the CPU oracle.

Reference: orc.block_forward in float64 with the plain bf16 storage model (orc.Bf16Storage) and se=True, fused=True: the raw depthwise
value is rounded to bf16, the activated value enters the mean unrounded, the gated product is rounded once.  Bound: the project's bf16
block bound of tests/test_block_infer_gpu.py.

Both SE convolution weights are multiplied by 4: at scale 1 the gates sit in 0.34-0.67 and differ between images by <= 0.03, so a
kernel that shared one image's gate across the batch, or left the gate out, would pass.  Every test first asserts on its REFERENCE
that the gates span >= 0.5 per image and that more than half of the outputs differ from the same block without SE by more than the
bound; only then does it look at the GPU.  Case E has four hidden channels only: four gates at x4 span 0.42-0.44 per image, below
the 0.5 this file asks of every case, so its two SE layers are multiplied by 8 (spans 0.6+); shape, reference and bound are the same.

The kernel is checked on every shape it can run (inference.POLICY = "all", atomnas_block_infer_se_runs).
"""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import atomnas_oracle as orc  # noqa: E402

from kutil import assert_close, randomize, sd64, widen_bn  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = dict(rtol=1.6e-2, atol=1.6e-2, outlier_frac=0.002)
BN_KW = {"momentum": 0.01, "eps": 1e-3}
SE_SCALE = 4.0


@pytest.fixture(autouse=True)
def _every_shape_the_kernel_runs(monkeypatch):
    import atomnas_amd.inference as inf
    monkeypatch.setattr(inf, "POLICY", "all")


def _widen_se(module, factor=SE_SCALE):
    """both dense layers of every gate x factor: gates that differ between channels and between images"""
    hit = 0
    with torch.no_grad():
        for n, p in module.named_parameters():
            if re.search(r"se_op\.se_(reduce|expand)\.weight$", n):
                p.mul_(factor)
                hit += 1
    assert hit and hit % 2 == 0, "no squeeze-and-excitation weights found"


def _depthwise_bn_bias(module, value):
    """depthwise-BN bias = value on every channel: act(bn_d(0)) >> 0, so a padding row of the 16-row MFMA tiles that entered the mean
    would inflate it (49 map pixels in 64 tile rows: by 64 / 49)"""
    hit = 0
    with torch.no_grad():
        for n, p in module.named_parameters():
            if re.match(r"depth_ops\.\d+\.\d+\.1\.bias$", n):
                p.fill_(value)
                hit += 1
    assert hit, "no depthwise BatchNorm found"


A = dict(inp=16, oup=16, channels=[16, 16, 16], ks=[3, 5, 7], hw=(7, 7), act="nn.Swish")       # residual; 49 pixels in 64 tile rows
CASES = {
    "A": A,
    "A_bias": dict(A, dbias=1.5),                                                                   # padding rows must not enter the mean
    "B": dict(inp=72, oup=112, channels=[200, 136], ks=[3, 5], hw=(14, 14), act="nn.Swish"),      # several chunks, K % 32 != 0, 2 pixel tiles per wave
    "C": dict(inp=24, oup=40, channels=[12, 20, 7], ks=[3, 5, 7], hw=(13, 9), act="nn.ReLU"),     # ragged segments, se_hid 12, odd non-square map
    "D": dict(inp=40, oup=40, channels=[30, 18], ks=[9, 11], hw=(5, 5), act="nn.ReLU6"),          # halo wider than the map
    "E": dict(inp=24, oup=24, channels=[1, 3], ks=[3, 7], hw=(16, 16), act="nn.Swish", se_scale=8.0),   # nearly pruned; 256 pixels: the largest whole map
}


def _build(cfg, stride=1):
    from atomnas_amd.models import mobilenet_base as mb
    blk = mb.InvertedResidualChannelsFused(cfg["inp"], cfg["oup"], stride, cfg["channels"], cfg["ks"], True, active_fn=mb.get_active_fn(cfg["act"]),
                                           batch_norm_kwargs=BN_KW, se_ratio=0.5)
    blk.compute_dtype = torch.bfloat16
    randomize(blk, 7)
    if cfg["act"] == "nn.ReLU6":
        widen_bn(blk, 4.0)
    _widen_se(blk, cfg.get("se_scale", SE_SCALE))
    if "dbias" in cfg:
        _depthwise_bn_bias(blk, cfg["dbias"])
    return blk


def _oracle_gates(fn):
    """runs fn() with orc.se_forward observed -> (fn's result, [gate [N, C] of every SE the oracle went through])"""
    gates, real = [], orc.se_forward

    def spy(x, sd, prefix, act):
        s = x.mean([2, 3], keepdim=True)
        s = orc._act(F.conv2d(s, sd[prefix + ".se_reduce.weight"], sd[prefix + ".se_reduce.bias"]), act)
        gates.append(torch.sigmoid(F.conv2d(s, sd[prefix + ".se_expand.weight"], sd[prefix + ".se_expand.bias"])).flatten(1))
        return real(x, sd, prefix, act)

    orc.se_forward = spy
    try:
        return fn(), gates
    finally:
        orc.se_forward = real


_REF = {}


def _case(key):
    """-> (block on the GPU in eval mode, input on the CPU, float64 reference), computed once per case and shared (left unchanged by
    its users).  The reference is checked to DEPEND on a per-image gate before anything runs on the GPU."""
    if key in _REF:
        return _REF[key]
    cfg = CASES[key]
    blk = _build(cfg)
    H, W = cfg["hw"]
    x = torch.randn(3, cfg["inp"], H, W, generator=torch.Generator().manual_seed(11)).bfloat16().float()
    spec = dict(eps=1e-3, momentum=0.01, act=cfg["act"])
    ob = dict(name="blk", inp=cfg["inp"], oup=cfg["oup"], stride=1, expand=True, channels=cfg["channels"], ks=cfg["ks"],
              res=cfg["inp"] == cfg["oup"], fused=True, se=True)
    sd = sd64(blk, "blk.")
    ref, (gate,) = _oracle_gates(lambda: orc.block_forward(x.bfloat16().double(), sd, ob, False, spec, q=orc.Bf16Storage))
    span = gate.max(1).values - gate.min(1).values
    assert float(span.min()) >= 0.5, "the gates of one image hardly differ (%s): the case would not see a wrong gate" % span.tolist()
    if key == "A":
        cross = (gate[:, None] - gate[None]).abs().amax((0, 1)).max()
        assert float(cross) >= 0.2, "the gates of two images hardly differ (%.3f): a gate shared across the batch would pass" % float(cross)
    plain = orc.block_forward(x.bfloat16().double(), sd, dict(ob, se=False), False, spec, q=orc.Bf16Storage)
    moved = ((ref - plain).abs() > BOUND["atol"] + BOUND["rtol"] * ref.abs()).double().mean()
    assert float(moved) > 0.5, "only %.2f of the outputs feel the gate: a kernel without it would pass" % float(moved)
    _REF[key] = (blk.cuda().eval(), x, ref)
    return _REF[key]


@pytest.mark.parametrize("key", sorted(CASES))
def test_fused_se_block_against_the_plain_bf16_oracle(gpu_lib, key):
    from atomnas_amd.inference import compile_for_inference
    cfg = CASES[key]
    blk, x, ref = _case(key)
    net = compile_for_inference(blk)
    out = net(x.cuda())
    torch.cuda.synchronize()
    assert [(k, why) for _, k, why in net.plan()] == [("fused", "")], net.plan()
    assert net._ok and all(net._ok.values()), "the launch fell back: the shape is outside the kernel's envelope"
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (3, cfg["oup"]) + cfg["hw"]
    assert_close("out " + key, out, ref, **BOUND)


@pytest.mark.parametrize("key", ["A", "B"])
def test_batch_invariance_and_determinism(gpu_lib, key):
    """image 0 alone and inside N = 3: identical bits; two launches on either side of a launch that keeps the stream busy: identical bits"""
    from atomnas_amd.inference import compile_for_inference
    blk, x, _ = _case(key)
    net = compile_for_inference(blk)
    xg = x.cuda()
    both = net(xg)
    alone = net(xg[:1].contiguous())
    assert [k for _, k, _ in net.plan()] == ["fused"] and net._ok and all(net._ok.values())
    assert torch.equal(both[:1], alone)
    big = torch.cat([xg] * 16)
    net(big)            # keeps the stream busy
    a = net(xg)
    net(big)
    b = net(xg)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, both)


@pytest.mark.parametrize("stride,hw", [(1, (17, 16)), (2, (14, 14))])
def test_se_blocks_outside_the_envelope_keep_the_existing_path(gpu_lib, stride, hw):
    """a map above 256 pixels and a stride-2 block: 'fallback' with the squeeze named as the reason, bit-equal to the block's own forward"""
    from atomnas_amd.inference import compile_for_inference
    blk = _build(dict(A, oup=16 if stride == 1 else 24), stride=stride).cuda().eval()
    x = torch.randn(3, 16, *hw, generator=torch.Generator().manual_seed(5)).cuda()
    net = compile_for_inference(blk)
    with torch.no_grad():
        want = blk(x)
    assert torch.equal(net(x), want)
    assert not any(net._ok.values())
    (name, kind, reason), = net.plan()   # a block on its own is planned at a nominal 14 x 14 map: the plan follows the map of the call
    assert kind == "fallback" and "squeeze" in reason, net.plan()


ROWS = [[8, 1, 1, [3], [16], False], [16, 2, 2, [3, 5, 7], [12, 20, 7], True], [24, 2, 2, [3, 5], [40, 24], True],
        [32, 2, 1, [3, 5, 7], [48, 48, 48], True], [40, 2, 2, [3, 7], [64, 64], True]]


def _tiny_plus():
    from atomnas_amd.models import searched_network as sn
    model = sn.Model(num_classes=10, input_size=64, input_channel=16, last_channel=64, dropout_ratio=0.0, se_ratio=0.5, batch_norm_momentum=0.01,
                     batch_norm_epsilon=1e-3, active_fn="nn.Swish", block="InvertedResidualChannelsFused", inverted_residual_setting=ROWS)
    randomize(model, 5)
    _widen_se(model)
    return model


def test_whole_model(gpu_lib):
    """a 9-block '+' network, input 64, N = 4: the plan fuses exactly the stride-1 expanding blocks whose map has <= 256 pixels, logits
    against the plain bf16 oracle (the bf16 whole-network bound of tests/test_block_infer_gpu.py::test_whole_model), graph replay
    bit-equal to the eager compiled model on two inputs, snapshot semantics of refresh() for the gate's tensors"""
    from atomnas_amd.inference import compile_for_inference
    model = _tiny_plus()
    sd = sd64(model)
    # the rows below stride the 64 x 64 input down to 4 x 4, not to the 2 x 2 that spec["pool"] = input_size // 32 assumes: the HIP tail
    # pools the whole final map (functional.tail_forward), and so does the reference here
    spec = dict(orc.spec_from_model(model), pool=4)
    assert len(spec["blocks"]) == 9 and all(b["se"] and b["fused"] for b in spec["blocks"])
    g = torch.Generator().manual_seed(21)
    x1, x2 = (torch.randn(4, 3, 64, 64, generator=g) for _ in range(2))
    ref, gates = _oracle_gates(lambda: orc.model_forward(x1.bfloat16().double(), sd, spec, False, q=orc.Bf16Storage))
    assert len(gates) == 9
    # the rule, from the structure alone
    want, hw = [], 32
    for b in spec["blocks"]:
        want.append("fused" if b["stride"] == 1 and b["expand"] and hw * hw <= 256 else "fallback")
        hw = (hw - 1) // b["stride"] + 1
    assert want.count("fused") == 5
    assert all(float((gt.max(1).values - gt.min(1).values).min()) >= 0.5 for gt, k in zip(gates, want) if k == "fused"), "flat gates in a fused block"

    model.cuda().eval()
    net = compile_for_inference(model)
    assert [k for _, k, _ in net.plan()] == want, net.plan()
    assert all("squeeze" in why for _, k, why in net.plan() if k == "fallback"), net.plan()
    out1 = net(x1.cuda())
    assert len(net._ok) == 5 and all(net._ok.values())
    assert out1.shape == (4, 10)
    assert_close("logits", out1, ref, rtol=3e-2, atol=3e-2)

    gnet = compile_for_inference(model, use_graph=True, batch_size=4)
    out2 = net(x2.cuda())
    assert not torch.equal(out1, out2)
    assert torch.equal(gnet(x1.cuda()), out1) and torch.equal(gnet(x2.cuda()), out2) and torch.equal(gnet(x1.cuda()), out1)

    # the snapshot does not follow an in-place update of a fused block's gate until refresh()
    fused = [m for (_, k, _), (_, m) in zip(net.plan(), net._blocks()) if k == "fused"]
    with torch.no_grad():
        fused[1].se_op.se_expand.bias.add_(1.0)
    assert torch.equal(net(x1.cuda()), out1) and torch.equal(gnet(x1.cuda()), out1)
    net.refresh()
    gnet.refresh()
    out3 = net(x1.cuda())
    assert not torch.equal(out3, out1)
    assert torch.equal(gnet(x1.cuda()), out3)
