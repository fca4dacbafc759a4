"""Inference path on the GPU: atomnas_block_infer (csrc/block_infer.hip) and atomnas_amd.inference against the CPU oracle.

Reference of every block case: orc.block_forward in float64 with the PLAIN bf16 storage model (orc.Bf16Storage: the rounding points
the fused kernel implements; not kutil.bf16_storage(), which follows the matrix-core depthwise predicate of the training path).
Bound: the project's bf16 block bound of tests/test_block_gpu.py.  The outlier allowance (0.2 %) cannot hide a padding or tile-seam
defect: border pixels are 36 % of a 10x10 map and seams at least 10 % of the multi-tile maps.

The kernel is checked on every shape it can RUN (inference.POLICY = "all", atomnas_block_infer_runs).  The default policy fuses only
the shapes the kernel measured faster for (atomnas_block_infer_supported): most of the maps below -- the multi-tile and
stride-2 ones that carry the seam and padding checks -- then take the existing path and would not exercise the kernel at all.
"""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import atomnas_oracle as orc  # noqa: E402

from kutil import assert_close, randomize, sd64, widen_bn  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = dict(rtol=1.6e-2, atol=1.6e-2, outlier_frac=0.002)
BN_KW = {"momentum": 0.01, "eps": 1e-3}


@pytest.fixture(autouse=True)
def _every_shape_the_kernel_runs(monkeypatch):
    import atomnas_amd.inference as inf
    monkeypatch.setattr(inf, "POLICY", "all")


def _expand_bn_bias(module, value):
    """expand-BN bias = value on every channel: act(bn(0)) >> 0, so a halo that is not zeroed is a large error on every border pixel"""
    hit = 0
    with torch.no_grad():
        for n, p in module.named_parameters():
            if re.match(r"ops\.\d+\.0\.1\.bias$|expand_conv\.1\.bias$", n):   # the BatchNorm of a branch's (or the fused block's) expand conv
                p.fill_(value)
                hit += 1
    assert hit, "no expand BatchNorm found"


C1 = dict(inp=8, oup=8, stride=1, channels=[16, 16, 16], ks=[3, 5, 7], hw=(14, 14))           # residual, aligned
C2 = dict(inp=8, oup=16, stride=2, channels=[12, 20, 7], ks=[3, 5, 7], hw=(15, 13))           # ragged segments, odd non-square, stride 2
C6 = dict(inp=40, oup=40, channels=[30, 18], ks=[9, 11])                                      # big kernels
C8 = dict(inp=16, oup=24, channels=[24, 24], ks=[3, 7], hw=(37, 29), N=2)                     # several tiles + remainders both ways
CASES = {
    "c1": C1,
    "c2": C2,
    "c3": dict(inp=16, oup=24, stride=2, channels=[96], ks=[5], hw=(10, 10)),                 # single branch, several chunks
    "c4": dict(inp=16, oup=8, stride=1, channels=[16], ks=[3], expand=False, hw=(12, 12)),    # no expand stage
    "c5": dict(inp=24, oup=24, stride=1, channels=[1, 3], ks=[3, 7], hw=(7, 7)),              # nearly pruned, residual
    "c6_s1": dict(C6, stride=1, hw=(14, 14)),
    "c6_s2": dict(C6, stride=2, hw=(14, 14)),
    "c6_s1_9x9": dict(C6, stride=1, hw=(9, 9)),
    "c6_s2_9x9": dict(C6, stride=2, hw=(9, 9)),
    "c7": dict(inp=16, oup=16, stride=1, channels=[8], ks=[11], hw=(5, 5)),                   # halo wider than the map
    "c8_s1": dict(C8, stride=1),
    "c8_s2": dict(C8, stride=2),
    "c9": dict(inp=72, oup=112, stride=1, channels=[200, 136], ks=[3, 5], hw=(14, 14)),       # K % 32 != 0, many chunks, wide accumulator
    "c10_relu6_c1": dict(C1, act="nn.ReLU6"),
    "c10_relu6_c2": dict(C2, act="nn.ReLU6"),
    "c10_swish_c1": dict(C1, act="nn.Swish"),
    "c10_swish_c2": dict(C2, act="nn.Swish"),
    "c11_fused_c2": dict(C2, fused=True),
    "c12_bias_c1": dict(C1, ebias=1.5),
    "c12_bias_c6_s1": dict(C6, stride=1, hw=(14, 14), ebias=1.5),
    "c12_bias_c6_s2": dict(C6, stride=2, hw=(14, 14), ebias=1.5),
    "c12_bias_c6_s1_9x9": dict(C6, stride=1, hw=(9, 9), ebias=1.5),
    "c12_bias_c6_s2_9x9": dict(C6, stride=2, hw=(9, 9), ebias=1.5),
    "c12_bias_c8_s1": dict(C8, stride=1, ebias=1.5),
    "c12_bias_c8_s2": dict(C8, stride=2, ebias=1.5),
}


def _build(cfg, se_ratio=None):
    from atomnas_amd.models import mobilenet_base as mb
    act_name = cfg.get("act", "nn.ReLU")
    args = (cfg["inp"], cfg["oup"], cfg["stride"], cfg["channels"], cfg["ks"], cfg.get("expand", True))
    if cfg.get("fused") or se_ratio is not None:
        blk = mb.InvertedResidualChannelsFused(*args, active_fn=mb.get_active_fn(act_name), batch_norm_kwargs=BN_KW, se_ratio=se_ratio)
    else:
        blk = mb.InvertedResidualChannels(*args, active_fn=mb.get_active_fn(act_name), batch_norm_kwargs=BN_KW)
    blk.compute_dtype = torch.bfloat16
    randomize(blk, 7)
    if act_name == "nn.ReLU6":
        widen_bn(blk, 4.0)
    if "ebias" in cfg:
        _expand_bn_bias(blk, cfg["ebias"])
    return blk, act_name


def _case(cfg):
    """-> (block on the GPU in eval mode, input [N, inp, H, W] bf16-representable on the CPU, float64 reference)"""
    blk, act_name = _build(cfg)
    N, (H, W) = cfg.get("N", 3), cfg["hw"]
    x = torch.randn(N, cfg["inp"], H, W, generator=torch.Generator().manual_seed(11)).bfloat16().float()
    spec = dict(eps=1e-3, momentum=0.01, act=act_name)
    ob = dict(name="blk", inp=cfg["inp"], oup=cfg["oup"], stride=cfg["stride"], expand=cfg.get("expand", True), channels=cfg["channels"],
              ks=cfg["ks"], res=cfg["stride"] == 1 and cfg["inp"] == cfg["oup"], fused=bool(cfg.get("fused")), se=False)
    ref = orc.block_forward(x.bfloat16().double(), sd64(blk, "blk."), ob, False, spec, q=orc.Bf16Storage)
    return blk.cuda().eval(), x, ref


_REF8 = {}


def _case8(stride):
    """case 8 and its reference, computed once and shared (block, x, ref are left unchanged by their users)"""
    if stride not in _REF8:
        _REF8[stride] = _case(CASES["c8_s%d" % stride])
    return _REF8[stride]


@pytest.mark.parametrize("key", sorted(CASES))
def test_fused_block_against_the_plain_bf16_oracle(gpu_lib, key):
    from atomnas_amd.inference import compile_for_inference
    cfg = CASES[key]
    blk, x, ref = _case8(cfg["stride"]) if key in ("c8_s1", "c8_s2") else _case(cfg)
    net = compile_for_inference(blk)
    out = net(x.cuda())
    torch.cuda.synchronize()
    assert [k for _, k, _ in net.plan()] == ["fused"], net.plan()
    assert net._ok and all(net._ok.values()), "the launch fell back: the shape is outside the kernel's envelope"
    s = cfg["stride"]
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (x.shape[0], cfg["oup"], (x.shape[2] - 1) // s + 1, (x.shape[3] - 1) // s + 1)
    assert_close("out " + key, out, ref, **BOUND)


def test_batch_invariance_and_determinism(gpu_lib):
    """image 0 of case 8 alone and inside N = 2: identical bits; two launches behind a launch that keeps the stream busy: identical bits"""
    from atomnas_amd.inference import compile_for_inference
    for stride in (1, 2):
        blk, x, _ = _case8(stride)
        net = compile_for_inference(blk)
        xg = x.cuda()
        both = net(xg)
        alone = net(xg[:1].contiguous())
        assert torch.equal(both[:1], alone)
        big = torch.cat([xg] * 16)
        net(big)            # keeps the stream busy
        a = net(xg)
        net(big)
        b = net(xg)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, both)


def test_se_block_falls_back_to_the_existing_path(gpu_lib):
    from atomnas_amd.inference import compile_for_inference
    blk, _ = _build(dict(C2, fused=True, act="nn.Swish"), se_ratio=0.5)
    blk.cuda().eval()
    x = torch.randn(3, 8, 15, 13, generator=torch.Generator().manual_seed(5)).cuda()
    net = compile_for_inference(blk)
    (name, kind, reason), = net.plan()
    assert kind == "fallback" and "squeeze" in reason
    with torch.no_grad():
        want = blk(x)
    assert torch.equal(net(x), want)


def test_measured_policy_keeps_slower_shapes_on_the_existing_path(gpu_lib, monkeypatch):
    """default policy: the multi-tile case 8 falls back (bit-equal to the block's own eval forward), the 14x14 case 1 is fused"""
    import atomnas_amd.inference as inf
    monkeypatch.setattr(inf, "POLICY", "measured")
    blk, x, _ = _case8(1)
    net = inf.compile_for_inference(blk)
    with torch.no_grad():
        want = blk(x.cuda())
    assert torch.equal(net(x.cuda()), want) and not any(net._ok.values())
    blk1, x1, ref1 = _case(CASES["c1"])
    net1 = inf.compile_for_inference(blk1)
    assert [k for _, k, _ in net1.plan()] == ["fused"]
    assert_close("c1 under the measured policy", net1(x1.cuda()), ref1, **BOUND)
    assert all(net1._ok.values())


def test_refusals(gpu_lib):
    from atomnas_amd import _lib
    from atomnas_amd.inference import compile_for_inference
    blk, _ = _build(C1)
    with pytest.raises(_lib.AtomnasHipError, match="GPU"):
        compile_for_inference(blk.eval())            # on the CPU
    blk.cuda().train()
    with pytest.raises(ValueError, match="eval"):
        compile_for_inference(blk)
    blk.eval()
    blk.compute_dtype = torch.float32
    with pytest.raises(ValueError, match="bf16"):
        compile_for_inference(blk)
    blk.compute_dtype = torch.bfloat16
    net = compile_for_inference(blk)
    with pytest.raises(RuntimeError, match="forward-only"):
        net(torch.randn(1, 8, 14, 14, device="cuda", requires_grad=True))


# tests/test_block_gpu.py::TINY
TINY = dict(num_classes=10, input_size=64, input_channel=16, last_channel=64, width_mult=1.0, dropout_ratio=0.0,
            batch_norm_momentum=0.01, batch_norm_epsilon=1e-3, active_fn="nn.ReLU",
            inverted_residual_setting=[[1, 8, 1, 1, [3]], [6, 16, 2, 2, [3, 5, 7]], [6, 24, 2, 2, [3, 5, 7]], [6, 32, 1, 2, [3, 5, 7]],
                                       [6, 40, 1, 2, [3, 5, 7]]])


def _tiny():
    from atomnas_amd.models import mobilenet_supernet as ms
    model = ms.Model(**TINY)
    randomize(model, 5)
    return model


def test_whole_model(gpu_lib):
    """TINY network, input 64, N = 4: logits against the plain bf16 oracle (the bf16 whole-network bound of tests/test_block_gpu.py),
    every block fused, graph replay bit-equal to the eager compiled model on two inputs, snapshot semantics of refresh()"""
    from atomnas_amd.inference import compile_for_inference
    model = _tiny()
    sd = sd64(model)
    spec = orc.spec_from_model(model)
    g = torch.Generator().manual_seed(21)
    x1, x2 = (torch.randn(4, 3, 64, 64, generator=g) for _ in range(2))
    ref = orc.model_forward(x1.bfloat16().double(), sd, spec, False, q=orc.Bf16Storage)
    model.cuda().eval()
    net = compile_for_inference(model)
    assert len(net.plan()) == 7 and all(kind == "fused" for _, kind, _ in net.plan()), net.plan()
    out1 = net(x1.cuda())
    assert net._ok and all(net._ok.values())
    assert out1.shape == (4, 10)
    assert_close("logits", out1, ref, rtol=3e-2, atol=3e-2)

    gnet = compile_for_inference(model, use_graph=True, batch_size=4)
    out2 = net(x2.cuda())
    assert not torch.equal(out1, out2)
    assert torch.equal(gnet(x1.cuda()), out1) and torch.equal(gnet(x2.cuda()), out2) and torch.equal(gnet(x1.cuda()), out1)

    # the snapshot does not follow an in-place update of a fused block's running statistics until refresh()
    bn = [m for m in model.features[3].modules() if isinstance(m, torch.nn.BatchNorm2d)][0]
    with torch.no_grad():
        bn.running_mean.add_(0.5)
    assert torch.equal(net(x1.cuda()), out1) and torch.equal(gnet(x1.cuda()), out1)
    net.refresh()
    gnet.refresh()
    out3 = net(x1.cuda())
    assert not torch.equal(out3, out1)
    assert torch.equal(gnet(x1.cuda()), out3)


def test_evaluate_with_fused_inference_scores_the_same(gpu_lib, monkeypatch):
    """train.evaluate with `fused_inference` on and off over synthetic batches whose labels sit far from every rank boundary: the same
    top-1 / top-5 error (the label is the arg max where its margin over the runner-up exceeds twice the bf16 whole-network bound, the
    arg min -- far below the top five of ten classes -- elsewhere)"""
    import train
    from atomnas_amd.utils import config as cfg
    monkeypatch.setenv("ATOMNAS_E2E_DIR", "/nonexistent")
    F = cfg.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_search.yml")])
    F["bn_calibration"] = False
    F["image_size"] = 64
    F["per_gpu_batch_size"] = 4
    F["model_kwparams"]["num_classes"] = 10
    model = _tiny().cuda().eval()
    g = torch.Generator().manual_seed(33)
    xs = [torch.randn(4, 3, 64, 64, generator=g).cuda() for _ in range(3)]
    batches = []
    with torch.no_grad():
        for x in xs:
            lg = model(x).float()
            top = lg.topk(2, dim=1)
            bound = 2 * (3e-2 + 3e-2 * float(lg.abs().max()))
            sure = (top.values[:, 0] - top.values[:, 1]) > bound
            low = lg.topk(6, dim=1).values[:, 5] - lg.min(dim=1).values > bound   # the arg min is clear of the top five
            assert bool(low.all())
            batches.append((x, torch.where(sure, top.indices[:, 0], lg.argmin(dim=1))))
    assert sum(int((y == model(x).argmax(1)).sum()) for x, y in batches) >= 1, "no sample with a clear arg max: the test would be vacuous"

    class Wrapper:
        module = model

    monkeypatch.setattr(train, "LOADERS", (None, None, None, object()))
    monkeypatch.setattr(train, "device_batches", lambda loader, steps: iter(batches))
    compiled = []
    import atomnas_amd.inference as inf
    real = inf.compile_for_inference
    monkeypatch.setattr(inf, "compile_for_inference", lambda m, **kw: compiled.append(real(m, **kw)) or compiled[-1])
    res_off, n_off, _ = train.evaluate(Wrapper, None)
    assert not compiled
    F["fused_inference"] = True
    res_on, n_on, _ = train.evaluate(Wrapper, None)
    assert len(compiled) == 1 and all(kind == "fused" for _, kind, _ in compiled[0].plan())
    assert n_on == n_off == 12
    assert res_on["top1_error"] == res_off["top1_error"] and res_on["top5_error"] == res_off["top5_error"]
    assert 0.0 <= res_on["top1_error"] < 1.0
