"""Module-level parity (GPU): InvertedResidualChannels / ConvBNReLU / whole model on the HIP path vs the CPU oracle.

fp32 storage must match the oracle (float64 evaluation of the same state_dict) to accumulation-order tolerance; bf16
storage to the tolerance of bf16 activations (stated per test).  Parameter gradients are read from p.grad (gradient arena).
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import atomnas_oracle as orc  # noqa: E402

from kutil import assert_close, bf16_storage  # noqa: E402
from kutil import randomize as _randomize, sd64 as _sd64, widen_bn as _widen_bn  # noqa: E402  (other test modules and tools import these names from here)

pytestmark = pytest.mark.gpu


BLOCKS = [
    dict(inp=8, oup=8, stride=1, channels=[16, 16, 16], ks=[3, 5, 7], expand=True),      # residual, aligned
    dict(inp=8, oup=16, stride=2, channels=[12, 20, 7], ks=[3, 5, 7], expand=True),      # ragged (post-shrink) widths
    dict(inp=16, oup=24, stride=2, channels=[96], ks=[5], expand=True),                  # single branch
    dict(inp=16, oup=8, stride=1, channels=[16], ks=[3], expand=False),                  # first block of the supernet
    dict(inp=24, oup=24, stride=1, channels=[1, 3], ks=[3, 7], expand=True),             # nearly pruned
    # ReLU6 (the MobileNetV2 baseline of apps/mobilenet): BN scales x4 so that the upper clamp is active
    dict(inp=8, oup=8, stride=1, channels=[16, 16, 16], ks=[3, 5, 7], expand=True, act="nn.ReLU6"),
    dict(inp=8, oup=16, stride=2, channels=[12, 20, 7], ks=[3, 5, 7], expand=True, act="nn.ReLU6"),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", BLOCKS)
def test_block_forward_backward(gpu_lib, cfg, dtype):
    from atomnas_amd.models import mobilenet_base as mb
    act_name = cfg.get("act", "nn.ReLU")
    act = mb.get_active_fn(act_name)
    bn_kw = {"momentum": 0.01, "eps": 1e-3}
    blk = mb.InvertedResidualChannels(cfg["inp"], cfg["oup"], cfg["stride"], cfg["channels"], cfg["ks"], cfg["expand"],
                                      active_fn=act, batch_norm_kwargs=bn_kw)
    blk.compute_dtype = dtype
    _randomize(blk, 7)
    if act_name == "nn.ReLU6":
        _widen_bn(blk, 4.0)
    N, H = 3, 14
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, cfg["inp"], H, H, generator=g)
    Ho = (H - 1) // cfg["stride"] + 1
    gout = torch.randn(N, cfg["oup"], Ho, Ho, generator=g)
    if dtype == torch.bfloat16:
        x, gout = x.bfloat16().float(), gout.bfloat16().float()
    sd0 = _sd64(blk, "blk.")

    blk.cuda().train()
    xg = x.cuda().requires_grad_(True)
    out = blk(xg)
    assert out.dtype == dtype and out.shape == (N, cfg["oup"], Ho, Ho)
    out.backward(gout.cuda().to(dtype))
    torch.cuda.synchronize()

    # oracle in float64 on the same state_dict
    spec = dict(eps=1e-3, momentum=0.01, act=act_name)
    ob = dict(name="blk", inp=cfg["inp"], oup=cfg["oup"], stride=cfg["stride"], expand=cfg["expand"], channels=cfg["channels"],
              ks=cfg["ks"], res=cfg["stride"] == 1 and cfg["inp"] == cfg["oup"])
    work = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running" not in k) else v) for k, v in sd0.items()}
    xo = x.double().requires_grad_(True)
    stats = {}
    q = orc.NoQuant if dtype == torch.float32 else bf16_storage()
    ref = orc.block_forward(xo, work, ob, True, spec, stats, q)
    ref.backward(gout.double())

    if dtype == torch.float32:
        t_act, t_grad = dict(rtol=1e-3, atol=1e-4), dict(rtol=2e-3, atol=2e-4)
    else:  # oracle emulates bf16 storage: what is left is fp32 accumulation order and rare double roundings / mask flips
        t_act = dict(rtol=1.6e-2, atol=1.6e-2, outlier_frac=0.002)
        t_grad = dict(rtol=2e-2, atol=2e-2, outlier_frac=0.01, rel_l2=0.02)
    assert_close("out", out, ref, **t_act)
    gscale = float(xo.grad.abs().max())
    extra = {k: v for k, v in t_grad.items() if k in ("outlier_frac", "rel_l2")}
    assert_close("dx", xg.grad, xo.grad, t_grad["rtol"], t_grad["atol"] * max(1.0, gscale), **extra)
    for name, p in blk.named_parameters():
        r = work["blk." + name].grad
        s = max(1e-2, float(r.abs().max()))
        assert_close("grad " + name, p.grad, r, t_grad["rtol"], t_grad["atol"] * s, **extra)
    for name, b in blk.named_buffers():
        if "running" in name:
            prefix = "blk." + name.rsplit(".", 1)[0]
            rm, rv = stats[prefix]
            assert_close(name, b, rm if name.endswith("mean") else rv, rtol=2e-3 if dtype == torch.float32 else 2e-2, atol=1e-4 if dtype == torch.float32 else 2e-3)
        elif "num_batches_tracked" in name:
            assert int(b) == 1


def test_block_eval_mode(gpu_lib):
    from atomnas_amd.models import mobilenet_base as mb
    cfg = BLOCKS[1]
    blk = mb.InvertedResidualChannels(cfg["inp"], cfg["oup"], cfg["stride"], cfg["channels"], cfg["ks"], cfg["expand"],
                                      active_fn=mb.get_active_fn("nn.ReLU"), batch_norm_kwargs={"momentum": 0.01, "eps": 1e-3})
    blk.compute_dtype = torch.float32
    _randomize(blk, 3)
    sd0 = _sd64(blk, "blk.")
    x = torch.randn(2, cfg["inp"], 10, 10)
    blk.cuda().eval()
    with torch.no_grad():
        out = blk(x.cuda())
    ob = dict(name="blk", inp=cfg["inp"], oup=cfg["oup"], stride=cfg["stride"], expand=True, channels=cfg["channels"], ks=cfg["ks"], res=False)
    ref = orc.block_forward(x.double(), sd0, ob, False, dict(eps=1e-3, momentum=0.01, act="nn.ReLU"))
    assert_close("eval out", out, ref, rtol=1e-3, atol=1e-4)
    assert all(int(b) == 0 for n, b in blk.named_buffers() if "num_batches" in n)


TINY = dict(num_classes=10, input_size=64, input_channel=16, last_channel=64, width_mult=1.0, dropout_ratio=0.0,
            batch_norm_momentum=0.01, batch_norm_epsilon=1e-3, active_fn="nn.ReLU",
            inverted_residual_setting=[[1, 8, 1, 1, [3]], [6, 16, 2, 2, [3, 5, 7]], [6, 24, 2, 2, [3, 5, 7]], [6, 32, 1, 2, [3, 5, 7]],
                                       [6, 40, 1, 2, [3, 5, 7]]])


def _hip_masks(taps):
    """ReLU masks of a HIP forward from functional.ACT_TAP entries, as NHWC-flattened [M, C] boolean tensors per activation, in the
    oracle's order of activations: ConvBNReLU -> one; atomic block -> per branch (expand, depthwise), as the oracle walks them"""
    from atomnas_amd.ops import Slab
    out, i = [], 0
    plain = lambda t: t.to_plain() if isinstance(t, Slab) else t
    while i < len(taps):
        kind, pl, raw, sc, sh = taps[i]
        if kind == "convbn":
            C = pl.cout
            out.append((plain(raw)[:, :C].float() * sc[:C] + sh[:C]) > 0)
            i += 1
            continue
        ex = taps[i] if kind == "expand" else None
        dw = taps[i + 1] if ex is not None else taps[i]
        assert dw[0] == "dw" and dw[1] is pl
        i += 2 if ex is not None else 1
        for sg, h in zip(pl.seg, pl.hid):
            for t in ([ex] if ex is not None else []) + [dw]:
                _, _, raw_t, sc_t, sh_t = t
                out.append((plain(raw_t)[:, sg:sg + h].float() * sc_t[sg:sg + h] + sh_t[sg:sg + h]) > 0)
    return out


def test_model_forward_backward_fp32_flips_detected_against_the_oracle(gpu_lib):
    """Whole tiny network, fp32 storage, all gradients against the float64 oracle.  A random-init ReLU network turns a 1e-7 forward
    difference into a 1e-3 ... 1e-2 gradient difference whenever one pre-activation near zero lands on the other side of zero ("mask
    flip"; the fp32 oracle does it against its own float64 run on 4 of 8 batches, profiles/r04_fp32_flip_noise.txt).  Round 4 inferred
    a flip from the size of the error; here flips are DETECTED: every ReLU mask of the HIP forward (functional.ACT_TAP: raw tensor and
    BatchNorm coefficients of every activation) is compared with the oracle's float64 mask.
      * no flipped element  -> every gradient tensor within a FIXED 1e-4 relative L2 (measured 4e-6 ... 7e-6);
      * flips               -> the number is reported and must be tiny (< 1e-5 of the activations); gradients within 5e-2.
    The batches are three of the seeds whose smallest |pre-activation| / rms is largest in float64 (>= 1.4e-6; tools search over 60
    seeds, margin asserted below), so all three are expected flip-free; at least two must be."""
    from atomnas_amd import functional as AF
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import optim as aopt
    clean = 0
    for seed in (53, 23, 44):
        model = ms.Model(**TINY)
        model.set_compute_dtype(torch.float32)
        _randomize(model, 5)
        sd0 = _sd64(model)
        spec = orc.spec_from_model(model)
        g = torch.Generator().manual_seed(seed)
        N = 6
        x = torch.randn(N, 3, 64, 64, generator=g)
        y = torch.randint(0, 10, (N,), generator=g)
        model.cuda().train()
        AF.ACT_TAP = []
        try:
            logits = model(x.cuda())
            taps = AF.ACT_TAP
        finally:
            AF.ACT_TAP = None
        loss = aopt.CrossEntropyLabelSmooth(10, 0.1, reduction="none")(logits, y.cuda()).mean()
        loss.backward()
        torch.cuda.synchronize()

        # float64 oracle with its pre-activations recorded
        pre, orig_act = [], orc._act

        def rec(t, name):
            pre.append(t.detach())
            return orig_act(t, name)
        work = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running" not in k) else v) for k, v in sd0.items()}
        orc._act = rec
        try:
            ref = orc.model_forward(x.double(), work, spec, True, {}, q=orc.NoQuant)
        finally:
            orc._act = orig_act
        rl = orc.ce_label_smooth(ref, y, 0.1).mean()
        rl.backward()
        rel = lambda a, b: float((a - b).norm() / max(float(b.norm()), 1e-30))
        assert rel(logits.double().cpu(), ref.detach()) < 2e-5 and abs(float(loss.detach()) - float(rl.detach())) < 1e-5
        margin = min(float((t.abs() / t.pow(2).mean(dim=(0, 2, 3), keepdim=True).sqrt().clamp_min(1e-30)).min()) for t in pre)
        assert margin > 1e-6, (seed, margin)   # the batch is one of the wide-margin ones (guards the seed list against drift)
        masks = _hip_masks(taps)
        assert len(masks) == len(pre), (len(masks), len(pre))
        flips = total = 0
        for m, t in zip(masks, pre):
            om = (t > 0).permute(0, 2, 3, 1).reshape(-1, t.shape[1])
            assert om.shape == m.shape, (om.shape, m.shape)
            flips += int((m.cpu() != om).sum())
            total += om.numel()
        g64 = {n: work[n].grad.double() for n, _ in model.named_parameters()}
        gnorm = max(float(v.norm()) for v in g64.values())
        hip = 0.0
        for name, p in model.named_parameters():
            if float(g64[name].norm()) > 1e-6 * gnorm:
                hip = max(hip, rel(p.grad.double().cpu(), g64[name]))
            else:   # a bias in front of another BatchNorm: the true gradient is zero, both sides hold rounding noise
                assert float(p.grad.abs().max()) < 1e-5 * gnorm, (name, float(p.grad.abs().max()), gnorm)
        if flips == 0:
            clean += 1
            assert hip < 1e-4, (seed, hip)
        else:
            assert flips < 1e-5 * total and hip < 5e-2, (seed, flips, total, hip)
    assert clean >= 2, clean


@pytest.mark.parametrize("dtype", [torch.bfloat16])
def test_model_forward_backward(gpu_lib, dtype):
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import optim as aopt
    model = ms.Model(**TINY)
    model.set_compute_dtype(dtype)
    _randomize(model, 5)
    sd0 = _sd64(model)
    spec = orc.spec_from_model(model)
    g = torch.Generator().manual_seed(3)
    N = 6
    x = torch.randn(N, 3, 64, 64, generator=g)
    y = torch.randint(0, 10, (N,), generator=g)
    model.cuda().train()
    crit = aopt.CrossEntropyLabelSmooth(10, 0.1, reduction="none")
    logits = model(x.cuda())
    loss = crit(logits, y.cuda()).mean()
    loss.backward()
    torch.cuda.synchronize()

    work = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running" not in k) else v) for k, v in sd0.items()}
    xin = x.bfloat16().double() if dtype == torch.bfloat16 else x.double()
    ref_logits = orc.model_forward(xin, work, spec, True, {}, q=orc.NoQuant if dtype == torch.float32 else bf16_storage())
    ref_loss = orc.ce_label_smooth(ref_logits, y, 0.1).mean()
    ref_loss.backward()
    # Bounds from tools/parity_diag.py on this very network (profiles/r03_parity_diag.txt; the kernels are bit-reproducible, so the
    # numbers do not move from run to run).  fp32 storage: logits relative L2 2.2e-6, worst gradient tensor 4.1e-6, no outliers.
    # bf16 storage against Bf16Storage: logits 1.4e-2; gradients per significant tensor cosine >= 0.950, norm ratio 0.79..1.07,
    # aggregate cosine 0.980 -- a 1-ulp forward difference flips bf16 roundings and ReLU masks, so whole-network bf16 gradients are
    # pinned in direction and scale here and element-wise per block (test_block_forward_backward, tests/test_parity_gpu.py).
    if dtype == torch.float32:
        ta = dict(rtol=1e-4, atol=1e-5)
    else:
        ta = dict(rtol=3e-2, atol=3e-2)
    assert_close("logits", logits, ref_logits, **ta)
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < (1e-5 if dtype == torch.float32 else 5e-3)
    gnorm = max(float(work[n].grad.norm()) for n, _ in model.named_parameters())
    for name, p in model.named_parameters():
        r = work[name].grad
        if dtype == torch.float32:
            if float(r.norm()) > 1e-6 * gnorm:
                s = max(1e-2, float(r.abs().max()))
                assert_close("grad " + name, p.grad, r, 1e-3, 1e-4 * s, outlier_frac=0.0, rel_l2=1e-4)
            else:   # a bias in front of another BatchNorm: the true gradient is zero, both sides hold rounding noise
                assert float(p.grad.abs().max()) < 1e-5 * gnorm, (name, float(p.grad.abs().max()), gnorm)
        elif float(r.norm()) > 1e-2 * gnorm:
            gg = p.grad.double().cpu().flatten()
            cos = float(torch.dot(gg, r.flatten()) / (gg.norm() * r.norm()))
            ratio = float(gg.norm() / r.norm())
            assert cos > 0.9 and 0.7 < ratio < 1.3, "grad %s: cosine %.3f norm ratio %.3f" % (name, cos, ratio)
    if dtype != torch.float32:
        ga = torch.cat([p.grad.double().cpu().flatten() for _, p in model.named_parameters()])
        ra = torch.cat([work[n].grad.flatten() for n, _ in model.named_parameters()])
        cos = float(torch.dot(ga, ra) / (ga.norm() * ra.norm()))
        assert cos > 0.95 and 0.9 < float(ga.norm() / ra.norm()) < 1.1, "all gradients: cosine %.3f norm ratio %.3f" % (cos, float(ga.norm() / ra.norm()))


@pytest.mark.parametrize("act", ["nn.ReLU", "nn.ReLU6"])
def test_cfg1_mobilenet_v2_on_the_gpu(gpu_lib, act):
    """BASELINE config 1: MobileNetV2-1.0 from apps/mobilenet (single-branch 3x3 blocks, ReLU; ReLU6 as in the original
    network) -- logits and loss against the oracle in fp32, gradients in aggregate."""
    import os
    os.environ.setdefault("ARNOLD_OUTPUT", "/tmp/atomnas_out")
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import config
    from atomnas_amd.utils import optim as aopt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    flags = config.load_app(["app:" + os.path.join(root, "apps/mobilenet/mobilenet_v2_mnas.yml")])
    kw = dict(flags.model_kwparams)
    kw["active_fn"] = act
    kw["dropout_ratio"] = 0.0
    model = ms.Model(**kw, input_size=96)
    model.set_compute_dtype(torch.float32)
    _randomize(model, 13)
    sd0 = _sd64(model)
    spec = orc.spec_from_model(model)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(4, 3, 96, 96, generator=g)
    y = torch.randint(0, 1000, (4,), generator=g)
    model.cuda().train()
    logits = model(x.cuda())
    loss = aopt.CrossEntropyLabelSmooth(1000, 0.1, reduction="none")(logits, y.cuda()).mean()
    loss.backward()
    torch.cuda.synchronize()
    work = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running" not in k) else v) for k, v in sd0.items()}
    ref = orc.model_forward(x.double(), work, spec, True, {})
    rl = orc.ce_label_smooth(ref, y, 0.1).mean()
    rl.backward()
    assert_close("logits", logits, ref, rtol=2e-3, atol=2e-3)
    assert abs(float(loss.detach()) - float(rl.detach())) < 1e-4
    num = den = 0.0
    for name, p in model.named_parameters():
        d = p.grad.double().cpu() - work[name].grad
        num += float((d * d).sum()); den += float((work[name].grad ** 2).sum())
    assert (num / den) ** 0.5 < 2e-2, (num / den) ** 0.5
