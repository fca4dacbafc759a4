"""MixConv-size atoms (kernel sizes 3, 5, 7, 9, 11 in one block) through every layer above the kernels (GPU): block parity against the
oracle, the fused SE / Swish block, whole training steps eager and as a replayed graph, dynamic shrinkage that thins the 9 x 9 branch and
drops the 11 x 11 one, the exported architecture, and the search entry point with its checkpoint.

Bounds are those of the files the cases are modelled on (tests/test_block_gpu.py, tests/test_train_step_gpu.py); the k = 9 / 11 branches
run csrc/dwconv_big.hip, which the oracle's bf16 storage model sees as plain fp32-accumulating kernels (atomnas_dwconv_mm_supported
answers 0 for them)."""
import collections
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import atomnas_oracle as orc  # noqa: E402

from kutil import assert_close, bf16_storage  # noqa: E402
from test_block_gpu import _randomize, _sd64  # noqa: E402

pytestmark = pytest.mark.gpu

KS = [3, 5, 7, 9, 11]
CHANNELS = [16, 8, 24, 9, 13]
# stem /2, first block /2, then four expanding blocks with the five sizes: 16 -> 8 (stride 2), 8 (stride 1, residual), 8 -> 4, 4 -> 2
TINY_MIX = dict(num_classes=10, input_size=64, input_channel=16, last_channel=64, width_mult=1.0, dropout_ratio=0.0,
                batch_norm_momentum=0.01, batch_norm_epsilon=1e-3, active_fn="nn.ReLU",
                inverted_residual_setting=[[1, 8, 1, 2, [3]], [6, 16, 2, 2, KS], [6, 24, 1, 2, KS], [6, 32, 1, 2, KS]])


def _block_bounds(dtype):
    """tests/test_block_gpu.py test_block_forward_backward"""
    if dtype == torch.float32:
        return dict(rtol=1e-3, atol=1e-4), dict(rtol=2e-3, atol=2e-4)
    return dict(rtol=1.6e-2, atol=1.6e-2, outlier_frac=0.002), dict(rtol=2e-2, atol=2e-2, outlier_frac=0.01, rel_l2=0.02)


def _check_block(blk, ob, act_name, dtype, x, gout):
    """forward, input gradient, every parameter gradient and the running statistics of one block against the oracle"""
    N, _, H, _ = x.shape
    if dtype == torch.bfloat16:
        x, gout = x.bfloat16().float(), gout.bfloat16().float()
    sd0 = _sd64(blk, "blk.")
    blk.cuda().train()
    xg = x.cuda().requires_grad_(True)
    out = blk(xg)
    assert out.dtype == dtype and out.shape == gout.shape
    out.backward(gout.cuda().to(dtype))
    torch.cuda.synchronize()
    spec = dict(eps=1e-3, momentum=0.01, act=act_name)
    work = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running" not in k) else v) for k, v in sd0.items()}
    xo = x.double().requires_grad_(True)
    stats = {}
    ref = orc.block_forward(xo, work, ob, True, spec, stats, orc.NoQuant if dtype == torch.float32 else bf16_storage())
    ref.backward(gout.double())
    t_act, t_grad = _block_bounds(dtype)
    assert_close("out", out, ref, **t_act)
    gscale = float(xo.grad.abs().max())
    extra = {k: v for k, v in t_grad.items() if k in ("outlier_frac", "rel_l2")}
    assert_close("dx", xg.grad, xo.grad, t_grad["rtol"], t_grad["atol"] * max(1.0, gscale), **extra)
    for name, p in blk.named_parameters():
        r = work["blk." + name].grad
        assert_close("grad " + name, p.grad, r, t_grad["rtol"], t_grad["atol"] * max(1e-2, float(r.abs().max())), **extra)
    for name, b in blk.named_buffers():
        if "running" in name:
            rm, rv = stats["blk." + name.rsplit(".", 1)[0]]
            assert_close(name, b, rm if name.endswith("mean") else rv, rtol=2e-3 if dtype == torch.float32 else 2e-2,
                         atol=1e-4 if dtype == torch.float32 else 2e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("stride", [1, 2])
def test_block_with_five_kernel_sizes(gpu_lib, stride, dtype):
    from atomnas_amd.models import mobilenet_base as mb
    blk = mb.InvertedResidualChannels(16, 24, stride, CHANNELS, KS, True, active_fn=mb.get_active_fn("nn.ReLU"),
                                      batch_norm_kwargs={"momentum": 0.01, "eps": 1e-3})
    blk.compute_dtype = dtype
    _randomize(blk, 7)
    g = torch.Generator().manual_seed(11)
    Ho = (14 - 1) // stride + 1
    x, gout = torch.randn(2, 16, 14, 14, generator=g), torch.randn(2, 24, Ho, Ho, generator=g)
    ob = dict(name="blk", inp=16, oup=24, stride=stride, expand=True, channels=CHANNELS, ks=KS, res=False)
    _check_block(blk, ob, "nn.ReLU", dtype, x, gout)


def test_fused_block_with_se_and_swish(gpu_lib):
    """padded-segment layout: one expand over all 70 hidden channels, the five depthwise branches on 16-aligned segments, SE, Swish"""
    from atomnas_amd.models import mobilenet_base as mb
    blk = mb.InvertedResidualChannelsFused(16, 16, 1, CHANNELS, KS, True, active_fn=mb.get_active_fn("nn.Swish"),
                                           batch_norm_kwargs={"momentum": 0.01, "eps": 1e-3}, se_ratio=0.5)
    blk.compute_dtype = torch.float32
    _randomize(blk, 9)
    g = torch.Generator().manual_seed(13)
    x, gout = torch.randn(2, 16, 14, 14, generator=g), torch.randn(2, 16, 14, 14, generator=g)
    ob = dict(name="blk", inp=16, oup=16, stride=1, expand=True, channels=CHANNELS, ks=KS, res=True, fused=True, se=True)
    _check_block(blk, ob, "nn.Swish", torch.float32, x, gout)


def _setup(seed=21):
    from atomnas_amd import engine
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import model_profiling as mp, optim as aopt, prune as aprune, rmsprop
    model = ms.Model(**TINY_MIX)
    model.set_compute_dtype(torch.float32)
    _randomize(model, seed)
    mp.model_profiling(model, 64, 64, verbose=False)
    sd = collections.OrderedDict((k, v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items())
    spec = orc.spec_from_model(model)
    model.cuda().train()
    pinfo = aprune.get_bn_to_prune(model, {"bn_prune_filter": "expansion_only_skip_expand1"}, verbose=False)
    opt = rmsprop.RMSprop(model.parameters(), lr=0.01, alpha=0.9, momentum=0.9, eps=1e-3, eps_inside_sqrt=True)
    ema = aopt.ExponentialMovingAverage(0.99)
    for n, p in model.named_parameters():
        ema.register(n, p)
    for n, b in model.named_buffers():
        if "running" in n:
            ema.register(n, b)
    return model, sd, spec, pinfo, opt, ema, engine


def _batches(steps, N):
    """Batch seed 15: of the seeds 0 .. 15 the one whose smallest |pre-activation| / rms over both compared iterations is largest IN THE
    FLOAT64 ORACLE (2.5e-6 and 4.4e-6; seed 5, which tests/test_train_step_gpu.py uses for its own network, has 6.4e-8 here: below fp32
    resolution, so a ReLU mask may legitimately differ from float64 and move whole gradient elements -- that file's docstrings and
    tests/test_block_gpu.py describe the effect).  test_three_steps_eager_graph_and_oracle asserts the margin."""
    g = torch.Generator().manual_seed(15)
    return [(torch.randn(N, 3, 64, 64, generator=g), torch.randint(0, 10, (N,), generator=g)) for _ in range(steps)]


def _snapshot(model, opt, ema):
    out = collections.OrderedDict(("model." + k, v.detach().clone()) for k, v in model.state_dict().items())
    for n, p in model.named_parameters():
        out["sq." + n] = opt.state[p]["square_avg"].detach().clone()
        out["buf." + n] = opt.state[p]["momentum_buffer"].detach().clone()
    for n in ema.average_names():
        out["ema." + n] = ema.average(n).detach().clone()
    return out


def test_three_steps_eager_graph_and_oracle(gpu_lib):
    """three training steps: the replayed graph gives the bits of the eager run; after two steps (the horizon
    tests/test_train_step_gpu.py states its bound for) parameters and EMA shadows are within that file's bound of the float64 oracle"""
    N, batches = 4, _batches(3, 4)
    runs = []
    for use_graph in (False, True):
        model, sd, spec, pinfo, opt, ema, engine = _setup()
        ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=1e-3, label_smoothing=0.1, batch_size=N, image_size=64, use_graph=use_graph)
        losses, after2 = [], None
        for step, (x, y) in enumerate(batches):
            ts.set_batch(x.cuda(), y.cuda())
            ts.step(lr=0.002 * (1 + step), rho=1e-3 * (1 + step))
            losses.append(ts.loss.tolist())
            if step == 1:
                torch.cuda.synchronize()
                after2 = (collections.OrderedDict((k, v.detach().clone()) for k, v in model.state_dict().items()),
                          {k: ema.average(k).detach().clone() for k in ema.average_names()})
        torch.cuda.synchronize()
        runs.append((losses, _snapshot(model, opt, ema), after2, ema, sd, spec, pinfo))
    (l0, s0, _, _, _, _, _), (l1, s1, after2, ema, sd, spec, pinfo) = runs
    assert l0 == l1 and all(v == v for row in l0 for v in row), (l0, l1)
    assert list(s0.keys()) == list(s1.keys())
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k

    names, pen, _ = orc.prune_penalties(spec, 64)
    assert names == pinfo.weight
    assert_close("penalties", torch.tensor(pinfo.penalty), torch.tensor(pen), rtol=1e-12, atol=0)
    opt_state = {}
    ema_o = collections.OrderedDict((k, v.clone()) for k, v in sd.items() if v.is_floating_point())
    pre, orig_act = [], orc._act

    def rec(t, name):
        pre.append(t.detach())
        return orig_act(t, name)
    orc._act = rec
    try:
        for step, (x, y) in enumerate(batches[:2]):
            ref = orc.train_step(sd, spec, opt_state, ema_o, x.double(), y, dict(lr=0.002 * (1 + step), rho=1e-3 * (1 + step), weight_decay=1e-3,
                                 wd_method="mnas", label_smoothing=0.1, alpha=0.9, eps=1e-3, momentum=0.9, ema_decay=ema.momentum_at(step + 1)),
                                 names, pen)
            assert abs(l1[step][0] - ref["loss"]) < 2e-5 * max(1, abs(ref["loss"])), (step, l1[step], ref["loss"])
            assert abs(l1[step][1] - ref["loss_l2"]) < 1e-5 * max(1, abs(ref["loss_l2"])), (step, l1[step], ref["loss_l2"])
            assert abs(l1[step][2] - ref["loss_l1"]) < 1e-4 * max(1e-3, abs(ref["loss_l1"])), (step, l1[step], ref["loss_l1"])
    finally:
        orc._act = orig_act
    margin = min(float((t.abs() / t.pow(2).mean(dim=(0, 2, 3), keepdim=True).sqrt().clamp_min(1e-30)).min()) for t in pre)
    assert margin > 1e-6, margin   # the batches are wide-margin ones in float64 (guards the seed against drift), see _batches
    msd, mema = after2
    for k, v in sd.items():
        if v.is_floating_point():
            assert_close("param " + k, msd[k], v, rtol=2e-4, atol=2e-5 * max(1e-3, float(v.abs().max())))
        else:
            assert int(msd[k]) == int(v) == 2, k
    for k in ema_o:
        assert_close("ema " + k, mema[k], ema_o[k], rtol=2e-4, atol=2e-5 * max(1e-3, float(ema_o[k].abs().max())))


def test_shrink_thins_the_9x9_branch_and_drops_the_11x11_branch(gpu_lib):
    sys.path.insert(0, ROOT)
    import train as T
    from atomnas_amd import runtime
    from atomnas_amd.models import searched_network as sn
    from atomnas_amd.utils import config, prune as aprune
    model, sd, spec, pinfo, opt, ema, engine = _setup()
    N, batches = 4, _batches(3, 4)
    ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=1e-3, batch_size=N, image_size=64, use_graph=True)
    for x, y in batches[:2]:   # non-trivial optimizer state and EMA shadows
        ts.set_batch(x.cuda(), y.cuda())
        ts.step(lr=0.002, rho=1e-3)
    torch.cuda.synchronize()

    # forced masks: in every expanding block every third atom of the 9 x 9 branch and the whole 11 x 11 branch die
    params = dict(model.named_parameters())
    masks = {}
    with torch.no_grad():
        for bname, blk in model.get_named_block_list().items():
            if list(blk.kernel_sizes) != KS:
                continue
            for i, bn_name in enumerate(blk.get_named_depthwise_bn(prefix=bname).keys()):
                h = blk.channels[i]
                dead = torch.zeros(h, dtype=torch.bool)
                if i == 3:
                    dead[::3] = True
                elif i == 4:
                    dead[:] = True
                masks[(bname, i)] = ~dead
                if bool(dead.any()):
                    w = params[bn_name + ".weight"]
                    w[dead.cuda()] = 0.0
                    ema.average(bn_name + ".weight")[dead.cuda()] = 0.0
    assert len(masks) == 4 * len(KS)
    torch.cuda.synchronize()
    pre = _snapshot(model, opt, ema)

    # the architecture the search would export, from the alive masks of the unshrunk network
    thr = 1e-3
    pinfo.add_info_list("mask", [params[n].detach().abs() > thr for n in pinfo.weight])
    _, infos = aprune.cal_pruned_flops(pinfo)
    kw = aprune.output_searched_network(model, infos, {"bn_prune_filter": "expansion_only_skip_expand1"})
    for row in kw["inverted_residual_setting"][1:]:
        assert row[3] == [3, 5, 7, 9] and row[4][3] == row[4][0] - (row[4][0] + 2) // 3, row

    class F(dict):
        __getattr__ = dict.__getitem__
    config.FLAGS.bind(F(image_size=64, use_distributed=False))
    wrapper = torch.nn.Module()
    wrapper.module = model
    T.shrink_model(wrapper, ema, opt, pinfo, thr, ema_only=False)
    runtime.manager_of(model).ensure()
    torch.cuda.synchronize()
    post = _snapshot(model, opt, ema)

    pat = re.compile(r"^(model|sq|buf|ema)\.(features\.\d+)\.ops\.(\d+)\.(.*)$")
    for k, v in post.items():
        m = pat.match(k)
        want = pre[k]
        if m and (m.group(2), int(m.group(3))) in masks and want.dim() > 0:
            keep = masks[(m.group(2), int(m.group(3)))].to(want.device)
            want = want[:, keep] if m.group(4) == "2.weight" else want[keep]   # the projection loses columns, everything else rows
        assert v.shape == want.shape and torch.equal(v, want), k
    gone = [k for k in pre if k not in post]
    assert gone and all(pat.match(k) and int(pat.match(k).group(3)) == 4 for k in gone), gone[:5]
    for bname, blk in model.get_named_block_list().items():
        if (bname, 0) in masks:
            assert list(blk.kernel_sizes) == [3, 5, 7, 9] and blk.channels[3] == int(masks[(bname, 3)].sum())

    # the exported kwargs build the searched network, and it takes the shrunk weights as they are
    searched = sn.Model(**kw, input_size=64, dropout_ratio=0.0, batch_norm_momentum=0.01, batch_norm_epsilon=1e-3)
    missing = searched.load_state_dict(model.state_dict(), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys

    # a step after the shrink runs through the rebuilt arenas and stays finite
    model.train()
    ts2 = engine.TrainStep(model, opt, ema, pinfo, weight_decay=1e-3, batch_size=N, image_size=64, use_graph=True)
    x, y = batches[2]
    ts2.set_batch(x.cuda(), y.cuda())
    ts2.step(lr=0.002, rho=1e-3)
    torch.cuda.synchronize()
    assert all(v == v and abs(v) < 1e4 for v in ts2.loss.tolist()), ts2.loss.tolist()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_search_entry_point_with_checkpoint_and_resume(gpu_lib, tmp_path):
    """`train.py app:tests/data/tiny_search_mix.yml`: one shortened epoch of the mix search with its validation, the final shrink and the
    checkpoint; then a resume for one more epoch"""
    env = dict(os.environ, ATOMNAS_E2E_DIR=str(tmp_path), ARNOLD_OUTPUT=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "app:" + os.path.join(ROOT, "tests", "data", "tiny_search_mix.yml")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert out.count(" val: ") >= 1 and "Prune threshold" in out and "Model Shrink to FLOPS" in out, out[-4000:]
    assert "[3, 5, 7, 9, 11]" in open(os.path.join(str(tmp_path), "latest_checkpoint.yml")).read()
    assert os.path.exists(os.path.join(str(tmp_path), "latest_checkpoint.pt"))
    r2 = subprocess.run(cmd + ["--resume", str(tmp_path), "--num_epochs", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out2 = r2.stdout + r2.stderr
    assert r2.returncode == 0, out2[-4000:]
    assert "Epoch 1/2" in out2 and "Epoch 0/2" not in out2, out2[-3000:]
