"""Stochastic depth through the executor, the training step and the entry point (GPU).

Block parity: the branch of a residual block is the oracle's block without its residual (orc.block_forward with res False: everything
up to and including the block-output BatchNorm, so the statistics are those of the undropped block); the test composes
out = x + keep / (1 - p) * branch under torch autograd in float64 with the keep mask read back from the device, which itself is compared
with the numpy transcription (tests/drop_connect_ref.py).  Tolerances: those of tests/test_block_gpu.py::test_block_forward_backward.
"""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import atomnas_oracle as orc  # noqa: E402

import drop_connect_ref as DR  # noqa: E402
from kutil import assert_close, bf16_storage, randomize, sd64, widen_bn  # noqa: E402
from test_block_gpu import BLOCKS, TINY  # noqa: E402

pytestmark = pytest.mark.gpu

BN_KW = {"momentum": 0.01, "eps": 1e-3}
# a residual fused block with SE and Swish: the shape of tests/test_fused_gpu.py::test_fused_block_batched_weight_gradients_...
FUSED = dict(inp=24, oup=24, stride=1, channels=[30, 50, 13], ks=[3, 5, 7], expand=True, act="nn.Swish", fused=True, se_ratio=0.5)
PARITY = [BLOCKS[0], BLOCKS[4], BLOCKS[5], FUSED]
N_PAR, H_PAR, P_PAR = 6, 7, 0.5


def _make_block(cfg, dtype, seed=7):
    from atomnas_amd.models import mobilenet_base as mb
    act_name = cfg.get("act", "nn.ReLU")
    args = (cfg["inp"], cfg["oup"], cfg["stride"], cfg["channels"], cfg["ks"], cfg["expand"])
    if cfg.get("fused"):
        blk = mb.InvertedResidualChannelsFused(*args, active_fn=mb.get_active_fn(act_name), batch_norm_kwargs=BN_KW, se_ratio=cfg["se_ratio"])
    else:
        blk = mb.InvertedResidualChannels(*args, active_fn=mb.get_active_fn(act_name), batch_norm_kwargs=BN_KW)
    blk.compute_dtype = dtype
    randomize(blk, seed)
    if act_name == "nn.ReLU6":
        widen_bn(blk, 4.0)
    return blk, act_name


def _set_step(blk, step):
    """materialises the block's arenas and sets the device step counter its mask is keyed by"""
    from atomnas_amd import runtime
    mgr = runtime.manager_of(blk)
    mgr.ensure()
    mgr.step_counter.fill_(step)
    return mgr


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", PARITY, ids=["block0", "block4", "block5-relu6", "fused-se-swish"])
def test_block_parity(gpu_lib, cfg, dtype):
    from atomnas_amd import functional as AF
    blk, act_name = _make_block(cfg, dtype)
    seed, index = 4242, 5
    step = DR.find_step(seed, index, N_PAR, P_PAR, lambda m: 0 < int(m.sum()) < N_PAR, start=3)
    want_keep = DR.keep_mask(seed, step, index, N_PAR, P_PAR)
    assert 0 < int(want_keep.sum()) < N_PAR
    blk.drop_connect_rate, blk.drop_connect_index, blk.dropout_seed = P_PAR, index, seed
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N_PAR, cfg["inp"], H_PAR, H_PAR, generator=g)
    gout = torch.randn(N_PAR, cfg["oup"], H_PAR, H_PAR, generator=g)
    if dtype == torch.bfloat16:
        x, gout = x.bfloat16().float(), gout.bfloat16().float()
    sd0 = sd64(blk, "blk.")

    blk.cuda().train()
    _set_step(blk, step)
    xg = x.cuda().requires_grad_(True)
    out = blk(xg)
    out.backward(gout.cuda().to(dtype))
    torch.cuda.synchronize()
    keep = AF.drop_connect_keep(blk)
    assert keep is not None and keep.dtype == torch.uint8 and np.array_equal(keep.cpu().numpy(), want_keep)

    spec = dict(eps=1e-3, momentum=0.01, act=act_name)
    ob = dict(name="blk", inp=cfg["inp"], oup=cfg["oup"], stride=1, expand=cfg["expand"], channels=cfg["channels"], ks=cfg["ks"], res=False,
              fused=bool(cfg.get("fused")), se=bool(cfg.get("fused")))
    work = {k: (v.clone().requires_grad_(True) if (v.is_floating_point() and "running" not in k) else v) for k, v in sd0.items()}
    xo = x.double().requires_grad_(True)
    stats = {}
    q = orc.NoQuant if dtype == torch.float32 else bf16_storage()
    branch = orc.block_forward(xo, work, ob, True, spec, stats, q)
    ks = keep.cpu().double().view(-1, 1, 1, 1) * DR.scale_of(P_PAR)
    ref = q.b(q.f(xo + ks * branch))
    ref.backward(gout.double())

    if dtype == torch.float32:
        t_act, t_grad = dict(rtol=1e-3, atol=1e-4), dict(rtol=2e-3, atol=2e-4)
    else:
        t_act = dict(rtol=1.6e-2, atol=1.6e-2, outlier_frac=0.002)
        t_grad = dict(rtol=2e-2, atol=2e-2, outlier_frac=0.01, rel_l2=0.02)
    assert_close("out", out, ref, **t_act)
    dropped = torch.from_numpy(want_keep == 0)
    assert torch.equal(out[dropped.cuda()], xg.detach().to(dtype)[dropped.cuda()]), "a dropped image is not the block's input"
    gscale = float(xo.grad.abs().max())
    extra = {k: v for k, v in t_grad.items() if k in ("outlier_frac", "rel_l2")}
    assert_close("dx", xg.grad, xo.grad, t_grad["rtol"], t_grad["atol"] * max(1.0, gscale), **extra)
    for name, p in blk.named_parameters():
        r = work["blk." + name].grad
        s = max(1e-2, float(r.abs().max()))
        assert_close("grad " + name, p.grad, r, t_grad["rtol"], t_grad["atol"] * s, **extra)
    for name, b in blk.named_buffers():
        if "running" in name:
            rm, rv = stats["blk." + name.rsplit(".", 1)[0]]
            assert_close(name, b, rm if name.endswith("mean") else rv, rtol=2e-3 if dtype == torch.float32 else 2e-2,
                         atol=1e-4 if dtype == torch.float32 else 2e-3)
        elif "num_batches_tracked" in name:
            assert int(b) == 1


def _record(fn):
    from atomnas_amd import ops
    ops.RECORD = rec = []
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.RECORD = None
    return out, rec


@pytest.mark.parametrize("case", ["no_residual", "eval"])
def test_unchanged_paths(gpu_lib, case):
    """a rate on a block without a residual connection, and on a residual block in eval(): the launches and the output of rate 0"""
    from atomnas_amd import functional as AF
    cfg = BLOCKS[1] if case == "no_residual" else BLOCKS[0]
    x = torch.randn(3, cfg["inp"], 14, 14, generator=torch.Generator().manual_seed(2)).cuda()
    res = []
    for rate in (0.0, 0.5):
        blk, _ = _make_block(cfg, torch.float32)
        blk.drop_connect_rate, blk.drop_connect_index = rate, 3
        blk.cuda().train(case == "no_residual")
        if case == "eval":
            with torch.no_grad():
                out, rec = _record(lambda: blk(x))
        else:
            xg = x.clone().requires_grad_(True)
            out, rec = _record(lambda: (lambda o: (o.backward(torch.ones_like(o)), o)[1])(blk(xg)))
        assert AF.drop_connect_keep(blk) is None
        res.append((out.detach().clone(), rec))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1] and len(res[0][1]) > 3
    assert not any(r["entry"] in ("bn_apply_drop", "drop_connect_bwd") for r in res[1][1])


# ---------------------------------------------------------------------------------------------------------------- training step
def _train_step(rate, use_graph, accum=None, kw_rate=True, seed=21):
    from atomnas_amd import engine
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import model_profiling as mp
    from atomnas_amd.utils import optim as aopt
    from atomnas_amd.utils import prune as aprune
    from atomnas_amd.utils import rmsprop
    model = ms.Model(**TINY, **(dict(drop_connect_rate=rate) if kw_rate else {}))
    model.set_compute_dtype(torch.float32)
    randomize(model, seed)
    mp.model_profiling(model, 64, 64, verbose=False)
    model.cuda().train()
    pinfo = aprune.get_bn_to_prune(model, {"bn_prune_filter": "expansion_only_skip_expand1"}, verbose=False)
    opt = rmsprop.RMSprop(model.parameters(), lr=0.01, alpha=0.9, momentum=0.9, eps=1e-3, eps_inside_sqrt=True)
    ema = aopt.ExponentialMovingAverage(0.99)
    for n, p in model.named_parameters():
        ema.register(n, p)
    for n, b in model.named_buffers():
        if "running" in n:
            ema.register(n, b)
    kw = {} if accum is None else dict(accum_steps=accum)
    return model, engine.TrainStep(model, opt, ema, pinfo, weight_decay=1e-3, batch_size=6, image_size=64, use_graph=use_graph, **kw)


def _batch(seed, n=6):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 64, 64, generator=g).cuda(), torch.randint(0, 10, (n,), generator=g).cuda()


def _dropping(model):
    return [b for b in model.get_named_block_list().values() if b.use_res_connect and b.drop_connect_rate > 0]


def _masks(model):
    from atomnas_amd import functional as AF
    torch.cuda.synchronize()
    return [AF.drop_connect_keep(b).cpu().numpy().copy() for b in _dropping(model)]


def _expected(model, counter, n=6):
    return [DR.keep_mask(model.dropout_seed, counter, b.drop_connect_index, n, b.drop_connect_rate) for b in _dropping(model)]


def test_steps_eager_and_captured(gpu_lib):
    """three steps with rate 0.5, eager and captured + replayed: the same parameters bit for bit, and after every step the keep masks of
    the transcription at that step's counter"""
    finals, seen = [], []
    for use_graph in (False, True):
        model, ts = _train_step(0.5, use_graph)
        assert len(_dropping(model)) == 2   # the second blocks of the 16- and 24-wide rows
        per_step = []
        for step in range(3):
            ts.set_batch(*_batch(50 + step))
            ts.step(lr=0.002, rho=1e-3)
            got, want = _masks(model), _expected(model, step)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (use_graph, step, got, want)
            per_step.append(np.concatenate(got))
        assert int(ts.mgr.step_counter) == 3
        assert not np.array_equal(per_step[0], per_step[1]) and not np.array_equal(per_step[1], per_step[2])
        assert any(0 < int(m.sum()) < m.size for m in per_step)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ts.mgr.P).all())
        finals.append({k: getattr(ts.mgr, k).detach().clone() for k in ("P", "S", "EMA", "SQ", "BUF", "CNT")})
        seen.append(per_step)
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k
    assert all(np.array_equal(a, b) for a, b in zip(seen[0], seen[1]))


def test_launch_lists(gpu_lib):
    """one eager step: rate 0.5 records as many launches as rate 0 (two of them replaced per dropping block); a model built with
    drop_connect_rate=0.0 records the launch list of one built without the keyword"""
    recs = {}
    for key, rate, kw_rate in (("none", 0.0, False), ("zero", 0.0, True), ("half", 0.5, True)):
        model, ts = _train_step(rate, False, kw_rate=kw_rate)
        ts.set_batch(*_batch(50))
        ts.step(lr=0.002, rho=1e-3)   # the first step creates the per-plan scratch buffers
        _, recs[key] = _record(lambda: ts.step(lr=0.002, rho=1e-3))
    assert recs["none"] == recs["zero"] and len(recs["none"]) > 50
    assert len(recs["half"]) == len(recs["none"])
    entries = lambda rec: collections.Counter(r["entry"] for r in rec)
    a, b = entries(recs["none"]), entries(recs["half"])
    nd = len(_dropping(model))
    assert nd == 2 and b["bn_apply_drop"] == nd and b["drop_connect_bwd"] == nd
    assert a["bn_apply"] - b["bn_apply"] == nd and a["act_bwd_stats"] - b["act_bwd_stats"] == nd
    assert a["bn_apply_drop"] == 0 and a["drop_connect_bwd"] == 0


def test_accumulated_step_draws_a_mask_per_micro_batch(gpu_lib):
    """grad_accum_steps 2: the masks of the two micro-batches of a step are those of counters c and c + 1 (read in eager mode: a captured
    accumulated step has one graph per kind of micro-batch, each with a keep tensor of its own); the captured step then equals the
    eager one bit for bit, so it drew the same masks"""
    finals = []
    for use_graph in (False, True):
        model, ts = _train_step(0.5, use_graph, accum=2)
        for group in range(2):
            c = int(ts.mgr.step_counter)
            assert c == 2 * group
            ts.set_batch(*_batch(60))
            ts.accumulate()
            first = _masks(model)
            ts.set_batch(*_batch(61))
            ts.step(lr=0.002, rho=1e-3)
            second = _masks(model)
            if not use_graph:
                assert all(np.array_equal(a, b) for a, b in zip(first, _expected(model, c)))
                assert all(np.array_equal(a, b) for a, b in zip(second, _expected(model, c + 1)))
                assert not np.array_equal(np.concatenate(first), np.concatenate(second))
        torch.cuda.synchronize()
        finals.append({k: getattr(ts.mgr, k).detach().clone() for k in ("P", "S", "EMA", "SQ", "BUF", "CNT")})
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k


def test_shrink_keeps_rates_and_indices(gpu_lib):
    """the forced shrink of tests/test_shrink_gpu.py / test_grad_accum_gpu.py on a model with a rate: attributes unchanged, a step runs"""
    sys.path.insert(0, ROOT)
    import train as T
    from atomnas_amd import engine
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import config, model_profiling as mp_, optim as aopt, prune as aprune, rmsprop
    g = torch.load(os.path.join(ROOT, "tests", "golden", "shrink.pt"), weights_only=False)
    model = ms.Model(**g["kw"], drop_connect_rate=0.5)
    model.set_compute_dtype(torch.float32)
    model.load_state_dict(g["sd_pre"])
    mp_.model_profiling(model, 64, 64, verbose=False)
    model.cuda().train()
    pinfo = aprune.get_bn_to_prune(model, {"bn_prune_filter": "expansion_only_skip_expand1"}, verbose=False)
    opt = rmsprop.RMSprop(model.parameters(), lr=0.002, alpha=0.9, momentum=0.9, eps=1e-3, eps_inside_sqrt=True)
    ema = aopt.ExponentialMovingAverage(0.99)
    for n, p in model.named_parameters():
        ema.register(n, p)
    for n, b in model.named_buffers():
        if "running" in n:
            ema.register(n, b)
    ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=1e-5, batch_size=8, image_size=64, use_graph=True)
    x, y = _batch(100, 8)
    ts.set_batch(x, y)
    ts.step(lr=0.002, rho=1e-4)
    before = [(b.drop_connect_rate, b.drop_connect_index) for b in model.get_named_block_list().values()]
    assert before[-1][0] > 0 and _dropping(model)
    v0, n0 = ts.mgr.version, ts.mgr.nP

    class F(dict):
        __getattr__ = dict.__getitem__
    config.FLAGS.bind(F(image_size=64, use_distributed=False))
    wrapper = torch.nn.Module()
    wrapper.module = model
    T.shrink_model(wrapper, ema, opt, pinfo, 1e-3, ema_only=False)
    assert [(b.drop_connect_rate, b.drop_connect_index) for b in model.get_named_block_list().values()] == before
    ts.step(lr=0.002, rho=1e-4)
    torch.cuda.synchronize()
    assert ts.mgr.version > v0 and ts.mgr.nP < n0
    assert bool(torch.isfinite(ts.loss).all()) and bool(torch.isfinite(ts.mgr.P).all())
    c = int(ts.mgr.step_counter) - 1
    live = [b for b in _dropping(model) if len(b.ops)]
    assert live
    from atomnas_amd import functional as AF
    for b in live:
        assert np.array_equal(AF.drop_connect_keep(b).cpu().numpy(), DR.keep_mask(model.dropout_seed, c, b.drop_connect_index, 8, b.drop_connect_rate))


def test_inference_ignores_the_rate(gpu_lib):
    from atomnas_amd import inference
    from atomnas_amd.models import mobilenet_supernet as ms
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    logits = []
    for rate in (0.0, 0.5):
        model = ms.Model(**TINY, drop_connect_rate=rate)
        randomize(model, 5)
        model.cuda().eval()
        net = inference.compile_for_inference(model)
        with torch.no_grad():
            logits.append(net(x).detach().clone())
    assert torch.equal(logits[0], logits[1]) and bool(torch.isfinite(logits[0]).all())


def test_train_entry_with_drop_connect(gpu_lib, tmp_path):
    env = dict(os.environ, ATOMNAS_E2E_DIR=str(tmp_path), ARNOLD_OUTPUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "app:" + os.path.join(ROOT, "tests", "data", "tiny_drop_connect.yml")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert out.count(" val: ") >= 2 and out.count(" step ") >= 6, out[-4000:]
    assert os.path.exists(os.path.join(str(tmp_path), "latest_checkpoint.pt"))
