"""Gradient accumulation on the GPU (engine.TrainStep(accum_steps=A)): A micro-batches run one after another on one card are, in
arithmetic, A more ranks of a data-parallel job with allreduce_bn.  Checked bit for bit: the fold kernel against torch, the
accumulated gradient arena against the in-order sum of single backward passes, a whole accumulated run against two real (gloo)
ranks, the BatchNorm running-statistics semantics, graph replay against eager launches, the in-graph collective form, the
dropout masks, the scalars, the misuse errors, a shrink between optimizer steps and the train.py entry point.

The model is the one of tests/test_distributed_gpu.py::_worker: input 64, batch 8, 10 classes, five blocks with k 3/5/7, RMSprop +
EMA + prune info."""
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("P", "SQ", "BUF", "EMA", "S", "SEMA", "CNT")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(8, 3, 64, 64, generator=g).cuda(), torch.randint(0, 10, (8,), generator=g).cuda()


def _make(accum=None, use_graph=True, dropout=0.0, **kw):
    """a fresh model (same initialisation every time) and its TrainStep; accum None: the constructor's default"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from atomnas_amd import engine
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import model_profiling as mp_
    from atomnas_amd.utils import optim as aopt
    from atomnas_amd.utils import prune as aprune
    from atomnas_amd.utils import rmsprop
    torch.manual_seed(7)
    model = ms.Model(num_classes=10, input_size=64, input_channel=16, last_channel=64, dropout_ratio=dropout, batch_norm_momentum=0.01,
                     batch_norm_epsilon=1e-3, active_fn="nn.ReLU",
                     inverted_residual_setting=[[1, 8, 1, 1, [3]], [6, 16, 2, 2, [3, 5, 7]], [6, 24, 1, 2, [3, 5, 7]], [6, 32, 1, 2, [3, 5, 7]],
                                                [6, 40, 1, 2, [3, 5, 7]]])
    model.apply(mb.init_weights_mnas)
    mp_.model_profiling(model, 64, 64, verbose=False)
    model.cuda().train()
    pinfo = aprune.get_bn_to_prune(model, {'bn_prune_filter': 'expansion_only_skip_expand1'}, verbose=False)
    opt = rmsprop.RMSprop(model.parameters(), lr=0.01, alpha=0.9, momentum=0.9, eps=1e-3, eps_inside_sqrt=True)
    ema = aopt.ExponentialMovingAverage(0.99)
    for n, p in model.named_parameters():
        ema.register(n, p)
    for n, b in model.named_buffers():
        if "running" in n:
            ema.register(n, b)
    if accum is not None:
        kw["accum_steps"] = accum
    return engine.TrainStep(model, opt, ema, pinfo, batch_size=8, image_size=64, use_graph=use_graph, **kw)


def _accum_step(ts, batches, **kw):
    """one optimizer step over len(batches) == ts.accum_steps micro-batches"""
    for x, y in batches[:-1]:
        ts.set_batch(x, y)
        ts.accumulate()
    ts.set_batch(*batches[-1])
    ts.step(**kw)


def _state(ts):
    torch.cuda.synchronize()
    return {k: getattr(ts.mgr, k).detach().clone() for k in STATE}


# ------------------------------------------------------------------------------------------------------------------ 1. fold kernel
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("A", [1, 2, 3])
def test_fold_kernel_matches_torch(gpu_lib, n, A):
    """acc = (first ? 0 : acc) + cur; then cur = base (not last) or cur = acc * inv_count (last): first / middle / last over A
    micro-batches, with and without a base, exact.  The buffers carry a guard band that must stay untouched."""
    from atomnas_amd import ops
    g = torch.Generator().manual_seed(n * 10 + A)
    inv = torch.tensor(1.0 / A, dtype=torch.float32)   # the kernel takes the factor as fp32
    pad = 8   # guard band behind the n floats (the buffers themselves stay 16-byte aligned)
    for with_base in (True, False):
        acc = torch.full((n + pad,), 777.0).cuda()      # stale contents: `first` must ignore them
        base = torch.randn(n + pad, generator=g).cuda() if with_base else None
        base0 = base.clone() if with_base else None
        cur = torch.empty(n + pad, device="cuda")
        want_acc = None
        for i in range(A):
            first, last = i == 0, i == A - 1
            c = torch.randn(n + pad, generator=g).cuda()
            cur.copy_(c)
            ops.accum_fold(acc, cur, base, n, first, last, float(inv))
            torch.cuda.synchronize()
            want_acc = (torch.zeros(n, device="cuda") if first else want_acc) + c[:n]
            want_cur = want_acc * inv.cuda() if last else (base[:n] if with_base else c[:n])
            assert torch.equal(acc[:n], want_acc), (n, A, i)
            assert torch.equal(cur[:n], want_cur), (n, A, i)
            assert torch.equal(cur[n:], c[n:]) and bool((acc[n:] == 777.0).all()), "wrote past n"
            assert not with_base or torch.equal(base, base0)


# ------------------------------------------------------------------------------------------------------------------ 2. gradient sum
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("A", [2, 3])
def test_accumulated_gradients_are_the_in_order_sum(gpu_lib, A, use_graph):
    """mgr.G after the A micro-batches == ((g1 + g2) + g3) of the arenas a single _fwd_bwd() leaves per batch (lr 0 and rho 0: the
    parameters stay where they are and the L1 term adds zeros, so the arena can be read after step())"""
    ts = _make(A, use_graph)
    batches = [_batch(100 + i) for i in range(A)]
    singles = []
    for x, y in batches:
        ts.set_batch(x, y)
        ts._fwd_bwd()
        torch.cuda.synchronize()
        singles.append(ts.mgr.G.detach().clone())
    assert not torch.equal(singles[0], singles[1])
    want = singles[0]
    for gq in singles[1:]:
        want = want + gq
    for _ in range(2):   # the second group starts from zero again
        _accum_step(ts, batches, lr=0.0, rho=0.0)
        torch.cuda.synchronize()
        assert ts.pending == 0
        assert torch.equal(ts.mgr.G, want), float((ts.mgr.G - want).abs().max())
    if use_graph:
        assert ts.g_mb is not None and ts.g_last is not None and ts.g_fwd_bwd is None   # only the graphs accumulation adds


# ------------------------------------------------------------------------------------------------------------------ 3. virtual = real ranks
def _rank_worker(rank, world, port, path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ts = _make(1, True, world_size=world, allreduce_bn=True)
        ts.set_batch(*_batch(100 + rank))
        losses = []
        for _ in range(3):
            ts.step(lr=0.003, rho=1e-4)
            losses.append(ts.loss.detach().cpu().clone())
        assert ts.comm_mode == "host"
        out = {k: v.cpu() for k, v in _state(ts).items()}
        out["losses"] = torch.stack(losses)
        torch.save(out, os.path.join(path, "rank%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_micro_batches_equal_two_real_ranks(gpu_lib, tmp_path):
    """world 2 x A 1 with allreduce_bn against world 1 x A 2 over the same two batches: every arena bit for bit after 3 steps"""
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    for p in procs:
        if p.is_alive():
            p.terminate()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]   # a failed rank ends the test here
    ref = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(world)]
    ts = _make(2, True)
    batches = [_batch(100), _batch(101)]
    losses = []
    for _ in range(3):
        _accum_step(ts, batches, lr=0.003, rho=1e-4)
        losses.append(ts.loss.detach().cpu().clone())
    got = _state(ts)
    for k in STATE:
        assert torch.equal(got[k].cpu(), ref[0][k]), (k, float((got[k].cpu().double() - ref[0][k].double()).abs().max()))
        assert torch.equal(ref[0][k], ref[1][k]) or k == "CNT", k   # the real ranks agree with each other (allreduce_bn)
    losses = torch.stack(losses)
    assert not torch.equal(ref[0]["losses"][:, 0], ref[1]["losses"][:, 0]), "ranks were supposed to see different batches"
    assert torch.equal(losses[:, 0], (ref[0]["losses"][:, 0] + ref[1]["losses"][:, 0]) * torch.tensor(0.5))   # mean of the CE means
    assert torch.equal(losses[:, 1:], ref[0]["losses"][:, 1:])                                               # L2, L1 as a rank has them


# ------------------------------------------------------------------------------------------------------------------ 4. statistics
def test_running_statistics_are_the_mean_over_the_micro_batches(gpu_lib):
    ts = _make(2, False)
    mgr = ts.mgr
    batches = [_batch(100), _batch(101)]
    s0, c0 = mgr.S.detach().clone(), mgr.CNT.detach().clone()
    alone = []
    for x, y in batches:   # what each batch alone leaves from the same starting statistics
        ts.set_batch(x, y)
        ts._fwd_bwd()
        torch.cuda.synchronize()
        alone.append(mgr.S.detach().clone())
        mgr.S.copy_(s0)
        mgr.CNT.copy_(c0)
    assert not torch.equal(alone[0], alone[1]) and not torch.equal(alone[0], s0)
    sema0 = mgr.SEMA.detach().clone()
    ts.set_batch(*batches[0])
    ts.accumulate()
    torch.cuda.synchronize()
    assert torch.equal(mgr.S, s0), "a micro-batch must leave the statistics of the start of the step (no compounding)"
    assert torch.equal(mgr.CNT, c0)
    ts.set_batch(*batches[1])
    ts.step(lr=0.003, rho=1e-4)
    torch.cuda.synchronize()
    want = (alone[0] + alone[1]) * torch.tensor(0.5, device="cuda")
    assert torch.equal(mgr.S, want), float((mgr.S - want).abs().max())
    assert torch.equal(mgr.CNT, c0 + 1)
    # the EMA of the statistics read the folded values
    from atomnas_amd import ops
    d = torch.tensor(float(mgr.hyper[ops.HYP_EMA_DECAY]), dtype=torch.float32, device="cuda")
    assert torch.allclose(mgr.SEMA, sema0 * d + (1.0 - d) * want, rtol=1e-6, atol=1e-7)


def test_one_micro_batch_is_the_plain_step(gpu_lib):
    a, b = _make(None, True), _make(1, True)
    x, y = _batch(100)
    for ts in (a, b):
        ts.set_batch(x, y)
        for _ in range(3):
            ts.step(lr=0.003, rho=1e-4)
    sa, sb = _state(a), _state(b)
    for k in STATE:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.loss, b.loss) and torch.equal(a.topk, b.topk)
    # nothing of the accumulation machinery exists at A = 1
    assert b.accum_steps == 1 and b.pending == 0
    assert b._acc is None and b._sacc is None and b._sbase is None and b._pool is None
    assert b.g_mb is None and b.g_last is None and b.g_all_last is None and b.g_fwd_bwd is not None
    with pytest.raises(RuntimeError):
        b.accumulate()
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            _make(bad, False)


# ------------------------------------------------------------------------------------------------------------------ 5. graph = eager
def test_graph_replay_equals_eager(gpu_lib):
    res = []
    batches = [_batch(100), _batch(101)]
    for use_graph in (False, True):
        ts = _make(2, use_graph)
        for _ in range(3):
            _accum_step(ts, batches, lr=0.003, rho=1e-4)
        st = _state(ts)
        st["loss"], st["topk"] = ts.loss.detach().clone(), ts.topk.detach().clone()
        res.append(st)
    for k in ("P", "S", "EMA", "SQ", "CNT", "loss", "topk"):
        assert torch.equal(res[0][k], res[1][k]), k


def _force_worker(port, out):
    """One rank, RCCL, collective forced on: the last micro-batch with its bucketed in-graph collectives (every bucket folded into the
    running sum before it travels) must equal the form without any collective bit for bit -- over one rank the sum is the identity."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ATOMNAS_FORCE_ALLREDUCE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        res = []
        batches = [_batch(100), _batch(101)]
        for force in (True, False):
            ts = _make(2, True, allreduce_bn=force)
            for _ in range(3):
                _accum_step(ts, batches, lr=0.003, rho=1e-4, reduce=force)
            st = _state(ts)
            st["loss"] = ts.loss.detach().clone()
            if force:
                assert ts.comm_mode == "graph" and ts.g_all_last is not None and ts.g_all is None, (ts.comm_mode, ts.g_all_last)
                assert len(ts._buckets) >= 1 and ts._fired == len(ts._buckets)
            res.append(st)
        for k in res[0]:
            assert torch.equal(res[0][k], res[1][k]), k
        out["ok"] = 1
    finally:
        dist.destroy_process_group()


def test_in_graph_collective_form_equals_the_form_without(gpu_lib):
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    p = ctx.Process(target=_force_worker, args=(_free_port(), out))
    p.start()
    p.join(timeout=300)
    if p.is_alive():
        p.terminate()
    assert p.exitcode == 0 and out.get("ok") == 1


# ------------------------------------------------------------------------------------------------------------------ 6. dropout
def test_micro_batches_draw_their_own_dropout_masks(gpu_lib):
    from atomnas_amd import functional as F
    ts = _make(2, False, dropout=0.2)
    x, y = _batch(100)
    F.TAIL_TAP = taps = []
    try:
        for _ in range(2):
            _accum_step(ts, [(x, y), (x, y)], lr=0.003, rho=1e-4)
        torch.cuda.synchronize()
    finally:
        F.TAIL_TAP = None
    masks = [t.clone() for t in taps]
    assert len(masks) == 4 and all(m is not None and 0.5 < float(m.float().mean()) < 0.95 for m in masks)
    for i in range(4):   # within a step (0, 1) / (2, 3) and between steps
        for j in range(i + 1, 4):
            assert not torch.equal(masks[i], masks[j]), (i, j)
    assert int(ts.mgr.step_counter) == 4   # once per micro-batch


# ------------------------------------------------------------------------------------------------------------------ 7. scalars, misuse, reset
def test_scalars_misuse_and_reset(gpu_lib):
    a, b = _make(2, True), _make(2, True)
    b0, b1, b2 = _batch(100), _batch(101), _batch(102)
    ce, hits, vec = [], [], []
    for x, y in (b0, b1):
        a.set_batch(x, y)
        a._fwd_bwd()
        torch.cuda.synchronize()
        ce.append(a.loss[0].clone()), hits.append(a.topk.clone()), vec.append(a.loss_vec.clone())
    keep_s, keep_c = a.mgr.S.clone(), a.mgr.CNT.clone()
    b.mgr.S.copy_(keep_s), b.mgr.CNT.copy_(keep_c)   # `a` has seen two forward passes above: give the twin the same statistics
    # a partial group, discarded: the full group after it equals the twin's fresh one
    a.set_batch(*b2)
    a.accumulate()
    assert a.pending == 1
    a.reset_accumulation()
    assert a.pending == 0
    for ts in (a, b):
        _accum_step(ts, [b0, b1], lr=0.003, rho=1e-4)
    sa, sb = _state(a), _state(b)
    for k in STATE:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.loss, b.loss)
    # contract item 5
    assert torch.equal(a.loss[0], (ce[0] + ce[1]) * torch.tensor(0.5, device="cuda"))
    assert torch.equal(a.topk, hits[0] + hits[1])
    assert torch.equal(a.loss_vec, vec[1])          # the last micro-batch's per-sample losses
    assert float(a.loss[1]) > 0 and float(a.loss[2]) > 0
    # misuse
    with pytest.raises(RuntimeError, match="accumulate"):
        a.step(lr=0.003)                            # pending != A - 1
    a.set_batch(*b0)
    a.accumulate()
    with pytest.raises(RuntimeError, match="step"):
        a.accumulate()                              # pending == A - 1
    a.mgr.mark_dirty()                              # an arena rebuild inside the group
    with pytest.raises(RuntimeError, match="rebuilt"):
        a.step(lr=0.003)
    a.reset_accumulation()
    _accum_step(a, [b0, b1], lr=0.003, rho=1e-4)    # and the step works again on the rebuilt arenas
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a.loss).all()) and bool(torch.isfinite(a.mgr.P).all())


def test_shrink_between_accumulated_steps(gpu_lib):
    """one forced shrink as in tests/test_shrink_gpu.py between two accumulated steps: the sums follow the rebuilt arenas"""
    sys.path.insert(0, ROOT)
    import train as T
    from atomnas_amd import engine
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import config, model_profiling as mp_, optim as aopt, prune as aprune, rmsprop
    g = torch.load(os.path.join(ROOT, "tests", "golden", "shrink.pt"), weights_only=False)
    model = ms.Model(**g["kw"])
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
    ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=1e-5, batch_size=8, image_size=64, use_graph=True, accum_steps=2)
    batches = [_batch(100), _batch(101)]
    _accum_step(ts, batches, lr=0.002, rho=1e-4)
    v0, n0 = ts.mgr.version, ts.mgr.nP

    class F(dict):
        __getattr__ = dict.__getitem__
    config.FLAGS.bind(F(image_size=64, use_distributed=False))
    wrapper = torch.nn.Module()
    wrapper.module = model
    T.shrink_model(wrapper, ema, opt, pinfo, 1e-3, ema_only=False)
    _accum_step(ts, batches, lr=0.002, rho=1e-4)
    torch.cuda.synchronize()
    assert ts.mgr.version > v0 and ts.mgr.nP < n0 and ts._acc.numel() == ts.mgr.nP + 256
    p1 = ts.mgr.P.detach().clone()
    assert bool(torch.isfinite(ts.loss).all()) and bool(torch.isfinite(p1).all())
    _accum_step(ts, batches, lr=0.002, rho=1e-4)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ts.mgr.P).all()) and float((ts.mgr.P - p1).abs().max()) > 0, "parameters did not move"


# ------------------------------------------------------------------------------------------------------------------ 8. entry point
def test_train_entry_accumulates(gpu_lib, tmp_path):
    """`python train.py app:tests/data/tiny_accum.yml` for one short epoch: 3 optimizer steps over 6 loader batches, a checkpoint"""
    env = dict(os.environ, ATOMNAS_E2E_DIR=str(tmp_path), ARNOLD_OUTPUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "app:" + os.path.join(ROOT, "tests", "data", "tiny_accum.yml"),
                        "--num_epochs", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "grad_accum_steps: 2" in out and "batch_size: 16" in out, out[-4000:]
    steps = [l for l in out.splitlines() if " step " in l and "img/s" in l]
    assert len(steps) == 6 // 2, out[-4000:]            # loader batches // 2
    assert " step 3 " in steps[-1] and " step 4 " not in out
    assert out.count(" val: ") == 1
    assert os.path.exists(os.path.join(str(tmp_path), "latest_checkpoint.pt"))
