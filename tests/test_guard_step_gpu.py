"""The guarded training step on the GPU (engine.TrainStep(clip_norm=, skip_nonfinite=)): with finite gradients and no clipping it is
the un-guarded step bit for bit in every step form; a step whose gradient arena holds a NaN is dropped (parameters, optimizer state,
both EMAs and the BatchNorm running statistics keep their bits) and the next step continues as if it had not happened; clipping equals
the un-guarded optimizer tail run with the reported gradient scale; two ranks reach the same verdict without a collective of their own.

Model and TrainStep: the ones of tests/test_grad_accum_gpu.py (input 64, batch 8, 10 classes, RMSprop + EMA + prune info)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import guard_util as U
from test_grad_accum_gpu import ROOT, STATE, _accum_step, _batch, _free_port, _make, _state

pytestmark = pytest.mark.gpu
ARENAS = STATE + ("G",)
LR, RHO = 0.003, 1e-4


def _all(ts):
    st = _state(ts)
    st["G"], st["loss"], st["topk"] = ts.mgr.G.detach().clone(), ts.loss.detach().clone(), ts.topk.detach().clone()
    return st


def _assert_same(a, b, keys=None, what=""):
    for k in keys or a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))


def _split_step(ts, poison=None, lr=LR, rho=RHO):
    """step() through its own seam: the forward-backward half, [NaN into one element of G], the collective, the optimizer half.  These
    are the pieces step() itself runs when it has a seam (no in-graph collective): eager launches or g_fwd_bwd + g_opt replays."""
    do_reduce, overlapped = ts._step_begin(lr, rho, None, None)
    assert not overlapped
    ts._half_fwd_bwd()
    if poison is not None:
        ts.mgr.G[poison] = float("nan")
    ts._half_reduce(do_reduce)
    ts._half_opt()
    ts._step_end()


# ------------------------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_guard_without_clipping_is_the_plain_step(gpu_lib, use_graph, A):
    """skip_nonfinite on finite data: GUARD_SCALE = hyper[HYP_GRAD_SCALE] * 1.0, so every arena equals the un-guarded twin's"""
    a, b = _make(A, use_graph, skip_nonfinite=True), _make(A, use_graph)
    batches = [_batch(100 + i) for i in range(A)]
    for _ in range(3):
        for ts in (a, b):
            _accum_step(ts, batches, lr=LR, rho=RHO)
    _assert_same(_all(a), _all(b))
    st = a.guard_state()
    assert st["ok"] is True and st["coef"] == 1.0 and st["skipped"] == 0 and st["clipped"] == 0
    want = float(torch.linalg.vector_norm(b.mgr.G.double())) / A   # hyper[HYP_GRAD_SCALE] = 1 / A
    assert abs(st["norm"] - want) <= U.norm_rel_bound(a.mgr.nP) * want
    # the twin owns nothing of the guard, and misuse is an error
    assert b._guard is None and b._guard_ws is None and (A > 1 or b._sbase is None)
    with pytest.raises(RuntimeError):
        b.guard_state()
    if use_graph and A == 1:
        assert a.g_fwd_bwd is not None and a.g_opt is not None


# ------------------------------------------------------------------------------------------------------------------ 2. skip at the seam
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_a_nan_in_the_gradient_arena_drops_the_step(gpu_lib, use_graph):
    """One clean step, then a step with a NaN written into G between its two halves: P, SQ, BUF, EMA, SEMA and S keep the bits they had
    before that step, the skipped counter reads 1.  The clean step after it equals the step of an un-guarded twin that never saw the
    poisoned one, once the twin has been advanced by what a dropped step advances: global_step (the EMA warm-up decay), the EMA's
    update count, the dropout counter and num_batches_tracked (CNT)."""
    from atomnas_amd import ops
    a, b = _make(1, use_graph, skip_nonfinite=True), _make(1, use_graph)
    x, y = _batch(100)
    for ts in (a, b):
        ts.set_batch(x, y)
        ts.step(lr=LR, rho=RHO)
    before = _state(a)
    updates = [i["num_updates"] for i in a.ema._info.values()]
    _split_step(a, poison=a.mgr.nP // 3)
    after = _state(a)
    _assert_same(after, before, ("P", "SQ", "BUF", "EMA", "SEMA", "S"), "dropped step")
    assert torch.equal(after["CNT"], before["CNT"] + 1)
    st = a.guard_state()
    assert st["ok"] is False and st["skipped"] == 1 and st["clipped"] == 0 and st["coef"] == 1.0 and st["norm"] != st["norm"]
    assert a.global_step == 2 and [i["num_updates"] for i in a.ema._info.values()] == [u + 1 for u in updates]
    assert int(a.mgr.step_counter) == 2
    # the twin catches up on the counters, then both take a clean step
    b.global_step += 1
    b.ema.note_updates(1, float(a.ema.momentum_at(2)))
    ops.add_i64(b.mgr.step_counter, 1)
    ops.add_i64(b.mgr.CNT, 1)
    x2, y2 = _batch(101)
    for ts in (a, b):
        ts.set_batch(x2, y2)
    _split_step(a)
    b.step(lr=LR, rho=RHO)
    _assert_same(_all(a), _all(b), what="clean step after the dropped one")
    assert a.guard_state()["skipped"] == 1 and a.guard_state()["ok"] is True
    assert float((a.mgr.P - before["P"]).abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ 3. skip end to end
def test_an_infinite_classifier_bias_is_skipped_end_to_end(gpu_lib):
    """step() unmodified, with graphs.  The poison is a classifier bias at +inf, and G becomes non-finite by the step's own arithmetic:
    every row's logit of that class is +inf; in k_ce_smooth (csrc/head.hip) the row maximum mx is +inf and expf(x - mx) of that column
    is expf(inf - inf) = NaN, so the row's sum, its log-sum-exp and every dlogit of the row are NaN; the classifier's weight and bias
    gradients are sums over those rows: NaN.  The step is dropped; with the poison removed training goes on with finite parameters."""
    a = _make(1, True, skip_nonfinite=True, clip_norm=1e3)
    x, y = _batch(100)
    a.set_batch(x, y)
    a.step(lr=LR, rho=RHO)
    bias = a.model.classifier[1].bias
    off = bias._atomnas_off
    assert bias.data_ptr() == a.mgr.P[off:].data_ptr(), "the bias is expected to live in the parameter arena"
    before = _state(a)
    with torch.no_grad():
        bias[0] = float("inf")
    a.step(lr=LR, rho=RHO)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(a.mgr.G).all()), "the poison did not reach the gradient arena"
    st = a.guard_state()
    assert st["ok"] is False and st["skipped"] == 1 and st["coef"] == 1.0
    after = _state(a)
    assert float(after["P"][off]) == float("inf")
    after["P"][off] = before["P"][off]
    _assert_same(after, before, ("P", "SQ", "BUF", "EMA", "SEMA", "S"), "dropped step")
    with torch.no_grad():
        bias[0] = before["P"][off]
    for _ in range(2):
        a.step(lr=LR, rho=RHO)
    torch.cuda.synchronize()
    st = a.guard_state()
    assert st["ok"] is True and st["skipped"] == 1 and st["norm"] == st["norm"] and st["norm"] < float("inf")
    for k in ("P", "SQ", "BUF", "EMA", "SEMA", "S"):
        assert bool(torch.isfinite(getattr(a.mgr, k)).all()), k
    assert bool(torch.isfinite(a.loss).all()) and float((a.mgr.P - before["P"]).abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ 4. clip
def test_clipping_equals_the_plain_tail_with_the_reported_scale(gpu_lib):
    """clip_norm = half the norm of the first step's gradient (from a guard-off twin's G, float64: after its step G holds the cross
    entropy gradient plus the L1 term, which is what the guard sees).  coef = clip / (norm + 1e-6) is then 0.5 up to the norm's error
    bound (tests/guard_util.py), the 1e-6 of the formula relative to the norm, and the roundings of the addition and the division
    (2^-23).  The step equals an un-guarded step whose optimizer half runs with hyper[HYP_GRAD_SCALE] = the reported GUARD_SCALE."""
    from atomnas_amd import ops
    x, y = _batch(100)
    b = _make(1, True)
    b.set_batch(x, y)
    b.step(lr=LR, rho=RHO)
    torch.cuda.synchronize()
    norm = float(torch.linalg.vector_norm(b.mgr.G.double()))
    a = _make(1, True, clip_norm=0.5 * norm)
    a.set_batch(x, y)
    a.step(lr=LR, rho=RHO)
    st = a.guard_state()
    print("norm %.9g reported %.9g coef %.9g" % (norm, st["norm"], st["coef"]))
    assert st["ok"] is True and st["clipped"] == 1 and st["skipped"] == 0
    assert abs(st["norm"] - norm) <= U.norm_rel_bound(a.mgr.nP) * norm
    assert abs(st["coef"] - 0.5) <= 0.5 * (U.norm_rel_bound(a.mgr.nP) + 1e-6 / norm + 2.0 ** -23)
    assert torch.equal(a._guard[ops.GUARD_SCALE], a._guard[ops.GUARD_COEF])   # hyper[HYP_GRAD_SCALE] is 1 on one rank
    c = _make(1, True)
    c.set_batch(x, y)
    c._step_begin(LR, RHO, None, None)
    c._half_fwd_bwd()
    c.mgr.hyper[ops.HYP_GRAD_SCALE:ops.HYP_GRAD_SCALE + 1].copy_(a._guard[ops.GUARD_SCALE:ops.GUARD_SCALE + 1])
    c._half_opt()
    c._step_end()
    sa, sc = _all(a), _all(c)
    _assert_same(sa, sc, what="clipped step")
    assert not torch.equal(sa["P"], _state(b)["P"]), "clipping changed nothing"


# ------------------------------------------------------------------------------------------------------------------ 5. two ranks
def _rank_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ts = _make(1, True, world_size=world, skip_nonfinite=True)
        ts.set_batch(*_batch(100 + rank))

        def gathered(t):
            mine = t.detach().cpu().clone()
            parts = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            return parts
        ts.step(lr=LR, rho=RHO)
        assert ts.comm_mode == "host"
        before = _state(ts)
        _split_step(ts, poison=(ts.mgr.nP // 3) if rank == 0 else None)   # rank 0 alone is poisoned, before the collective
        after = _state(ts)
        st = ts.guard_state()
        assert st["ok"] is False and st["skipped"] == 1, (rank, st)   # both ranks: the NaN travelled with the sum
        for k in ("P", "SQ", "BUF", "EMA", "SEMA", "S"):
            assert torch.equal(after[k], before[k]), (rank, k)
        ts.step(lr=LR, rho=RHO)
        torch.cuda.synchronize()
        st = ts.guard_state()
        assert st["ok"] is True and st["skipped"] == 1, (rank, st)
        parts = gathered(ts.mgr.P)
        assert torch.equal(parts[0], parts[1]), "ranks diverged"
        assert bool(torch.isfinite(ts.mgr.P).all()) and float((ts.mgr.P - before["P"]).abs().max()) > 0
        norms = gathered(ts._guard)
        assert torch.equal(norms[0].view(torch.int32), norms[1].view(torch.int32)), "the verdict differs between the ranks"
        out[rank] = 1
    finally:
        dist.destroy_process_group()


def test_two_ranks_skip_together(gpu_lib):
    world = 2
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    for p in procs:
        if p.is_alive():
            p.terminate()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]   # a failed rank ends the test here
    assert sorted(out.keys()) == list(range(world))


# ------------------------------------------------------------------------------------------------------------------ 6. one-graph form
def _one_graph_worker(port, out):
    """One rank, RCCL, collective forced on: the step is ONE graph with the bucketed collectives inside and _opt() at its end.  The
    guarded form equals the un-guarded one on finite data, drops the step with the infinite classifier bias (see test 3), and a
    step(reduce=False) between reducing steps (the two-graph pair, on the same guard vector) keeps counting."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ATOMNAS_FORCE_ALLREDUCE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        x, y = _batch(100)
        res = []
        for guard in (True, False):
            ts = _make(1, True, skip_nonfinite=guard)
            ts.set_batch(x, y)
            for _ in range(3):
                ts.step(lr=LR, rho=RHO)
            assert ts.comm_mode == "graph" and ts.g_all is not None and ts.g_fwd_bwd is None, (ts.comm_mode, ts.g_all)
            res.append(_all(ts))
        _assert_same(res[0], res[1], what="one-graph form")
        ts = _make(1, True, skip_nonfinite=True)
        ts.set_batch(x, y)
        ts.step(lr=LR, rho=RHO)
        bias = ts.model.classifier[1].bias
        off = bias._atomnas_off
        before = _state(ts)
        with torch.no_grad():
            bias[0] = float("inf")
        ts.step(lr=LR, rho=RHO)                 # the one graph
        ts.step(lr=LR, rho=RHO, reduce=False)   # g_fwd_bwd + g_opt
        after = _state(ts)
        assert ts.g_all is not None and ts.g_fwd_bwd is not None
        st = ts.guard_state()
        assert st["ok"] is False and st["skipped"] == 2, st
        after["P"][off] = before["P"][off]
        _assert_same(after, before, ("P", "SQ", "BUF", "EMA", "SEMA", "S"), "dropped steps")
        with torch.no_grad():
            bias[0] = before["P"][off]
        ts.step(lr=LR, rho=RHO)
        st = ts.guard_state()
        assert st["ok"] is True and st["skipped"] == 2 and bool(torch.isfinite(ts.mgr.P).all())
        assert float((ts.mgr.P - before["P"]).abs().max()) > 0
        out["ok"] = 1
    finally:
        dist.destroy_process_group()


def test_one_graph_form_with_in_graph_collectives(gpu_lib):
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    p = ctx.Process(target=_one_graph_worker, args=(_free_port(), out))
    p.start()
    p.join(timeout=300)
    if p.is_alive():
        p.terminate()
    assert p.exitcode == 0 and out.get("ok") == 1


# ------------------------------------------------------------------------------------------------------------------ 7. entry point
def test_train_entry_logs_the_guard(gpu_lib, tmp_path):
    """`python train.py app:tests/data/tiny_guard.yml` for one short epoch: every log line carries gnorm / skipped / clipped"""
    env = dict(os.environ, ATOMNAS_E2E_DIR=str(tmp_path), ARNOLD_OUTPUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "app:" + os.path.join(ROOT, "tests", "data", "tiny_guard.yml"),
                        "--num_epochs", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    steps = [l for l in out.splitlines() if " step " in l and "img/s" in l]
    assert len(steps) == 3, out[-4000:]
    for l in steps:
        assert " gnorm " in l and " skipped 0 " in l and " clipped " in l, l
        assert float(l.split(" gnorm ")[1].split()[0]) > 0
    assert os.path.exists(os.path.join(str(tmp_path), "latest_checkpoint.pt"))
