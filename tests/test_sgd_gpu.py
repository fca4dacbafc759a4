"""The fused SGD optimizer on the GPU (atomnas_fused_sgd_ema behind atomnas_amd.utils.sgd.SGD and engine.TrainStep) against
torch.optim.SGD in float64 on the CPU: arithmetic on given gradients, the whole training step (eager and hipGraph replay), shrink,
checkpoint exchange with torch.optim.SGD, two data-parallel ranks, and the train.py entry point with tests/data/tiny_sgd.yml.

Tolerances are the ones tests/test_train_step_gpu.py::test_optimizer_and_ema_arithmetic uses for this kind of comparison: parameters
and EMA rtol 1e-5, atol 1e-5 * max(1e-3, max|ref|); momentum_buffer rtol 1e-4, atol 1e-6; the L2 value rtol 1e-5."""
import collections
import os
import re
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import atomnas_oracle as orc  # noqa: E402

from kutil import assert_close  # noqa: E402
from test_block_gpu import TINY, _randomize  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(0.9, True), (0.9, False), (0.0, False)]


def _setup(momentum=0.9, nesterov=True, seed=21):
    """tests/test_train_step_gpu.py:_setup with the SGD optimizer"""
    from atomnas_amd import engine
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import model_profiling as mp_
    from atomnas_amd.utils import optim as aopt
    from atomnas_amd.utils import prune as aprune
    from atomnas_amd.utils import sgd
    model = ms.Model(**TINY)
    model.set_compute_dtype(torch.float32)
    _randomize(model, seed)
    mp_.model_profiling(model, 64, 64, verbose=False)
    sd = collections.OrderedDict((k, v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items())
    spec = orc.spec_from_model(model)
    model.cuda().train()
    pinfo = aprune.get_bn_to_prune(model, {'bn_prune_filter': 'expansion_only_skip_expand1'}, verbose=False)
    opt = sgd.SGD(model.parameters(), lr=0.01, momentum=momentum, nesterov=nesterov)
    ema = aopt.ExponentialMovingAverage(0.99)
    for n, p in model.named_parameters():
        ema.register(n, p)
    for n, b in model.named_buffers():
        if 'running' in n:
            ema.register(n, b)
    return model, sd, spec, pinfo, opt, ema, engine


def _has_l2(name, shape, method):
    """cal_l2_loss of the reference (utils/optim.py:210-249): which tensors carry weight decay"""
    if method == 'slimmable':
        return (len(shape) == 4 and shape[1] != 1) or len(shape) == 2
    return len(shape) in (2, 4) or (len(shape) == 1 and 'classifier' in name)


def _torch_sgd_step(p_before, grads, bufs, lr, momentum, nesterov):
    """One torch.optim.SGD.step in float64 on the CPU.  p_before / grads: {name: tensor}; bufs: {name: momentum_buffer} or None before
    the first step (torch then sets buf = g).  Returns (parameters, momentum buffers) after the step."""
    names = list(p_before)
    ps = [torch.nn.Parameter(p_before[n].detach().double().cpu().clone()) for n in names]
    ref = torch.optim.SGD(ps, lr=lr, momentum=momentum, nesterov=nesterov, weight_decay=0)
    for n, p in zip(names, ps):
        p.grad = grads[n].detach().double().cpu().clone()
        if bufs is not None and momentum > 0:
            ref.state[p]['momentum_buffer'] = bufs[n].detach().double().cpu().clone()
    ref.step()
    return ({n: p.detach() for n, p in zip(names, ps)},
            {n: ref.state[p]['momentum_buffer'] for n, p in zip(names, ps)} if momentum > 0 else None)


def _check(model, opt, ref_p, ref_buf, momentum, tag=""):
    for n, p in model.named_parameters():
        s = max(1e-3, float(ref_p[n].abs().max()))
        assert_close(tag + "param " + n, p.detach(), ref_p[n], rtol=1e-5, atol=1e-5 * s)
        if momentum > 0:
            assert set(opt.state[p].keys()) == {'momentum_buffer'}, (n, opt.state[p].keys())
            assert_close(tag + "buf " + n, opt.state[p]['momentum_buffer'], ref_buf[n], rtol=1e-4, atol=1e-6)
        else:
            assert p not in opt.state or len(opt.state[p]) == 0


# ------------------------------------------------------------------------------------------------- 5. arithmetic on given gradients
@pytest.mark.parametrize("wd_method", ["slimmable", "mnas"])
@pytest.mark.parametrize("momentum,nesterov", CASES)
def test_sgd_and_ema_arithmetic_on_given_gradients(gpu_lib, momentum, nesterov, wd_method):
    """The SGD twin of test_optimizer_and_ema_arithmetic: 3 steps, random gradients written into p.grad, lr and rho varying per step,
    the L2 and L1 regulariser gradients on top; reference = torch.optim.SGD on float64 copies fed g + wd*p + rho*penalty*sign(p)."""
    model, sd, spec, pinfo, opt, ema, engine = _setup(momentum, nesterov)
    from atomnas_amd import runtime
    from atomnas_amd.utils import optim as aopt
    from atomnas_amd.utils import prune as aprune
    mgr = runtime.manager_of(model)
    ema.attach(mgr)
    mgr.ensure()
    names, pen, _ = orc.prune_penalties(spec, 64)
    g = torch.Generator().manual_seed(11)
    params = collections.OrderedDict(model.named_parameters())
    ref_p = {n: sd[n].clone() for n in params}
    ref_buf = None
    ref_ema = collections.OrderedDict((k, v.clone()) for k, v in sd.items() if v.is_floating_point())
    for step in range(3):
        lr, rho, wd = 0.003 * (step + 1), 2e-3 * (step + 1), 1e-3
        opt.zero_grad()
        grads = {n: torch.randn(p.shape, generator=g) * 0.05 for n, p in params.items()}
        for n, p in params.items():
            p.grad.copy_(grads[n].cuda())
        (aopt.cal_l2_loss(model, wd, wd_method) + aprune.cal_bn_l1_loss([params[n] for n in pinfo.weight], pinfo.penalty, rho)).backward()
        opt.param_groups[0]['lr'] = lr
        opt.step()
        d = ema.momentum_at(step + 1)
        ema.update_all(step + 1)
        torch.cuda.synchronize()
        full = {}
        for n in params:
            gr = grads[n].double()
            if _has_l2(n, tuple(ref_p[n].shape), wd_method):
                gr = gr + wd * ref_p[n]
            if n in names:
                gr = gr + rho * pen[names.index(n)] * torch.sign(ref_p[n])
            full[n] = gr
        ref_p, ref_buf = _torch_sgd_step(ref_p, full, ref_buf, lr, momentum, nesterov)
        for k in ref_ema:
            orc.ema_update(ref_ema[k], ref_p[k] if k in ref_p else sd[k], d)
        _check(model, opt, ref_p, ref_buf, momentum, "step %d " % step)
        for k in ref_ema:
            s = max(1e-3, float(ref_ema[k].abs().max()))
            assert_close("ema " + k, ema.average(k), ref_ema[k], rtol=1e-5, atol=1e-5 * s)
    assert (mgr.BUF is not None) == (momentum > 0)


def test_sgd_needs_no_square_avg_arena(gpu_lib):
    model, sd, spec, pinfo, opt, ema, engine = _setup()
    from atomnas_amd import runtime
    mgr = runtime.manager_of(model)
    mgr.attach_optimizer(opt)
    mgr.ensure()
    assert mgr.SQ is None and mgr.BUF is not None and mgr.BUF.numel() == mgr.nP
    assert all(set(opt.state[p].keys()) == {'momentum_buffer'} for p in model.parameters())


@pytest.mark.parametrize("momentum,nesterov", CASES)
def test_raw_entry_point_odd_length_and_null_arguments(gpu_lib, momentum, nesterov):
    """atomnas_fused_sgd_ema on n = 1000003 (not a multiple of 4 or 256): ema == NULL and wd_chunk == NULL, buf == NULL for momentum 0;
    everything outside [0, n) is NaN before and must be NaN after (a tail overrun would overwrite it); then with wd_chunk, ema and the
    L2 value against the float64 sum."""
    from atomnas_amd import ops
    n, pad = 1000003, 516   # pad keeps the slices 16-byte aligned
    g = torch.Generator().manual_seed(2)
    hyper = torch.tensor([0.05, 0.0, -1.0, 0.5, 0, 0, 0, 0], dtype=torch.float32).cuda()   # lr, rho, EMA decay (< 0: skip), grad scale

    def padded(x):
        t = torch.full((n + 2 * pad,), float('nan'), dtype=torch.float32)
        t[pad:pad + n] = x
        return t.cuda()
    p0, g0, b0, e0 = (torch.randn(n, generator=g) for _ in range(4))
    P, G, B = padded(p0), padded(g0), padded(b0)
    ops.fused_sgd_ema(P[pad:], G[pad:], B[pad:] if momentum > 0 else None, None, None, n, hyper, momentum, nesterov)
    torch.cuda.synchronize()
    for t in (P, B):
        assert bool(torch.isnan(t[:pad]).all()) and bool(torch.isnan(t[pad + n:]).all()), "write outside [0, n)"
    rp, rb = _torch_sgd_step({'x': p0}, {'x': g0.double() * 0.5}, {'x': b0}, 0.05, momentum, nesterov)
    assert_close("raw param", P[pad:pad + n], rp['x'], rtol=1e-5, atol=1e-5 * float(rp['x'].abs().max()))
    if momentum > 0:
        assert_close("raw buf", B[pad:pad + n], rb['x'], rtol=1e-4, atol=1e-6)
    else:
        assert torch.equal(B[pad:pad + n].cpu(), b0)   # not touched
    # the same call with every optional argument: wd per 256-element chunk, EMA, L2 value
    nch = (n + 255) // 256
    wdc = (torch.rand(nch, generator=g) * 1e-2).float()
    wdc[::3] = 0.0
    hyper[2] = 0.9
    P, G, B, E = padded(p0), padded(g0), padded(b0), padded(e0)
    l2 = torch.full((3,), float('nan'), dtype=torch.float32).cuda()
    ops.fused_sgd_ema(P[pad:], G[pad:], B[pad:] if momentum > 0 else None, E[pad:], wdc.cuda(), n, hyper, momentum, nesterov,
                      l2_value=l2[1:2])
    torch.cuda.synchronize()
    for t in (P, B, E):
        assert bool(torch.isnan(t[:pad]).all()) and bool(torch.isnan(t[pad + n:]).all()), "write outside [0, n)"
    assert bool(torch.isnan(l2[0])) and bool(torch.isnan(l2[2]))
    wd_el = wdc.double().repeat_interleave(256)[:n]
    rp, rb = _torch_sgd_step({'x': p0}, {'x': g0.double() * 0.5 + wd_el * p0.double()}, {'x': b0}, 0.05, momentum, nesterov)
    assert_close("raw param (wd)", P[pad:pad + n], rp['x'], rtol=1e-5, atol=1e-5 * float(rp['x'].abs().max()))
    if momentum > 0:
        assert_close("raw buf (wd)", B[pad:pad + n], rb['x'], rtol=1e-4, atol=1e-6)
    re_ = e0.double().clone()
    orc.ema_update(re_, rp['x'], 0.9)
    assert_close("raw ema", E[pad:pad + n], re_, rtol=1e-5, atol=1e-5 * float(re_.abs().max()))
    want = 0.5 * float((wd_el * p0.double() ** 2).sum())
    assert abs(float(l2[1]) - want) <= 1e-5 * abs(want), (float(l2[1]), want)


# ------------------------------------------------------------------------------------------------- 6. whole step, eager and graph
def _snapshot(model, ema):
    p = {n: q.detach().double().cpu().clone() for n, q in model.named_parameters()}
    e = {k: ema.average(k).detach().double().cpu().clone() for k in ema.average_names()}
    return p, e


def _step_and_check(ts, model, opt, ema, momentum, nesterov, lr, rho, wd, wd_method, ref_buf, tag):
    """One TrainStep.step checked against torch.optim.SGD in float64 on THIS step's gradient: the arena's p.grad after the step (data
    gradient summed over the ranks + world * L1 term; forward / backward are pinned against the oracle elsewhere) over world, plus
    wd * p at the parameters before the step.  ref_buf: the reference's own momentum buffers from the step before (None: first step).
    Returns the new ones."""
    p_before, e_before = _snapshot(model, ema)
    d = ema.momentum_at(ts.global_step + 1)
    ts.step(lr=lr, rho=rho)
    torch.cuda.synchronize()
    full = {}
    want_l2 = 0.0
    for n, p in model.named_parameters():
        gr = p.grad.detach().double().cpu() / max(ts.world_size, 1)
        if _has_l2(n, tuple(p.shape), wd_method):
            gr = gr + wd * p_before[n]
            want_l2 += 0.5 * wd * float((p_before[n] ** 2).sum())
        full[n] = gr
    ref_p, ref_buf = _torch_sgd_step(p_before, full, ref_buf, lr, momentum, nesterov)
    _check(model, opt, ref_p, ref_buf, momentum, tag)
    buffers = dict(model.named_buffers())
    for k, shadow in e_before.items():
        orc.ema_update(shadow, ref_p[k] if k in ref_p else buffers[k].detach().double().cpu(), d)
        s = max(1e-3, float(shadow.abs().max()))
        assert_close(tag + "ema " + k, ema.average(k), shadow, rtol=1e-5, atol=1e-5 * s)
    got = ts.loss.tolist()
    assert all(v == v for v in got), got
    assert abs(got[1] - want_l2) <= 1e-5 * abs(want_l2), (tag, got[1], want_l2)
    return ref_buf


def _batches(count, N=6, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(N, 3, 64, 64, generator=g), torch.randint(0, 10, (N,), generator=g)) for _ in range(count)]


def _two_steps(use_graph, momentum, nesterov, check):
    model, sd, spec, pinfo, opt, ema, engine = _setup(momentum, nesterov)
    ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=1e-3, wd_method='slimmable', label_smoothing=0.1, batch_size=6,
                          image_size=64, use_graph=use_graph)
    ref_buf = None
    for step, (x, y) in enumerate(_batches(2)):
        lr, rho = 0.02 * (1 + step), 1e-3 * (1 + step)
        ts.set_batch(x.cuda(), y.cuda())
        if check:
            ref_buf = _step_and_check(ts, model, opt, ema, momentum, nesterov, lr, rho, 1e-3, 'slimmable', ref_buf, "step %d " % step)
        else:
            ts.step(lr=lr, rho=rho)
    torch.cuda.synchronize()
    return ts, model, opt, ema, pinfo


@pytest.mark.parametrize("momentum,nesterov", CASES)
@pytest.mark.parametrize("use_graph", [False, True])
def test_train_step_matches_torch_sgd(gpu_lib, use_graph, momentum, nesterov):
    _two_steps(use_graph, momentum, nesterov, check=True)


def test_train_step_graph_equals_eager_and_is_reproducible(gpu_lib):
    runs = [_two_steps(use_graph, 0.9, True, check=False)[0].mgr for use_graph in (False, True, True, False)]
    for name in ("P", "BUF", "EMA"):
        ref = getattr(runs[0], name)
        assert float(ref.abs().max()) > 0
        for r in runs[1:]:
            assert torch.equal(getattr(r, name), ref), name


# ------------------------------------------------------------------------------------------------- 7. shrink under SGD
def test_shrink_under_sgd(gpu_lib):
    """After two steps, gammas (model and EMA shadow) of some channels and of one whole branch are set to zero and train.shrink_model
    runs, as in tests/test_shrink_gpu.py.  The optimizer's re-keying protocol is observed through its own two methods; the expected
    buffers are computed here by boolean indexing of the old ones on the CPU."""
    sys.path.insert(0, ROOT)
    import train as T
    from atomnas_amd.utils import config
    momentum, nesterov = 0.9, True
    ts, model, opt, ema, pinfo = _two_steps(True, momentum, nesterov, check=True)
    g = torch.Generator().manual_seed(9)
    blocks = list(model.get_named_block_list().items())
    with torch.no_grad():
        for bi, (bname, blk) in enumerate(blocks):
            for j, (nm, bn) in enumerate(blk.get_named_depthwise_bn().items()):
                if bi == 1 and j == 1:
                    dead = torch.ones(bn.weight.numel(), dtype=torch.bool)       # a whole branch goes
                elif bi == 0:
                    dead = torch.zeros(bn.weight.numel(), dtype=torch.bool)     # an untouched block
                else:
                    dead = torch.rand(bn.weight.numel(), generator=g) < 0.3
                    dead[0] = False
                bn.weight[dead.cuda()] = 0.0
                ema.average("{}.{}.weight".format(bname, nm))[dead.cuda()] = 0.0
    torch.cuda.synchronize()
    old_name = {id(p): n for n, p in model.named_parameters()}
    old_buf = {n: opt.state[p]['momentum_buffer'].detach().cpu().clone() for n, p in model.named_parameters()}
    n_before = len(opt.param_groups[0]['params'])
    masked, dropped = [], []
    orig_mask, orig_drop = opt.compress_mask, opt.compress_drop

    def spy_mask(info, verbose=False):
        masked.append((old_name[id(info['var_old'])], info['var_new'], info['mask'].detach().cpu().clone().bool(),
                       tuple(info['var_old'].shape)))
        return orig_mask(info, verbose=verbose)

    def spy_drop(info, verbose=False):
        dropped.append(info['var_old'])
        return orig_drop(info, verbose=verbose)
    opt.compress_mask, opt.compress_drop = spy_mask, spy_drop

    class F(dict):
        __getattr__ = dict.__getitem__
    config.FLAGS.bind(F(image_size=64, use_distributed=False))
    wrapper = torch.nn.Module()
    wrapper.module = model
    T.shrink_model(wrapper, ema, opt, pinfo, 1e-3, ema_only=False)
    del opt.compress_mask, opt.compress_drop
    ts.mgr.ensure()
    torch.cuda.synchronize()
    assert masked and dropped
    params = opt.param_groups[0]['params']
    assert set(id(p) for p in params) == set(id(p) for p in model.parameters())
    assert len(params) == n_before - len(dropped)
    # re-keyed variables are appended, in the order they were re-keyed
    assert [id(p) for p in params[-len(masked):]] == [id(v) for _, v, _, _ in masked]
    shrunk = 0
    for oname, var_new, mask, old_shape in masked:
        new_shape = tuple(var_new.shape)
        if new_shape == old_shape:
            want = old_buf[oname]
        elif new_shape[0] != old_shape[0]:
            want = old_buf[oname][mask]
            shrunk += 1
        else:
            want = old_buf[oname][:, mask]
            shrunk += 1
        assert set(opt.state[var_new].keys()) == {'momentum_buffer'}
        assert torch.equal(opt.state[var_new]['momentum_buffer'].cpu(), want), oname
    assert shrunk > 0
    touched = {id(v) for _, v, _, _ in masked}
    for n, p in model.named_parameters():   # parameters the shrink did not touch keep their buffer through the arena rebuild
        if id(p) not in touched:
            assert torch.equal(opt.state[p]['momentum_buffer'].cpu(), old_buf[old_name[id(p)]]), n
    for v in dropped:
        assert v not in opt.state and all(v is not q for q in params)
    assert ts.mgr.SQ is None
    # a third step through the rebuilt arenas, against the same reference arithmetic
    x, y = _batches(3)[2]
    ts.set_batch(x.cuda(), y.cuda())
    bufs = {n: opt.state[p]['momentum_buffer'].detach().double().cpu().clone() for n, p in model.named_parameters()}
    _step_and_check(ts, model, opt, ema, momentum, nesterov, 0.02, 3e-3, 1e-3, 'slimmable', bufs, "after shrink ")


# ------------------------------------------------------------------------------------------------- 8. checkpoint
def _given_step(model, opt, grads, lr):
    opt.zero_grad()
    for n, p in model.named_parameters():
        p.grad.copy_(grads[n].cuda())
    opt.param_groups[0]['lr'] = lr
    opt.step()
    torch.cuda.synchronize()


def _grads(model, g):
    return {n: torch.randn(p.shape, generator=g) * 0.05 for n, p in model.named_parameters()}


@pytest.mark.parametrize("momentum,nesterov", [(0.9, True), (0.9, False)])
def test_state_dict_continues_in_torch_sgd(gpu_lib, momentum, nesterov):
    model, sd, spec, pinfo, opt, ema, engine = _setup(momentum, nesterov)
    from atomnas_amd import runtime
    runtime.manager_of(model).ensure()
    g = torch.Generator().manual_seed(4)
    for step in range(2):
        _given_step(model, opt, _grads(model, g), 0.01 * (step + 1))
    state = opt.state_dict()
    names = [n for n, _ in model.named_parameters()]
    assert sorted(state['state'].keys()) == list(range(len(names)))
    assert all(set(v.keys()) == {'momentum_buffer'} for v in state['state'].values())
    cpu = [torch.nn.Parameter(p.detach().double().cpu().clone()) for p in model.parameters()]
    theirs = torch.optim.SGD(cpu, lr=1.0)
    theirs.load_state_dict(state)
    assert theirs.param_groups[0]['momentum'] == momentum and theirs.param_groups[0]['nesterov'] == nesterov
    assert theirs.param_groups[0]['lr'] == 0.02
    grads = _grads(model, g)
    for n, q in zip(names, cpu):
        q.grad = grads[n].double()
    theirs.param_groups[0]['lr'] = 0.03
    theirs.step()
    _given_step(model, opt, grads, 0.03)
    _check(model, opt, dict(zip(names, (q.detach() for q in cpu))), {n: theirs.state[q]['momentum_buffer'] for n, q in zip(names, cpu)},
           momentum)


@pytest.mark.parametrize("momentum,nesterov", [(0.9, True), (0.9, False)])
def test_torch_sgd_state_dict_continues_here(gpu_lib, momentum, nesterov):
    model, sd, spec, pinfo, opt, ema, engine = _setup(momentum, nesterov)
    from atomnas_amd import runtime
    mgr = runtime.manager_of(model)
    mgr.attach_optimizer(opt)
    opt._mgr = mgr
    mgr.ensure()
    names = [n for n, _ in model.named_parameters()]
    cpu = [torch.nn.Parameter(sd[n].clone()) for n in names]
    theirs = torch.optim.SGD(cpu, lr=0.01, momentum=momentum, nesterov=nesterov)
    g = torch.Generator().manual_seed(6)
    for step in range(2):
        grads = _grads(model, g)
        for n, q in zip(names, cpu):
            q.grad = grads[n].double()
        theirs.param_groups[0]['lr'] = 0.01 * (step + 1)
        theirs.step()
    with torch.no_grad():
        for q, p in zip(cpu, model.parameters()):
            p.copy_(q.detach().float().cuda())
    assert not mgr.dirty
    opt.load_state_dict(theirs.state_dict())
    assert mgr.dirty   # the loaded tensors are ordinary tensors: the arenas are rebuilt around them at the next use
    assert opt.param_groups[0]['lr'] == 0.02
    grads = _grads(model, g)
    for n, q in zip(names, cpu):
        q.grad = grads[n].double()
    theirs.param_groups[0]['lr'] = 0.03
    theirs.step()
    _given_step(model, opt, grads, 0.03)
    assert not mgr.dirty
    for p in model.parameters():   # the state lives in the momentum arena again
        assert opt.state[p]['momentum_buffer'].untyped_storage().data_ptr() == mgr.BUF.untyped_storage().data_ptr()
    _check(model, opt, dict(zip(names, (q.detach() for q in cpu))), {n: theirs.state[q]['momentum_buffer'] for n, q in zip(names, cpu)},
           momentum)


# ------------------------------------------------------------------------------------------------- 9. two gloo ranks on one device
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from atomnas_amd.utils import optim as aopt
        momentum, nesterov, wd = 0.9, True, 1e-3
        model, sd, spec, pinfo, opt, ema, engine = _setup(momentum, nesterov)   # same seed: same initialisation on every rank
        ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=wd, wd_method='slimmable', batch_size=6, image_size=64, use_graph=True,
                              world_size=world)
        ref_buf, summed = None, []
        for step, (x, y) in enumerate(_batches(2, seed=100 + rank)):   # every rank its own batches
            ts.set_batch(x.cuda(), y.cuda())
            ref_buf = _step_and_check(ts, model, opt, ema, momentum, nesterov, 0.02 * (step + 1), 1e-3, wd, 'slimmable', ref_buf,
                                      "rank %d step %d " % (rank, step))
            summed.append(ts.mgr.G.detach().clone())   # sum over the ranks (+ world * L1 term)
        assert ts.comm_mode == "host"
        for arena in (ts.mgr.P, ts.mgr.BUF, ts.mgr.G):
            mine = arena.detach().cpu()
            parts = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            assert all(torch.equal(q, parts[0]) for q in parts), "ranks diverged"
        lo = ts.loss[0:1].detach().cpu()
        both = [torch.zeros_like(lo) for _ in range(world)]
        dist.all_gather(both, lo)
        assert not torch.equal(both[0], both[1]), "ranks were supposed to see different batches"
        if rank == 0:
            # one process, fed the mean of the ranks' gradients (the L1 term is part of it: world * L1 / world), L2 through cal_l2_loss
            model1, _, _, _, opt1, _, _ = _setup(momentum, nesterov)
            from atomnas_amd import runtime
            mgr1 = runtime.manager_of(model1)
            mgr1.attach_optimizer(opt1)
            opt1._mgr = mgr1
            mgr1.ensure()
            assert mgr1.nP == ts.mgr.nP
            for step, gsum in enumerate(summed):
                opt1.zero_grad()
                mgr1.G.copy_(gsum / world)
                aopt.cal_l2_loss(model1, wd, 'slimmable').backward()
                opt1.param_groups[0]['lr'] = 0.02 * (step + 1)
                opt1.step()
            torch.cuda.synchronize()
            ref_p = {n: p.detach() for n, p in model1.named_parameters()}
            ref_b = {n: opt1.state[p]['momentum_buffer'] for n, p in model1.named_parameters()}
            _check(model, opt, ref_p, ref_b, momentum, "one process ")
        out[rank] = 1
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu_sgd(gpu_lib):
    world = 2
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    for p in procs:
        if p.is_alive():
            p.terminate()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert sorted(out.keys()) == list(range(world))


# ------------------------------------------------------------------------------------------------- 10. entry point
def test_train_entry_with_sgd(gpu_lib, tmp_path):
    """`python train.py app:tests/data/tiny_sgd.yml`: two epochs with the shrink and the checkpoint, then a resume from `latest`.
    (`use_distributed: False` comes from the file: on the command line the value would be cast by bool("False"), as in the
    reference's utils/config.py, and switch the process group ON.)"""
    app = "app:" + os.path.join(ROOT, "tests", "data", "tiny_sgd.yml")
    env = dict(os.environ, ATOMNAS_E2E_DIR=str(tmp_path), ARNOLD_OUTPUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), app], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert out.count(" val: ") >= 2 and "Prune threshold" in out and "Model Shrink to FLOPS" in out, out[-4000:]
    steps = re.findall(r"Epoch (\d+)/2 step (\d+) loss (\S+) l2 (\S+) l1 (\S+) lr (\S+) ", out)
    assert len(steps) == 6, out[-4000:]
    vals = [[float(v) for v in s[2:]] for s in steps]
    assert all(v == v and abs(v) != float('inf') for row in vals for v in row), vals
    assert all(row[0] > 0 and row[1] > 0 for row in vals), vals          # CE and the 'slimmable' L2 value
    ckpt = torch.load(os.path.join(str(tmp_path), "latest_checkpoint.pt"), map_location="cpu", weights_only=False)
    st = ckpt['optimizer']['state']
    assert ckpt['last_epoch'] == 1 and len(st) == len(ckpt['optimizer_param_names']) > 0
    assert all(set(v.keys()) == {'momentum_buffer'} for v in st.values())
    assert any(float(v['momentum_buffer'].abs().max()) > 0 for v in st.values())
    g0 = ckpt['optimizer']['param_groups'][0]
    assert g0['momentum'] == 0.9 and g0['nesterov'] is True and g0['weight_decay'] == 0
    # what the resume does with it (train.py load_checkpoint), in this process: the buffers come back, by name
    sys.path.insert(0, ROOT)
    import common as mc
    import train as T
    from atomnas_amd.utils import config
    from atomnas_amd.utils import optim as aopt
    from atomnas_amd.utils.sgd import SGD
    os.environ.update(ATOMNAS_E2E_DIR=str(tmp_path), ARNOLD_OUTPUT=str(tmp_path))
    os.environ.setdefault("DATA_LMDB", "/tmp/none")
    flags = config.load_app([app])
    mc.setup_distributed(T.NUM_IMAGENET_TRAIN)
    model, wrapper = mc.get_model()
    ema = mc.setup_ema(model)
    opt = aopt.get_optimizer(wrapper, flags)
    assert type(opt) is SGD
    last_epoch, _ = T.load_checkpoint(ckpt, wrapper, opt, ema)
    assert last_epoch == 1
    from atomnas_amd import runtime
    mgr = runtime.manager_of(model)
    mgr.attach_optimizer(opt)
    mgr.ensure()     # materialise: the loaded state moves into the momentum arena
    assert mgr.SQ is None and mgr.BUF is not None
    table = dict(wrapper.named_parameters())
    for i, n in enumerate(ckpt['optimizer_param_names']):
        buf = opt.state[table[n]]['momentum_buffer']
        assert buf.untyped_storage().data_ptr() == mgr.BUF.untyped_storage().data_ptr() and torch.equal(buf.cpu(), st[i]['momentum_buffer']), n
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), app, "--resume", str(tmp_path), "--num_epochs", "3"],
                        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out2 = r2.stdout + r2.stderr
    assert r2.returncode == 0, out2[-4000:]
    assert "Epoch 2/3" in out2 and "Epoch 0/3" not in out2 and "Epoch 1/3" not in out2, out2[-3000:]
    ckpt2 = torch.load(os.path.join(str(tmp_path), "latest_checkpoint.pt"), map_location="cpu", weights_only=False)
    assert ckpt2['last_epoch'] == 2
    assert all(set(v.keys()) == {'momentum_buffer'} for v in ckpt2['optimizer']['state'].values())
