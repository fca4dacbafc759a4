"""Knowledge distillation in the training step on the GPU (engine.TrainStep(teacher=, distill_alpha=, distill_temperature=)): with alpha = 0
it is the step without a teacher bit for bit; the gradient of the combined objective matches float64 autograd of the oracle's student
forward with the reference loss (tests/distill_ref.py) on the teacher logits the kernels produced; eager launches and graph replay
agree bit for bit; accumulated steps report the mean over their micro-batches and run the teacher on each micro-batch's own images; a
dropped guarded step and a shrink of the student leave the teacher untouched; misuse is a ValueError before any device work.

Student and TrainStep: the ones of tests/test_grad_accum_gpu.py (input 64, batch 8, 10 classes, RMSprop + EMA + prune info).  The teacher
is another tiny network with its own initialisation, non-trivial running statistics and a dropout layer (which eval mode must ignore)."""
import collections
import copy
import os
import sys

import pytest
import torch

import distill_ref as D
from test_grad_accum_gpu import ROOT, STATE, _accum_step, _batch, _make, _state

pytestmark = pytest.mark.gpu
LR, RHO = 0.003, 1e-4


def _teacher(num_classes=10, seed=99, dtype=None):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.models import mobilenet_supernet as ms
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    t = ms.Model(num_classes=num_classes, input_size=64, input_channel=16, last_channel=96, dropout_ratio=0.2, batch_norm_momentum=0.01,
                 batch_norm_epsilon=1e-3, active_fn="nn.ReLU",
                 inverted_residual_setting=[[1, 8, 1, 1, [3]], [6, 16, 1, 2, [3, 5]], [6, 24, 2, 2, [3]], [6, 32, 1, 2, [5]], [6, 40, 1, 2, [3, 7]]])
    t.apply(mb.init_weights_mnas)
    with torch.no_grad():
        for n, b in t.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(torch.randn(b.shape) * 0.1)
            elif n.endswith("running_var"):
                b.copy_(torch.rand(b.shape) * 0.5 + 0.75)
        t.classifier[1].weight.mul_(8.0)   # logits of order one: a soft target that is not uniform
    torch.random.set_rng_state(state)
    if dtype is not None:
        t.set_compute_dtype(dtype)
    return t.cuda()


def _all(ts):
    st = _state(ts)
    st["G"], st["loss"], st["topk"] = ts.mgr.G.detach().clone(), ts.loss.detach().clone(), ts.topk.detach().clone()
    return st


def _same(a, b, what=""):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))


def _teacher_state(t):
    from atomnas_amd import runtime
    torch.cuda.synchronize()
    mgr = runtime.manager_of(t)
    st = {k: v.detach().clone() for k, v in t.state_dict().items()}
    st["<step counter>"] = mgr.step_counter.detach().clone()
    st["<CNT>"] = mgr.CNT.detach().clone()
    return st


# ------------------------------------------------------------------------------------------------------------------ 1. alpha = 0
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_alpha_zero_is_the_step_without_a_teacher(gpu_lib, use_graph):
    a, b = _make(1, use_graph, teacher=_teacher(), distill_alpha=0.0, distill_temperature=2.0), _make(1, use_graph)
    for i in range(3):
        x, y = _batch(100 + i)
        for ts in (a, b):
            ts.set_batch(x, y)
            ts.step(lr=LR, rho=RHO)
    _same(_all(a), _all(b), "alpha = 0")
    assert torch.equal(a.loss_vec, b.loss_vec)
    assert float(a.kd) > 0 and bool(torch.isfinite(a.kd_vec).all())   # the soft term is still reported
    # the twin owns nothing of the feature
    assert b.teacher is None and b.kd is None and b.kd_vec is None and b.teacher_logits is None and b._teacher_out is None


# ------------------------------------------------------------------------------------------------------------------ 2. gradient
def test_gradient_matches_autograd_of_the_reference_loss(gpu_lib):
    """fp32 storage, alpha = 0.5, T = 2, a differently initialised teacher: loss, kd and the gradient arena after one step against
    float64 autograd of oracle.model_forward + distill_ref's loss on the teacher logits the kernels left in ts.teacher_logits.  Bounds:
    those of tests/test_train_step_gpu.py::test_train_steps_match_oracle (loss 2e-5 relative, gradients 1e-4 in relative L2)."""
    from test_train_step_gpu import _setup, orc
    model, sd, spec, pinfo, opt, ema, engine = _setup(torch.float32)
    teacher = _teacher(dtype=torch.float32)
    N, alpha, T = 6, 0.5, 2.0
    ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=1e-3, label_smoothing=0.1, batch_size=N, image_size=64, use_graph=False,
                          teacher=teacher, distill_alpha=alpha, distill_temperature=T)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, 3, 64, 64, generator=g)
    y = torch.randint(0, 10, (N,), generator=g)
    ts.set_batch(x.cuda(), y.cuda())
    ts.step(lr=0.002, rho=0.0)   # rho 0: the arena holds the data gradient alone
    torch.cuda.synchronize()
    tl = ts.teacher_logits.double().cpu()
    assert bool(torch.isfinite(tl).all()) and float(tl.std()) > 1e-2
    work = {}
    params = collections.OrderedDict()
    for k, v in sd.items():
        if v.is_floating_point() and "running_" not in k:
            params[k] = v.detach().clone().requires_grad_(True)
            work[k] = params[k]
        else:
            work[k] = v
    logits = orc.model_forward(x.double(), work, spec, True, {})
    ce = orc.ce_label_smooth(logits, y, 0.1)
    kd = D.kd_term(logits, tl, T)
    loss = ((1 - alpha) * ce + alpha * kd).mean()
    loss.backward()
    loss, kd = loss.detach(), kd.detach()
    got_loss, got_kd = float(ts.loss[0]), float(ts.kd)
    print("distill step: loss %.7f (ref %.7f) kd %.7f (ref %.7f)" % (got_loss, float(loss), got_kd, float(kd.mean())))
    assert abs(got_loss - float(loss)) < 2e-5 * max(1, abs(float(loss)))
    assert abs(got_kd - float(kd.mean())) < 2e-5 * max(1, abs(float(kd.mean())))
    assert float(kd.mean()) > 1e-3, "the soft term is trivial on these inputs"
    num = den = 0.0
    for n, p in model.named_parameters():
        r = params[n].grad
        dd = p.grad.double().cpu() - r
        num += float((dd * dd).sum())
        den += float((r * r).sum())
    print("distill step: gradient relative L2 error %.3g" % ((num / den) ** 0.5))
    assert (num / den) ** 0.5 < 1e-4, (num / den) ** 0.5
    # and the soft term does reach the gradient: the CE gradient alone is far from it
    for p in params.values():
        p.grad = None
    orc.ce_label_smooth(orc.model_forward(x.double(), work, spec, True, {}), y, 0.1).mean().backward()
    far = sum(float(((p.grad.double().cpu() - params[n].grad) ** 2).sum()) for n, p in model.named_parameters())
    assert (far / den) ** 0.5 > 1e-2


# ------------------------------------------------------------------------------------------------------------------ 3. eager == graph
def test_eager_and_captured_steps_are_bit_identical(gpu_lib):
    a = _make(1, False, teacher=_teacher(), distill_alpha=0.5, distill_temperature=2.0)
    b = _make(1, True, teacher=_teacher(), distill_alpha=0.5, distill_temperature=2.0)
    for i in range(3):
        x, y = _batch(100 + i)
        for ts in (a, b):
            ts.set_batch(x, y)
            ts.step(lr=LR, rho=RHO)
    _same(_all(a), _all(b), "eager against graph")
    assert torch.equal(a.kd, b.kd) and torch.equal(a.kd_vec, b.kd_vec) and torch.equal(a.teacher_logits, b.teacher_logits)
    assert torch.equal(a.loss_vec, b.loss_vec) and float(a.kd) > 0
    assert b.g_fwd_bwd is not None and a.g_fwd_bwd is None
    # and the soft term changes the training: a twin without a teacher has moved elsewhere
    c = _make(1, True)
    for i in range(3):
        c.set_batch(*_batch(100 + i))
        c.step(lr=LR, rho=RHO)
    assert not torch.equal(c.mgr.P, b.mgr.P)


# ------------------------------------------------------------------------------------------------------------------ 4. accumulation
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_accumulated_step_reports_the_mean_over_its_micro_batches(gpu_lib, use_graph):
    kw = dict(teacher=None, distill_alpha=0.5, distill_temperature=2.0)
    ts = _make(2, use_graph, **dict(kw, teacher=_teacher()))
    one = _make(1, use_graph, **dict(kw, teacher=_teacher()))
    batches = [_batch(100), _batch(101)]
    # the single-batch twin at lr 0, rho 0 stays at the initial parameters: its steps give each micro-batch's own figures
    per = []
    for x, y in batches:
        one.set_batch(x, y)
        one.step(lr=0.0, rho=0.0)
        torch.cuda.synchronize()
        per.append((one.kd.clone(), one.loss[0:1].clone(), one.teacher_logits.clone(), one.kd_vec.clone()))
    assert not torch.equal(per[0][2], per[1][2])
    ts.set_batch(*batches[0])
    ts.accumulate()
    torch.cuda.synchronize()
    assert torch.equal(ts.teacher_logits, per[0][2]) and torch.equal(ts.kd_vec, per[0][3])
    ts.set_batch(*batches[1])
    ts.step(lr=LR, rho=RHO)
    torch.cuda.synchronize()
    assert torch.equal(ts.teacher_logits, per[1][2]) and torch.equal(ts.kd_vec, per[1][3])
    half = torch.tensor(0.5, device="cuda")
    assert torch.equal(ts.kd, (per[0][0] + per[1][0]) * half), (ts.kd, per[0][0], per[1][0])
    assert torch.equal(ts.loss[0:1], (per[0][1] + per[1][1]) * half)
    assert float(ts.loss[1]) > 0   # the L2 value of the optimizer tail still arrives next to them


# ------------------------------------------------------------------------------------------------------------------ 5. guarded step
def test_a_dropped_guarded_step_leaves_the_teacher_untouched(gpu_lib):
    from test_guard_step_gpu import _split_step
    teacher = _teacher()
    a = _make(1, True, skip_nonfinite=True, teacher=teacher, distill_alpha=0.5, distill_temperature=2.0)
    x, y = _batch(100)
    a.set_batch(x, y)
    a.step(lr=LR, rho=RHO)
    t0, before = _teacher_state(teacher), _state(a)
    _split_step(a, poison=a.mgr.nP // 3)
    after = _state(a)
    for k in ("P", "SQ", "BUF", "EMA", "SEMA", "S"):
        assert torch.equal(after[k], before[k]), k
    st = a.guard_state()
    assert st["ok"] is False and st["skipped"] == 1
    _same(_teacher_state(teacher), t0, "teacher after a dropped step")
    assert float(a.kd) > 0 and bool(torch.isfinite(a.kd_vec).all())
    a.step(lr=LR, rho=RHO)
    assert a.guard_state()["ok"] is True and not torch.equal(_state(a)["P"], before["P"])
    _same(_teacher_state(teacher), t0, "teacher after the clean step")


# ------------------------------------------------------------------------------------------------------------------ 6. teacher untouched
def test_five_steps_and_a_shrink_leave_the_teacher_untouched(gpu_lib):
    """the student of tests/test_shrink_gpu.py (golden pre-shrink weights: a forced shrink removes atoms) next to a teacher: two steps, the
    shrink, three more steps.  The teacher's state_dict, counters and arena version keep their values; no tensor of it is known to the
    optimizer, the EMA, the student's modules or the student's state_dict (what a checkpoint is written from)."""
    sys.path.insert(0, ROOT)
    import train as T
    from atomnas_amd import engine, runtime
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import config, model_profiling as mp_, optim as aopt, prune as aprune, rmsprop
    g = torch.load(os.path.join(ROOT, "tests", "golden", "shrink.pt"), weights_only=False)
    model = ms.Model(**g["kw"])
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
    teacher = _teacher(num_classes=model.num_classes)
    ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=1e-5, batch_size=8, image_size=64, use_graph=True, teacher=teacher,
                          distill_alpha=0.5, distill_temperature=2.0)
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    tmgr = runtime.manager_of(teacher)
    t0, tv = _teacher_state(teacher), tmgr.version
    gen = torch.Generator().manual_seed(3)

    def step():
        x = torch.randn(8, 3, 64, 64, generator=gen).cuda()
        y = torch.randint(0, model.num_classes, (8,), generator=gen).cuda()
        ts.set_batch(x, y)
        ts.step(lr=0.002, rho=1e-4)
    step()
    step()
    v0, n0 = ts.mgr.version, ts.mgr.nP

    class F(dict):
        __getattr__ = dict.__getitem__
    config.FLAGS.bind(F(image_size=64, use_distributed=False))
    wrapper = torch.nn.Module()
    wrapper.module = model
    T.shrink_model(wrapper, ema, opt, pinfo, 1e-3, ema_only=False)
    step()
    torch.cuda.synchronize()
    assert ts.mgr.version > v0 and ts.mgr.nP < n0, "the forced shrink removed nothing"
    step()
    step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ts.mgr.P).all()) and bool(torch.isfinite(ts.loss).all()) and float(ts.kd) > 0
    _same(_teacher_state(teacher), t0, "teacher after five steps and a shrink")
    assert tmgr.version == tv and not teacher.training
    tensors = {id(p) for p in teacher.parameters()} | {id(b) for b in teacher.buffers()}
    ptrs = {p.data_ptr() for p in teacher.parameters()} | {b.data_ptr() for b in teacher.buffers()}
    assert not tensors & {id(p) for grp in opt.param_groups for p in grp["params"]}
    assert all(m is not teacher for m in model.modules())
    student_sd = wrapper.state_dict()
    assert not ptrs & {v.data_ptr() for v in student_sd.values()}
    names = set(dict(model.named_parameters())) | {n for n, _ in model.named_buffers() if "running" in n}
    assert set(ema.average_names()) == names
    assert not ptrs & {ema.average(n).data_ptr() for n in ema.average_names()}
    ckpt = {"model": student_sd, "optimizer": opt.state_dict(), "ema": ema.state_dict()}
    held = [v for v in ckpt["model"].values()] + [v for v in ckpt["ema"]["shadow"].values()]
    held += [v for s in ckpt["optimizer"]["state"].values() for v in s.values() if torch.is_tensor(v)]
    assert not ptrs & {v.data_ptr() for v in held}


# ------------------------------------------------------------------------------------------------------------------ 7. constructor
def test_constructor_refuses_misuse(gpu_lib):
    from atomnas_amd import engine
    base = _make(1, False)
    model, opt = base.model, base.optimizer
    kw = dict(batch_size=8, image_size=64, use_graph=False)
    with pytest.raises(ValueError, match="needs a teacher"):
        engine.TrainStep(model, opt, **kw, distill_alpha=0.5)
    with pytest.raises(ValueError, match="is the student"):
        engine.TrainStep(model, opt, **kw, teacher=model, distill_alpha=0.5)
    with pytest.raises(ValueError, match="classes"):
        engine.TrainStep(model, opt, **kw, teacher=_teacher(num_classes=11), distill_alpha=0.5)
    t = _teacher()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            engine.TrainStep(model, opt, **kw, teacher=t, distill_alpha=0.5, distill_temperature=bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            engine.TrainStep(model, opt, **kw, teacher=t, distill_alpha=bad)
    assert t.training   # refused before anything was done to the teacher
