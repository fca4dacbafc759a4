"""Checkpoint round trip (GPU): a run stopped after step 4 and resumed through train.checkpoint_state -> torch.save -> torch.load ->
fresh objects -> train.resume_run computes, bit for bit, what the uninterrupted run computes in steps 5 - 7.

The steps are bit-reproducible (tests/test_determinism_gpu.py), so every comparison is torch.equal: any difference is state the
checkpoint or the resume path loses.  What the parent commit lost: the dropout / stochastic-depth counter (back to 0 at every arena
rebuild, i.e. after every shrink and every resume), the global step under max_steps_per_epoch (tests/test_resume_host.py), and the
prune table of a shrunk run (penalties normalised over the atoms of the supernet the run started from; a table rebuilt from the
exported network has other penalties, in another order).

The loop below is train.py's inner loop on counter-filled batches that are a function of the micro-batch index; FLAGS._steps_per_epoch
is 2, so the learning rate (warm-up, then decay per epoch), rho (linear warm-up over 3 epochs) and the EMA warm-up all move over the 7 steps.
"""
import collections
import io
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kutil import counter_fill, randomize  # noqa: E402
from test_block_gpu import TINY  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH, SIZE, STEPS, STOP, SHRINK_AT = 8, 64, 7, 4, 2
THR = 1e-3

CASES = collections.OrderedDict([
    ("rmsprop_bf16_graph", dict()),
    ("rmsprop_f32_eager", dict(flags=dict(compute_dtype="f32"), use_graph=False)),
    ("sgd_nesterov", dict(flags=dict(optimizer="sgd", nesterov=True, weight_decay=1e-4, weight_decay_method="slimmable",
                                     lr_scheduler="linear_decaying", lr_stepwise=True))),
    ("shrunk", dict(shrink=True)),
    ("drop_connect", dict(shrink=True, se=True)),
    ("accum2", dict(flags=dict(grad_accum_steps=2, batch_size=2 * BATCH))),
    # the averaged gradient of this network has a norm of 10 ... 13 in every one of the 7 steps (printed by the test): 0.5 clips them
    ("guarded", dict(flags=dict(grad_clip_norm=0.5, skip_nonfinite_steps=True))),
])


def _flags(case):
    from atomnas_amd.utils import config
    F = config.AttrDict(dict(
        image_size=SIZE, use_distributed=False, per_gpu_batch_size=BATCH, batch_size=BATCH, grad_accum_steps=1, num_epochs=6,
        optimizer="rmsprop", alpha=0.9, momentum=0.9, epsilon=1e-3, eps_inside_sqrt=True,
        weight_decay=1e-4, weight_decay_method="mnas", label_smoothing=0.1,
        lr=0.02, base_lr=0.01, epoch_warmup=1, lr_scheduler="exp_decaying", lr_stepwise=False, exp_decaying_lr_gamma=0.9,
        exp_decay_epoch_interval=1, moving_average_decay=0.99, moving_average_decay_adjust=False,
        prune_params=dict(method="network_slimming", bn_prune_filter="expansion_only_skip_expand1", rho=1e-3, epoch_free=0, epoch_warmup=3,
                          scheduler="linear", stepwise=True),
        _steps_per_epoch=2, _global_step=0))
    F.update(CASES[case].get("flags", {}))
    config.FLAGS.bind(F)
    return F


def _model_kw(case):
    """TINY of tests/test_block_gpu.py with dropout 0.2; `se`: the fused SE supernet of tests/data/tiny_search_se.yml with stochastic depth"""
    if not CASES[case].get("se"):
        return dict(TINY, dropout_ratio=0.2)
    from atomnas_amd.utils import config
    bound = config.FLAGS._target   # load_app installs what it reads as FLAGS: put the run's own back
    keep = {k: os.environ.get(k) for k in ("ARNOLD_OUTPUT", "ATOMNAS_E2E_DIR")}
    os.environ.update(ARNOLD_OUTPUT="unused", ATOMNAS_E2E_DIR="unused")
    try:
        kw = dict(config.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_search_se.yml")]).model_kwparams)
    finally:
        config.FLAGS.bind(bound)
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k)
            else:
                os.environ[k] = v
    kw.update(input_size=SIZE, dropout_ratio=0.2, drop_connect_rate=0.5)
    return kw


_BATCHES = {}


def _batch(i):
    """micro-batch i of every run, on the device (built once)"""
    if i not in _BATCHES:
        x = (counter_fill(torch.empty(BATCH, 3, SIZE, SIZE), 1000 + i) * 4).float()
        _BATCHES[i] = (x.cuda(), ((torch.arange(BATCH) * 3 + i) % 10).cuda())
    return _BATCHES[i]


class _Run(object):
    """model, optimizer, EMA, scheduler, prune table and TrainStep as train.train_val_test builds them, and its inner loop"""

    def __init__(self, case, model, F):
        import common as mc
        from atomnas_amd.utils import model_profiling as mp, optim, prune
        self.case, self.F, self.model = case, F, model
        if F.get("compute_dtype", "bf16") == "f32":
            model.set_compute_dtype(torch.float32)
        model.cuda()
        self.wrapper = mc._SingleProcessWrapper(model)
        self.ema = mc.setup_ema(model)
        self.optimizer = optim.get_optimizer(self.wrapper, F)
        self.sched = optim.get_lr_scheduler(self.optimizer, F)
        mp.model_profiling(model, SIZE, SIZE, verbose=False)
        F._bn_to_prune = prune.get_bn_to_prune(model, F.prune_params, verbose=False)
        self.rho = prune.get_rho_scheduler(F.prune_params, F._steps_per_epoch)
        self.log, self.counters, self.guard = [], [], []

    def train_step(self):
        import common as mc
        from atomnas_amd import engine
        F = self.F
        clip_norm, skip_nonfinite = mc.guard_options()
        self.step = engine.TrainStep(self.model, self.optimizer, self.ema, F._bn_to_prune, weight_decay=F.weight_decay,
                                     wd_method=F.weight_decay_method, label_smoothing=F.label_smoothing,
                                     batch_size=F.per_gpu_batch_size, image_size=F.image_size, world_size=1, allreduce_bn=False,
                                     accum_steps=mc.grad_accum_steps(), clip_norm=clip_norm, skip_nonfinite=skip_nonfinite,
                                     **({"use_graph": False} if CASES[self.case].get("use_graph") is False else {}))
        self.model.train()

    def steps(self, first, last):
        F, step, accum = self.F, self.step, self.step.accum_steps
        for i in range(first, last):
            if CASES[self.case].get("shrink") and i == SHRINK_AT:
                self.shrink()
            for mb in range(accum):
                step.set_batch(*_batch(i * accum + mb))
                if step.pending < accum - 1:
                    step.accumulate()
                    continue
                step.global_step = F._global_step
                lr, rho = self.optimizer.param_groups[0]["lr"], self.rho(F._global_step)
                step.step(lr=lr, rho=rho)
                self.sched.step()
                F._global_step += 1
            self.log.append((step.loss.clone(), lr, rho))
            self.counters.append(int(step.mgr.step_counter))
            if step.guarded:
                self.guard.append(step.guard_state())
        step.reset_accumulation()

    def shrink(self):
        """tests/test_configs_gpu.py::test_cfg3_atomnas_a_forced_dead_atoms_shrink on three blocks: gamma and its shadow 0 on all but 1 and 3
        atoms of two branches of one block, on a whole branch of another, on a seeded third of a third block; then train.shrink_model"""
        import train as T
        blocks = [(n, b) for n, b in self.model.get_named_block_list().items() if b.expand]
        g = torch.Generator().manual_seed(11)
        # (expanding block: {branch: atoms kept} or None for the seeded third); `se`: 4 searched blocks, the third is the residual one
        few, whole, third = (2, 1, 3) if CASES[self.case].get("se") else (1, 3, 5)
        plan = {few: {0: 1, 1: 3}, whole: {1: 0}, third: None}
        with torch.no_grad():
            for bi, spec in plan.items():
                name, b = blocks[bi]
                for i, (bn_name, bn) in enumerate(b.get_named_depthwise_bn(prefix=name).items()):
                    n = bn.weight.numel()
                    if spec is None:
                        dead = torch.rand(n, generator=g) < 1.0 / 3.0
                    elif i in spec:
                        dead = torch.ones(n, dtype=torch.bool)
                        dead[torch.randperm(n, generator=g)[:spec[i]]] = False
                    else:
                        continue
                    bn.weight[dead.cuda()] = 0.0
                    self.ema.average(bn_name + ".weight")[dead.cuda()] = 0.0
        before = [list(b.channels) for _, b in blocks]
        T.shrink_model(self.wrapper, self.ema, self.optimizer, self.F._bn_to_prune, THR, ema_only=False)
        after = [list(b.channels) for _, b in blocks]
        assert after[few][:2] == [1, 3] and len(after[whole]) == len(before[whole]) - 1 and sum(after[third]) < sum(before[third]), (before, after)
        if CASES[self.case].get("se"):
            assert blocks[few][1].use_res_connect and blocks[few][1].drop_connect_rate > 0   # the block that drops its branch per image

    def state(self):
        torch.cuda.synchronize()
        pname = {id(p): n for n, p in self.model.named_parameters()}
        opt = {pname[id(p)]: {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st.items()} for p, st in self.optimizer.state.items()}
        return dict(sd=collections.OrderedDict((k, v.detach().clone()) for k, v in self.model.state_dict().items()), opt=opt,
                    lr=self.optimizer.param_groups[0]["lr"],
                    shadow={n: self.ema.average(n).detach().clone() for n in self.ema.average_names()},
                    info={n: dict(v) for n, v in self.ema._info.items()}, log=list(self.log), counters=list(self.counters),
                    global_step=self.F._global_step, last_epoch=self.sched.last_epoch)


def _fresh_model(case, seed):
    from atomnas_amd.models import mobilenet_supernet as ms
    model = ms.Model(**_model_kw(case))
    randomize(model, seed)
    return model


def _run_a(case):
    run = _Run(case, _fresh_model(case, 5), _flags(case))
    run.train_step()
    run.steps(0, STEPS)
    return run


def _run_b(case, counter=None):
    """4 steps, checkpoint through a file image, everything built anew (another initialisation: the checkpoint must bring every value),
    resume_run, 3 steps.  counter: overrides the restored dropout counter (the negative control)."""
    import train as T
    from atomnas_amd import runtime
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.models import searched_network as sn
    head = _Run(case, _fresh_model(case, 5), _flags(case))
    head.train_step()
    head.steps(0, STOP)
    state = T.checkpoint_state(head.wrapper, head.optimizer, head.ema, STOP // head.F._steps_per_epoch - 1, 1.0, {"top1_error": 0.5})
    buf = io.BytesIO()
    torch.save(state, buf)
    ckpt = torch.load(io.BytesIO(buf.getvalue()), map_location="cpu", weights_only=False)
    if CASES[case].get("shrink"):
        kw = _model_kw(case)
        model = sn.Model(**mb.output_network(head.model), input_size=SIZE, batch_norm_momentum=kw["batch_norm_momentum"],
                         batch_norm_epsilon=kw["batch_norm_epsilon"], dropout_ratio=kw["dropout_ratio"],
                         drop_connect_rate=kw.get("drop_connect_rate", 0.0))
        randomize(model, 6)
        # re-keyed variables are appended to the optimizer's list (utils/arena_optimizer.py compress_mask): the name map is needed
        assert ckpt["optimizer_param_names"] != [n for n, _ in head.wrapper.named_parameters()]
        assert sorted(ckpt["optimizer_param_names"]) == sorted(n for n, _ in head.wrapper.named_parameters())
    else:
        model = _fresh_model(case, 6)
    del head
    tail = _Run(case, model, _flags(case))
    last_epoch, best_val = T.resume_run(ckpt, tail.wrapper, tail.optimizer, tail.ema, tail.sched, tail.F._bn_to_prune)
    assert (last_epoch, best_val) == (STOP // 2 - 1, 0.5)
    if counter is not None:
        runtime.manager_of(model).set_step_counter(counter)
    tail.train_step()
    tail.steps(STOP, STEPS)
    return tail, ckpt


_A = {}


def _a_state(case):
    """the uninterrupted run of a case, computed once and never modified"""
    if case not in _A:
        run = _run_a(case)
        _A[case] = (run.state(), run)
    return _A[case]


def _differences(a, b):
    """everything that differs between the final states of two runs (steps 5 - 7 of the logs): the scalars first, then tensor names"""
    bad = []
    if a["counters"][STOP:] != b["counters"]:
        bad.append("dropout counters %r %r" % (a["counters"][STOP:], b["counters"]))
    for key in ("global_step", "last_epoch", "lr"):
        if a[key] != b[key]:
            bad.append("%s %r %r" % (key, a[key], b[key]))
    for i, ((la, lra, ra), (lb, lrb, rb)) in enumerate(zip(a["log"][STOP:], b["log"])):
        if not torch.equal(la, lb) or lra != lrb or ra != rb:
            bad.append("step %d: loss %s lr %r rho %r | loss %s lr %r rho %r" % (STOP + i + 1, la.tolist(), lra, ra, lb.tolist(), lrb, rb))
    if list(a["sd"]) != list(b["sd"]):
        bad.append("state_dict keys")
    if set(a["opt"]) != set(b["opt"]):
        bad.append("optimizer state names")
    if set(a["shadow"]) != set(b["shadow"]):
        bad.append("EMA names")
    bad += ["ema info %s %r %r" % (n, a["info"][n], b["info"].get(n)) for n in a["info"] if a["info"][n] != b["info"].get(n)]
    bad += ["sd " + k for k in a["sd"] if k in b["sd"] and not torch.equal(a["sd"][k], b["sd"][k])]
    for n in a["opt"]:
        for k, v in a["opt"][n].items():
            w = b["opt"].get(n, {}).get(k)
            if not (torch.equal(v, w) if torch.is_tensor(v) and torch.is_tensor(w) else v == w):
                bad.append("opt %s %s" % (n, k))
    bad += ["ema " + n for n in a["shadow"] if n in b["shadow"] and not torch.equal(a["shadow"][n], b["shadow"][n])]
    return bad


@pytest.mark.parametrize("case", list(CASES))
def test_resumed_run_equals_the_uninterrupted_run(gpu_lib, case):
    """Run A: 7 steps.  Run B: 4 steps, checkpoint, fresh objects, resume, 3 steps.  torch.equal on every state_dict entry
    (num_batches_tracked included), the optimizer state by parameter name and its lr, every EMA shadow and _info counter, and the loss
    triple, lr and rho of steps 5 - 7.  The shrunk cases drop atoms before step 3 and rebuild run B from the exported architecture
    through models.searched_network.  Wall time of one case: 0.2 - 0.4 s on an MI355X, 2.3 s for the
    first case of a process (two short runs and their graph captures).

    With the parent commit's behaviour put back one defect at a time (a zero counter at every materialisation and nothing restored on
    resume; no prune table in the checkpoint): `rmsprop_bf16_graph` fails with 796 differing entries, the first `dropout counters [5, 6, 7]
    [1, 2, 3]`, then the loss of step 5 and every parameter, statistic, optimizer state and EMA shadow; `shrunk` fails on run A alone, `assert [1, 2, 1, 2, 3, 4, ...] == [1, 2, 3, 4, 5, 6,
    ...]: At index 2 diff: 1 != 3`; `shrunk` without the prune table fails with 759 differing entries."""
    a, run_a = _a_state(case)
    accum = run_a.step.accum_steps
    # the counter is the number of micro-batches drawn so far -- also after the rebuild that follows the shrink, not 0 again
    assert a["counters"] == [accum * (i + 1) for i in range(STEPS)], a["counters"]
    lrs, rhos = [l[1] for l in a["log"]], [l[2] for l in a["log"]]
    assert len(set(lrs[STOP:])) > 1 and len(set(rhos[STOP - 1:])) > 1, (lrs, rhos)   # the schedules move across the resumed steps
    assert all(bool(torch.isfinite(l[0]).all()) and float(l[0][0]) > 0 for l in a["log"])
    assert all(float(l[0][2]) > 0 for l in a["log"][1:])   # the L1 term is live from the second step on
    if case == "guarded":
        print("gradient norms", [g["norm"] for g in run_a.guard])
    b, ckpt = _run_b(case)
    assert ckpt["dropout_counter"] == accum * STOP and ckpt["global_step"] == STOP
    bs = b.state()
    if case == "guarded":
        # at least one of steps 5 - 7 was clipped, in both runs.  The cumulative skipped / clipped counters are per-process log
        # values (run B starts them at 0) and are not part of the comparison; norm and coefficient of every step are
        assert b.guard[-1]["clipped"] >= 1 and run_a.guard[-1]["clipped"] - run_a.guard[STOP - 1]["clipped"] == b.guard[-1]["clipped"]
        for ga, gb in zip(run_a.guard[STOP:], b.guard):
            assert (ga["norm"], ga["coef"], ga["ok"]) == (gb["norm"], gb["coef"], gb["ok"]), (ga, gb)
        assert any(g["coef"] < 1.0 for g in b.guard)
    bad = _differences(a, bs)
    assert not bad, (len(bad), bad[:8])


def test_a_resume_that_loses_the_dropout_counter_is_seen(gpu_lib):
    """Negative control: run B with the counter left at 0 (what the parent commit did) must differ from run A -- in the loss of the
    first resumed step already, since it draws another dropout mask.  Wall time: 0.2 s (run A is shared with the case above)."""
    case = "rmsprop_bf16_graph"
    a, _ = _a_state(case)
    b, _ = _run_b(case, counter=0)
    bad = _differences(a, b.state())
    assert any(d.startswith("step %d" % (STOP + 1)) for d in bad) and any(d.startswith("sd ") for d in bad), bad[:12]
    assert any(d.startswith("dropout counters") for d in bad)


def _tail_mask(model, counter, xy):
    """the classifier-dropout keep mask [N, features] of a training forward of `model` at a counter value"""
    from atomnas_amd import functional as AF
    from atomnas_amd import runtime
    mgr = runtime.manager_of(model)
    mgr.ensure()
    keep = int(mgr.step_counter)
    mgr.step_counter.fill_(counter)
    AF.TAIL_TAP = []
    try:
        with torch.no_grad():
            model(xy[0])
        mask = AF.TAIL_TAP[-1].clone()
    finally:
        AF.TAIL_TAP = None
        mgr.step_counter.fill_(keep)
    return mask


def test_the_first_step_after_a_shrink_draws_a_new_dropout_mask(gpu_lib):
    """The counter value the first step after the shrink ran with (run A of `shrunk`: its counter after that step, minus one) against
    the counter of step 0, in two tail launches on the same batch: p = 0.2 over 8 x 64 features, so equal masks mean equal counters.
    The parent commit rebuilt the counter at 0 with the arenas: the two launches were the same launch.  Wall time: 0.1 s (run A is shared with the `shrunk` case)."""
    a, run = _a_state("shrunk")
    used = a["counters"][SHRINK_AT] - 1
    assert used == SHRINK_AT, (used, a["counters"])
    model = _fresh_model("shrunk", 5).cuda().train()
    m0, m1 = _tail_mask(model, 0, _batch(0)), _tail_mask(model, used, _batch(0))
    assert m0.shape == (BATCH, 64) and 0.6 < float(m0.float().mean()) < 0.95
    assert torch.equal(m0, _tail_mask(model, 0, _batch(0)))
    assert not torch.equal(m0, m1)
