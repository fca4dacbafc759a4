"""Host side of a resumed run (no GPU): the loaders' shuffle follows the epoch of the run, not the number of passes of the process;
train.resume_run puts the schedules where the uninterrupted loop has them when `max_steps_per_epoch` shortens the epochs; a checkpoint
without the keys this project adds still resumes.  The device side is tests/test_resume_gpu.py."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TINY = dict(num_classes=10, input_size=64, input_channel=16, last_channel=64, width_mult=1.0, dropout_ratio=0.2,
            batch_norm_momentum=0.01, batch_norm_epsilon=1e-3, active_fn="nn.ReLU",
            inverted_residual_setting=[[1, 8, 1, 1, [3]], [6, 16, 2, 1, [3, 5]]])


# ---------------------------------------------------------------------------------------------------------------- loader order
class _Samples(object):
    """a dataset whose sample i is (i, box, flip, i): the batches spell the index order"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i, (0, 0, 1, 1), False, i


def _passes(loader, k):
    return [[b[3].tolist() for b in loader] for _ in range(k)]


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("world", [1, 2])
def test_decoded_loader_set_epoch(world, drop_last):
    """set_epoch(k): the next pass is pass k of a fresh loader and the passes after it count on; without it the passes are numbered
    from the construction (seed + 0, seed + 1, ...), which is written out here with torch.randperm.  Wall time: milliseconds."""
    from atomnas_amd.utils.dataflow import DecodedLoader
    n, bs, seed = 23, 4, 5   # 23: no multiple of the batch nor of the world, so the wrap-around and the short batch are there
    for rank in range(world):
        mk = lambda: DecodedLoader(_Samples(n), bs, True, rank=rank, world=world, drop_last=drop_last, seed=seed)
        fresh = _passes(mk(), 4)
        per_rank = (n + world - 1) // world
        for k, got in enumerate(fresh):   # today's order, stated independently of the loader
            idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed + k)).tolist()
            idx = (idx + idx[:per_rank * world - n])[rank:per_rank * world:world]
            want = [idx[i:i + bs] for i in range(0, per_rank, bs)]
            if drop_last and len(want[-1]) < bs:
                want.pop()
            assert got == want, (rank, k)
        assert fresh[0] != fresh[1] and fresh[1] != fresh[2]
        for k in (2, 0, 3):
            ld = mk()
            _passes(ld, 1)   # a pass already made must not matter
            ld.set_epoch(k)
            assert _passes(ld, 1)[0] == fresh[k], (rank, k)
            if k < 3:
                assert _passes(ld, 1)[0] == fresh[k + 1], (rank, k)
        ld = DecodedLoader(_Samples(n), bs, False, rank=rank, world=world, drop_last=drop_last, seed=seed)
        first = _passes(ld, 1)[0]
        ld.set_epoch(3)
        assert _passes(ld, 1)[0] == first   # no shuffle: every epoch the index order


@pytest.mark.parametrize("world", [1, 2])
def test_resident_loader_set_epoch(world):
    """ResidentLoader's index logic needs no device (the upload happens when a pass is iterated): set_epoch(k) gives the index list of
    pass k of a fresh loader; on one rank that is DecodedLoader's order.  Wall time: milliseconds."""
    from atomnas_amd.utils.dataflow import DecodedLoader
    from atomnas_amd.utils.image_store import ResidentLoader, ResidentStore
    n, bs, seed = 23, 4, 5
    for rank in range(world):
        res = ResidentStore(_Samples(n), rank, world, seed)
        assert res.pool is None
        mk = lambda: ResidentLoader(res, bs, True, False, seed)
        ld = mk()
        fresh = []
        for k in range(4):   # what __iter__ does around the upload: take the list, count the pass
            fresh.append(ld._indices())
            ld.epoch += 1
        assert fresh[0] != fresh[1] and all(sorted(f) == sorted(res.share) for f in fresh)
        for k in (2, 0, 3):
            ld = mk()
            ld.epoch += 1
            ld.set_epoch(k)
            assert ld._indices() == fresh[k]
        if world == 1:
            host = DecodedLoader(_Samples(n), bs, True, seed=seed)
            host.set_epoch(2)
            assert [i for b in _passes(host, 1)[0] for i in b] == fresh[2]
        assert res.pool is None


def test_train_sets_the_epoch_of_the_train_and_calibration_loaders():
    """train.py's epoch loop calls set_epoch(epoch) on LOADERS[0] and LOADERS[1] before it draws a batch (read from the source: the
    loop itself needs a GPU; tests/test_resume_gpu.py runs it).  Wall time: milliseconds."""
    import inspect
    import train as T
    src = inspect.getsource(T.train_val_test)
    loop = src[src.index("for epoch in range(last_epoch + 1"):]
    assert "LOADERS[:2]" in loop and "loader.set_epoch(epoch)" in loop
    assert loop.index("loader.set_epoch(epoch)") < loop.index("device_batches(LOADERS[0]")


# ---------------------------------------------------------------------------------------------------------------- scheduler
def _flags(**kw):
    from atomnas_amd.utils import config
    F = config.AttrDict(dict(
        image_size=64, use_distributed=False, per_gpu_batch_size=8, batch_size=8, grad_accum_steps=1, num_epochs=6,
        optimizer="rmsprop", alpha=0.9, momentum=0.9, epsilon=1e-3, eps_inside_sqrt=True, nesterov=True,
        lr=0.02, base_lr=0.01, epoch_warmup=1, lr_scheduler="exp_decaying", lr_stepwise=False, exp_decaying_lr_gamma=0.9,
        exp_decay_epoch_interval=1, moving_average_decay=0.99, moving_average_decay_adjust=False,
        prune_params=dict(method="network_slimming", bn_prune_filter="expansion_only_skip_expand1", rho=1e-3, epoch_free=0, epoch_warmup=3,
                          scheduler="linear", stepwise=True),
        _steps_per_epoch=5, max_steps_per_epoch=3, _global_step=0))
    F.update(kw)
    config.FLAGS.bind(F)
    return F


def _objects(F, seed):
    import common as mc
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import model_profiling as mp, optim, prune
    torch.manual_seed(seed)
    model = ms.Model(**TINY)
    for p in model.parameters():
        torch.nn.init.normal_(p, std=0.1)
    wrapper = mc._SingleProcessWrapper(model)
    ema = mc.setup_ema(model)
    optimizer = optim.get_optimizer(wrapper, F)
    sched = optim.get_lr_scheduler(optimizer, F)
    mp.model_profiling(model, 64, 64, verbose=False)
    F._bn_to_prune = prune.get_bn_to_prune(model, F.prune_params, verbose=False)
    return model, wrapper, ema, optimizer, sched


def _loop(F, optimizer, sched, epochs):
    """the bookkeeping of train.py's loop, without the device step -> [(global step, lr the step used)]"""
    import warnings
    import train as T
    seen = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # torch: scheduler.step() before optimizer.step() -- there is no device step here
        for _ in range(epochs):
            for _ in range(T.optimizer_steps_per_epoch()):
                seen.append((F._global_step, optimizer.param_groups[0]["lr"]))
                sched.step()
                F._global_step += 1
    return seen


NEW_KEYS = ("global_step", "dropout_counter", "prune_penalty")


@pytest.mark.parametrize("old_format", [False, True])
@pytest.mark.parametrize("sched_kw", [dict(lr_scheduler="exp_decaying", lr_stepwise=False),
                                      dict(lr_scheduler="linear_decaying", lr_stepwise=True)], ids=["exp_decaying_warmup", "linear_decaying"])
def test_resume_run_restores_the_schedules_under_max_steps_per_epoch(sched_kw, old_format):
    """Epochs shortened to 3 of the schedule's 5 steps.  The uninterrupted loop reaches global step 6 after two epochs; a run resumed from
    the checkpoint of epoch 1 must stand there too -- last_epoch of the scheduler, FLAGS._global_step, the learning rate of every later
    step -- with our checkpoint and with one that lacks the additional keys (the reference's format), which derives the step from
    max_steps_per_epoch.  The parent commit resumed at (last_epoch + 1) * _steps_per_epoch = 10.  Wall time: 0.1 s."""
    import train as T
    from atomnas_amd import runtime
    F = _flags(**sched_kw)
    model, wrapper, ema, optimizer, sched = _objects(F, 1)
    head = _loop(F, optimizer, sched, 2)
    assert [g for g, _ in head] == list(range(6)) and F._global_step == 6 and sched.last_epoch == 6
    ckpt = T.checkpoint_state(wrapper, optimizer, ema, 1, 1.0, {"top1_error": 0.5})
    assert ckpt["global_step"] == 6 and ckpt["dropout_counter"] == 0 and ckpt["last_epoch"] == 1 and ckpt["meters"] == (None, None)
    tail = _loop(F, optimizer, sched, 2)
    lrs = [lr for _, lr in head + tail]
    assert len(set(lrs)) > 4   # the schedule moves: warm-up then decay

    if old_format:
        for k in NEW_KEYS + ("optimizer_param_names",):
            del ckpt[k]
    F2 = _flags(**sched_kw)
    model2, wrapper2, ema2, optimizer2, sched2 = _objects(F2, 2)
    last_epoch, best_val = T.resume_run(ckpt, wrapper2, optimizer2, ema2, sched2, F2._bn_to_prune)
    assert (last_epoch, best_val) == (1, 0.5)
    assert sched2.last_epoch == 6 and F2._global_step == 6
    assert optimizer2.param_groups[0]["lr"] == tail[0][1]
    assert _loop(F2, optimizer2, sched2, 2) == tail
    for (k, a), (_, b) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert torch.equal(a, b), k
    # written: the counter of the checkpoint (no step ran here); derived: one draw per step of the 6
    assert runtime.manager_of(model2)._counter_start == (6 if old_format else 0)


def test_old_checkpoint_derives_the_dropout_counter_from_the_micro_batches():
    """a checkpoint without `dropout_counter` and `global_step`: the counter is global step x grad_accum_steps (one draw per
    micro-batch), here 2 epochs x 3 steps x 2; tests/golden/checkpoint_ref.pt, which the reference wrote, has none of the additional keys
    and loads through the same path (tests/test_configs_gpu.py steps it).  Wall time: 0.1 s."""
    import train as T
    from atomnas_amd import runtime
    F = _flags(grad_accum_steps=2)
    model, wrapper, ema, optimizer, sched = _objects(F, 1)
    ckpt = T.checkpoint_state(wrapper, optimizer, ema, 1, 1.0, {"top1_error": 0.5})
    for k in NEW_KEYS:
        del ckpt[k]
    F2 = _flags(grad_accum_steps=2)
    model2, wrapper2, ema2, optimizer2, sched2 = _objects(F2, 2)
    T.resume_run(ckpt, wrapper2, optimizer2, ema2, sched2, F2._bn_to_prune)
    assert F2._global_step == 6 and runtime.manager_of(model2)._counter_start == 12
    ref = torch.load(os.path.join(ROOT, "tests", "golden", "checkpoint_ref.pt"), weights_only=False)["checkpoint"]
    assert not any(k in ref for k in NEW_KEYS + ("optimizer_param_names",))


def test_prune_table_order_and_penalties_travel_with_the_checkpoint():
    """The penalties are normalised over the atoms of the network get_bn_to_prune walks, and a shrink re-inserts re-keyed names: a
    table rebuilt from a shrunk network has other values in another order.  load_penalty_state puts back both, and refuses a table
    over other gammas.  Wall time: milliseconds."""
    from atomnas_amd.utils.prune import PruneInfo
    a = PruneInfo(["x", "y", "z"], [1.0, 2.0, 3.0])
    a.add_info_list("per_channel_flops", [10, 20, 30])
    a._info["y2"] = a._info.pop("y")   # re-keyed by a shrink: now last
    state = a.penalty_state()
    assert state == [["x", 1.0], ["z", 3.0], ["y2", 2.0]]
    b = PruneInfo(["x", "y2", "z"], [0.5, 0.25, 0.125])
    b.add_info_list("per_channel_flops", [10, 20, 30])
    b.load_penalty_state(state)
    assert b.weight == ["x", "z", "y2"] and b.penalty == [1.0, 3.0, 2.0] and b.get_info_list("per_channel_flops") == [10, 30, 20]
    with pytest.raises(ValueError, match="other BatchNorm weights"):
        PruneInfo(["x", "y", "z"], [1, 1, 1]).load_penalty_state(state)
