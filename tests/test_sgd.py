"""Host side of the fused SGD optimizer (atomnas_amd/utils/sgd.py), no GPU: the factory, the constructor's checks, the
state_dict() format against the installed torch.optim.SGD and the `linear_decaying` schedule it goes with
(utils/optim.py:252-332 of the reference)."""
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params():
    torch.manual_seed(3)
    return [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]


def test_get_optimizer_builds_the_fused_sgd():
    from atomnas_amd.utils import optim
    from atomnas_amd.utils.sgd import SGD
    model = torch.nn.Linear(3, 2)
    flags = types.SimpleNamespace(optimizer='sgd', lr=0.25, momentum=0.9, nesterov=True)
    opt = optim.get_optimizer(model, flags)
    assert type(opt) is SGD
    g = opt.param_groups[0]
    assert g['lr'] == 0.25 and g['momentum'] == 0.9 and g['nesterov'] is True and g['weight_decay'] == 0 and g['dampening'] == 0
    assert [id(p) for p in g['params']] == [id(p) for p in model.parameters()]
    flags = types.SimpleNamespace(optimizer='sgd', lr=0.5, momentum=0.0, nesterov=False)
    g = optim.get_optimizer(model, flags).param_groups[0]
    assert g['lr'] == 0.5 and g['momentum'] == 0.0 and g['nesterov'] is False


def test_constructor_checks_and_no_cpu_fallback():
    from atomnas_amd._lib import AtomnasHipError
    from atomnas_amd.utils.rmsprop import RMSprop
    from atomnas_amd.utils.sgd import SGD
    for kw in (dict(lr=-0.1), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-4), dict(lr=0.1, nesterov=True),
               dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            torch.optim.SGD(_params(), **kw)   # torch's own checks ...
        with pytest.raises(ValueError):
            SGD(_params(), **kw)               # ... are this class's
    with pytest.raises(NotImplementedError):
        SGD(_params(), lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(NotImplementedError):
        SGD(_params(), lr=0.1, weight_decay=1e-4)
    a, b = _params()
    with pytest.raises(NotImplementedError):
        SGD([dict(params=[a]), dict(params=[b], lr=0.2)], lr=0.1)
    for opt in (SGD(_params(), lr=0.1, momentum=0.9, nesterov=True), RMSprop(_params(), lr=0.1)):
        for p in opt.param_groups[0]['params']:
            p.grad = torch.ones_like(p)
        with pytest.raises(AtomnasHipError):
            opt.step()   # host tensors: there is no CPU arithmetic to fall back to


@pytest.mark.parametrize("kw", [dict(lr=0.1, momentum=0.9, nesterov=True), dict(lr=0.05, momentum=0.8), dict(lr=0.2)])
def test_state_dict_round_trips_with_torch_sgd(kw):
    from atomnas_amd.utils.sgd import SGD
    params = _params()
    ours, theirs = SGD(params, **kw), torch.optim.SGD(params, lr=1.0)
    sd = ours.state_dict()
    assert sd['state'] == {}
    theirs.load_state_dict(sd)
    ref = torch.optim.SGD(params, **kw)
    assert theirs.param_groups[0].keys() == ref.param_groups[0].keys() == ours.param_groups[0].keys()
    for k, v in ref.param_groups[0].items():
        if k != 'params':
            assert theirs.param_groups[0][k] == v and ours.param_groups[0][k] == v, k
    assert sd['param_groups'][0].keys() == ref.state_dict()['param_groups'][0].keys()
    # ... one torch step on CPU (momentum buffers appear), and back
    for p in params:
        p.grad = torch.full_like(p, 0.5)
    theirs.step()
    back = SGD(params, lr=1.0)
    back.load_state_dict(theirs.state_dict())
    assert back.param_groups[0]['lr'] == kw['lr'] and back.param_groups[0]['momentum'] == kw.get('momentum', 0)
    if kw.get('momentum', 0) > 0:
        for p in params:
            assert set(back.state[p].keys()) == {'momentum_buffer'}
            assert torch.equal(back.state[p]['momentum_buffer'], theirs.state[p]['momentum_buffer'])
    else:
        assert len(back.state) == 0
    assert back.state_dict()['state'].keys() == theirs.state_dict()['state'].keys()


@pytest.mark.parametrize("lr, base_lr", [(0.4, 0.1), (0.05, 0.1)])
def test_linear_decaying_schedule_over_sgd(lr, base_lr):
    """the reference's formulas (utils/optim.py:252-306): warm-up `r + i / warmup * (1 - r)`, r = base_lr / lr, for i <= warmup when
    lr > base_lr, then `1 - i / (num_epochs * steps_per_epoch)`; scheduler.step() writes lr * multiplier into the group."""
    from atomnas_amd.utils import optim
    from atomnas_amd.utils.sgd import SGD
    steps_per_epoch, num_epochs, epoch_warmup = 7, 10, 2
    flags = types.SimpleNamespace(lr=lr, base_lr=base_lr, _steps_per_epoch=steps_per_epoch, lr_scheduler='linear_decaying',
                                  num_epochs=num_epochs)
    flags.get = lambda k, d=None: {'lr_stepwise': True, 'epoch_warmup': epoch_warmup}.get(k, d)
    opt = SGD(_params(), lr=lr, momentum=0.9, nesterov=True)
    sched = optim.get_lr_scheduler(opt, flags)
    warmup, total = epoch_warmup * steps_per_epoch, num_epochs * steps_per_epoch

    def expected(i):
        if lr > base_lr and i <= warmup:
            r = base_lr / lr
            return r + i / warmup * (1 - r)
        return 1 - i / total

    lam = sched.lr_lambdas[0]
    for i in range(total + 1):
        assert lam(i) == expected(i), i
    assert expected(total) == 0.0 and (expected(0) == base_lr / lr if lr > base_lr else expected(0) == 1.0)
    for i in range(total + 1):
        assert abs(opt.param_groups[0]['lr'] - lr * expected(i)) <= 1e-15, i
        sched.step()


def test_sgd_test_config_resolves_on_cpu(tmp_path):
    """The config of the SGD entry-point test (tests/test_sgd_gpu.py) loads without a GPU."""
    os.environ["ATOMNAS_E2E_DIR"] = str(tmp_path)
    os.environ.setdefault("ARNOLD_OUTPUT", str(tmp_path))
    os.environ.setdefault("DATA_LMDB", "/tmp/none")
    from atomnas_amd.utils import config
    # no `--use_distributed False` on the command line: an override is cast with the type of the value it replaces, and bool("False")
    # is True (the reference's utils/config.py:15-22 does the same); the file itself says False through tiny_search.yml
    flags = config.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_sgd.yml")])
    assert flags.optimizer == "sgd" and flags.momentum == 0.9 and flags.nesterov is True
    assert flags.weight_decay == 1e-4 and flags.weight_decay_method == "slimmable" and flags.lr_scheduler == "linear_decaying"
    assert flags.num_epochs == 2 and flags.max_steps_per_epoch == 3 and flags.use_distributed is False
