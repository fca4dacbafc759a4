"""SGD with momentum / Nesterov momentum (torch.optim.SGD's arithmetic at dampening 0, what the reference builds for `optimizer: sgd`,
utils/optim.py:311-316) as one fused launch over the parameter arena.

`SGD(model.parameters(), lr, momentum, nesterov=..., weight_decay=0)`; `step()` reads `p.grad` (views into the gradient arena) and
updates every parameter and its `momentum_buffer` in a single kernel (atomnas_fused_sgd_ema).  `state[p]['momentum_buffer']` is a
per-parameter view into the momentum arena and exists only for momentum > 0, and `param_groups` carries the keys of the installed
torch.optim.SGD, so `state_dict()` and torch's load into each other.  The buffer starts at zero: momentum * 0 + g equals torch's
first-step `buf = g` only without dampening, which is therefore refused.  Arena plumbing and the shrink protocol: arena_optimizer.py.
"""
import torch

from .. import ops
from .arena_optimizer import ArenaOptimizer


class SGD(ArenaOptimizer):
    _NAME = 'SGD'
    _LOG_NAME = 'SGD'
    _STATE_ARENAS = (('momentum_buffer', 'BUF', lambda group: group['momentum'] > 0),)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        # torch's own argument checks (ValueError for negative values and for Nesterov without momentum or with dampening) and the
        # group keys of the installed build, from a throw-away instance: state_dict() then round-trips with torch.optim.SGD
        defaults = dict(torch.optim.SGD([torch.zeros(1)], lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                        nesterov=nesterov).defaults)
        if dampening != 0:
            raise NotImplementedError('dampening is not implemented (the reference uses none; the zero-initialised momentum buffer '
                                      'equals torch\'s first step only without it)')
        if weight_decay != 0:
            raise NotImplementedError('weight decay enters through cal_l2_loss (utils/optim.py), as in the reference configs')
        super().__init__(params, defaults)

    def launch_fused(self, mgr, ema_arena, wd_chunk, l2_value, ws, guard=None):
        """guard: the verdict vector of a guarded step (engine.TrainStep): the guarded entry is launched instead"""
        group = self.param_groups[0]
        ops.fused_sgd_ema(mgr.P, mgr.G, mgr.BUF if group['momentum'] > 0 else None, ema_arena, wd_chunk, mgr.nP, mgr.hyper,
                          group['momentum'], group['nesterov'], l2_value=l2_value, ws=ws, guard=guard)
