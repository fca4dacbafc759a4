"""TF-flavoured RMSprop with the reference's interface (utils/rmsprop.py) as one fused launch over the parameter arena.

`RMSprop(model.parameters(), lr, alpha, momentum, eps, eps_inside_sqrt, weight_decay=0)`; `step()` reads `p.grad`
(views into the gradient arena) and updates every parameter, `square_avg` and `momentum_buffer` in a single kernel
(atomnas_fused_rmsprop_ema).
`state[p]['square_avg']` / `['momentum_buffer']` remain per-parameter tensors (arena views) so that `state_dict()` keeps the
reference's format, and `compress_mask` / `compress_drop` keep the reference's re-keying protocol for dynamic shrinkage.
"""
from .. import ops
from .arena_optimizer import ArenaOptimizer


class RMSprop(ArenaOptimizer):
    _NAME = 'RMSprop'
    _LOG_NAME = 'RMSProp'
    _STATE_ARENAS = (('square_avg', 'SQ'), ('momentum_buffer', 'BUF', lambda group: group['momentum'] > 0))
    _WITH_STEP = True
    needs_square_avg = True

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, eps_inside_sqrt=False, weight_decay=0, momentum=0, centered=False):
        for label, v in (('learning rate', lr), ('epsilon value', eps), ('momentum value', momentum),
                         ('weight_decay value', weight_decay), ('alpha value', alpha)):
            if not 0.0 <= v:
                raise ValueError('Invalid {}: {}'.format(label, v))
        if centered:
            raise NotImplementedError('centered RMSprop is not on the AtomNAS hot path')
        if weight_decay != 0:
            raise NotImplementedError('weight decay enters through cal_l2_loss (utils/optim.py), as in the reference configs')
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, eps_inside_sqrt=eps_inside_sqrt, centered=centered,
                        weight_decay=weight_decay)
        super().__init__(params, defaults)

    def launch_fused(self, mgr, ema_arena, wd_chunk, l2_value, ws, guard=None):
        """guard: the verdict vector of a guarded step (engine.TrainStep): the guarded entry is launched instead"""
        group = self.param_groups[0]
        ops.fused_rmsprop_ema(mgr.P, mgr.G, mgr.SQ, mgr.BUF if group['momentum'] > 0 else None, ema_arena, wd_chunk, mgr.nP, mgr.hyper,
                              group['alpha'], group['eps'], group['eps_inside_sqrt'], group['momentum'], l2_value=l2_value, ws=ws, guard=guard)
