"""What every fused arena optimizer shares: finding the arena manager of its parameters, keeping per-parameter state tensors as
views into the optimizer arenas (so that `state_dict()` keeps torch's format), the step()/launch() pair and the reference's re-keying
protocol for dynamic shrinkage (utils/rmsprop.py:134-182).  A subclass supplies its arithmetic as one fused launch:

    _NAME            how the class is called in messages
    _STATE_ARENAS    ((state key, manager attribute), ...) in the order the state is created; a key whose `needs` callable (third
                     entry, optional, taking the parameter group) is false is left out
    launch_fused(mgr, ema_arena, wd_chunk, l2_value, ws)   the kernel call (capturable: reads lr / EMA decay / 1/world from mgr.hyper)
"""
import logging

import torch
from torch.optim.optimizer import Optimizer

from .. import ops
from .common import check_tensor_in, index_tensor_in


class ArenaOptimizer(Optimizer):
    _NAME = 'ArenaOptimizer'
    _LOG_NAME = 'ArenaOptimizer'
    _STATE_ARENAS = ()
    _WITH_STEP = False        # state[p]['step'] (what the reference's RMSprop keeps; torch.optim.SGD has none)
    needs_square_avg = False  # runtime.ArenaManager allocates the SQ arena only for an optimizer that says so

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise NotImplementedError('one parameter group (the reference never uses more)')
        self._mgr = None
        self._steps = 0

    # ---- arena plumbing
    def _manager(self):
        params = self.param_groups[0]['params']
        mgr = None
        for p in params:
            m = getattr(p, '_atomnas_mgr', None)
            if m is not None:
                mgr = m
                break
        if mgr is None:
            raise ops._lib.AtomnasHipError(
                '{}.step needs arena-backed parameters: run the model on the GPU once (or call '
                'atomnas_amd.runtime.manager_of(model).ensure()) before the first step; there is no CPU fallback'.format(self._NAME))
        if self._mgr is not mgr:
            self._mgr = mgr
            mgr.attach_optimizer(self)
        mgr.ensure()
        return mgr

    def _on_materialize(self, mgr):
        """Called by the arena manager after (re)building arenas: make sure every parameter has its state views."""
        group = self.param_groups[0]
        keys = [(k, a) for k, a, *needs in self._STATE_ARENAS if not needs or needs[0](group)]
        for p in group['params']:
            off = getattr(p, '_atomnas_off', None)
            if off is None or getattr(p, '_atomnas_mgr', None) is not mgr:
                raise RuntimeError('optimizer holds a parameter that is not part of the model arena')
            if not keys:
                continue   # a stateless optimizer keeps `state` empty, as torch's does
            st = self.state[p]
            shape, strides = tuple(p.shape), (tuple(p.stride()) if not p.is_contiguous() else None)
            if keys[0][0] not in st:
                if self._WITH_STEP:
                    st['step'] = self._steps
                for key, arena in keys:
                    st[key] = _view(getattr(mgr, arena), off, shape, strides)

    def load_state_dict(self, state_dict):
        """torch's index-ordered format (what utils/common.py:123-137 saves).  The loaded state tensors are ordinary tensors; they
        move into the optimizer arenas at the next materialisation."""
        super().load_state_dict(state_dict)
        if self._mgr is not None:
            self._mgr.mark_dirty()

    def zero_grad(self, set_to_none=False):
        """Gradients live in one arena: a single memset (the kernels accumulate into it during backward)."""
        mgr = self._mgr or self._manager()
        mgr.ensure()
        mgr.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        mgr = self._manager()
        group = self.param_groups[0]
        mgr.hyper_host[ops.HYP_LR] = float(group['lr'])
        mgr.push_hyper()
        self.launch(mgr)
        self._steps += 1
        return loss

    def launch(self, mgr):
        """The device part of step(): capturable into a hipGraph (reads lr / EMA decay from mgr.hyper)."""
        self.launch_fused(mgr, None, None, None, None)

    def launch_fused(self, mgr, ema_arena, wd_chunk, l2_value, ws):
        """The optimizer tail of engine.TrainStep: the update of every parameter and its state on g * hyper[GRAD_SCALE] + wd * p, the
        EMA of the parameters (ema_arena) and the value of the L2 regulariser (l2_value, through the workspace ws) in one launch."""
        raise NotImplementedError

    # ---- dynamic shrinkage protocol (utils/rmsprop.py:134-182)
    def compress_mask(self, info, verbose=False):
        var_old, var_new, mask_hook, mask = info['var_old'], info['var_new'], info['mask_hook'], info['mask']
        if verbose:
            logging.info('{} compress: {} -> {}'.format(self._LOG_NAME, info['var_old_name'], info['var_new_name']))
        for group in self.param_groups:
            index = index_tensor_in(var_old, group['params'], raise_error=False)
            if index is None:
                continue
            if check_tensor_in(var_old, self.state):
                state = self.state.pop(var_old)
                if len(state) != 0:
                    new_state = {'step': state['step']} if 'step' in state else {}
                    for key in ('square_avg', 'momentum_buffer', 'grad_avg'):
                        if key in state:
                            new_state[key] = torch.zeros_like(var_new.data, device=var_old.device)
                            mask_hook(new_state[key], state[key], mask)
                    self.state[var_new] = new_state
            del group['params'][index]
            group['params'].append(var_new)  # appended, as in the reference: optimizer order != model order after a shrink
            if self._mgr is not None:
                self._mgr.mark_dirty()
            return
        raise AssertionError('Var: {} not in {}'.format(info['var_old_name'], self._LOG_NAME))

    def compress_drop(self, info, verbose=False):
        var_old = info['var_old']
        if verbose:
            logging.info('{} drop: {}'.format(self._LOG_NAME, info['var_old_name']))
        assert info['type'] == 'variable'
        for group in self.param_groups:
            index = index_tensor_in(var_old, group['params'], raise_error=False)
            if index is None:
                continue
            if check_tensor_in(var_old, self.state):
                self.state.pop(var_old)
            del group['params'][index]
            if self._mgr is not None:
                self._mgr.mark_dirty()
            return
        raise AssertionError('Var: {} not in {}'.format(info['var_old_name'], self._LOG_NAME))


def _view(arena, off, shape, strides):
    if strides is None:
        n = 1
        for s in shape:
            n *= s
        return arena[off:off + n].view(shape)
    return torch.as_strided(arena, shape, strides, off)
