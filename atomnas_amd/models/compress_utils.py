"""Dynamic network shrinkage with the reference's protocol (models/compress_utils.py).

`copmress_inverted_residual_channels(m, masks, ema=, optimizer=, prune_info=, prefix=)` (the misspelling is the reference's
public name) rebuilds a block from per-branch alive masks: new (smaller) branch modules are built, and for every tensor an
`info` dict {var_old_name, var_old, type, mask, module_class, var_new_name, var_new, mask_hook} is handed to the optimizer,
the EMA and the PruneInfo in the reference's order (shared pw_bn -> kept branches -> dropped branches) before the module is
swapped.  The data movement behind `mask_hook` is the index-packed channel gather of libatomnas_hip.so
(atomnas_mask_index + atomnas_gather_dim) -- there is no host copy of the weights.  After a shrink the arenas of the owning
model are rebuilt lazily (runtime.ArenaManager.materialize) at the next forward / optimizer step.
`compress_inverted_residual_channels_fused` is the same protocol for InvertedResidualChannelsFused, which the reference cannot shrink.
"""
import functools
import itertools
import warnings

import torch
from torch import nn

from .. import ops
from ..utils.common import add_prefix


class _build_on(object):
    """Builds replacement modules directly on the device, without running their initialisers: every parameter and buffer of a rebuilt
    branch is overwritten by the shrink's gathers / copies (the reference builds on the host, initialises, then moves: ~630 small
    host-to-device copies and as many random initialisations per shrink of the supernet, for values that are thrown away)."""

    def __init__(self, device):
        self.dev = torch.device(device)

    def __enter__(self):
        self.ctx = self.dev
        self.ctx.__enter__()   # first: if the device context cannot be entered nothing has been patched yet
        self.saved = (nn.Conv2d.reset_parameters, nn.modules.batchnorm._NormBase.reset_parameters)
        nn.Conv2d.reset_parameters = lambda self_: None
        nn.modules.batchnorm._NormBase.reset_parameters = lambda self_: None
        return self

    def __exit__(self, *exc):
        nn.Conv2d.reset_parameters, nn.modules.batchnorm._NormBase.reset_parameters = self.saved
        self.ctx.__exit__(*exc)
        return False


def _mask_along_dim(lhs, rhs, mask, dim=0):
    """lhs <- rhs[mask] (dim 0) / rhs[:, mask] (dim 1), on device."""
    if dim not in (0, 1):
        raise NotImplementedError()
    if lhs.numel() == 0:
        return
    ops.gather_by_mask(lhs.data, rhs.data, mask, dim)


def _copy(lhs, rhs, *args):
    lhs.data.copy_(rhs.data)


def _scatter_by_bool(items, flags, pad=None):
    it = iter(items)
    out = [next(it) if f else pad for f in flags]
    assert next(it, None) is None
    return out


def build_default_info(m_new, m_old, mask, attr, mask_hook, var_type='variable', prefix_new=None, prefix_old=None):
    assert var_type in ('variable', 'buffer')
    info = {'var_old_name': add_prefix(attr, prefix_old), 'var_old': getattr(m_old, attr), 'type': var_type, 'mask': mask,
            'module_class': type(m_old)}
    if m_new is not None:
        info.update({'var_new_name': add_prefix(attr, prefix_new), 'var_new': getattr(m_new, attr), 'mask_hook': mask_hook})
    return info


def compress_conv(m_new, m_old, mask, dim, prefix_new=None, prefix_old=None, gather=_mask_along_dim):
    assert m_new is None or isinstance(m_new, nn.Conv2d)
    assert isinstance(m_old, nn.Conv2d) and dim in (0, 1)
    mk = functools.partial(build_default_info, m_new, m_old, mask, prefix_new=prefix_new, prefix_old=prefix_old)
    infos = [mk('weight', functools.partial(gather, dim=dim))]
    if m_old.bias is not None:
        infos.append(mk('bias', gather if dim == 0 else _copy))
    return infos


def compress_bn(m_new, m_old, mask, prefix_new=None, prefix_old=None, gather=_mask_along_dim):
    assert m_new is None or isinstance(m_new, nn.BatchNorm2d)
    assert isinstance(m_old, nn.BatchNorm2d)
    assert m_new is None or m_new.affine == m_old.affine
    infos = []
    if m_old.affine:
        mk = functools.partial(build_default_info, m_new, m_old, mask, prefix_new=prefix_new, prefix_old=prefix_old)
        infos += [mk('weight', gather), mk('bias', gather)]
    if m_old.track_running_stats:
        mkb = functools.partial(build_default_info, m_new, m_old, mask, var_type='buffer', prefix_new=prefix_new, prefix_old=prefix_old)
        infos += [mkb('running_var', gather), mkb('running_mean', gather), mkb('num_batches_tracked', _copy)]
    return infos


def adjust_bn(m_new, m_old, post_hook_params, **kwargs):
    """The shared pw_bn keeps every channel; the reference attaches (and then disables) a running-mean correction."""
    mask = torch.ones_like(m_new.weight, dtype=torch.bool)
    if ops.gather_deferring():
        ops.register_mask(mask, None, mask.numel())   # every channel kept: a strided copy in the shrink's job table, no index
    infos = compress_bn(m_new, m_old, mask, **kwargs)
    for info in infos:
        if 'running_mean' in info['var_old_name']:
            info['post_hook_params'] = post_hook_params
            info['post_hook'] = None  # models/compress_utils.py:201-204: warns and skips the adjustment
    return infos


def compress_conv_bn_relu(m_new, m_old, mask, prefix_new=None, prefix_old=None, dim=0, gather=_mask_along_dim):
    from . import mobilenet_base as mb
    assert m_new is None or isinstance(m_new, mb.ConvBNReLU)
    assert isinstance(m_old, mb.ConvBNReLU)
    old = list(m_old.children())
    new = [None] * len(old) if m_new is None else list(m_new.children())
    return (compress_conv(new[0], old[0], mask, dim=dim, prefix_new='{}.0'.format(prefix_new), prefix_old='{}.0'.format(prefix_old),
                          gather=gather) +
            compress_bn(new[1], old[1], mask, prefix_new='{}.1'.format(prefix_new), prefix_old='{}.1'.format(prefix_old), gather=gather))


def _protocol(ema, optimizer, prune_info, verbose):
    """(update, clean) of one block's shrink: what happens to a kept / a dropped tensor in the optimizer, the EMA and the PruneInfo."""
    def is_prunable_bn_var(info):
        return prune_info is not None and issubclass(info['module_class'], nn.BatchNorm2d) and info['type'] == 'variable'

    def update(infos):
        for info in infos:
            if optimizer is not None and info['type'] != 'buffer':
                optimizer.compress_mask(info, verbose=verbose)
            if ema is not None and 'num_batches_tracked' not in info['var_old_name']:
                ema.compress_mask(info, verbose=verbose)
            if is_prunable_bn_var(info) and prune_info.compress_check_exist(info):
                prune_info.compress_mask(info, verbose=verbose)
            info['mask_hook'](info['var_new'], info['var_old'], info['mask'])
            if 'post_hook' in info:
                warnings.warn('Do not adjust bn mean!!!')

    def clean(infos):
        for info in infos:
            if optimizer is not None and info['type'] != 'buffer':
                optimizer.compress_drop(info, verbose=verbose)
            if ema is not None and 'num_batches_tracked' not in info['var_old_name']:
                ema.compress_drop(info, verbose=verbose)
            if is_prunable_bn_var(info) and prune_info.compress_check_exist(info):
                prune_info.compress_drop(info, verbose=verbose)

    return update, clean


def _swap_done(m):
    """the structure changed: the arenas of the owning model are rebuilt at the next use"""
    pl = getattr(m, '_plan', None)
    if pl is not None and getattr(pl, 'mgr', None) is not None:
        pl.mgr.mark_dirty()
    object.__setattr__(m, '_plan', None)


def copmress_inverted_residual_channels(m, masks, ema=None, optimizer=None, prune_info=None, prefix=None, verbose=False):
    update, clean = _protocol(ema, optimizer, prune_info, verbose)
    assert len(m.kernel_sizes) == len(masks)
    device = m.pw_bn.weight.device
    hidden = [ops.mask_count(mask) for mask in masks]   # from the shrink's one mask launch when it registered them, else mask.sum().item()
    keeps = [h > 0 for h in hidden]
    m.channels, m.kernel_sizes = [list(itertools.compress(x, keeps)) for x in (hidden, m.kernel_sizes)]
    with _build_on(device):
        new_ops, new_pw_bn = m._build(m.channels, m.kernel_sizes, m.expand)
    for mod in list(new_ops.modules()) + [new_pw_bn]:   # train / eval state follows the block
        mod.training = m.training
    idx_depth, idx_proj = (1, 2) if m.expand else (0, 1)
    new_padded = _scatter_by_bool(list(new_ops), keeps)
    new_idx_padded = _scatter_by_bool(list(range(len(new_ops))), keeps)

    keep_infos, drop_infos = [], []
    for new_op, new_i, old_op, old_i, mask in zip(new_padded, new_idx_padded, m.ops, range(len(m.ops)), masks):
        old_ch = list(old_op.children())
        new_ch = [None] * len(old_ch) if new_op is None else list(new_op.children())
        bucket = drop_infos if new_op is None else keep_infos
        if m.expand:
            bucket.append(compress_conv_bn_relu(new_ch[0], old_ch[0], mask, add_prefix('ops.{}.0'.format(new_i), prefix),
                                                add_prefix('ops.{}.0'.format(old_i), prefix)))
        bucket.append(compress_conv_bn_relu(new_ch[idx_depth], old_ch[idx_depth], mask,
                                            add_prefix('ops.{}.{}'.format(new_i, idx_depth), prefix),
                                            add_prefix('ops.{}.{}'.format(old_i, idx_depth), prefix)))
        bucket.append(compress_conv(new_ch[idx_proj], old_ch[idx_proj], mask, dim=1,
                                    prefix_new=add_prefix('ops.{}.{}'.format(new_i, idx_proj), prefix),
                                    prefix_old=add_prefix('ops.{}.{}'.format(old_i, idx_proj), prefix)))
    name_pw = add_prefix('pw_bn', prefix)
    pw_infos = adjust_bn(new_pw_bn, m.pw_bn, None, prefix_new=name_pw, prefix_old=name_pw)

    if ema is not None:
        ema.compress_start()
    if prune_info is not None:
        prune_info.compress_start()
    update(pw_infos)           # must come first for the EMA bookkeeping (reference note)
    for infos in keep_infos:
        update(infos)
    for infos in drop_infos:   # dropped branches last
        clean(infos)

    del m.ops
    del m.pw_bn
    m.ops, m.pw_bn = new_ops, new_pw_bn
    _swap_done(m)


def _mask_segments(lhs, rhs, segs, dim=0):
    """The fused block's concatenated mask (the per-branch masks in branch order) as one gather per kept branch slice, on views:
    lhs[new_start : new_start + kept] <- rhs[start : start + hidden][mask] along `dim` for every segment of `segs`."""
    if dim not in (0, 1):
        raise NotImplementedError()
    for mask, start, hidden, new_start, kept in segs:
        ops.gather_by_mask(lhs.data.narrow(dim, new_start, kept), rhs.data.narrow(dim, start, hidden), mask, dim)


def compress_inverted_residual_channels_fused(m, masks, ema=None, optimizer=None, prune_info=None, prefix=None, verbose=False):
    """The shrink of an expanding InvertedResidualChannelsFused, with the protocol of the plain block.  Its expand conv, SE gate and
    projection span all hidden channels: they are gathered with the concatenated mask (_mask_segments); the depthwise branches with their
    own.  A branch without a live atom is dropped and the remaining ones renumbered; a block without a live atom becomes the identity and
    every tensor of it is dropped."""
    from . import mobilenet_base as mb
    if not m.expand:
        raise RuntimeError('Not search_first')
    update, clean = _protocol(ema, optimizer, prune_info, verbose)
    assert len(m.kernel_sizes) == len(masks) == len(m.depth_ops)
    old_project = m.project_conv
    device = old_project[0].weight.device
    old_hidden = list(m.channels)
    hidden = [ops.mask_count(mask) for mask in masks]
    keeps = [h > 0 for h in hidden]
    segs, start, new_start = [], 0, 0
    for mask, h_old, h_new in zip(masks, old_hidden, hidden):
        assert mask.numel() == h_old
        if h_new > 0:
            segs.append((mask, start, h_old, new_start, h_new))
        start += h_old
        new_start += h_new
    m.channels, m.kernel_sizes = [list(itertools.compress(x, keeps)) for x in (hidden, m.kernel_sizes)]
    with _build_on(device):
        new_expand, new_depth, new_project, new_se = m._build(m.channels, m.kernel_sizes, m.expand, m.se_ratio)
    for top in (new_expand, new_depth, new_project, new_se):   # train / eval state follows the block
        for mod in top.modules():
            mod.training = m.training
    alive = len(new_depth) > 0
    has_se = isinstance(m.se_op, mb.SqueezeAndExcitation)
    name = functools.partial(add_prefix, prefix=prefix)

    # tensors over all hidden channels: the concatenated mask; None for the new module when the block dies
    wide = functools.partial(dict, gather=_mask_segments)
    shared = compress_conv_bn_relu(new_expand if alive else None, m.expand_conv, segs, name('expand_conv'), name('expand_conv'), **wide())
    if has_se:
        new_r, new_e = (new_se.se_reduce, new_se.se_expand) if alive else (None, None)
        shared += compress_conv(new_r, m.se_op.se_reduce, segs, dim=1, prefix_new=name('se_op.se_reduce'),
                                prefix_old=name('se_op.se_reduce'), **wide())
        shared += compress_conv(new_e, m.se_op.se_expand, segs, dim=0, prefix_new=name('se_op.se_expand'),
                                prefix_old=name('se_op.se_expand'), **wide())
    shared += compress_conv(new_project[0] if alive else None, old_project[0], segs, dim=1, prefix_new=name('project_conv.0'),
                            prefix_old=name('project_conv.0'), **wide())
    name_bn = name('project_conv.1')
    if alive:
        out_bn_infos = adjust_bn(new_project[1], old_project[1], None, prefix_new=name_bn, prefix_old=name_bn)
    else:
        out_bn_infos = compress_bn(None, old_project[1], None, prefix_new=name_bn, prefix_old=name_bn)

    keep_infos, drop_infos = [], []
    new_padded = _scatter_by_bool(list(new_depth), keeps)
    new_idx_padded = _scatter_by_bool(list(range(len(new_depth))), keeps)
    for new_op, new_i, old_op, old_i, mask in zip(new_padded, new_idx_padded, m.depth_ops, range(len(m.depth_ops)), masks):
        old_cbr = list(old_op.children())[1]
        new_cbr = None if new_op is None else list(new_op.children())[1]
        (drop_infos if new_op is None else keep_infos).append(
            compress_conv_bn_relu(new_cbr, old_cbr, mask, name('depth_ops.{}.1'.format(new_i)), name('depth_ops.{}.1'.format(old_i))))

    if ema is not None:
        ema.compress_start()
    if prune_info is not None:
        prune_info.compress_start()
    if alive:
        update(out_bn_infos)       # the tensors that keep their names first, as the plain block's pw_bn
        update(shared)
        for infos in keep_infos:   # ascending: a renumbered branch only ever takes the name of a dropped or already moved one
            update(infos)
    else:
        clean(out_bn_infos)
        clean(shared)
    for infos in drop_infos:       # dropped branches last
        clean(infos)

    del m.expand_conv, m.depth_ops, m.project_conv, m.se_op
    m.expand_conv, m.depth_ops, m.project_conv, m.se_op = new_expand, new_depth, new_project, new_se
    _swap_done(m)
