"""Glue between train.py and the hot path, with the reference's function names (common.py): model factory, forward_loss,
EMA setup / EMA-model extraction, derived batch size / learning rate / steps per epoch, MAC stamping."""
import copy
import importlib
import logging
import math

import torch

from atomnas_amd.models import mobilenet_base as mb
from atomnas_amd.utils import distributed as udist
from atomnas_amd.utils import optim
from atomnas_amd.utils.common import get_params_by_name
from atomnas_amd.utils.config import FLAGS
from atomnas_amd.utils.model_profiling import model_profiling


class Meters(object):
    """Device-side running sums (loss, top-1 / top-5 hits, samples): no per-step host synchronisation; flushed (one small
    all-reduce when distributed) every log interval -- replaces the list-backed ScalarMeters + all_gather of common.py:83-114."""

    def __init__(self, phase, device):
        self.phase = phase
        self.acc = torch.zeros(4, dtype=torch.float64, device=device)   # loss sum, top1 hits, top5 hits, samples

    def add(self, loss_vec, topk_correct):
        self.acc[0] += loss_vec.detach().double().sum()
        self.acc[1] += topk_correct[0].double()
        self.acc[2] += topk_correct[1].double()
        self.acc[3] += loss_vec.numel()

    def flush(self):
        acc = self.acc.clone()
        if FLAGS.use_distributed:
            torch.distributed.all_reduce(acc)
        self.acc.zero_()
        loss, t1, t5, n = acc.tolist()
        n = max(n, 1.0)
        return {'loss': loss / n, 'top1_error': 1.0 - t1 / n, 'top5_error': 1.0 - t5 / n}


def get_meters(phase, device='cuda'):
    return Meters(phase, device)


def get_model():
    """Model from FLAGS.model (module path, e.g. models.mobilenet_supernet) and FLAGS.model_kwparams, initialised and wrapped
    for data parallelism (common.py:127-146)."""
    model_lib = importlib.import_module(FLAGS.model)
    model = model_lib.Model(**FLAGS.model_kwparams, input_size=FLAGS.image_size)
    if FLAGS.reset_parameters:
        method = FLAGS.get('reset_param_method', None)
        if method == 'slimmable':
            model.apply(mb.init_weights_slimmable)
        elif method == 'mnas':
            model.apply(mb.init_weights_mnas)
        elif method is not None:
            raise ValueError('Unknown init method: {}'.format(method))
        logging.info('Init model by: {}'.format(method))
    if FLAGS.get('compute_dtype', 'bf16') == 'f32':
        model.set_compute_dtype(torch.float32)
    model.cuda()
    if FLAGS.use_distributed:
        wrapper = udist.AllReduceDistributedDataParallel(model)
    else:
        wrapper = _SingleProcessWrapper(model)
    return model, wrapper


class _SingleProcessWrapper(torch.nn.Module):
    """`.module` indirection without torch.nn.DataParallel (one process drives one GPU here)."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, *a, **kw):
        return self.module(*a, **kw)


def unwrap_model(model_wrapper):
    return model_wrapper.module


def setup_ema(model):
    """EMA over all parameters and BN running statistics; decay adjusted to the global batch size (common.py:42-64)."""
    if FLAGS.moving_average_decay <= 0.0:
        return None
    decay = FLAGS.moving_average_decay
    if FLAGS.moving_average_decay_adjust:
        decay = optim.ExponentialMovingAverage.adjust_momentum(decay, FLAGS.moving_average_decay_base_batch / FLAGS.batch_size)
    logging.info('Moving average for model parameters: {}'.format(decay))
    ema = optim.ExponentialMovingAverage(decay)
    for name, p in model.named_parameters():
        ema.register(name, p)
    for name, b in model.named_buffers():
        if 'running_var' in name or 'running_mean' in name:
            ema.register(name, b)
    return ema


def forward_loss(model, criterion, input, target, meter):
    """Forward + per-sample loss; top-k hits are counted on device by the criterion (common.py:67-80 does two host syncs)."""
    output = model(input)
    loss = criterion(output, target)
    if meter is not None:
        topk = getattr(criterion, 'topk_correct', None)
        if topk is None:   # plain CrossEntropyLoss in validation
            _, pred = output.topk(5)
            hit = pred.eq(target.view(-1, 1))
            topk = torch.stack([hit[:, :1].any(1).sum(), hit.any(1).sum()])
        meter.add(loss, topk)
        if getattr(criterion, 'topk_correct', None) is not None:
            criterion.topk_correct.zero_()
    return torch.mean(loss)


def get_ema_model(ema, model_wrapper):
    """A copy of the model carrying the EMA weights (common.py:155-172).  The copy materialises its own arenas; when the EMA
    shadows live in the source model's EMA arenas (they do once engine.TrainStep has run) the 799 per-name copies of the reference
    are TWO arena copies: the shadow arenas have the parameter / statistics arenas' layout by construction."""
    if ema is None:
        return model_wrapper
    from atomnas_amd import runtime
    src = unwrap_model(model_wrapper)
    clone = copy.deepcopy(src)   # modules and tensors only: plans and the arena manager are not followed (runtime.py __deepcopy__)
    clone.cuda()
    smgr = getattr(src, '_arena', None)
    cmgr = runtime.manager_of(clone)
    cmgr.ensure()
    with torch.no_grad():
        if (smgr is not None and not smgr.dirty and getattr(ema, '_mgr', None) is smgr and smgr.EMA is not None
                and cmgr.param_slots == smgr.param_slots and cmgr.buffer_slots == smgr.buffer_slots
                and set(ema.average_names()) == set(cmgr.param_slots) | set(k for k, v in cmgr.buffer_slots.items() if v[0] == 'S')):
            cmgr.P.copy_(smgr.EMA)
            cmgr.S.copy_(smgr.SEMA)
        else:
            table = dict(clone.named_parameters())
            table.update(dict(clone.named_buffers()))
            for name in ema.average_names():
                table[name].copy_(ema.average(name))
    return _SingleProcessWrapper(clone)


def profiling(model, use_cuda=True):
    logging.info('Start model profiling, use_cuda:{}.'.format(use_cuda))
    model_profiling(model, FLAGS.image_size, FLAGS.image_size, verbose=False)


def grad_accum_steps():
    """the yaml's grad_accum_steps (default 1) as a positive int; anything else is a ValueError"""
    a = FLAGS.get('grad_accum_steps', 1)
    if isinstance(a, bool) or not isinstance(a, (int, float)) or int(a) != a or int(a) < 1:
        raise ValueError('grad_accum_steps must be a positive integer, got {!r}'.format(a))
    return int(a)


def guard_options():
    """the yaml's guarded-step keys -> (clip_norm or None, skip_nonfinite): grad_clip_norm (float; absent or 0: no clipping; negative:
    ValueError) and skip_nonfinite_steps (bool, default False)"""
    c = FLAGS.get('grad_clip_norm', None)
    if c is not None and (isinstance(c, bool) or not isinstance(c, (int, float)) or not c >= 0):
        raise ValueError('grad_clip_norm must be a non-negative number (0 or absent: no clipping), got {!r}'.format(c))
    s = FLAGS.get('skip_nonfinite_steps', False)
    if not isinstance(s, bool):
        raise ValueError('skip_nonfinite_steps must be true or false, got {!r}'.format(s))
    return (float(c) if c else None), s


DISTILL_KEYS = ('model', 'model_kwparams', 'checkpoint', 'alpha', 'temperature')


def distill_options():
    """the yaml's `distill:` block -> None (absent: off) or dict(model=, model_kwparams=, checkpoint=, alpha=, temperature=).
    model defaults to the run's own `model`, alpha to 0.5, temperature to 1; keys of the form 'model_kwparams.x' override entries of
    model_kwparams, as dotted keys do at the top level of a yaml.  Unknown keys, a missing architecture, alpha outside [0, 1], a
    temperature that is not positive and finite and a class count other than the student's are ValueErrors."""
    d = FLAGS.get('distill', None)
    if d is None:
        return None
    if not isinstance(d, dict):
        raise ValueError('distill must be a mapping (model, model_kwparams, checkpoint, alpha, temperature), got {!r}'.format(d))
    d = dict(d)
    dotted = [k for k in d if isinstance(k, str) and '.' in k]
    plain = {k: v for k, v in d.items() if k not in dotted}
    unknown = sorted(str(k) for k in plain if k not in DISTILL_KEYS)
    if unknown:
        raise ValueError('unknown distill key(s) {}: the block takes {}'.format(', '.join(unknown), ', '.join(DISTILL_KEYS)))
    kw = plain.get('model_kwparams', None)
    if not isinstance(kw, dict):
        raise ValueError('distill.model_kwparams must be the teacher\'s architecture (a mapping, e.g. `!include best_model.yml`), got {!r}'
                         .format(kw))
    kw = copy.deepcopy(dict(kw))
    for k in dotted:
        parts = k.split('.')
        if parts[0] != 'model_kwparams' or len(parts) < 2:
            raise ValueError('distill override {!r}: only model_kwparams.<name> can be overridden'.format(k))
        node = kw
        for part in parts[1:-1]:
            node = node[part]
        node[parts[-1]] = d[k]
    alpha, temperature = optim.check_distill(plain.get('alpha', 0.5), plain.get('temperature', 1.0))
    classes, own = kw.get('num_classes', 1000), FLAGS.model_kwparams.get('num_classes', 1000)
    if classes != own:
        raise ValueError('the distill teacher classifies {} classes, the model {}'.format(classes, own))
    ckpt = plain.get('checkpoint', None)
    if ckpt is not None and not isinstance(ckpt, str):
        raise ValueError('distill.checkpoint must be a file name, got {!r}'.format(ckpt))
    return dict(model=plain.get('model', None) or FLAGS.model, model_kwparams=kw, checkpoint=ckpt, alpha=alpha, temperature=temperature)


def teacher_state_dict(ckpt):
    """What a teacher loads from a checkpoint file's content: the EMA weights and statistics where the file carries an EMA (they are what
    a run validates and what best_model.pt is chosen by), over the model's own entries for everything the EMA does not track
    (num_batches_tracked); a bare state_dict as it is.  Keys lose a wrapper's `module.` prefix."""
    from atomnas_amd.utils.common import unwrap_state_dict
    if not (isinstance(ckpt, dict) and 'model' in ckpt):
        return unwrap_state_dict(ckpt, verbose=False)
    sd = dict(unwrap_state_dict(ckpt['model'], verbose=False))
    ema = ckpt.get('ema')
    if ema:
        shadow = dict(ema.get('shadow') or {})
        for name, v in unwrap_state_dict(shadow, verbose=False).items():
            if name in sd:
                sd[name] = v
    return sd


def get_teacher():
    """The frozen teacher of a distilling run (`distill:`), or None: built with the run's image_size and compute_dtype, loaded from
    distill.checkpoint, on the device, in eval mode.  distill_options() holds its alpha and temperature."""
    opts = distill_options()
    if opts is None:
        return None
    model_lib = importlib.import_module(opts['model'])
    teacher = model_lib.Model(**opts['model_kwparams'], input_size=FLAGS.image_size)
    if FLAGS.get('compute_dtype', 'bf16') == 'f32':
        teacher.set_compute_dtype(torch.float32)
    if opts['checkpoint']:
        ckpt = torch.load(opts['checkpoint'], map_location='cpu', weights_only=False)
        teacher.load_state_dict(teacher_state_dict(ckpt))
        logging.info('Loaded distill teacher {}.'.format(opts['checkpoint']))
    else:
        logging.warning('distill: no checkpoint, the teacher keeps its initial weights')
    teacher.cuda()
    teacher.eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    return teacher


def all_steps_skipped(skipped_before, skipped_now, steps):
    """The abort rule of a guarded run: True when `steps` > 0 optimizer steps ran since the counter read `skipped_before` and every one
    of them was dropped (the cumulative counter of engine.TrainStep.guard_state() advanced by all of them).  One dropped step among good
    ones is what the guard is for; nothing but dropped steps is a run that has gone bad and must stop before it writes a checkpoint."""
    return steps > 0 and skipped_now - skipped_before >= steps


def setup_distributed(num_images=None):
    """batch_size = world * per_gpu_batch_size * grad_accum_steps; lr = base_lr * batch / base_total_batch; steps per epoch =
    ceil(N / batch) (common.py:185-209; the micro-batches of an accumulated step count as further ranks: engine.TrainStep)."""
    accum = grad_accum_steps()
    if FLAGS.use_distributed:
        udist.init_dist()
        FLAGS.batch_size = udist.get_world_size() * FLAGS.per_gpu_batch_size * accum
    else:
        FLAGS.batch_size = FLAGS.per_gpu_batch_size * accum
    FLAGS._loader_batch_size = FLAGS.per_gpu_batch_size
    if 'base_lr' in FLAGS:
        FLAGS.lr = FLAGS.base_lr * (FLAGS.batch_size / FLAGS.base_total_batch)
    if num_images:
        FLAGS._steps_per_epoch = math.ceil(num_images / FLAGS.batch_size)
