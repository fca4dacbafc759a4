#!/usr/bin/env python
"""AtomNAS supernet training on MI355X:  python train.py app:apps/slimming/shrink/atomnas_c.yml [--dotted.key value ...]

Same entry, yaml semantics and loop order as the reference's train.py (run_one_epoch :130-250, per-epoch validate / mask /
shrink :364-411, checkpoint :395-411), with the iteration executed by atomnas_amd.engine.TrainStep (one replayed hipGraph
per iteration, RCCL all-reduce of the gradient arena).  Under a launcher (torch.distributed.run) one process drives one GPU.
Input: `dataset: imagenet1k_fake` (synthetic, device resident: the benchmark protocol) or any decoded source through the reference's
factories utils.dataflow.data_transforms / dataset / data_loader (`dataset: imagenet1k_decoded_fake`, or a module of your own) ->
utils.dataflow.DevicePrefetcher (crop / PIL-exact bilinear resize / flip / normalize on the GPU) -> TrainStep.set_batch.  JPEG decoding
and LMDB reading are not available in this image.
"""
import logging
import os
import sys
import time

import torch

from atomnas_amd import engine
from atomnas_amd.models import mobilenet_base as mb
from atomnas_amd.utils import config as cfg
from atomnas_amd.utils import distributed as udist
from atomnas_amd.utils import optim, prune
from atomnas_amd.utils.common import bn_calibration, get_params_by_name, set_random_seed

NUM_IMAGENET_TRAIN = 1281167


LOADERS = None   # (train_loader, calib_loader, val_loader, test_loader) when the yaml names a decoded data source; None: synthetic batches


def device_batches(loader, steps):
    """at most `steps` batches of `loader` through the GPU input pipeline (train.py:215-218 of the reference: DataPrefetcher);
    steps=None: every batch of the loader, the short last one included"""
    from atomnas_amd.utils import dataflow
    tf = getattr(getattr(loader, 'dset', None), 'transform', None)   # the split's DeviceTransform: resampling filter, mean, std
    kw = dict(filter=tf.filter, mean=tf.mean, std=tf.std) if isinstance(tf, dataflow.DeviceTransform) else {}
    from atomnas_amd.utils.image_store import DecodedStore
    # a decoded store hands out unpinned views of the page cache: one staged copy per batch instead of one pageable copy per image
    pre = dataflow.DevicePrefetcher(loader, image_size=cfg.FLAGS.image_size, staging=isinstance(getattr(loader, 'dset', None), DecodedStore), **kw)
    try:
        for i, (x, y) in enumerate(pre):
            if steps is not None and i >= steps:
                break
            yield x, y
    finally:
        pre.close()


def fake_batches(batch, image_size, num_classes, steps, seed):
    """Device-resident synthetic batches (normal images, uniform labels); the reference's FakeData is all zeros."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(batch, 3, image_size, image_size, device='cuda', generator=g)
    y = torch.randint(0, num_classes, (batch,), device='cuda', generator=g)
    for _ in range(steps):
        yield x, y


def shrink_model(model_wrapper, ema, optimizer, prune_info, threshold=1e-3, ema_only=False):
    """Discard dead atomic blocks (train.py:27-81): mask = |gamma| > thr OR |gamma_ema| > thr (EMA only at the last epoch)."""
    import common as mc
    FLAGS = cfg.FLAGS
    model = mc.unwrap_model(model_wrapper)
    # all alive masks in one launch over the parameter / EMA arenas (the reference: 63 x abs, compare, or, sum().item())
    from atomnas_amd import runtime
    blocks = list(model.get_named_block_list().items())
    gammas, per_block = [], []
    for block_name, block in blocks:
        assert isinstance(block, (mb.InvertedResidualChannels, mb.InvertedResidualChannelsFused))
        # a fused block that does not expand has no atoms to search: it is left alone
        bns = block.get_depthwise_bn() if block.expand or isinstance(block, mb.InvertedResidualChannels) else []
        per_block.append(len(bns))
        gammas.extend(bn.weight for bn in bns)
    if ema is not None:
        ema.attach(runtime.manager_of(model))
    from atomnas_amd import ops
    all_masks, all_index, kept = prune.alive_masks(gammas, threshold, mode=0 if ema is None else (2 if ema_only else 1), with_index=True)
    all_masks = [m.clone() for m in all_masks]   # the arenas are rebuilt while the blocks are compressed
    # Job-list repack: the masks' kept-channel indices and counts are known from that one launch (one device -> host copy for the counts);
    # every gather of the shrink -- weights, BatchNorm vectors, RMSprop state, EMA shadows (models/compress_utils.py:31-37,
    # utils/rmsprop.py:134-165, utils/optim.py:134-153) -- is recorded by the per-tensor protocol and runs as ONE launch at the end
    for m, idx, k in zip(all_masks, all_index, kept.tolist() if kept is not None else []):
        ops.register_mask(m, idx, k)
    ops.gather_defer(True)
    try:
        pos = 0
        for (block_name, block), n in zip(blocks, per_block):
            masks = all_masks[pos:pos + n]
            pos += n
            if n == 0 and isinstance(block, mb.InvertedResidualChannelsFused):
                continue   # not searched, or already the identity: no tensor to repack
            block.compress_by_mask(masks, ema=ema, optimizer=optimizer, prune_info=prune_info, prefix=block_name, verbose=False)
    finally:
        ops.gather_defer(False)   # flush
        ops.clear_masks()
    if optimizer is not None:
        assert set(id(p) for p in optimizer.param_groups[0]['params']) == set(id(p) for p in model.parameters())
    mc.profiling(model)
    logging.info('Model Shrink to FLOPS: {}'.format(model.n_macs))
    logging.info('Current model: {}'.format(mb.output_network(model)))


def calibrate_bn(model, epoch):
    """BN calibration of the eval model (cumulative statistics over `bn_calibration_steps` batches of the calib loader: the train
    split with the train transforms), then allreduce_bn when distributed (val.py:125-142 of the reference)"""
    FLAGS = cfg.FLAGS
    model.eval()
    model.apply(bn_calibration)
    with torch.no_grad():
        calib = (device_batches(LOADERS[1], FLAGS.bn_calibration_steps) if LOADERS is not None and LOADERS[1] is not None else
                 fake_batches(FLAGS.bn_calibration_per_gpu_batch_size, FLAGS.image_size, FLAGS.model_kwparams['num_classes'],
                              FLAGS.bn_calibration_steps, 7 + epoch))
        for x, y in calib:
            model(x)
    if FLAGS.use_distributed:
        udist.allreduce_bn(model)


def eval_net(model):
    """What an evaluation pass calls: the model itself, or with `fused_inference` its compilation for inference (atomnas_amd/inference.py:
    one fused launch per atomic block).  Compiled AFTER the BatchNorm calibration, which needs batch statistics and stays on the
    model's own path; the compiled network folds the calibrated statistics into constants."""
    if not cfg.FLAGS.get('fused_inference', False):
        return model
    from atomnas_amd.inference import compile_for_inference
    return compile_for_inference(model)


def validate(epoch, model_wrapper, ema, criterion, meters, steps):
    """EMA model -> BN calibration (cumulative statistics) -> evaluation (train.py:419-458), on synthetic batches."""
    import common as mc
    FLAGS = cfg.FLAGS
    eval_wrapper = mc.get_ema_model(ema, model_wrapper)
    model = mc.unwrap_model(eval_wrapper)
    if FLAGS.get('bn_calibration', False):
        calibrate_bn(model, epoch)
    model.eval()
    net = eval_net(model)
    with torch.no_grad():
        val = (device_batches(LOADERS[2], steps) if LOADERS is not None and LOADERS[2] is not None else
               fake_batches(FLAGS.per_gpu_batch_size, FLAGS.image_size, FLAGS.model_kwparams['num_classes'], steps, 11))
        for x, y in val:
            mc.forward_loss(net, criterion, x, y, meters)
    return meters.flush(), eval_wrapper


EVAL_MAX_ACTIVATION_BYTES = 1 << 31


def check_eval_size(model, batch):
    """Refuses a forward whose largest activation tensor (the expanded hidden tensor of a block at its input resolution, or the stem
    output) reaches 2^31 bytes: the forward / statistics kernels are verified up to the bench step's 1.85 GB tensors, and some of them
    address a whole tensor with 32-bit byte offsets.  The AtomNAS-C supernet at a calibration batch of 512 (512 x 112^2 x 288 bf16,
    3.7 GB) is refused; searched networks are far below the limit."""
    elt = 4 if getattr(model, 'compute_dtype', torch.bfloat16) == torch.float32 else 2
    res = cfg.FLAGS.image_size // 2   # the stem's stride-2 output
    worst, where = batch * res * res * ((model.input_channel + 7) // 8 * 8) * elt, 'stem'
    for name, b in model.get_named_block_list().items():
        hidden = (sum(b.channels) + 7) // 8 * 8
        nbytes = batch * res * res * hidden * elt
        if nbytes > worst:
            worst, where = nbytes, name
        res = (res + b.stride - 1) // b.stride
    if worst >= EVAL_MAX_ACTIVATION_BYTES:
        raise ValueError('evaluation at batch {}: the hidden tensor of {} is {:.2f} GB, at or above the forward kernels\' limit of '
                         '2^31 bytes per activation tensor; lower per_gpu_batch_size / bn_calibration_per_gpu_batch_size'.format(
                             batch, where, worst / 1e9))
    return worst


def evaluate(model_wrapper, ema, epoch=0, phase='test'):
    """The reference's testing workflow (val.py:109-145, run_one_epoch :17-63): EMA model (if any) -> BN calibration (if
    `bn_calibration`) -> one pass over the WHOLE test loader, the short last batch included, with per-sample cross entropy (no
    smoothing) and top-1 / top-5 reduced over ranks.  Distributed, every rank sees the same number of samples: the index list is
    padded by wrapping around (DistributedSampler, mirrored by DecodedLoader), so a few samples count twice, as in the reference.
    -> (results, samples counted over all ranks, eval model wrapper)"""
    import common as mc
    FLAGS = cfg.FLAGS
    if LOADERS is None or LOADERS[3] is None:
        raise ValueError("evaluation needs a test loader: a decoded `dataset` (imagenet1k, imagenet1k_decoded_fake or a module of "
                         "your own), not {}".format(FLAGS.get('dataset', 'imagenet1k_fake')))
    eval_wrapper = mc.get_ema_model(ema, model_wrapper)
    model = mc.unwrap_model(eval_wrapper)
    check_eval_size(model, max(FLAGS.per_gpu_batch_size, FLAGS.bn_calibration_per_gpu_batch_size if FLAGS.get('bn_calibration', False) else 0))
    if FLAGS.get('bn_calibration', False):
        if not FLAGS.use_distributed:
            logging.warning('Only GPU0 is used when calibration when use DataParallel')
        calibrate_bn(model, epoch)
    criterion = optim.CrossEntropyLabelSmooth(FLAGS.model_kwparams['num_classes'], 0.0, reduction='none')
    meters = mc.get_meters(phase)
    model.eval()
    net = eval_net(model)
    seen = 0
    with torch.no_grad():
        for x, y in device_batches(LOADERS[3], None):
            mc.forward_loss(net, criterion, x, y, meters)
            seen += x.shape[0]
    if FLAGS.use_distributed:
        n = torch.tensor([seen], dtype=torch.float64, device='cuda')
        torch.distributed.all_reduce(n)
        seen = int(n.item())
    results = meters.flush()
    if udist.is_master():
        logging.info('Epoch {}/{} {}: '.format(epoch, FLAGS.num_epochs, phase) + ', '.join('{}: {:.4f}'.format(k, v) for k, v in results.items()))
        logging.info('Epoch {}/{} {} samples: {}, results: {}'.format(epoch, FLAGS.num_epochs, phase, seen, repr(results)))
    return results, seen, eval_wrapper


def load_pretrained(path, model_wrapper, ema):
    """`pretrained:` of the reference (train.py:276-296): EMA dict (if any) and model weights of a checkpoint written by
    utils/common.py:123-137 (or a bare state_dict), optionally remapped by position onto this model's keys."""
    FLAGS = cfg.FLAGS
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    if ema and isinstance(ckpt, dict) and ckpt.get('ema'):
        ema.load_state_dict(ckpt['ema'])
        ema.to(next(model_wrapper.parameters()).device)
    if isinstance(ckpt, dict) and 'model' in ckpt:
        ckpt = ckpt['model']
    if FLAGS.get('pretrained_model_remap_keys', False):
        ckpt = {new: ckpt[old] for new, old in zip(model_wrapper.state_dict().keys(), ckpt.keys())}
    from atomnas_amd.utils.common import unwrap_state_dict
    target = set(model_wrapper.state_dict().keys())
    if not any(k in target for k in ckpt):   # saved through the other wrapper form (`module.` prefix present / absent)
        stripped = unwrap_state_dict(ckpt, verbose=False)
        ckpt = stripped if any(k in target for k in stripped) else {'module.' + k: v for k, v in ckpt.items()}
    model_wrapper.load_state_dict(ckpt)
    logging.info('Loaded model {}.'.format(path))


def load_checkpoint(ckpt, model_wrapper, optimizer, ema):
    """`resume:` of the reference (train.py:299-317) on a checkpoint dict in the reference's format (utils/common.py:123-137:
    'model', 'optimizer' -- torch's index-ordered optimizer state_dict --, 'ema' = {info, shadow, param}, 'last_epoch',
    'best_val').  Checkpoints written here carry the optimizer's parameter ORDER by name as well: after a shrink it differs from
    the model's (re-keyed variables are appended, utils/rmsprop.py:134-165) and torch maps saved state by position."""
    target = set(model_wrapper.state_dict().keys())
    sd = ckpt['model']
    if not any(k in target for k in sd):
        sd = ({k[len('module.'):]: v for k, v in sd.items()} if all(k.startswith('module.') for k in sd)
              else {'module.' + k: v for k, v in sd.items()})
    model_wrapper.load_state_dict(sd)
    names = ckpt.get('optimizer_param_names')
    if names:
        table = dict(model_wrapper.named_parameters())
        if not any(n in table for n in names):   # written under the other wrapper form: same normalisation as the model keys
            names = ([n[len('module.'):] for n in names] if all(n.startswith('module.') for n in names)
                     else ['module.' + n for n in names])
        optimizer.param_groups[0]['params'] = [table[n] for n in names]
    optimizer.load_state_dict(ckpt['optimizer'])
    if ema:
        ema.load_state_dict(ckpt['ema'])
        ema.to(next(model_wrapper.parameters()).device)
    return ckpt['last_epoch'], ckpt['best_val']


def optimizer_steps_per_epoch():
    """optimizer steps the training loop takes per epoch: `max_steps_per_epoch` where the yaml shortens the epochs, else the epoch of
    the schedules (FLAGS._steps_per_epoch, which the learning-rate and rho schedules keep measuring in)"""
    FLAGS = cfg.FLAGS
    return FLAGS.get('max_steps_per_epoch', None) or FLAGS._steps_per_epoch


def checkpoint_state(model_wrapper, optimizer, ema, epoch, best_val, results):
    """The checkpoint dict in the reference's format (utils/common.py:123-137) plus what a resumed run needs to compute what the
    uninterrupted one would: the optimizer's parameter order by name (load_checkpoint), the global step, the dropout counter, and the
    order and penalties of the prune table (normalised over the supernet the run started from, re-keyed by every shrink)."""
    import common as mc
    from atomnas_amd import runtime
    FLAGS = cfg.FLAGS
    pname = {id(p): n for n, p in model_wrapper.named_parameters()}
    counter = runtime.manager_of(mc.unwrap_model(model_wrapper)).step_counter
    prune_info = FLAGS.get('_bn_to_prune', None)
    return {'model': {k: v.detach().clone() for k, v in model_wrapper.state_dict().items()}, 'optimizer': optimizer.state_dict(),
            'optimizer_param_names': [pname[id(p)] for p in optimizer.param_groups[0]['params']],
            'ema': ema.state_dict() if ema else None, 'last_epoch': epoch, 'best_val': min(best_val, results['top1_error']),
            # the reference's resume unpacks `train_meters, val_meters = checkpoint['meters']` (train.py:313): a pair
            'meters': (None, None),
            'global_step': int(FLAGS._global_step), 'dropout_counter': int(counter) if counter is not None else 0,
            'prune_penalty': prune_info.penalty_state() if prune_info is not None else None}


def resume_run(ckpt, model_wrapper, optimizer, ema, lr_scheduler, prune_info=None):
    """Continues the run that wrote `ckpt` -> (last_epoch, best_val): load_checkpoint, then the bookkeeping that is not a tensor of the
    model, the optimizer or the EMA -- the global step (FLAGS._global_step, the scheduler's last_epoch: they drive the learning rate,
    rho and the EMA warm-up), the dropout counter and the prune table.  A checkpoint without the additional keys (the reference's,
    or an older one of ours) derives them: optimizer steps per epoch x epochs done, x micro-batches per step for the counter."""
    import common as mc
    from atomnas_amd import runtime
    FLAGS = cfg.FLAGS
    last_epoch, best_val = load_checkpoint(ckpt, model_wrapper, optimizer, ema)
    global_step = ckpt.get('global_step')
    if global_step is None:
        global_step = (last_epoch + 1) * optimizer_steps_per_epoch()
    lr_scheduler.last_epoch = global_step
    FLAGS._global_step = global_step
    counter = ckpt.get('dropout_counter')
    if counter is None:
        counter = global_step * mc.grad_accum_steps()
    runtime.manager_of(mc.unwrap_model(model_wrapper)).set_step_counter(counter)
    if prune_info is not None and ckpt.get('prune_penalty') is not None:
        prune_info.load_penalty_state(ckpt['prune_penalty'])
    return last_epoch, best_val


def train_val_test():
    import common as mc
    FLAGS = cfg.FLAGS
    model, model_wrapper = mc.get_model()
    ema = mc.setup_ema(model)
    if FLAGS.get('pretrained', None):
        load_pretrained(FLAGS.pretrained, model_wrapper, ema)
    if FLAGS.get('test_only', False):   # train.py:350-357 of the reference: evaluate, then stop (no optimizer, no step, no checkpoint)
        if udist.is_master():
            logging.info('Start testing.')
        FLAGS._global_step = 0
        evaluate(model_wrapper, ema)
        return
    optimizer = optim.get_optimizer(model_wrapper, FLAGS)
    lr_scheduler = optim.get_lr_scheduler(optimizer, FLAGS)
    last_epoch, best_val = -1, 1.0
    FLAGS._global_step = 0
    assert FLAGS.profiling, '`m.macs` is used for calculating penalty'
    mc.profiling(model)   # (shapes only: nothing runs, so it may precede the checkpoint)
    FLAGS._bn_to_prune = prune.get_bn_to_prune(model, FLAGS.prune_params, verbose=udist.is_master())
    if FLAGS.resume:
        ckpt = torch.load(os.path.join(FLAGS.resume, 'latest_checkpoint.pt'), map_location='cpu', weights_only=False)
        last_epoch, best_val = resume_run(ckpt, model_wrapper, optimizer, ema, lr_scheduler, FLAGS._bn_to_prune)
    rho_scheduler = prune.get_rho_scheduler(FLAGS.prune_params, FLAGS._steps_per_epoch)
    clip_norm, skip_nonfinite = mc.guard_options()   # a bad value stops the run here, before anything is captured
    distill = mc.distill_options()                   # so does a bad `distill:` block
    teacher = mc.get_teacher()                       # None without the block; validation, shrink and checkpoints see the student only
    distill_kw = dict(teacher=teacher, distill_alpha=distill['alpha'], distill_temperature=distill['temperature']) if distill else {}
    step = engine.TrainStep(model, optimizer, ema, FLAGS._bn_to_prune, weight_decay=FLAGS.weight_decay,
                            wd_method=FLAGS.weight_decay_method, label_smoothing=FLAGS.label_smoothing,
                            batch_size=FLAGS.per_gpu_batch_size, image_size=FLAGS.image_size,
                            world_size=udist.get_world_size_fallback(),
                            allreduce_bn=bool(FLAGS.use_distributed and FLAGS.get('allreduce_bn', False)), accum_steps=mc.grad_accum_steps(),
                            clip_norm=clip_norm, skip_nonfinite=skip_nonfinite, **distill_kw)
    guard_seen = [0, FLAGS._global_step]   # the guard's skipped counter and the global step at the last check

    def check_guard(where):
        """-> guard_state().  Every optimizer step since the last check dropped: stop, before a checkpoint is written (every rank
        reaches the same verdict, so every rank stops)"""
        st = step.guard_state()
        if mc.all_steps_skipped(guard_seen[0], st['skipped'], FLAGS._global_step - guard_seen[1]):
            raise RuntimeError('step {} ({}): the gradients of every optimizer step since step {} were not finite and the steps were '
                               'skipped; stopping before a checkpoint is written'.format(FLAGS._global_step, where, guard_seen[1]))
        guard_seen[:] = [st['skipped'], FLAGS._global_step]
        return st
    accum = step.accum_steps   # loader batches per optimizer step; _steps_per_epoch / max_steps_per_epoch count optimizer steps
    val_criterion = optim.CrossEntropyLabelSmooth(FLAGS.model_kwparams['num_classes'], 0.0, reduction='none')
    val_meters = mc.get_meters('val')
    steps_per_epoch = optimizer_steps_per_epoch()
    rank = udist.get_rank_fallback()
    for epoch in range(last_epoch + 1, FLAGS.num_epochs):
        model.train()
        t0, seen = time.time(), 0
        for loader in (LOADERS[:2] if LOADERS is not None else ()):   # the shuffle of epoch k, whether or not the run started at 0
            if hasattr(loader, 'set_epoch'):                            # (train.py:155 / val.py:36 of the reference)
                loader.set_epoch(epoch)
        batches = (device_batches(LOADERS[0], steps_per_epoch * accum) if LOADERS is not None else
                   fake_batches(FLAGS.per_gpu_batch_size, FLAGS.image_size, FLAGS.model_kwparams['num_classes'], steps_per_epoch * accum,
                                FLAGS.get('random_seed', 0) + rank + 1000 * epoch))
        for x, y in batches:
            if x.shape[0] != FLAGS.per_gpu_batch_size:
                continue   # a short last batch: the captured step has a static batch (drop_last: True avoids drawing it)
            step.set_batch(x, y)
            seen += x.shape[0]
            if step.pending < accum - 1:
                step.accumulate()
                continue
            step.global_step = FLAGS._global_step
            step.step(lr=optimizer.param_groups[0]['lr'], rho=rho_scheduler(FLAGS._global_step))
            lr_scheduler.step()   # (allreduce_bn, when configured, happens inside the step: before the EMA, as in the reference)
            FLAGS._global_step += 1
            if FLAGS._global_step % FLAGS.log_interval == 0:
                # a guarded run reads the verdict on every rank (they all hold the same one): a run gone bad stops everywhere
                st = check_guard('log interval') if step.guarded else None
                if udist.is_master():
                    ce, l2, l1 = step.loss.tolist()   # the only host synchronisation of the interval
                    kd = float(step.kd) if step.kd is not None else None   # distilling: `loss` is the combined objective, kd its soft term
                    dt = time.time() - t0
                    line = 'Epoch {}/{} step {} loss {:.4f} l2 {:.4f} l1 {:.4f} lr {:.5f} {:.0f} img/s/GPU'.format(
                        epoch, FLAGS.num_epochs, FLAGS._global_step, ce, l2, l1, optimizer.param_groups[0]['lr'], seen / dt)
                    if kd is not None:
                        line += ' kd {:.4f}'.format(kd)
                    if st is not None:
                        line += ' gnorm {:.4f} skipped {} clipped {}'.format(st['norm'], st['skipped'], st['clipped'])
                    logging.info(line)
        # a trailing partial group of the epoch is dropped, as a short last batch is -- here, so that the shrink and the checkpoint below
        # see the dropout counter of the whole steps only
        step.reset_accumulation()
        if step.guarded:
            check_guard('end of epoch {}'.format(epoch))
        results, eval_wrapper = validate(epoch, model_wrapper, ema, val_criterion, val_meters, FLAGS.get('val_steps', 4))
        if udist.is_master():
            logging.info('Epoch {} val: {}'.format(epoch, results))
        if FLAGS.prune_params['method'] is not None:
            thr = FLAGS.model_shrink_threshold
            eval_model = mc.unwrap_model(eval_wrapper)
            masks = prune.cal_mask_network_slimming_by_threshold(get_params_by_name(eval_model, FLAGS._bn_to_prune.weight), thr)
            FLAGS._bn_to_prune.add_info_list('mask', masks)
            flops_pruned, infos = prune.cal_pruned_flops(FLAGS._bn_to_prune)
            if udist.is_master():
                logging.info('Prune threshold: {}, flops pruned: {}, flops remain: {}'.format(thr, flops_pruned, model.n_macs - flops_pruned))
            if flops_pruned >= FLAGS.model_shrink_delta_flops or epoch == FLAGS.num_epochs - 1:
                shrink_model(model_wrapper, ema, optimizer, FLAGS._bn_to_prune, thr, ema_only=(epoch == FLAGS.num_epochs - 1))
        if udist.is_master() and FLAGS.get('log_dir', None):
            os.makedirs(FLAGS.log_dir, exist_ok=True)
            kw = mb.output_network(model)
            state = checkpoint_state(model_wrapper, optimizer, ema, epoch, best_val, results)
            torch.save(state, os.path.join(FLAGS.log_dir, 'latest_checkpoint.pt'))
            with open(os.path.join(FLAGS.log_dir, 'latest_checkpoint.yml'), 'w') as f:
                f.write(str(kw))
            if results['top1_error'] < best_val:
                best_val = results['top1_error']
                torch.save(state, os.path.join(FLAGS.log_dir, 'best_model.pt'))
                with open(os.path.join(FLAGS.log_dir, 'best_model.yml'), 'w') as f:
                    f.write(str(kw))


def build_datasets(FLAGS):
    """(train_set, val_set, test_set) of a decoded source through the reference's factories (train.py:330-339 /
    utils/dataflow.py:92-267), or None for the synthetic `imagenet1k_fake`"""
    if FLAGS.get('dataset', 'imagenet1k_fake') == 'imagenet1k_fake':
        return None
    from atomnas_amd.utils import dataflow
    if FLAGS.get('bn_calibration', False):
        FLAGS._loader_batch_size_calib = FLAGS.bn_calibration_per_gpu_batch_size
    return dataflow.dataset(*dataflow.data_transforms(FLAGS), FLAGS)


def main():
    import common as mc
    FLAGS = cfg.load_app(sys.argv[1:])
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(message)s')
    global LOADERS
    num_train = NUM_IMAGENET_TRAIN
    sets = build_datasets(FLAGS)
    if sets is not None and sets[0] is not None:
        num_train = len(sets[0])
    mc.setup_distributed(num_train)
    if sets is not None:
        from atomnas_amd.utils import dataflow
        LOADERS = dataflow.data_loader(*sets, FLAGS)
    if udist.is_master():
        logging.info(FLAGS)
    set_random_seed(FLAGS.get('random_seed', 0))
    train_val_test()


if __name__ == '__main__':
    main()
