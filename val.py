#!/usr/bin/env python
"""Checkpoint evaluation on MI355X:  python val.py app:apps/eval/eval_shrink.yml [--dotted.key value ...]

Same entry and semantics as the reference's val.py: `test_only` is forced on, the model and its EMA are built from the yaml, the
`pretrained` checkpoint (model + `ema`) is loaded, and train.evaluate runs the EMA model through BN calibration (if configured) and one
pass over the whole test loader.  No optimizer, no training step, no train loader and no checkpoint.  The test loader of a
distributed run pads every rank to the same sample count by wrapping around (DistributedSampler): a few samples count twice, as in
the reference.
"""
import logging
import sys

import train
from atomnas_amd.utils import config as cfg
from atomnas_amd.utils import distributed as udist
from atomnas_amd.utils.common import set_random_seed


def val():
    import common as mc
    FLAGS = cfg.FLAGS
    model, model_wrapper = mc.get_model()
    ema = mc.setup_ema(model)
    if FLAGS.get('pretrained', None):
        train.load_pretrained(FLAGS.pretrained, model_wrapper, ema)
    if udist.is_master():
        logging.info(model_wrapper)
        logging.info('Start testing.')
    FLAGS._global_step = 0
    return train.evaluate(model_wrapper, ema)


def main():
    FLAGS = cfg.load_app(sys.argv[1:])
    FLAGS.test_only = True
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(message)s')
    sets = train.build_datasets(FLAGS)
    import common as mc
    mc.setup_distributed(len(sets[0]) if sets is not None and sets[0] is not None else None)
    if sets is not None:
        from atomnas_amd.utils import dataflow
        train.LOADERS = dataflow.data_loader(*sets, FLAGS)
    if udist.is_master():
        logging.info(FLAGS)
    set_random_seed(FLAGS.get('random_seed', 0))
    val()


if __name__ == '__main__':
    main()
