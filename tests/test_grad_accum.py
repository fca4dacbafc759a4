"""Gradient accumulation, host side: the derived total batch / learning rate / steps per epoch with grad_accum_steps micro-batches
per optimizer step (common.setup_distributed), the tiny_accum.yml fixture, and the rejection of bad values."""
import math
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
YML = os.path.join(ROOT, "tests", "data", "tiny_accum.yml")


def _load(*opts):
    from atomnas_amd.utils import config as cfg
    os.environ.setdefault("ATOMNAS_E2E_DIR", tempfile.gettempdir())
    return cfg.load_app(["app:" + YML] + list(opts))


@pytest.mark.parametrize("accum", [1, 2, 8])
def test_setup_distributed_counts_micro_batches_as_ranks(accum):
    import common as mc
    flags = _load("--grad_accum_steps", str(accum), "--per_gpu_batch_size", "256")
    assert flags.use_distributed is False
    mc.setup_distributed(1281167)
    assert flags.batch_size == 256 * accum
    assert flags._loader_batch_size == 256                      # the loader keeps drawing micro-batches
    assert flags.lr == flags.base_lr * (256 * accum / flags.base_total_batch)
    assert flags._steps_per_epoch == math.ceil(1281167 / (256 * accum))


def test_tiny_accum_fixture_resolves():
    import common as mc
    flags = _load()
    assert flags.grad_accum_steps == 2 and mc.grad_accum_steps() == 2
    assert flags.per_gpu_batch_size == 8 and flags.max_steps_per_epoch == 3   # inherited from the tiny search config
    mc.setup_distributed(64)
    assert flags.batch_size == 16 and flags._steps_per_epoch == 4


def test_default_is_one_micro_batch():
    import common as mc
    from atomnas_amd.utils import config as cfg
    os.environ.setdefault("ATOMNAS_E2E_DIR", tempfile.gettempdir())
    flags = cfg.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_search.yml")])
    assert mc.grad_accum_steps() == 1
    mc.setup_distributed(64)
    assert flags.batch_size == flags.per_gpu_batch_size == 8


@pytest.mark.parametrize("bad", [0, -1, 1.5, "2", True, None])
def test_bad_grad_accum_steps_raise(bad):
    import common as mc
    flags = _load()
    flags.grad_accum_steps = bad
    with pytest.raises(ValueError):
        mc.grad_accum_steps()
    with pytest.raises(ValueError):
        mc.setup_distributed(64)
