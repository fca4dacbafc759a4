"""Guarded training step, host side: the yaml keys grad_clip_norm / skip_nonfinite_steps (common.guard_options), the tiny_guard.yml
fixture, the argument checks of engine.TrainStep that run before any device work, and train.py's abort rule as a pure function of the
skipped counter between two log lines (common.all_steps_skipped)."""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DATA = os.path.join(ROOT, "tests", "data")


def _load(name, *opts):
    from atomnas_amd.utils import config as cfg
    os.environ.setdefault("ATOMNAS_E2E_DIR", tempfile.gettempdir())
    return cfg.load_app(["app:" + os.path.join(DATA, name)] + list(opts))


def test_tiny_guard_fixture_resolves():
    import common as mc
    flags = _load("tiny_guard.yml")
    assert flags.grad_clip_norm == 5.0 and flags.skip_nonfinite_steps is True
    assert flags.per_gpu_batch_size == 8 and flags.max_steps_per_epoch == 3   # inherited from the tiny search config
    assert mc.guard_options() == (5.0, True)


def test_guard_is_off_by_default_and_zero_means_off():
    import common as mc
    flags = _load("tiny_search.yml")
    assert flags.get("grad_clip_norm", None) is None and flags.get("skip_nonfinite_steps", False) is False
    assert mc.guard_options() == (None, False)
    flags.grad_clip_norm = 0
    assert mc.guard_options() == (None, False)
    flags.grad_clip_norm = 0.0
    flags.skip_nonfinite_steps = True
    assert mc.guard_options() == (None, True)
    flags.grad_clip_norm = 2
    assert mc.guard_options() == (2.0, True)


def test_keys_are_overridden_from_the_command_line():
    """(the entry's --key value options override keys a yaml sets, converted to the type of the yaml's value: the guard fixture is the
    base)  A negative norm given there is refused like one in the yaml."""
    import common as mc
    _load("tiny_guard.yml", "--grad_clip_norm", "1.5")
    assert mc.guard_options() == (1.5, True)
    _load("tiny_guard.yml", "--grad_clip_norm", "-1")
    with pytest.raises(ValueError):
        mc.guard_options()


@pytest.mark.parametrize("bad", [-1, -0.5, float("nan"), "1.0", True])
def test_bad_grad_clip_norm_raises(bad):
    import common as mc
    flags = _load("tiny_guard.yml")
    flags.grad_clip_norm = bad
    with pytest.raises(ValueError):
        mc.guard_options()


@pytest.mark.parametrize("bad", [1, "yes", None])
def test_bad_skip_nonfinite_steps_raises(bad):
    import common as mc
    flags = _load("tiny_guard.yml")
    flags.skip_nonfinite_steps = bad
    with pytest.raises(ValueError):
        mc.guard_options()


def test_train_step_rejects_a_bad_clip_norm_before_any_device_work():
    """the check is the constructor's first statement: with a bad value it raises before it looks at the model (None here)"""
    from atomnas_amd import engine
    with pytest.raises(TypeError):
        engine.TrainStep(None, None, clip_norm="1.0")
    with pytest.raises(ValueError):
        engine.TrainStep(None, None, clip_norm=-2.0)
    for bad in ("1.0", [1.0], True, object()):
        with pytest.raises(TypeError):
            engine.check_clip_norm(bad)
    for bad in (-1, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            engine.check_clip_norm(bad)
    assert engine.check_clip_norm(None) is None and engine.check_clip_norm(0) is None and engine.check_clip_norm(0.0) is None
    assert engine.check_clip_norm(2) == 2.0 and engine.check_clip_norm(0.25) == 0.25 and engine.check_clip_norm(float("inf")) == float("inf")


def test_abort_rule():
    """between two looks at the cumulative counter: abort exactly when at least one optimizer step ran and all of them were dropped"""
    import common as mc
    assert mc.all_steps_skipped(0, 0, 10) is False            # nothing dropped
    assert mc.all_steps_skipped(0, 1, 10) is False            # one bad step among good ones: what the guard is for
    assert mc.all_steps_skipped(3, 12, 10) is False           # nine of ten
    assert mc.all_steps_skipped(3, 13, 10) is True            # all ten
    assert mc.all_steps_skipped(0, 1, 1) is True              # log_interval 1: the one step of the interval
    assert mc.all_steps_skipped(5, 5, 0) is False             # no step since the last look (a log line at the end of an epoch)
    assert mc.all_steps_skipped(5, 6, 0) is False


def test_train_reads_the_guard_where_it_reads_the_loss():
    """train.py appends the guard's fields to the log line and checks the abort rule before validate() and the checkpoint"""
    src = open(os.path.join(ROOT, "train.py")).read()
    assert "gnorm" in src and "skipped" in src and "clipped" in src
    body = src[src.index("def train_val_test"):]
    assert body.index("check_guard('end of epoch") < body.index("validate(epoch") < body.index("torch.save(state")
    step_code = open(os.path.join(ROOT, "atomnas_amd", "engine.py")).read().split("    def step(")[1]   # step() and its pieces
    assert ".item()" not in step_code and ".tolist()" not in step_code
