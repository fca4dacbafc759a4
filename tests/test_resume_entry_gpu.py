"""`python train.py ... --resume` against the run it continues (GPU, two child processes): three shortened epochs of the AtomNAS-C
search with classifier dropout, uninterrupted, and the third epoch again from the checkpoint of the second."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    return out


def _epoch_lines(out, epoch):
    """what the run logs about an epoch, without the time stamps and the throughput: the step lines (step, loss, l2, l1, lr as printed)
    and the validation result"""
    steps = re.findall(r"Epoch %d/3 step (\d+) loss (\S+) l2 (\S+) l1 (\S+) lr (\S+) " % epoch, out)
    val = re.findall(r"Epoch %d val: (\{.*\})" % epoch, out)
    return steps, val


def _same(name, a, b):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b), name
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a.keys()) == list(b.keys()), name
        for k in a:
            _same("%s.%s" % (name, k), a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), name
        for i, (x, y) in enumerate(zip(a, b)):
            _same("%s[%d]" % (name, i), x, y)
    else:
        assert a == b, (name, a, b)


def test_resumed_entry_repeats_the_last_epoch_of_the_uninterrupted_run(gpu_lib, tmp_path):
    """Child A: three epochs x 3 steps of tests/data/tiny_search.yml with dropout_ratio 0.2 (synthetic batches, seeded per epoch),
    through tests/resume_entry_driver.py, which keeps a copy of every epoch's checkpoint.  Child B: train.py --resume from A's copy of
    epoch 1.  B's log of epoch 2 (steps, validation) equals A's digit for digit, and every entry of B's final latest_checkpoint.pt
    equals A's: model, optimizer state, EMA shadows and counters, global step, dropout counter, prune table.
    Wall time: 12 s on an MI355X (two children; each builds the full-size supernet, captures the step and validates)."""
    app = str(tmp_path / "three_epochs.yml")
    with open(app, "w") as f:
        f.write("_default: !include %s\nnum_epochs: 3\n'model_kwparams.dropout_ratio': 0.2\n" % os.path.join(ROOT, "tests", "data", "tiny_search.yml"))
    a_dir, b_dir, copies = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "copies")
    out_a = _run([os.path.join(ROOT, "tests", "resume_entry_driver.py"), copies, "app:" + app],
                 dict(os.environ, ATOMNAS_E2E_DIR=a_dir, ARNOLD_OUTPUT=a_dir))
    assert sorted(os.listdir(copies)) == ["epoch0", "epoch1", "epoch2"]
    out_b = _run([os.path.join(ROOT, "train.py"), "app:" + app, "--resume", os.path.join(copies, "epoch1")],
                 dict(os.environ, ATOMNAS_E2E_DIR=b_dir, ARNOLD_OUTPUT=b_dir))
    assert "Epoch 2/3" in out_b and "Epoch 0/3" not in out_b and "Epoch 1/3" not in out_b, out_b[-3000:]
    steps_a, val_a = _epoch_lines(out_a, 2)
    steps_b, val_b = _epoch_lines(out_b, 2)
    assert len(steps_a) == 3 and [s[0] for s in steps_a] == ["7", "8", "9"] and len(val_a) == 1, out_a[-3000:]
    assert steps_b == steps_a, (steps_a, steps_b)
    assert val_b == val_a, (val_a, val_b)
    # the driver's copy is what the run itself wrote
    load = lambda *p: torch.load(os.path.join(*p), map_location="cpu", weights_only=False)
    ck_a, ck_b = load(a_dir, "latest_checkpoint.pt"), load(b_dir, "latest_checkpoint.pt")
    _same("copy", load(copies, "epoch2", "latest_checkpoint.pt"), ck_a)
    assert ck_a["last_epoch"] == 2 and ck_a["global_step"] == 9 and ck_a["dropout_counter"] == 9
    _same("checkpoint", ck_a, ck_b)
