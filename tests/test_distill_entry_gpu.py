"""`python train.py app:tests/data/tiny_distill.yml` end to end on the GPU, as a fresh child process: the tiny "+" search of
tiny_search_se.yml distilled from a frozen teacher that the test writes (architecture yaml + checkpoint with an EMA) -- two shortened
epochs with the final shrink.  The log lines carry `kd`, the checkpoint holds the student only and loads into a network built from the
exported architecture alone."""
import os
import subprocess
import sys

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TEACHER_KW = dict(num_classes=10, input_channel=16, last_channel=64, dropout_ratio=0.2, batch_norm_momentum=0.1, batch_norm_epsilon=1e-3,
                  active_fn="nn.ReLU",
                  inverted_residual_setting=[[8, 1, 1, [3], [16], False], [16, 1, 2, [3, 5], [24, 24], True], [24, 1, 2, [3], [48], True],
                                             [32, 1, 2, [3], [64], True], [40, 1, 2, [5], [64], True]])


def write_teacher(tmp_path):
    """architecture yaml + a checkpoint in train.py's format (wrapper prefix, an EMA whose shadows differ from the raw weights)"""
    sys.path.insert(0, ROOT)
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.models import searched_network as sn
    torch.manual_seed(31)
    t = sn.Model(**TEACHER_KW, input_size=64)
    t.apply(mb.init_weights_mnas)
    sd = {k: v.clone() for k, v in t.state_dict().items()}
    shadow = {k: (v * 4.0 if k.startswith("classifier") else v.clone()) for k, v in sd.items() if v.is_floating_point() and "num_batches" not in k}
    arch, ckpt = str(tmp_path / "teacher.yml"), str(tmp_path / "teacher.pt")
    with open(arch, "w") as f:
        yaml.safe_dump(TEACHER_KW, f)
    torch.save({"model": {"module." + k: v for k, v in sd.items()}, "ema": {"info": {}, "shadow": shadow, "param": {}}, "last_epoch": 0}, ckpt)
    return arch, ckpt


def test_distilling_train_entry_runs_two_epochs(gpu_lib, tmp_path):
    arch, ckpt = write_teacher(tmp_path)
    out_dir = tmp_path / "run"
    env = dict(os.environ, ATOMNAS_E2E_DIR=str(out_dir), ARNOLD_OUTPUT=str(out_dir), ATOMNAS_TEACHER_FILE=arch, ATOMNAS_TEACHER_CHECKPOINT=ckpt)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "app:" + os.path.join(ROOT, "tests", "data", "tiny_distill.yml")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    steps = [ln for ln in out.splitlines() if " step " in ln and " loss " in ln]
    assert len(steps) >= 6 and all(" kd " in ln for ln in steps), out[-4000:]
    kd = [float(ln.split(" kd ")[1].split()[0]) for ln in steps]
    assert all(v == v and v > 0 for v in kd), kd
    assert "Loaded distill teacher" in out and out.count(" val: ") >= 2 and "Model Shrink to FLOPS" in out, out[-4000:]
    # the checkpoint is the student's alone: it loads into a network built from the exported architecture, without any teacher
    path = os.path.join(str(out_dir), "latest_checkpoint.pt")
    assert os.path.exists(path)
    state = torch.load(path, map_location="cpu", weights_only=False)
    with open(os.path.join(str(out_dir), "latest_checkpoint.yml")) as f:
        kw = yaml.safe_load(f)
    sys.path.insert(0, ROOT)
    from atomnas_amd.models import searched_network as sn
    from atomnas_amd.utils.common import unwrap_state_dict
    student = sn.Model(**kw, input_size=64)
    student.load_state_dict(unwrap_state_dict(state["model"], verbose=False))   # strict: no key of a teacher, none missing
    assert set(state["ema"]["shadow"]) <= set(unwrap_state_dict(state["model"], verbose=False))
    assert not any("teacher" in k or "distill" in k for k in state)
