"""Host side of knowledge distillation (CPU): the `distill:` yaml block and its validation (common.distill_options / get_teacher), what
a teacher loads from a checkpoint, the argument checks of engine.TrainStep that run before any device work, and the ctypes binding of
atomnas_ce_distill against its prototype."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from atomnas_amd.utils import config  # noqa: E402

ARCH = os.path.join(ROOT, "apps", "searched", "models", "atomnas_c.yml")


def _bind(distill=None, **kw):
    flags = dict(model="models.searched_network", model_kwparams={"num_classes": 1000}, image_size=224, **kw)
    if distill is not None:
        flags["distill"] = distill
    config.FLAGS.bind(config.AttrDict(flags))


def test_no_distill_block_means_no_teacher():
    import common as mc
    _bind()
    assert mc.distill_options() is None and mc.get_teacher() is None


def test_distill_options_defaults_and_overrides():
    import common as mc
    _bind({"model_kwparams": {"num_classes": 1000, "batch_norm_momentum": 0.1}, "model_kwparams.batch_norm_momentum": 0.01,
           "checkpoint": "t.pt"})
    o = mc.distill_options()
    assert o["model"] == "models.searched_network" and o["alpha"] == 0.5 and o["temperature"] == 1.0 and o["checkpoint"] == "t.pt"
    assert o["model_kwparams"] == {"num_classes": 1000, "batch_norm_momentum": 0.01}
    assert config.FLAGS.distill["model_kwparams"]["batch_norm_momentum"] == 0.1   # the flags themselves are left alone
    _bind({"model": "models.mobilenet_supernet", "model_kwparams": {}, "alpha": 1, "temperature": 4})
    o = mc.distill_options()
    assert o["model"] == "models.mobilenet_supernet" and o["alpha"] == 1.0 and o["temperature"] == 4.0 and o["checkpoint"] is None


@pytest.mark.parametrize("block, match", [
    ("teacher.pt", "mapping"),
    ({"alpha": 0.5}, "model_kwparams"),
    ({"model_kwparams": {}, "alpha": -0.1}, "alpha"),
    ({"model_kwparams": {}, "alpha": 1.5}, "alpha"),
    ({"model_kwparams": {}, "alpha": float("nan")}, "alpha"),
    ({"model_kwparams": {}, "alpha": "half"}, "alpha"),
    ({"model_kwparams": {}, "alpha": True}, "alpha"),
    ({"model_kwparams": {}, "temperature": 0}, "temperature"),
    ({"model_kwparams": {}, "temperature": -2.0}, "temperature"),
    ({"model_kwparams": {}, "temperature": float("inf")}, "temperature"),
    ({"model_kwparams": {"num_classes": 10}}, "classes"),
    ({"model_kwparams": {}, "temprature": 2.0}, "unknown distill key"),
    ({"model_kwparams": {}, "alpha.x": 1}, "only model_kwparams"),
    ({"model_kwparams": {}, "checkpoint": 3}, "checkpoint"),
])
def test_distill_options_refuses_bad_blocks(block, match):
    import common as mc
    _bind(block)
    with pytest.raises(ValueError, match=match):
        mc.distill_options()
    with pytest.raises(ValueError, match=match):
        mc.get_teacher()


def test_the_yaml_keys_resolve(tmp_path, monkeypatch):
    """tests/data/tiny_distill.yml and the AtomNAS-C recipe: include chain, environment expansion, the dotted overrides inside the block"""
    import common as mc
    monkeypatch.setenv("ATOMNAS_E2E_DIR", str(tmp_path))
    monkeypatch.setenv("ARNOLD_OUTPUT", str(tmp_path))
    monkeypatch.setenv("DATA_LMDB", "/tmp/none")
    arch = tmp_path / "teacher.yml"
    arch.write_text("{num_classes: 10, input_channel: 16, batch_norm_momentum: 0.1}\n")
    monkeypatch.setenv("ATOMNAS_TEACHER_FILE", str(arch))
    monkeypatch.setenv("ATOMNAS_TEACHER_CHECKPOINT", str(tmp_path / "teacher.pt"))
    flags = config.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_distill.yml")])
    assert flags.num_epochs == 2 and flags.model_kwparams.num_classes == 10 and flags.model_kwparams.se_ratio is not None
    o = mc.distill_options()
    assert o == dict(model="models.searched_network", model_kwparams={"num_classes": 10, "input_channel": 16, "batch_norm_momentum": 0.01},
                     checkpoint=str(tmp_path / "teacher.pt"), alpha=0.5, temperature=2.0)
    monkeypatch.setenv("TEACHER_FILE", ARCH)
    monkeypatch.setenv("TEACHER_CHECKPOINT", "/nowhere/best_model.pt")
    flags = config.load_app(["app:" + os.path.join(ROOT, "apps", "searched", "atomnas_c", "atomnas_c_distill.yml")])
    assert flags.model == "models.searched_network" and flags.model_kwparams.dropout_ratio == 0.28
    o = mc.distill_options()
    assert o["alpha"] == 0.5 and o["temperature"] == 1.0 and o["checkpoint"] == "/nowhere/best_model.pt"
    assert o["model_kwparams"]["batch_norm_momentum"] == 0.01 and o["model_kwparams"]["batch_norm_epsilon"] == 1e-3
    assert o["model_kwparams"]["inverted_residual_setting"] == flags.model_kwparams.inverted_residual_setting
    # without the block the same recipe distils nothing
    flags = config.load_app(["app:" + os.path.join(ROOT, "apps", "searched", "atomnas_c", "atomnas_c.yml")])
    assert mc.distill_options() is None


def test_a_teacher_gets_the_ema_weights_of_a_checkpoint():
    import common as mc
    w, s = torch.ones(3), torch.full((3,), 2.0)
    ckpt = {"model": {"module.a.weight": w, "module.a.running_mean": w, "module.a.num_batches_tracked": torch.tensor(5)},
            "ema": {"shadow": {"a.weight": s, "a.running_mean": s, "gone.weight": s}}}
    sd = mc.teacher_state_dict(ckpt)
    assert set(sd) == {"a.weight", "a.running_mean", "a.num_batches_tracked"}
    assert torch.equal(sd["a.weight"], s) and torch.equal(sd["a.running_mean"], s) and int(sd["a.num_batches_tracked"]) == 5
    sd = mc.teacher_state_dict(dict(ckpt, ema=None))
    assert torch.equal(sd["a.weight"], w)
    sd = mc.teacher_state_dict({"module.a.weight": w})   # a bare state_dict, either wrapper form
    assert set(sd) == {"a.weight"}


def test_train_step_checks_come_before_device_work():
    """engine.check_teacher on CPU modules: nothing here touches a GPU"""
    from atomnas_amd import engine

    class Net(torch.nn.Linear):
        def __init__(self, k):
            super().__init__(4, k)
            self.num_classes = k
    m, t = Net(10), Net(10)
    assert engine.check_teacher(m, None, 0.0, 1.0) == (0.0, 1.0)
    assert engine.check_teacher(m, t, 1, 4) == (1.0, 4.0)
    for args, match in (((m, None, 0.5, 1.0), "needs a teacher"), ((m, m, 0.5, 1.0), "is the student"), ((m, Net(11), 0.5, 1.0), "classes"),
                        ((m, t, 0.5, 0.0), "temperature"), ((m, t, 0.5, -1.0), "temperature"), ((m, t, -0.5, 1.0), "alpha"),
                        ((m, t, 1.01, 1.0), "alpha"), ((m, None, 0.0, 0.0), "temperature"), ((m, torch.nn.Linear(4, 10), 0.5, 1.0), "classes")):
        with pytest.raises(ValueError, match=match):
            engine.check_teacher(*args)


def test_distill_criterion_checks_its_options():
    from atomnas_amd.utils import optim
    c = optim.DistillCrossEntropy(10, 0.1, 0.3, 2.0, reduction="mean")
    assert (c.alpha, c.temperature, c.topk_correct) == (0.3, 2.0, None)
    for a, t in ((-0.1, 1.0), (1.1, 1.0), (0.5, 0.0), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            optim.DistillCrossEntropy(10, 0.1, a, t)
    with pytest.raises(ValueError):
        optim.DistillCrossEntropy(10, 0.1, 0.5, 1.0, reduction="max")


def test_ce_distill_binding_matches_its_prototype():
    """atomnas_ce_distill in atomnas_amd/_lib.py against include/atomnas_hip.h: the argument list of the issue, position by position"""
    from atomnas_amd import _lib
    header = open(os.path.join(ROOT, "include", "atomnas_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+atomnas_ce_distill\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m, "atomnas_ce_distill is not declared"
    decls = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert decls == ["const float* logits", "int ldl", "const float* teacher", "int ldt", "const long long* target", "float eps", "float alpha",
                     "float temperature", "int B", "int K", "float* loss_per_sample", "float* kd_per_sample", "void* dlogits", "int ldd",
                     "float gscale", "int* topk_correct", "int dtype", "void* stream"]
    kind = lambda d: ctypes.c_void_p if "*" in d else {"int": ctypes.c_int, "float": ctypes.c_float}[d.split()[0]]
    assert _lib.SIGNATURES["atomnas_ce_distill"] == [kind(d) for d in decls]
    assert _lib.ABI_VERSION == 9 and "#define ATOMNAS_ABI_VERSION 9" in open(os.path.join(ROOT, "include", "atomnas_hip.h")).read()
    src = open(os.path.join(ROOT, "atomnas_amd", "csrc", "head.hip")).read()
    assert 'extern "C" int atomnas_ce_distill(' in src and "k_ce_smooth<float>" in src
