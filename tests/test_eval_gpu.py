"""Checkpoint evaluation end to end on the GPU: a tiny search writes a checkpoint + exported architecture, `val.py
app:apps/eval/eval_shrink.yml` scores it in a fresh process, an independent count (the oracle restatement on the same calibrated EMA
weights and the same preprocessed batches) agrees, and `train.py --test_only True` gives the same numbers without training.  Plus the
searched networks' forward at the eval configs' batch sizes."""
import ast
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import atomnas_oracle as orc  # noqa: E402

from kutil import assert_close  # noqa: E402
from test_block_gpu import _sd64  # noqa: E402

pytestmark = pytest.mark.gpu
CLASSES = ("n01440764", "n01443537", "n01484850")
NVAL = 5 * len(CLASSES)   # 15 val images at a batch of 4: three full batches and a short last one of 3


def _image_folder(root):
    from PIL import Image
    rng = np.random.RandomState(1)
    for split, per_class in (("train", 12), ("val", NVAL // len(CLASSES))):
        for c in CLASSES:
            d = os.path.join(root, split, c)
            os.makedirs(d)
            for k in range(per_class):
                H, W = int(rng.randint(60, 200)), int(rng.randint(60, 200))
                Image.fromarray(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(d, "%03d.png" % k))


def _eval_app(tmp_path, data):
    """apps/eval/eval_shrink.yml for one process on the tiny image folder (a bool cannot be switched off from the command line: the
    reference's cast makes `--use_distributed False` true)"""
    p = os.path.join(str(tmp_path), "eval_tiny.yml")
    with open(p, "w") as f:
        f.write("_default: !include %s\n" % os.path.join(ROOT, "apps", "eval", "eval_shrink.yml"))
        f.write("dataset: imagenet1k\ndataset_dir: %s\nuse_distributed: False\nallreduce_bn: False\nper_gpu_batch_size: 4\n"
                "bn_calibration_steps: 2\nbn_calibration_per_gpu_batch_size: 8\ndata_loader_workers: 2\nnum_epochs: 2\n" % data)
    return "app:" + p


def _results(out, phase="test"):
    m = re.search(r"Epoch 0/\d+ %s samples: (\d+), results: (\{.*\})" % phase, out)
    assert m, out[-4000:]
    return int(m.group(1)), ast.literal_eval(m.group(2))


def test_val_py_scores_a_search_checkpoint(gpu_lib, tmp_path):
    data, run = str(tmp_path / "data"), str(tmp_path / "search")
    _image_folder(data)
    env = dict(os.environ, ATOMNAS_E2E_DIR=run, ARNOLD_OUTPUT=str(tmp_path / "out"))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train.py"),
                        "app:" + os.path.join(ROOT, "tests", "data", "tiny_search_decoded.yml"), "--dataset", "imagenet1k", "--dataset_dir", data],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    # the search writes best_model.{pt,yml} only when top-1 improves on 1.0, which a random 1000-way head rarely does on three
    # classes; latest_checkpoint.{pt,yml} comes from the same writer (train.py) in the same format
    ckpt = "best_model" if os.path.exists(os.path.join(run, "best_model.yml")) else "latest_checkpoint"
    env.update(FILE=run, CHECKPOINT=ckpt)
    app = _eval_app(tmp_path, data)
    before = sorted(os.listdir(run))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "val.py"), app],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert re.search(r"Epoch 0/2 test: loss: [0-9.]+, top1_error: [0-9.]+, top5_error: [0-9.]+", out), out[-3000:]
    n_val, res_val = _results(out)
    assert n_val == NVAL   # every val image, the short last batch included

    # train.py with test_only: the same numbers, no training step, no checkpoint
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "train.py"), app, "--test_only", "True"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    out2 = r.stdout + r.stderr
    assert r.returncode == 0, out2[-4000:]
    assert _results(out2) == (n_val, res_val)
    assert " step " not in out2 and "Prune threshold" not in out2
    assert sorted(os.listdir(run)) == before and not os.path.exists(str(tmp_path / "out"))

    # the independent count: the same evaluation in this process, then the oracle on its calibrated weights and batches
    import common as mc
    import train
    from atomnas_amd.utils import config as cfg
    from atomnas_amd.utils import dataflow
    from atomnas_amd.utils.common import set_random_seed
    os.environ.update(FILE=run, CHECKPOINT=ckpt, ARNOLD_OUTPUT=str(tmp_path / "out"))
    F = cfg.load_app([app])
    sets = train.build_datasets(F)
    mc.setup_distributed(len(sets[0]))
    train.LOADERS = dataflow.data_loader(*sets, F)
    set_random_seed(F.get("random_seed", 0))
    try:
        model, wrapper = mc.get_model()
        ema = mc.setup_ema(model)
        train.load_pretrained(F.pretrained, wrapper, ema)
        res, n, eval_wrapper = train.evaluate(wrapper, ema)
        assert (n, res) == (n_val, res_val)
        net = mc.unwrap_model(eval_wrapper)
        spec = orc.spec_from_model(net)
        sd = {k: (v.float() if v.is_floating_point() else v).cuda() for k, v in _sd64(net).items()}   # the oracle in fp32 on the GPU
        hits, near, loss, seen, worst = np.zeros(2), 0, 0.0, 0, 0.0
        for x, y in train.device_batches(train.LOADERS[3], None):
            with torch.no_grad():
                logits = orc.model_forward(x, sd, spec, False, q=orc.Bf16Storage()).double()   # where the bf16 path rounds
                mine = net(x).double()
            err = float((mine - logits).abs().max())
            worst = max(worst, err)
            # bf16 end to end through a barely trained network: the bound of tests/test_parity_gpu.py's end-to-end test
            assert float((mine - logits).norm() / max(float(logits.norm()), 1e-30)) < 0.3
            bound = 2 * err   # the measured kernel error of the batch, on either side of a rank boundary
            top = logits.topk(6, dim=1).values
            for i in range(x.shape[0]):
                t = float(logits[i, y[i]])
                for k in (1, 5):
                    # distance of the label's logit from the top-k boundary: a smaller one may rank either way on the HIP path
                    margin = t - float(top[i, k]) if t >= float(top[i, k - 1]) else float(top[i, k - 1]) - t
                    if margin < bound:
                        near += 1
            pred = logits.topk(5, dim=1).indices
            hit = pred.eq(y.view(-1, 1))
            hits += [float(hit[:, :1].any(1).sum()), float(hit.any(1).sum())]
            loss += float(torch.nn.functional.cross_entropy(logits, y, reduction="sum"))
            seen += x.shape[0]
    finally:
        train.LOADERS = None
    assert seen == NVAL
    print("samples %d, oracle top-1 / top-5 hits %s, label logits within the kernel bound (%.3g) of a rank boundary: %d" % (seen, hits, 2 * worst, near))
    assert abs(res_val["loss"] - loss / seen) <= 2 * worst + 1e-6   # cross entropy moves by at most twice the largest logit error
    got = np.array([(1 - res_val["top1_error"]) * seen, (1 - res_val["top5_error"]) * seen])
    assert np.all(np.abs(np.round(got) - hits) <= near), (got, hits, near)


def _searched(name):
    from atomnas_amd import configs
    from atomnas_amd.models import searched_network as sn
    from test_block_gpu import _randomize
    model = sn.Model(**dict(configs.searched_kwparams(name), input_size=224))
    model.set_compute_dtype(torch.float32)
    _randomize(model, 17)
    return model


def _sd32(model):
    return {k: (v.float() if v.is_floating_point() else v).cuda() for k, v in _sd64(model).items()}


@pytest.mark.parametrize("name", ["atomnas_c", "atomnas_c_plus"])
def test_searched_eval_logits_at_the_eval_batch_sizes(gpu_lib, name):
    """eval logits at N = 1 (the configs' "perfect evaluation"), 7 (a ragged tail) and 64 (per_gpu_batch_size) against the oracle (fp32
    on the GPU), with the bounds of the full-size eval test (tests/test_configs_gpu.py cfg 4)"""
    model = _searched(name)
    sd = _sd32(model)
    spec = orc.spec_from_model(model)
    model.cuda().eval()
    g = torch.Generator().manual_seed(3)
    for n in (1, 7, 64):
        x = torch.randn(n, 3, 224, 224, generator=g).cuda()
        with torch.no_grad():
            got = model(x)
            ref = orc.model_forward(x, sd, spec, False)
        assert tuple(got.shape) == (n, 1000)
        assert_close("logits N=%d" % n, got, ref, rtol=2e-3, atol=2e-4 * max(1.0, float(ref.abs().max())))


def test_searched_calibration_statistics_at_batch_512(gpu_lib):
    """BN calibration (cumulative statistics) of the searched AtomNAS-C at bn_calibration_per_gpu_batch_size = 512 against the oracle"""
    from atomnas_amd.utils.common import bn_calibration
    model = _searched("atomnas_c")
    model.eval()
    model.apply(bn_calibration)
    sd = _sd32(model)
    spec = dict(orc.spec_from_model(model), momentum=None)
    model.cuda()
    x = torch.randn(512, 3, 224, 224, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        model(x)
        stats = {}
        orc.model_forward(x, sd, spec, True, stats)
    torch.cuda.synchronize()
    msd = model.state_dict()
    assert len(stats) == sum(1 for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))
    for prefix, (rm, rv) in stats.items():
        for k, v in ((prefix + ".running_mean", rm), (prefix + ".running_var", rv)):
            s = max(1e-3, float(v.abs().max()))
            assert_close(k, msd[k], v, rtol=2e-3, atol=2e-4 * s)
