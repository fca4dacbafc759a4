"""Checkpoint evaluation (val.py, train.py with `test_only`, apps/eval/*.yml) and the input pipeline's host side for oversize crop
boxes, without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pil_resize as pr  # noqa: E402


def _supernet_c():
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import config as cfg
    c = cfg.Config(os.path.join(ROOT, "apps", "slimming", "shrink", "atomnas_c.yml"))
    return ms.Model(**c.model_kwparams, input_size=224)


def _export(model, d, name="best_model"):
    """what a search run writes (train.py): str(mb.output_network(model)) next to the checkpoint"""
    from atomnas_amd.models import mobilenet_base as mb
    with open(os.path.join(d, name + ".yml"), "w") as f:
        f.write(str(mb.output_network(model)))


@pytest.mark.parametrize("app", ["eval.yml", "eval_se.yml", "eval_shrink.yml"])
def test_eval_configs_load(app, tmp_path, monkeypatch):
    from atomnas_amd.utils import config as cfg
    model = _supernet_c()
    _export(model, str(tmp_path))
    monkeypatch.setenv("FILE", str(tmp_path))
    monkeypatch.setenv("CHECKPOINT", "best_model")
    monkeypatch.setenv("TRAIN_CONFIG", os.path.join(ROOT, "apps", "searched", "atomnas_c", "atomnas_c.yml"))
    monkeypatch.setenv("ARNOLD_OUTPUT", str(tmp_path))
    F = cfg.load_app(["app:" + os.path.join(ROOT, "apps", "eval", app), "--per_gpu_batch_size", "32"])
    assert F.test_only is True and F.bn_calibration is True and F.allreduce_bn is True
    assert F.per_gpu_batch_size == 32 and F.bn_calibration_steps == 256 and F.bn_calibration_per_gpu_batch_size == 512
    assert F.model == "models.searched_network"
    assert F.model_kwparams["batch_norm_momentum"] == 0.01 and F.model_kwparams["batch_norm_epsilon"] == 1e-3
    if app == "eval_se.yml":
        assert F.model_kwparams["se_ratio"] == 0.5
    if app == "eval_shrink.yml":
        assert F.pretrained == os.path.join(str(tmp_path), "best_model.pt")
        rows = F.model_kwparams["inverted_residual_setting"]
        assert rows == [[b.output_dim, 1, b.stride, b.kernel_sizes, b.channels, b.expand] for b in model.get_named_block_list().values()]
        assert rows[0][5] is False and rows[1][5] is True   # Python's True / False parse as YAML booleans


def test_exported_search_network_loads_into_the_searched_network(tmp_path, monkeypatch):
    """eval_shrink.yml on what a search writes: the exported rows build models.searched_network and the supernet's state dict loads
    into it key for key"""
    from atomnas_amd.models import searched_network as sn
    from atomnas_amd.utils import config as cfg
    model = _supernet_c()
    _export(model, str(tmp_path))
    monkeypatch.setenv("FILE", str(tmp_path))
    monkeypatch.setenv("CHECKPOINT", "best_model")
    monkeypatch.setenv("ARNOLD_OUTPUT", str(tmp_path))
    F = cfg.load_app(["app:" + os.path.join(ROOT, "apps", "eval", "eval_shrink.yml")])
    net = sn.Model(**F.model_kwparams, input_size=F.image_size)
    net.load_state_dict(model.state_dict(), strict=True)
    assert set(net.state_dict()) == set(model.state_dict())


def test_test_only_builds_no_train_loader_and_no_optimizer(monkeypatch, tmp_path):
    import common as mc
    import train
    from atomnas_amd import engine
    from atomnas_amd.utils import config as cfg
    from atomnas_amd.utils import dataflow
    from atomnas_amd.utils import optim
    monkeypatch.setenv("ATOMNAS_E2E_DIR", str(tmp_path))
    F = cfg.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_search_decoded.yml"), "--test_only", "True"])
    assert F.test_only is True
    sets = train.build_datasets(F)
    mc.setup_distributed(len(sets[0]))
    loaders = dataflow.data_loader(*sets, F)
    assert loaders[0] is None and loaders[1] is not None and loaders[3] is not None   # no train loader; calibration on the train split
    assert loaders[1].batch_size == F.bn_calibration_per_gpu_batch_size and loaders[1].shuffle

    class _M(torch.nn.Module):
        pass

    calls = []
    monkeypatch.setattr(mc, "get_model", lambda: (_M(), _M()))
    monkeypatch.setattr(mc, "setup_ema", lambda model: None)

    def _no(*a, **k):
        raise AssertionError("test_only built a training object")
    monkeypatch.setattr(optim, "get_optimizer", _no)
    monkeypatch.setattr(optim, "get_lr_scheduler", _no)
    monkeypatch.setattr(engine, "TrainStep", _no)
    monkeypatch.setattr(train, "evaluate", lambda w, ema, *a, **k: calls.append((w, ema)))
    train.train_val_test()
    assert len(calls) == 1 and calls[0][1] is None
    assert not os.listdir(str(tmp_path))   # no checkpoint


def test_evaluate_needs_a_test_loader(monkeypatch):
    import train
    from atomnas_amd.utils import config as cfg
    cfg.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_search.yml")])
    monkeypatch.setattr(train, "LOADERS", None)
    with pytest.raises(ValueError, match="test loader"):
        train.evaluate(None, None)


def test_eval_refuses_the_supernet_at_calibration_batch_512():
    """the AtomNAS-C supernet's 112 x 112 x 288 hidden tensor at N = 512 is 3.7 GB: above the 2^31-byte activation limit of the forward
    kernels -> refused before any launch; at the bench batch (256) and for a searched network at 512 it passes"""
    import train
    from atomnas_amd import configs
    from atomnas_amd.models import searched_network as sn
    from atomnas_amd.utils import config as cfg
    cfg.load_app(["app:" + os.path.join(ROOT, "apps", "slimming", "shrink", "atomnas_c.yml")])
    model = _supernet_c()
    with pytest.raises(ValueError, match="2\\^31 bytes"):
        train.check_eval_size(model, 512)
    assert train.check_eval_size(model, 256) == 256 * 112 * 112 * 288 * 2
    net = sn.Model(**dict(configs.searched_kwparams("atomnas_c"), input_size=224))
    assert train.check_eval_size(net, 512) < train.EVAL_MAX_ACTIVATION_BYTES


def test_check_box_routes_large_scales_and_rejects_outside_boxes():
    from atomnas_amd.utils import dataflow as DF
    assert DF.check_box(4000, 6000, (0, 0, 2016, 2016), 224) is False        # exactly 9 S: the one-pass kernel
    assert DF.check_box(4000, 6000, (0, 0, 2017, 100), 224) is True          # above 9 S: the two-pass path
    assert DF.check_box(4000, 6000, (250, 1250, 3500, 3500), 224) is True    # the centre crop of a 6000 x 4000 val image
    for box in ((0, 0, 4001, 10), (-1, 0, 10, 10), (0, 5990, 10, 11), (0, 0, 0, 5)):
        with pytest.raises(ValueError):
            DF.check_box(4000, 6000, box, 224)


def test_pil_resize_restatement_is_bit_identical_to_pil_at_large_scales():
    """oracle/pil_resize.py against PIL itself at 10x to 25x down-scaling, bilinear and bicubic (the range of the two-pass kernel)"""
    from PIL import Image
    rng = np.random.RandomState(11)
    n = 0
    for t in range(8):
        S = int(rng.choice([8, 12, 16, 24]))
        fh, fw = float(rng.uniform(10, 25)), float(rng.uniform(10, 25))
        h, w = int(fh * S), int(fw * S)
        H, W = h + int(rng.randint(0, 40)), w + int(rng.randint(0, 40))
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        i, j = int(rng.randint(0, H - h + 1)), int(rng.randint(0, W - w + 1))
        for filt, pf in ((pr.BILINEAR, Image.BILINEAR), (pr.BICUBIC, Image.BICUBIC)):
            ref = np.asarray(Image.fromarray(img).crop((j, i, j + w, i + h)).resize((S, S), pf))
            assert np.array_equal(pr.resize_u8(img[i:i + h, j:j + w], S, S, filt), ref), (t, filt, (H, W), (i, j, h, w), S)
        n += 1
    assert n == 8
