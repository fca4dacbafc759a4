"""Searching the "+" space, host side: the supernet with Squeeze-and-Excitation, the prune info of fused blocks (the per-atom cost
and its exact identity against the profiler's stamps), the export of a fused search and the unchanged export of a plain one."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [[1, 8, 1, 2, [3]], [6, 16, 1, 2, [3, 5, 7]], [6, 24, 2, 2, [3, 5, 7]], [6, 32, 1, 2, [3, 5]]]


def _fused_supernet(se_ratio, active_fn="nn.Swish"):
    from atomnas_amd.models import mobilenet_supernet as ms
    return ms.Model(num_classes=10, input_size=64, input_channel=16, last_channel=128, batch_norm_momentum=0.01, batch_norm_epsilon=1e-3,
                    active_fn=active_fn, block="InvertedResidualChannelsFused", inverted_residual_setting=ROWS, se_ratio=se_ratio)


@pytest.mark.parametrize("se_ratio", [None, 0.25])
def test_fused_prune_info_cost_identity(se_ratio):
    """sum_i hidden_i * cost_i == block.n_macs, exactly and in integers, for every expanding fused block; the cost is the closed form of
    the issue (inp*H*W + k^2*Ho*Wo + oup*Ho*Wo (+ Ho*Wo + 2*se_hid)); the penalties' atom-weighted mean is 1 within the formula's 1e-5"""
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.utils import model_profiling as mp, prune
    model = _fused_supernet(se_ratio)
    mp.model_profiling(model, 64, 64, verbose=False)
    info = prune.get_bn_to_prune(model, {"bn_prune_filter": "expansion_only_skip_expand1"}, verbose=False)
    known = dict(model.named_parameters())
    assert len(info.weight) == 3 + 3 + 3 + 2 and all(n in known for n in info.weight)
    cost = dict(zip(info.weight, info.get_info_list("per_channel_flops")))
    res, seen = 32, 0
    for name, b in model.get_named_block_list().items():
        assert isinstance(b, mb.InvertedResidualChannelsFused)
        out = (res - 1) // b.stride + 1
        if b.expand:
            names = ["{}.depth_ops.{}.1.1.weight".format(name, i) for i in range(len(b.channels))]
            assert [n for n in info.weight if n.startswith(name + ".")] == names
            costs = [cost[n] for n in names]
            assert all(isinstance(c, int) for c in costs)
            assert sum(h * c for h, c in zip(b.channels, costs)) == b.n_macs
            se = 0 if se_ratio is None else out * out + 2 * int(round(b.input_dim * se_ratio))
            assert costs == [b.input_dim * res * res + k * k * out * out + b.output_dim * out * out + se for k in b.kernel_sizes]
            seen += len(names)
        else:
            assert not any(n.startswith(name + ".") for n in info.weight)   # the fixed first row is skipped by *_skip_expand1
        res = out
    assert seen == len(info.weight)
    numel = [known[n].numel() for n in info.weight]
    mean = sum(n * p for n, p in zip(numel, info.penalty)) / sum(numel)
    assert abs(mean - 1.0) <= 1e-5
    equal = prune.get_bn_to_prune(model, {"bn_prune_filter": "equal_penalty_skip_expand1"}, verbose=False)
    assert equal.weight == info.weight and equal.penalty == [1] * len(info.weight)
    with pytest.raises(RuntimeError, match="Not search_first"):   # `expansion_only` reaches the block that does not expand
        prune.get_bn_to_prune(model, {"bn_prune_filter": "expansion_only"}, verbose=False)


def test_supernet_builds_squeeze_and_excitation():
    from atomnas_amd import configs
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.models import mobilenet_supernet as ms
    with pytest.raises(NotImplementedError, match="SE module not supported for block"):
        ms.Model(num_classes=10, input_size=64, inverted_residual_setting=ROWS, se_ratio=0.25)
    model = _fused_supernet(0.25)
    for b in model.get_named_block_list().values():
        assert isinstance(b.se_op, mb.SqueezeAndExcitation)
        assert b.se_op.n_hidden == int(round(b.input_dim * 0.25)) and b.se_op.n_feature == sum(b.channels)
    assert all(isinstance(b.se_op, mb.Identity) for b in _fused_supernet(None).get_named_block_list().values())
    kw = configs.model_kwparams("atomnas_c_se_supernet")
    assert (kw["block"], kw["active_fn"], kw["se_ratio"]) == ("InvertedResidualChannelsFused", "nn.Swish", 0.25)
    assert kw["inverted_residual_setting"] == configs.model_kwparams("atomnas_c_supernet")["inverted_residual_setting"]


def test_plain_export_is_unchanged():
    """output_network of a plain supernet: exactly the keys and rows it had before fused blocks could be exported"""
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.utils import config as cfg
    c = cfg.Config(os.path.join(ROOT, "apps", "slimming", "shrink", "atomnas_c.yml"))
    model = ms.Model(**c.model_kwparams, input_size=224)
    want = {"input_channel": 32, "last_channel": 1280, "width_mult": 1.0, "round_nearest": 8, "active_fn": "nn.ReLU", "num_classes": 1000,
            "inverted_residual_setting": [[b.output_dim, 1, b.stride, b.kernel_sizes, b.channels, b.expand]
                                          for b in model.get_named_block_list().values()]}
    got = mb.output_network(model)
    assert got == want and list(got.keys()) == list(want.keys())


def test_search_configs_load(monkeypatch, tmp_path):
    from atomnas_amd.utils import config as cfg
    monkeypatch.setenv("ARNOLD_OUTPUT", str(tmp_path))
    monkeypatch.setenv("ATOMNAS_E2E_DIR", str(tmp_path))
    F = cfg.load_app(["app:" + os.path.join(ROOT, "apps", "slimming", "shrink", "atomnas_c_se.yml")])
    plain = cfg.Config(os.path.join(ROOT, "apps", "slimming", "shrink", "atomnas_c.yml"))
    kw = dict(F.model_kwparams)
    assert (kw.pop("block"), kw.pop("se_ratio"), kw.pop("active_fn")) == ("InvertedResidualChannelsFused", 0.25, "nn.Swish")
    assert kw == {k: v for k, v in plain.model_kwparams.items() if k != "active_fn"}
    assert F.prune_params == plain.prune_params and F.model == "models.mobilenet_supernet"
    T = cfg.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_search_se.yml")])
    assert T.image_size == 64 and T.per_gpu_batch_size == 8 and T.model_kwparams["num_classes"] == 10
    assert T.model_kwparams["inverted_residual_setting"] == ROWS and T.model_kwparams["se_ratio"] == 0.25


def test_fused_export_loads_through_eval_shrink(monkeypatch, tmp_path):
    """the export of a fused search carries `block` and `se_ratio`; apps/eval/eval_shrink.yml builds models.searched_network from it and the
    supernet's state dict loads key for key.  A row without a live atom (hiddens == []) is the empty block: no tensor at all."""
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.models import searched_network as sn
    from atomnas_amd.utils import config as cfg
    model = _fused_supernet(0.25)
    kw = mb.output_network(model)
    assert kw["block"] == "InvertedResidualChannelsFused" and kw["se_ratio"] == 0.25
    assert "se_ratio" not in mb.output_network(_fused_supernet(None)) and mb.output_network(_fused_supernet(None))["block"] == kw["block"]
    with open(os.path.join(str(tmp_path), "best_model.yml"), "w") as f:
        f.write(str(kw))
    monkeypatch.setenv("FILE", str(tmp_path))
    monkeypatch.setenv("CHECKPOINT", "best_model")
    monkeypatch.setenv("ARNOLD_OUTPUT", str(tmp_path))
    F = cfg.load_app(["app:" + os.path.join(ROOT, "apps", "eval", "eval_shrink.yml")])
    assert F.model_kwparams["block"] == "InvertedResidualChannelsFused" and F.model_kwparams["se_ratio"] == 0.25
    net = sn.Model(**F.model_kwparams, input_size=64)
    net.load_state_dict(model.state_dict(), strict=True)
    assert list(net.state_dict()) == list(model.state_dict())
    assert mb.output_network(net) == kw   # the searched network exports itself the same way

    rows = [list(r) for r in kw["inverted_residual_setting"]]
    rows[3] = [24, 1, 1, [], [], True]
    empty = sn.Model(**dict(F.model_kwparams, inverted_residual_setting=rows), input_size=64)
    blk = empty.get_named_block_list()["features.4"]
    assert len(blk.depth_ops) == 0 and all(isinstance(m, mb.Identity) for m in (blk.expand_conv, blk.se_op, blk.project_conv))
    assert not any(k.startswith("features.4.") for k in empty.state_dict()) and not list(blk.parameters())
    x = torch.zeros(1, 24, 4, 4)
    assert blk(x) is x
    from atomnas_amd import runtime
    plans = {pl.name: pl for _, pl, _ in runtime.arena_layout(empty, torch.bfloat16).plans}
    assert plans["features.4"].nb == 0 and plans["features.3"].nb == 3   # the runtime plans it as the identity
