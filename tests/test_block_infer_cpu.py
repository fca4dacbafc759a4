"""Inference path without a GPU: the envelope of the fused block kernel (atomnas_block_infer_supported is a pure host predicate) over
the networks of atomnas_amd.configs and a committed table, and the host side of atomnas_amd.inference."""
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUPERNETS = ("atomnas_c_supernet", "atomnas_a_supernet", "atomnas_mix_supernet", "mobilenet_v2_1.0")
# non-SE blocks per network: the supernets' 1 + 4 + 4 + 4 + 4 + 4 + 1 rows, MobileNetV2's 1 + 2 + 3 + 4 + 3 + 3 + 1, the searched net's 22
N_BLOCKS = {"atomnas_c": 22, "atomnas_c_supernet": 22, "atomnas_a_supernet": 22, "atomnas_mix_supernet": 22, "mobilenet_v2_1.0": 17}
# Blocks atomnas_block_infer_supported answers 1 for: the kernel RUNS every block of every network (atomnas_block_infer_runs), but it
# measured slower than the existing path on all maps above 14x14, on stride 2, on outputs wider than 192 and on the supernets' wide
# hidden layers (profiles/infer_bench.txt), so those shapes are reported as unsupported and fall back.  What is left: the
# 14x14 and 7x7 stride-1 stages of the searched network and of MobileNetV2 up to 140,000 hidden channels x window pixels.
FUSED = {"atomnas_c": ["11", "12", "13", "15", "16", "17", "19", "20", "21"], "atomnas_c_supernet": [], "atomnas_a_supernet": [],
         "atomnas_mix_supernet": [], "mobilenet_v2_1.0": ["8", "9", "10", "11", "15", "16"]}


@pytest.fixture(scope="module")
def ops():
    from atomnas_amd import build, ops
    build.build_library()
    return ops


def _model(name):
    from atomnas_amd import configs
    from atomnas_amd.models import mobilenet_supernet as ms, searched_network as sn
    if name == "atomnas_c":
        return sn.Model(**dict(configs.searched_kwparams(name), input_size=224))
    return ms.Model(**dict(configs.model_kwparams(name), input_size=224))


@pytest.mark.parametrize("name", ("atomnas_c",) + SUPERNETS)
def test_every_block_of_the_networks_is_inside_the_envelope(ops, name):
    """224 x 224, batch 256, bf16: the kernel runs every non-SE block of the searched AtomNAS-C, the three supernets and MobileNetV2;
    the blocks it is reported as supported for are those of the measured table"""
    from atomnas_amd.inference import block_shapes
    shapes = block_shapes(_model(name), batch_size=256)
    assert len(shapes) == N_BLOCKS[name]
    assert shapes[0][1]["H"] == 112 and shapes[-1][1]["H"] == 7 and not any(s["se"] for _, s in shapes)
    refused = [(n, s) for n, s in shapes if not ops.block_infer_supported(dtype=torch.bfloat16, profitable=False, **s)]
    assert not refused, refused
    assert [n for n, s in shapes if ops.block_infer_supported(dtype=torch.bfloat16, **s)] == FUSED[name]
    # the same blocks in fp32 storage, with a 4x4 kernel or with stride 3 are outside, for both predicates
    for n, s in shapes:
        for prof in (False, True):
            assert not ops.block_infer_supported(dtype=torch.float32, profitable=prof, **s), n
            assert not ops.block_infer_supported(dtype=torch.bfloat16, profitable=prof, **dict(s, seg_k=[4] * len(s["seg_k"]))), n
            assert not ops.block_infer_supported(dtype=torch.bfloat16, profitable=prof, **dict(s, stride=3, residual=False)), n


def test_se_blocks_are_outside_the_envelope(ops):
    from atomnas_amd import configs
    from atomnas_amd.inference import block_shapes
    from atomnas_amd.models import searched_network as sn
    shapes = block_shapes(sn.Model(**dict(configs.searched_kwparams("atomnas_c_plus"), input_size=224)), batch_size=256)
    assert len(shapes) == 22 and all(s["se"] and s["act"] == 3 for _, s in shapes)
    assert not any(ops.block_infer_supported(dtype=torch.bfloat16, profitable=False, **s) for _, s in shapes)
    assert all(ops.block_infer_supported(dtype=torch.bfloat16, profitable=False, **dict(s, se=False)) for _, s in shapes)   # the SE alone keeps them out


def test_envelope_table(ops):
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "block_infer_envelope.json")))
    assert len(rows) >= 25
    wrong = []
    for r in rows:
        s = dict(r["shape"])
        got = ops.block_infer_supported(s.pop("N"), s.pop("H"), s.pop("W"), s.pop("inp"), s.pop("oup"), s.pop("seg_off"), s.pop("seg_ch"),
                                        s.pop("seg_k"), s.pop("stride"), s.pop("act"), s.pop("expand"), s.pop("residual"), s.pop("se"), s.pop("dtype"),
                                        profitable=r.get("predicate", "runs") == "supported")
        assert not s
        if int(got) != r["want"]:
            wrong.append((r["why"], r["want"], int(got)))
    assert not wrong, wrong


def test_the_predicate_needs_no_gpu_and_the_symbols_are_bound(ops):
    from atomnas_amd import _lib
    assert "atomnas_block_infer" in _lib.SIGNATURES and "atomnas_block_infer_supported" in _lib.NO_STATUS and "atomnas_block_infer_runs" in _lib.NO_STATUS
    assert ops.block_infer_supported(1, 14, 14, 8, 8, [0], [16], [3], 1, 1, True, True, False, torch.bfloat16) is True
    assert ops.block_infer_supported(1, 14, 14, 8, 8, [], [], [], 1, 1, True, True, False, torch.bfloat16) is False


def test_compile_refuses_cpu_training_and_fp32_models():
    from atomnas_amd import _lib
    from atomnas_amd.inference import compile_for_inference
    from atomnas_amd.models import mobilenet_supernet as ms
    tiny = dict(num_classes=10, input_size=64, input_channel=16, last_channel=64, width_mult=1.0, dropout_ratio=0.0, batch_norm_momentum=0.01,
                batch_norm_epsilon=1e-3, active_fn="nn.ReLU", inverted_residual_setting=[[1, 8, 1, 1, [3]], [6, 16, 2, 2, [3, 5, 7]]])
    model = ms.Model(**tiny)
    with pytest.raises(ValueError, match="eval"):
        compile_for_inference(model.train())
    model.eval()
    with pytest.raises(_lib.AtomnasHipError, match="GPU"):
        compile_for_inference(model)
    model.set_compute_dtype(torch.float32)
    with pytest.raises(ValueError, match="bf16"):
        compile_for_inference(model)
    with pytest.raises(TypeError):
        compile_for_inference(torch.nn.Linear(2, 2).eval())
    with pytest.raises(ValueError, match="batch_size"):
        compile_for_inference(model.set_compute_dtype(torch.bfloat16), use_graph=True)


def test_fused_inference_flag_defaults_to_off(monkeypatch):
    """`fused_inference` absent: train.eval_net hands back the model itself (nothing of the inference path is imported or run)"""
    import train
    from atomnas_amd.utils import config as cfg
    monkeypatch.setenv("ATOMNAS_E2E_DIR", "/nonexistent")
    cfg.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_search.yml")])
    sentinel = object()
    assert train.eval_net(sentinel) is sentinel
    F = cfg.load_app(["app:" + os.path.join(ROOT, "tests", "data", "tiny_search.yml")])
    F["fused_inference"] = True
    with pytest.raises(TypeError, match="compile_for_inference takes"):
        train.eval_net(torch.nn.Linear(2, 2).eval())
