"""Envelope of the fused block kernel WITH Squeeze-and-Excitation, without a GPU: atomnas_block_infer_se_runs / _supported are pure host
predicates (csrc/block_infer.hip bi_plan).  The kernel takes an SE block only where one workgroup owns the whole map: stride 1,
expanding, at most 256 output pixels; the predicates of atomnas_block_infer (no SE operands) keep refusing every SE block."""
import pytest
import torch

BF16 = torch.bfloat16
# a 14 x 14 stride-1 block of the kind the searched "+" networks have: the edges below change one thing at a time
BASE = dict(N=256, H=14, W=14, inp=80, oup=80, seg_off=[0, 48, 112], seg_ch=[48, 64, 80], seg_k=[3, 5, 7], stride=1, act=3, expand=True,
            residual=True, se_hid=40)


@pytest.fixture(scope="module")
def ops():
    from atomnas_amd import build, ops
    build.build_library()
    return ops


@pytest.fixture(scope="module")
def cplus_shapes():
    from atomnas_amd import configs
    from atomnas_amd.inference import block_shapes
    from atomnas_amd.models import searched_network as sn
    return block_shapes(sn.Model(**dict(configs.searched_kwparams("atomnas_c_plus"), input_size=224)), 256)


def _whole_map(s):
    """the rule of the issue, from the shape alone"""
    Ho, Wo = (s["H"] - 1) // s["stride"] + 1, (s["W"] - 1) // s["stride"] + 1
    return s["stride"] == 1 and s["expand"] and Ho * Wo <= 256


def test_atomnas_c_plus_blocks_with_a_whole_map_are_inside(ops, cplus_shapes):
    assert len(cplus_shapes) == 22 and all(s["se"] and s["se_hid"] >= 1 for _, s in cplus_shapes)
    want = [n for n, s in cplus_shapes if _whole_map(s)]
    assert len(want) == 11
    got = [n for n, s in cplus_shapes if ops.block_infer_se_supported(dtype=BF16, profitable=False, **s)]
    assert got == want
    # atomnas_block_infer has no SE operands: its predicates refuse all 22, as before
    assert not any(ops.block_infer_supported(s["N"], s["H"], s["W"], s["inp"], s["oup"], s["seg_off"], s["seg_ch"], s["seg_k"], s["stride"],
                                             s["act"], s["expand"], s["residual"], True, BF16, profitable=False) for _, s in cplus_shapes)
    assert not any(ops.block_infer_supported(dtype=BF16, profitable=prof, **s) for _, s in cplus_shapes for prof in (False, True))


def test_block_shapes_keeps_its_keys_and_adds_se_hid(cplus_shapes):
    from atomnas_amd import configs
    from atomnas_amd.inference import block_shapes
    from atomnas_amd.models import searched_network as sn
    keys = {"N", "H", "W", "inp", "oup", "seg_off", "seg_ch", "seg_k", "stride", "act", "expand", "residual", "se", "se_hid"}
    assert all(set(s) == keys for _, s in cplus_shapes)
    assert [s["se_hid"] for _, s in cplus_shapes] == [int(round(s["inp"] * 0.5)) for _, s in cplus_shapes]   # se_ratio 0.5 of the block's input
    plain = block_shapes(sn.Model(**dict(configs.searched_kwparams("atomnas_c"), input_size=224)), 256)
    assert all(set(s) == keys and not s["se"] and s["se_hid"] == 0 for _, s in plain)


def _runs(ops, **change):
    return ops.block_infer_se_supported(dtype=change.pop("dtype", BF16), profitable=False, **dict(BASE, **change))


def test_edges_of_the_envelope(ops):
    assert _runs(ops)
    # the largest whole map is 256 pixels (k <= 5: with the 7 x 7 halo, 80 input channels and a 16 x 16 map it is the LDS that refuses)
    assert _runs(ops, H=16, W=16, seg_k=[3, 5, 5])
    assert not _runs(ops, H=17, W=16, seg_k=[3, 5, 5])
    assert not _runs(ops, H=16, W=16) and _runs(ops, H=16, W=16, inp=24, oup=24, se_hid=12)
    # stride 2 and a block without the expand stage stay on the existing path
    assert not _runs(ops, stride=2, residual=False)
    assert not _runs(ops, expand=False, inp=192, seg_off=[0, 48, 112], seg_ch=[48, 64, 80])
    assert ops.block_infer_supported(256, 14, 14, 192, 80, [0, 48, 112], [48, 64, 80], [3, 5, 7], 1, 3, False, False, False, BF16, profitable=False)
    # the gate's hidden units: 1 .. 512
    assert not _runs(ops, se_hid=0) and _runs(ops, se_hid=1) and _runs(ops, se_hid=512) and not _runs(ops, se_hid=513)
    # padded hidden channels: up to 4096 (a 7 x 7 map, so that LDS is not what refuses)
    wide = dict(H=7, W=7, seg_off=[0, 2048], seg_k=[3, 5])
    assert _runs(ops, seg_ch=[2048, 2048], **wide)
    assert not _runs(ops, seg_ch=[2048, 2064], **wide)
    assert ops.block_infer_supported(256, 7, 7, 80, 80, [0, 2048], [2048, 2064], [3, 5], 1, 3, True, True, False, BF16, profitable=False)   # SE alone refuses it
    # bf16 storage only
    assert not _runs(ops, dtype=torch.float32)
    # what the plain envelope refuses is refused here as well
    assert not _runs(ops, seg_k=[3, 4, 7]) and not _runs(ops, stride=3, residual=False) and not _runs(ops, inp=81)
    assert not ops.block_infer_se_supported(256, 14, 14, 80, 80, [], [], [], 1, 3, True, True, 40, BF16, profitable=False)
    # a block without SE is not this entry's
    assert not ops.block_infer_se_supported(dtype=BF16, profitable=False, **dict(BASE, se=False))


def test_profitable_implies_runs(ops, cplus_shapes):
    tried = [s for _, s in cplus_shapes] + [dict(s, N=n) for _, s in cplus_shapes for n in (1, 8)]
    tried += [dict(BASE, se=True, **c) for c in (dict(), dict(H=16, W=16), dict(H=17, W=16), dict(H=7, W=7), dict(N=1), dict(se_hid=513))]
    for s in tried:
        if ops.block_infer_se_supported(dtype=BF16, profitable=True, **s):
            assert ops.block_infer_se_supported(dtype=BF16, profitable=False, **s), s


def test_measured_policy_on_atomnas_c_plus(ops, cplus_shapes):
    """atomnas_block_infer_se_supported: the 14 x 14 blocks of up to 192 padded hidden channels, up to batch 64, measured faster
    (profiles/infer_bench_se.txt); the wide block 14, the 7 x 7 stage and the batches at which the whole network measured
    slower (128, 256) stay on the existing path"""
    for n_img in (1, 8, 64):
        got = [n for n, s in cplus_shapes if ops.block_infer_se_supported(dtype=BF16, **dict(s, N=n_img))]
        assert got == ["11", "12", "13", "15", "16", "17"], (n_img, got)
    for n_img in (65, 128, 256):
        assert not any(ops.block_infer_se_supported(dtype=BF16, **dict(s, N=n_img)) for _, s in cplus_shapes)


def test_the_symbols_are_bound(ops):
    from atomnas_amd import _lib
    assert "atomnas_block_infer_se" in _lib.SIGNATURES
    assert "atomnas_block_infer_se_runs" in _lib.NO_STATUS and "atomnas_block_infer_se_supported" in _lib.NO_STATUS
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ("atomnas_block_infer_se", "atomnas_block_infer_se_runs", "atomnas_block_infer_se_supported"))
    assert _lib.ABI_VERSION == 9
