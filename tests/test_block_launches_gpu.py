"""Block executors (GPU): what atomnas_amd/functional.py launches for each form of a block's backward, and what comes out.

tests/golden/block_launches.json (tools/make_block_launches.py, generated from functional.py BEFORE block_backward was restructured
around project_bwd_form / expand_bwd_form) holds, for the smallest shapes at which each form of the projection backward (fused / dp /
prologue) and of the expand backward (noe_fused / noe_segments / noe_gemms / e) is taken, for the fused block with and without its
SqueezeAndExcitation in both weight-gradient forms, for the tiny network, the stand-alone SE and an eval-mode forward: the ordered
library calls, the ordered rows of the launch recorder, and the SHA-1 of every result.  The kernels are bit-reproducible
(tests/test_determinism_gpu.py), so equal launches give equal digests, and a difference means the executors changed what a step
launches: find the change and fix the code, never regenerate the table from the code under change.

The cases run in one child interpreter with the caller's ATOMNAS_* variables stripped (the library and functional.py read their
switches once per process).
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_block_launches as gen  # noqa: E402

HEADER, TABLE = gen.load()


def test_table_has_every_case_and_every_form():
    """(no GPU needed) the committed table has the generator's cases in the generator's order, every one of the seven forms was taken
    by the case that lists it, and the launches that tell the forms apart are where the generator's self-checks expect them"""
    gen.check(TABLE)
    assert all(r["calls"] and r["digests"] and all(len(v) == 40 for v in r["digests"].values()) for r in TABLE)
    assert [r["name"] for r in TABLE if not r["rows"]] == ["standalone_se_bf16"]   # the launch recorder does not cover the SE entries
    assert HEADER["cus"] > 0 and HEADER["device"]


@pytest.fixture(scope="module")
def child(gpu_lib):
    return gen.in_child(timeout=240)


def _first_difference(a, b):
    return next(((i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y), (min(len(a), len(b)), "<end>", "<end>"))


@pytest.mark.gpu
def test_library_calls_match_the_pinned_table(child):
    """(a) the ordered entry-point names of every library call, every case"""
    bad = [(w["name"], len(g["calls"]), len(w["calls"]), _first_difference(g["calls"], w["calls"]))
           for g, w in zip(child["cases"], TABLE) if g["calls"] != w["calls"]]
    assert len(child["cases"]) == len(TABLE) and not bad, "(case, calls got, calls pinned, first difference (index, got, pinned)): %s" % bad[:4]


@pytest.mark.gpu
def test_recorder_rows_match_the_pinned_table(child):
    """(b) the ordered rows of the launch recorder, every case"""
    bad = [(w["name"], len(g["rows"]), len(w["rows"]), _first_difference(g["rows"], w["rows"]))
           for g, w in zip(child["cases"], TABLE) if g["rows"] != w["rows"]]
    assert len(child["cases"]) == len(TABLE) and not bad, "(case, rows got, rows pinned, first difference (index, got, pinned)): %s" % bad[:4]


@pytest.mark.gpu
def test_result_digests_match_the_pinned_table(child):
    """(c) output, input gradient, parameter gradients and buffers bit for bit, on the device the table was written on"""
    if child["header"]["cus"] != HEADER["cus"]:
        pytest.skip("the digests are for %s (%d CUs): the grids are sized from the CU count, this device has %d"
                    % (HEADER["device"], HEADER["cus"], child["header"]["cus"]))
    bad = [(w["name"], sorted(k for k in set(g["digests"]) | set(w["digests"]) if g["digests"].get(k) != w["digests"].get(k)))
           for g, w in zip(child["cases"], TABLE) if g["digests"] != w["digests"]]
    assert len(child["cases"]) == len(TABLE) and not bad, "(case, tensors whose bytes differ): %s" % bad[:4]
