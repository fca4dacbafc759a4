"""Pointwise dispatch (GPU): which kernel family, instance and grid the host path of csrc/pwconv.hip takes for a shape.

tests/golden/pw_dispatch.json (tools/make_pw_dispatch.py, generated from the library BEFORE the host code was restructured around one
argument block and one plan per family) holds, for the smallest shapes on both sides of every hand-over of launch_nt
(sw -> swg -> st -> small -> ws -> generic), the SHA-1 of what ONE ops.gemm_nt call wrote: the output bytes and the WHOLE statistics
buffer (rows pre-filled with NaN, stat_rows = ops.stat_rows_for(N)).  atomnas_pw_gemm_nt has no query that names its choice; the
statistics buffer is the observable a host change moves, because its layout depends on the family and on its grid: which partial rows
are written, which are zero-filled and which sums land in which row.  The output digest alone would not see a changed grid.  The
kernels are bit-reproducible (tests/test_determinism_gpu.py), so equal digests mean the same decision and a difference means a changed
one: find the predicate and fix the code, never regenerate the table from the code under change.

Also pinned: the answers of atomnas_expand_bwd_supported and atomnas_project_bwd_dp_supported, the outputs of ops.expand_bwd on both
sides of its streaming hand-over (again with ATOMNAS_XB_STREAM=0) and of ops.project_bwd for every accumulator width, and a second
column of gemm_nt digests taken with ATOMNAS_NT_SW=0 ATOMNAS_NT_SWG=0 ATOMNAS_NT_ST=0.  The library reads its switches once per
process: every setting runs in a child interpreter with the caller's ATOMNAS_NT_* / ATOMNAS_XB_* variables stripped.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_pw_dispatch as gen  # noqa: E402

TABLE = json.load(open(os.path.join(HERE, "golden", "pw_dispatch.json")))


def _spec(rows, recorded):
    return [{k: v for k, v in r.items() if k not in recorded} for r in rows]


def test_table_has_every_row_the_generator_writes():
    """(no GPU needed) section by section, the committed rows are the generator's rows in the generator's order (the row index seeds
    the inputs), every recorded value is present, and the switches-off column differs where a switched-off family served the row"""
    assert _spec(TABLE["gemm_nt"], ("out", "stats", "out_off", "stats_off")) == gen.nt_rows()
    assert _spec(TABLE["expand_bwd_supported"], ("ok",)) == gen.xb_query_rows()
    assert _spec(TABLE["project_bwd_dp_supported"], ("ok",)) == gen.pb_query_rows()
    assert _spec(TABLE["expand_bwd"], ("gx", "dwe", "gx_xs0", "dwe_xs0")) == gen.xb_rows()
    assert _spec(TABLE["project_bwd"], ("gh", "stats", "dwp")) == gen.pb_rows()
    sha = lambda r, keys: all(isinstance(r[k], str) and len(r[k]) == 40 for k in keys)
    assert all(sha(r, ("out", "stats", "out_off", "stats_off")) for r in TABLE["gemm_nt"])
    assert all(sha(r, ("gx", "dwe", "gx_xs0", "dwe_xs0")) for r in TABLE["expand_bwd"])
    assert all(sha(r, ("gh", "stats", "dwp")) for r in TABLE["project_bwd"])
    assert {r["family"] for r in TABLE["gemm_nt"]} == {"sw", "swg", "st", "small", "ws", "generic"}
    # a table whose two columns agree everywhere would pin no switch: the st rows and the wide-stage swg row move their statistics when
    # the families are off (the sw rows and the 64-row-stage swg rows do not: at these sizes k_gemm_nt_ws walks the same 64-row blocks
    # in the same number of row slots and adds in the same order), the rows of the other families never see the switches
    moved = {r["family"] for r in TABLE["gemm_nt"] if (r["out"], r["stats"]) != (r["out_off"], r["stats_off"])}
    assert moved == {"swg", "st"}
    # both answers occur in each query
    assert {r["ok"] for r in TABLE["expand_bwd_supported"]} == {0, 1} and {r["ok"] for r in TABLE["project_bwd_dp_supported"]} == {0, 1}


@pytest.fixture(scope="module")
def whole_chip(gpu_lib):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip("the table is for a whole MI355X (256 CUs): the grids are sized from the CU count, this device has %d" % cus)


def _assert_rows(section, got, keys, table=TABLE):
    rows = table[section]
    assert len(got) == len(rows)
    bad = [(i, {k: v for k, v in r.items() if len(str(v)) < 40}, [k for k, g in zip(keys, a) if r[k] != g])
           for i, (r, a) in enumerate(zip(rows, got)) if [r[k] for k in keys] != list(a)]
    assert not bad, "%s: %d of %d rows differ from the pinned table (row index, row, differing digests), first %s" % (
        section, len(bad), len(rows), bad[:4])


@pytest.mark.gpu
def test_default_dispatch_matches_the_pinned_table(whole_chip):
    """gemm_nt digests, both queries, expand_bwd and project_bwd digests with every switch at its default"""
    got = gen.in_child("default")
    _assert_rows("gemm_nt", got["gemm_nt"], ("out", "stats"))
    _assert_rows("expand_bwd_supported", [[a] for a in got["expand_bwd_supported"]], ("ok",))
    _assert_rows("project_bwd_dp_supported", [[a] for a in got["project_bwd_dp_supported"]], ("ok",))
    _assert_rows("expand_bwd", got["expand_bwd"], ("gx", "dwe"))
    _assert_rows("project_bwd", got["project_bwd"], ("gh", "stats", "dwp"))


@pytest.mark.gpu
def test_dispatch_with_the_streaming_families_switched_off(whole_chip):
    """ATOMNAS_NT_SW=0 ATOMNAS_NT_SWG=0 ATOMNAS_NT_ST=0: the rows of those families fall through to small / ws / generic"""
    _assert_rows("gemm_nt", gen.in_child("off")["gemm_nt"], ("out_off", "stats_off"))


@pytest.mark.gpu
def test_expand_bwd_with_the_streaming_kernel_switched_off(whole_chip):
    """ATOMNAS_XB_STREAM=0: every shape on k_expand_bwd"""
    _assert_rows("expand_bwd", gen.in_child("xs0")["expand_bwd"], ("gx_xs0", "dwe_xs0"))
