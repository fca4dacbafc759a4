"""Weight-gradient dispatch (GPU): which kernel family, instance and row chunks the host path of csrc/pwconv_tn.hip takes for a shape.

tests/golden/tn_dispatch.json (tools/make_tn_dispatch.py, generated from the library BEFORE the host code was restructured around one
argument block and one plan per family) holds, for the smallest shapes on both sides of every hand-over (dma -> slab for bf16,
generic for fp32), the SHA-1 of what ONE ops.gemm_tn call wrote: `out` and the WHOLE caller-owned workspace (pre-filled with NaN).
atomnas_pw_gemm_tn has no query; the workspace is the observable a host change moves: how many partials are written, which rows each
covers and whether ws is touched at all.  The kernels are bit-reproducible (tests/test_determinism_gpu.py), so equal digests mean the
same decision and a difference means a changed one: find the predicate and fix the code, never regenerate the table from the code
under change.  A second column is taken with ATOMNAS_TN_DMA=0; the library reads the switch once per process, so every setting runs
in a child interpreter with the caller's ATOMNAS_TN_* variables stripped.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import make_tn_dispatch as gen  # noqa: E402
from test_pw_dispatch_gpu import _assert_rows, whole_chip  # noqa: E402,F401

TABLE = json.load(open(os.path.join(HERE, "golden", "tn_dispatch.json")))
DIGESTS = ("out", "ws_sha", "out_dma0", "ws_sha_dma0")


def test_table_has_every_row_the_generator_writes():
    """(no GPU needed) the committed rows are the generator's rows in the generator's order (the row index seeds the inputs), every
    digest is present, all three families occur, and the rows that ATOMNAS_TN_DMA=0 moves are the ones recorded with the table: tn3
    rows only, and at least one (where tn3 and tn2 happen to chunk alike the two columns may agree)"""
    rows = TABLE["gemm_tn"]
    assert [{k: v for k, v in r.items() if k not in DIGESTS} for r in rows] == gen.tn_rows()
    assert all(isinstance(r[k], str) and len(r[k]) == 40 for r in rows for k in DIGESTS)
    assert {r["family"] for r in rows} == {"tn3", "tn2", "generic"}
    moved = [i for i, r in enumerate(rows) if (r["out"], r["ws_sha"]) != (r["out_dma0"], r["ws_sha_dma0"])]
    assert moved and moved == TABLE["moved"]
    assert all(rows[i]["family"] == "tn3" for i in moved)


@pytest.mark.gpu
def test_default_dispatch_matches_the_pinned_table(whole_chip):
    _assert_rows("gemm_tn", gen.answer("default"), ("out", "ws_sha"), TABLE)


@pytest.mark.gpu
def test_dispatch_with_the_dma_family_switched_off(whole_chip):
    """ATOMNAS_TN_DMA=0: the tn3 rows fall through to k_gemm_tn2"""
    _assert_rows("gemm_tn", gen.answer("dma0"), ("out_dma0", "ws_sha_dma0"), TABLE)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [0, 1])
def test_unsupported_prologue_pair_raises(gpu_lib, dt):
    """(BNRELU, BNRELU) is none of the six pairs the kernels are instantiated for: an error for both storage types, no launch"""
    from atomnas_amd._lib import AtomnasHipError
    m = gen.Maker(0, dt)
    M, NU, NV = 256, 40, 72
    kw = dict(gen.prologue(m, "u", gen.PRO_BNRELU, M, NU, "plain"), **gen.prologue(m, "v", gen.PRO_BNRELU, M, NV, "plain"))
    out = m.torch.zeros(NU, NV, dtype=m.torch.float32, device="cuda")
    with pytest.raises(AtomnasHipError, match="unsupported prologue pair"):
        m.ops.gemm_tn(m.act(M, NU, "plain"), NU, m.act(M, NV, "plain"), NV, out, NV, 1, M, **kw)
