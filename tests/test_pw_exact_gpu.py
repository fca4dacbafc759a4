"""Pointwise kernels against exact integers (GPU): atomnas_pw_gemm_nt, atomnas_pw_gemm_tn, atomnas_gram / atomnas_xb_coeffs /
atomnas_expand_bwd and atomnas_project_bwd at the smallest shapes at which each kernel family and instance exists.

tests/exact_ref.py builds every case from small integers (tests/test_pw_exact.py shows, on the CPU, that every sum then stays below
2^24), so the fp32 accumulators, the partial rows of the statistics and the workspace partials hold exact integers and the comparison is
torch.equal: the output's valid region (the reference rounded ONCE to the storage type), zero padding columns, the statistics summed
over their partial rows in float64 against [sum c_stored, sum c_stored^2 or c_stored z], no NaN left in any statistics row, and
pre-fill + reference for the outputs that accumulate.  A mismatch is a finding in the kernel or its plan; it is never resolved by a
tolerance.

Swish twins (activation code 3, the same cases) are not exact.  Their outputs keep the project's bound of one output rounding,
kutil.tol(dtype) with the absolute part scaled by max|C| as test_gemm_nt scales it.  Their statistics are compared with the sums of the
STORED output, so the output's own rounding drops out and what is left is the kernel's fp32 summation of M terms per channel.  Every
fp32 addition rounds its result by at most 2^-24 of it (half an ulp).  The kernels add the 16 rows of a tile across lanes, then tile
after tile into a wave's row, then the waves' rows into a partial row; the partial rows are summed here in float64.  A term therefore
passes through few additions whose result is as large as the whole partial sum, and the partial sums of signed terms grow like
sqrt(M) max|term|, far below the worst case M max|term|: bounding every addition's result by M max|term| / (additions a term passes)
gives the absolute floor M 2^-24 max|term|.  rtol 1e-5 is for channels whose terms share a sign (sum c^2): there the sum itself is of
order M mean|term| and the roundings are relative to it, about 2^-24 per level of the reduction.
"""
import json
import os
import subprocess
import sys

import pytest

import exact_ref as X

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _id(r):
    return "-".join("%s%s" % (k, r[k]) for k in sorted(r) if r[k] not in (0, None, "plain") or k in ("M",))


def _run(fn, r):
    bad = fn(r)
    assert not bad, "%d mismatches, first: %s" % (len(bad), bad[0])


@pytest.fixture(scope="module")
def cus(gpu_lib):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("r", X.nt_cases() + X.nt_twins(), ids=_id)
def test_gemm_nt_exact(gpu_lib, cus, r):
    if r["whole_chip"] and cus != 256:
        pytest.skip("the eight-wave swg form needs 256 CUs ((M + 127) / 128 >= CUs), this device has %d" % cus)
    _run(X.run_nt, r)


@pytest.mark.parametrize("r", X.tn_cases() + X.tn_twins(), ids=_id)
def test_gemm_tn_exact(gpu_lib, r):
    _run(X.run_tn, r)


@pytest.mark.parametrize("r", X.xb_cases(), ids=_id)
def test_gram_xb_coeffs_expand_bwd_exact(gpu_lib, r):
    _run(X.run_xb, r)


@pytest.mark.parametrize("r", X.pb_cases() + X.pb_twins(), ids=_id)
def test_project_bwd_exact(gpu_lib, r):
    _run(X.run_pb, r)


def test_supported_queries_answer_both_ways(gpu_lib):
    import torch
    from atomnas_amd import ops
    for inp, hid, ok in X.XB_QUERIES:
        assert ops.expand_bwd_supported(inp, hid, torch.bfloat16) == bool(ok), (inp, hid)
    for r in X.pb_cases() + X.PB_QUERIES_NO:
        assert bool(gpu_lib.atomnas_project_bwd_dp_supported(*X.pb_query(r))) == X.pb_expected(r), r


def test_exact_with_the_streaming_families_switched_off(gpu_lib):
    """The gemm_nt and expand tables once more in ONE fresh interpreter with the sw / swg / st families and the streaming expand
    backward off (the library reads its switches once per process): the streaming shapes fall through to ws / generic / k_expand_bwd
    with their slab-major operands and must give the same exact answers."""
    env = {k: v for k, v in os.environ.items() if not k.startswith(("ATOMNAS_NT_", "ATOMNAS_XB_"))}
    env.update(ATOMNAS_NT_SW="0", ATOMNAS_NT_SWG="0", ATOMNAS_NT_ST="0", ATOMNAS_XB_STREAM="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "exact_ref.py"), "--child", "nt,xb"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-2000:]
    bad = json.loads(p.stdout.strip().splitlines()[-1])
    assert bad == [], "%d mismatches, first: %s" % (len(bad), bad[:3])
