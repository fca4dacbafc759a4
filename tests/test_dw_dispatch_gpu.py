"""Depthwise dispatch (GPU, predicate calls only -- no kernel is launched): which kernel family the library takes for a shape.

tests/golden/dw_dispatch.json (tools/make_dw_dispatch.py, generated from the library BEFORE the host code was restructured around one
plan per launch) holds the answers of atomnas_dwconv_mm_supported and atomnas_dwconv_cw_supported, forward and backward, for every
depthwise launch of the training step and for the small shapes at which one family hands over to the next, in both storage types.
The queries and the entry points share one decision (csrc/dwconv.hip dw_pick and the <family>_plan functions under it), so a change of
the dispatch shows here; the parity tests take their bf16 rounding model from the first query (tests/kutil.py).
"""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROWS = json.load(open(os.path.join(HERE, "golden", "dw_dispatch.json")))


def ask(lib):
    """[[mm forward, mm backward, cw forward, cw backward]] in row order"""
    return [[int(f(r["N"], r["H"], r["W"], r["C"], r["k"], r["stride"], r["dt"], d))
             for f in (lib.atomnas_dwconv_mm_supported, lib.atomnas_dwconv_cw_supported) for d in (0, 1)] for r in ROWS]


def _assert_equal(got, want):
    bad = [(r, g, w) for r, g, w in zip(ROWS, got, want) if g != w]
    assert not bad, "%d of %d rows differ ([mm fwd, mm bwd, cw fwd, cw bwd] got / want), first %s" % (len(bad), len(ROWS), bad[:3])


def test_table_covers_the_step_and_the_hand_over_shapes():
    """(no GPU needed) the committed table has every row the generator would write, and every family and hand-over shows in it"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_dw_dispatch
    have = {(r["N"], r["H"], r["W"], r["C"], r["k"], r["stride"], r["dt"]) for r in ROWS}
    want = {s + (dt,) for s in make_dw_dispatch.shapes() for dt in (0, 1)}
    assert want <= have, sorted(want - have)[:5]
    bench = [r for r in json.load(open(os.path.join(HERE, "golden", "bench_shapes.json"))) if r["entry"] in ("dwconv_fwd", "dwconv_bwd")]
    assert len(bench) == 58 and all((r["N"], r["H"], r["W"], r["C"], r["k"], r["stride"], r["dt"]) in have for r in bench)
    # every family and every hand-over is present: a table of zeros would pin nothing
    col = lambda i: {(r["stride"], r["dt"], r["k"]) for r in ROWS if (r["mm"] + r["cw"])[i]}
    assert col(0) >= {(1, 1, 5), (1, 1, 7), (2, 1, 3), (2, 1, 5), (2, 1, 7)} and not any(dt == 0 for _, dt, _ in col(0))
    assert col(1) == {(1, 1, 7)}
    assert {s for s, _, _ in col(2)} == {1} and {s for s, _, _ in col(3)} == {1, 2}
    edge = {(r["H"], r["W"], r["k"], r["stride"]): r for r in ROWS if r["dt"] == 1 and (r["N"], r["C"]) in ((2, 16), (1, 16), (4, 32), (8, 32))}
    assert edge[(12, 12, 5, 1)]["mm"] + edge[(12, 12, 5, 1)]["cw"] == [0, 0, 0, 0]      # width not a multiple of 7
    assert edge[(8, 119, 5, 1)]["mm"] + edge[(8, 119, 5, 1)]["cw"] == [0, 0, 0, 0]      # 17 strips
    assert edge[(70, 14, 7, 1)]["mm"] == [1, 1] and edge[(70, 14, 7, 1)]["cw"] == [1, 1]   # row ring, even tile height (3 x 24 rows)
    assert edge[(62, 14, 7, 1)]["mm"] == [0, 0] and edge[(62, 14, 7, 1)]["cw"] == [1, 1]   # row ring, odd tile height (2 x 31 rows)
    assert edge[(28, 28, 3, 2)]["mm"][0] == 0 and edge[(28, 28, 5, 2)]["mm"][0] == 1    # stride 2, k = 3 on a small map
    assert edge[(14, 14, 7, 1)]["mm"] == [1, 0] and edge[(14, 14, 7, 1)]["cw"][1] == 1  # backward k = 7 on a whole-image tile


def ask_in_child(**switches):
    """the answers of a fresh interpreter: the library reads the ATOMNAS_DW_* switches once per process, so the caller's own are
    stripped and only `switches` are set"""
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("ATOMNAS_DW_")}, **switches)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_queries_match_the_pinned_dispatch(gpu_lib):
    """the default dispatch, whatever switches the caller's environment carries"""
    _assert_equal(ask_in_child(), [r["mm"] + r["cw"] for r in ROWS])


@pytest.mark.gpu
def test_dw_mm_38_switches_only_the_stride2_forward_off(gpu_lib):
    """ATOMNAS_DW_MM's default is 166 = 38 + 128; 38 was the default of the stride-1 kernels alone, bit 7 (128) is the stride-2
    forward: with 38 exactly the stride-2 forward rows answer 0."""
    want = [[0 if r["stride"] == 2 else r["mm"][0], r["mm"][1]] + r["cw"] for r in ROWS]
    assert sum(r["mm"][0] for r in ROWS if r["stride"] == 2) > 0
    _assert_equal(ask_in_child(ATOMNAS_DW_MM="38"), want)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from atomnas_amd import _lib
    print(json.dumps(ask(_lib.load())))
