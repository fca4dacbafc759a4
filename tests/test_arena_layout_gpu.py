"""Arena layout (GPU): what ArenaManager.materialize builds, read back from the arenas, against tests/golden/arena_layout.json.

Every small case of tools/make_arena_layout.py (the tiny network without an optimizer, with RMSprop + EMA, with momentum-free SGD, with
changed blocks and after a real shrink; the fused networks; the stand-alone modules) is materialised as the generator did and its
whole record -- arena sizes, which optimizer arenas exist, slots, decoded job tables, fold jobs, and every plan attribute with the arena,
offset, shape, stride and dtype of every view -- must equal the table, which was written from the runtime.py before its layout became
runtime.arena_layout.  No forward is run; the full-size models are held by tests/test_arena_layout.py on the CPU.
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_arena_layout as gen  # noqa: E402

pytestmark = pytest.mark.gpu

HEADER, TABLE = gen.load()
CASES = [c for c in gen.cases() if not c.get("full")]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_materialized_arenas_match_table(gpu_lib, case):
    sys.path.insert(0, ROOT)   # the shrunk case goes through train.shrink_model
    model, mgr = gen.materialize(case)
    got, want = gen.record(model, mgr), TABLE[case["name"]]
    assert sorted(got) == sorted(k for k in want if k != "name")
    for key in got:
        if key != "plans":
            assert got[key] == want[key], key
    assert [n for n, _ in got["plans"]] == [n for n, _ in want["plans"]]
    for (name, g), (_, w) in zip(got["plans"], want["plans"]):
        assert sorted(g) == sorted(w), (name, sorted(set(g) ^ set(w)))
        for k in w:
            assert g[k] == w[k], (name, k, g[k], w[k])
