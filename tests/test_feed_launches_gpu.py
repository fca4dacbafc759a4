"""DevicePrefetcher (GPU): what atomnas_amd/utils/dataflow.py launches for each form of a batch, with which tables, and what comes out.

tests/golden/feed_launches.json (tools/make_feed_launches.py, generated from dataflow.py BEFORE the prefetcher was restructured
around batch_plan and the slot object) holds, for the synthetic loader with both filters, four fixed batches (colour with a two-pass
crop box, plain, window with a two-pass image, the first again into a used slot), their staged forms, a resident batch and four
refused batches: every launch with its sizes, modes, slot list and the SHA-1 of the device tables it was given, the SHA-1 of every
(x, y) handed out, and the refusals.  The kernels are integer resamplers followed by a fixed fp32 normalise, so equal tables on
equal pixels give equal bytes: the digests are an equality.  A difference means the prefetcher changed what a batch launches: find the
change and fix the code, never regenerate the table from the code under change.

The cases run in one child interpreter with the caller's ATOMNAS_* variables stripped."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import make_feed_launches as gen  # noqa: E402

HEADER, TABLE = gen.load()
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def child(gpu_lib):
    got = gen.in_child(timeout=120)
    assert [r["name"] for r in got["cases"]] == [r["name"] for r in TABLE] and got["header"]["size"] == HEADER["size"]
    return got["cases"]


def test_launches_and_tables_match_the_pinned_table(child):
    """every launch in order: entry, n or m, size, out_mode, filter, max_rows, the selected slots, both table digests"""
    bad = [(w["name"], len(g["calls"]), len(w["calls"]), next(((i, x, y) for i, (x, y) in enumerate(zip(g["calls"], w["calls"])) if x != y), None))
           for g, w in zip(child, TABLE) if g["calls"] != w["calls"]]
    assert not bad, "(case, calls got, calls pinned, first difference (index, got, pinned)): %s" % bad[:3]


def test_outputs_match_the_pinned_table(child):
    """every (x, y) handed out, bit for bit"""
    bad = [(w["name"], [i for i, (x, y) in enumerate(zip(g["outputs"], w["outputs"])) if x != y], len(g["outputs"]), len(w["outputs"]))
           for g, w in zip(child, TABLE) if g["outputs"] != w["outputs"]]
    assert not bad, "(case, batches whose bytes differ, batches got, batches pinned): %s" % bad


def test_refusals_match_the_pinned_table(child):
    assert [(g["name"], g["error"]) for g in child] == [(w["name"], w["error"]) for w in TABLE]
