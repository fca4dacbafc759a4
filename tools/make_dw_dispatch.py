#!/usr/bin/env python
"""Writes tests/golden/dw_dispatch.json: which depthwise kernel family the library takes, shape by shape.

Every row is a shape (N, H, W, C, k, stride, storage type) with the answers of atomnas_dwconv_mm_supported and
atomnas_dwconv_cw_supported for the forward and the backward.  tests/test_dw_dispatch_gpu.py asserts the library under test against
the table, so the table PINS a dispatch: generate it from the library whose behaviour is to be kept (ATOMNAS_HIP_LIB=<that build>),
never from the code under change, and with the ATOMNAS_DW_* switches unset.  Rows:

  * every depthwise launch of the training step (tests/golden/bench_shapes.json), in both storage types;
  * the small shapes at which one family hands over to the next, for k = 3, 5, 7 and both strides: CW_SHAPES / CW2_SHAPES of
    tests/test_kernels_gpu.py and EDGE_SHAPES below.

    python tools/make_dw_dispatch.py [out.json]        (GPU box: the LDS limit is queried from the device; predicate calls only)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (N, C, H, W)
EDGE_SHAPES = [(2, 16, 12, 12),    # width not a multiple of 7: no channel-pair geometry
               (1, 16, 8, 119),    # 17 strips per row: more than the 16 a tile row holds
               (1, 16, 70, 14),    # row-ring tiles (H * strips = 140 > 64, at most 32 rows each): three tiles of 24 rows, an even height
               (1, 16, 62, 14),    # row-ring tiles of an ODD height (two of 31 rows): no row pairs for the matrix cores
               (4, 32, 28, 28),    # small map: the stride-2 k = 3 forward stays on the tile kernels
               (8, 32, 14, 14)]    # whole-image tiles: the k = 7 backward stays on the packed-FMA rows


def shapes():
    from test_kernels_gpu import CW_SHAPES, CW2_SHAPES
    out = []
    for r in json.load(open(os.path.join(ROOT, "tests", "golden", "bench_shapes.json"))):
        if r["entry"] in ("dwconv_fwd", "dwconv_bwd"):
            out.append((r["N"], r["H"], r["W"], r["C"], r["k"], r["stride"]))
    for (N, C, H, W) in list(CW_SHAPES) + list(CW2_SHAPES) + EDGE_SHAPES:
        out += [(N, H, W, C, k, s) for k in (3, 5, 7) for s in (1, 2)]
    return sorted(set(out))


def answers(lib, N, H, W, C, k, stride, dt):
    """[mm forward, mm backward, cw forward, cw backward]"""
    return [int(f(N, H, W, C, k, stride, dt, d)) for f in (lib.atomnas_dwconv_mm_supported, lib.atomnas_dwconv_cw_supported) for d in (0, 1)]


def main():
    from atomnas_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "dw_dispatch.json")
    assert not [v for v in os.environ if v.startswith("ATOMNAS_DW_")], "unset the ATOMNAS_DW_* switches: the table pins the defaults"
    lib = _lib.load()
    rows = []
    for (N, H, W, C, k, s) in shapes():
        for dt in (0, 1):
            mf, mb, cf, cb = answers(lib, N, H, W, C, k, s, dt)
            rows.append(dict(N=N, H=H, W=W, C=C, k=k, stride=s, dt=dt, mm=[mf, mb], cw=[cf, cb]))
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n")
    print("%d rows (%d mm forward, %d mm backward, %d cw forward, %d cw backward) from %s -> %s" % (
        len(rows), sum(r["mm"][0] for r in rows), sum(r["mm"][1] for r in rows), sum(r["cw"][0] for r in rows),
        sum(r["cw"][1] for r in rows), _lib.LIB_PATH, out))


if __name__ == "__main__":
    main()
