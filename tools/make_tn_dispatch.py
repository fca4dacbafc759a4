#!/usr/bin/env python
"""Writes tests/golden/tn_dispatch.json: what the weight-gradient host path decides, shape by shape, as digests of what it writes.

atomnas_pw_gemm_tn has no query, so the observable is the caller's workspace: every row is ONE ops.gemm_tn call (outside any
reduce_defer window) on inputs made on the CPU (numpy.random.default_rng(row index), rounded to the storage type), with a caller-owned
ws pre-filled with NaN (ops.tn_workspace(NU, NV) floats unless the row says otherwise), and the row records the SHA-1 of `out` and of
the WHOLE ws.  How many partials are written, which rows each covers and whether ws is touched at all are exactly what the host
decides (csrc/pwconv_tn.hip, host side: dma -> slab for bf16, generic for fp32).  The rows are the smallest shapes on both sides of
every hand-over; a second pair of digests is taken with ATOMNAS_TN_DMA=0, and "moved" lists the rows whose two pairs differ.

tests/test_tn_dispatch_gpu.py asserts the library under test against the table, so the table PINS a dispatch: generate it from the
library whose behaviour is to be kept (ATOMNAS_HIP_LIB=<that build>), never from the code under change, on a whole MI355X (256 CUs:
the row chunks are sized from the CU count).  Both settings are run twice; the file is written only if the two runs agree.

    python tools/make_tn_dispatch.py [out.json]      (GPU box)
    python tools/make_tn_dispatch.py --emit MODE     (what a child prints: MODE = default | dma0)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_pw_dispatch import PRO_BNBWD, PRO_BNRELU, PRO_NONE, Maker, in_child, sha  # noqa: E402

MODES = {"default": {}, "dma0": {"ATOMNAS_TN_DMA": "0"}}
PAIRS = [(PRO_NONE, PRO_NONE), (PRO_NONE, PRO_BNBWD), (PRO_BNBWD, PRO_BNRELU), (PRO_BNRELU, PRO_BNBWD), (PRO_BNBWD, PRO_NONE),
         (PRO_NONE, PRO_BNRELU)]   # the supported prologue pairs (u_mode, v_mode)


def _tn(family, M, NU, NV, **kw):
    """family: the kernel family that serves the row with every switch at its default.  ws: "auto" = ops.tn_workspace(NU, NV),
    "none" = ws=False, an integer = that many partials of NU * NV floats.  t: transposed output (si = 1, sj = NU)"""
    r = dict(family=family, M=M, NU=NU, NV=NV, dt=1, u_mode=PRO_NONE, v_mode=PRO_NONE, v="plain", t=0, ws="auto")
    r.update(kw)
    return r


def tn_rows():
    """the rows, in table order (the row index seeds the inputs)"""
    rows = []
    relu = dict(v_mode=PRO_BNRELU)
    # tn3 (k_gemm_tn3): U plain, V none / BNRELU, NU >= 32, NV >= 256, M >= 1024, a workspace for >= 8 row chunks
    rows.append(_tn("tn3", 1024, 32, 256, **relu))                       # accept edge: 8 chunks of 128 rows
    for s in [(1023, 32, 256), (1024, 24, 256), (1024, 32, 248)]:        # decline edges
        rows.append(_tn("tn2", *s, **relu))
    rows.append(_tn("tn3", 1024, 32, 256))
    rows.append(_tn("tn2", 1024, 32, 256, v_mode=PRO_BNBWD))
    rows.append(_tn("tn2", 1024, 32, 256, u_mode=PRO_BNBWD, v_mode=PRO_BNRELU))
    rows.append(_tn("tn2", 1024, 32, 256, ws="none", **relu))
    rows.append(_tn("tn2", 1024, 32, 256, ws=7, **relu))                # fewer than 8 partials
    for nu in (64, 72, 96, 104, 192, 200, 320):                          # UTT buckets 4 | 6 | 12 | 10
        rows.append(_tn("tn3", 1024, nu, 256, **relu))
    rows.append(_tn("tn2", 1024, 328, 256, **relu))                     # past 320: k_gemm_tn2<..., 20, ...>
    rows.append(_tn("tn3", 1024, 32, 256, v="slab", **relu))
    rows.append(_tn("tn3", 1024, 32, 256, t=1, **relu))
    # the binding cap on the chunk count: residency (two U tiles x two V tiles, two workgroups per CU: 128 < M / 128 = 257 < 256
    # partials; a ragged M, so that the rounding to whole 32-row stages shows), M / 128 (23 -> 16), the workspace (16 < 32)
    rows.append(_tn("tn3", 33000, 200, 256, **relu))
    rows.append(_tn("tn3", 3000, 64, 256, **relu))
    rows.append(_tn("tn3", 4096, 64, 256, ws=16, **relu))
    # tn2 (k_gemm_tn2), V with the BatchNorm-backward prologue so that tn3 never takes the row: UTT buckets 2 | 4 | 6 | 12 | 10 | 20
    bwd = dict(v_mode=PRO_BNBWD)
    for nu in (32, 40, 64, 72, 96, 104, 192, 200, 320, 328):
        rows.append(_tn("tn2", 2048, nu, 256, **bwd))
    rows.append(_tn("tn2", 2048, 64, 248, **bwd))                       # <UTT, 1, 128> instead of the wide V tile <UTT, 2, 64>
    for s in [(1024, 64, 256), (1023, 64, 256), (2047, 64, 248)]:        # XCD order from 8 chunks on (2048, 64, 248 is above)
        rows.append(_tn("tn2", *s, **bwd))
    for um, vm in PAIRS:                                                 # tn3 serves the two pairs it can
        rows.append(_tn("tn3" if um == PRO_NONE and vm != PRO_BNBWD else "tn2", 2048, 64, 256, u_mode=um, v_mode=vm))
    rows.append(_tn("tn2", 2048, 64, 256, v="slab", **bwd))
    rows.append(_tn("tn2", 2048, 64, 256, t=1, **bwd))
    rows.append(_tn("tn2", 2048, 64, 256, ws="none", **bwd))
    # generic (k_gemm_tn, fp32): two chunks, one chunk (direct accumulation, ws untouched), one | two U tiles, no workspace
    for s in [(300, 40, 72), (256, 40, 72), (300, 320, 72), (300, 328, 72)]:
        rows.append(_tn("generic", *s, dt=0))
    rows.append(_tn("generic", 300, 40, 72, dt=0, ws="none"))
    return rows


def prologue(m, which, mode, M, C, lay):
    """gemm_tn's keyword arguments of one operand's prologue (which: "u" / "v")"""
    if mode == PRO_BNRELU:
        return {which + "_mode": mode, which + "c1": m.cvec(C, 0.2, 1.0), which + "c2": m.cvec(C, 0.3), which + "_relu": True}
    if mode == PRO_BNBWD:
        return {which + "_mode": mode, which + "2": m.act(M, C, lay), which + "c1": m.cvec(C, 0.2, 1.0), which + "c2": m.cvec(C, 0.2),
                which + "c3": m.cvec(C, 0.2)}
    return {}


def run_tn(i, r):
    m = Maker(i, r["dt"])
    torch, ops = m.torch, m.ops
    M, NU, NV = r["M"], r["NU"], r["NV"]
    u, v = m.act(M, NU, "plain"), m.act(M, NV, r["v"])
    kw = dict(prologue(m, "u", r["u_mode"], M, NU, "plain"), **prologue(m, "v", r["v_mode"], M, NV, r["v"]))
    out = torch.zeros((NV, NU) if r["t"] else (NU, NV), dtype=torch.float32, device="cuda")
    si, sj = (1, NU) if r["t"] else (NV, 1)
    if r["ws"] == "none":
        ws = torch.empty(0, dtype=torch.float32, device="cuda")
    else:
        ws = ops.tn_workspace(NU, NV, "cuda") if r["ws"] == "auto" else torch.empty(r["ws"] * NU * NV, dtype=torch.float32, device="cuda")
        ws.fill_(float("nan"))
    ops.gemm_tn(u, NU, v, NV, out, si, sj, M, ws=ws if ws.numel() else False, **kw)
    torch.cuda.synchronize()
    return [sha(out), sha(ws)]


def emit(mode):
    return {"gemm_tn": [run_tn(i, r) for i, r in enumerate(tn_rows())]}


def answer(mode):
    """the digests of every row from a fresh interpreter with the caller's ATOMNAS_TN_* variables stripped and the mode's set"""
    return in_child(mode, script=__file__, modes=MODES, strip=("ATOMNAS_TN_",))["gemm_tn"]


def answers():
    return {mode: answer(mode) for mode in MODES}


def table(ans):
    rows = [dict(r, out=a[0], ws_sha=a[1], out_dma0=b[0], ws_sha_dma0=b[1]) for r, a, b in zip(tn_rows(), ans["default"], ans["dma0"])]
    return {"gemm_tn": rows, "moved": [i for i, (a, b) in enumerate(zip(ans["default"], ans["dma0"])) if a != b]}


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--emit":
        print(json.dumps(emit(sys.argv[2])))
        return
    import torch
    from atomnas_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == 256, "the table is for a whole MI355X (256 CUs), this device has %d" % cus
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "tn_dispatch.json")
    first, second = answers(), answers()
    assert first == second, "two runs of the same library disagree: rows %s" % [
        i for mode in MODES for i, (a, b) in enumerate(zip(first[mode], second[mode])) if a != b]
    t = table(first)
    with open(out, "w") as f:
        f.write('{\n"gemm_tn": [\n' + ",\n".join(json.dumps(r, sort_keys=True) for r in t["gemm_tn"]) + '\n],\n"moved": %s\n}\n' % json.dumps(t["moved"]))
    print("%d rows, moved by ATOMNAS_TN_DMA=0: %s, from %s -> %s" % (len(t["gemm_tn"]), t["moved"], _lib.LIB_PATH, out))
    not_tn3 = [i for i in t["moved"] if t["gemm_tn"][i]["family"] != "tn3"]
    assert t["moved"] and not not_tn3, "ATOMNAS_TN_DMA=0 moved rows that tn_rows() does not label tn3 (or none at all): %s" % not_tn3


if __name__ == "__main__":
    main()
