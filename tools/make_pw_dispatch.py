#!/usr/bin/env python
"""Writes tests/golden/pw_dispatch.json: what the pointwise host path decides, shape by shape, as digests of what its launches write.

atomnas_pw_gemm_nt has no query that names the kernel family it takes, so the table pins the decision through its effects: every
row is ONE ops.gemm_nt call on inputs made on the CPU (numpy.random.default_rng(row index), rounded to the storage type) and the
SHA-1 of the output bytes and of the WHOLE statistics buffer (rows pre-filled with NaN, stat_rows = ops.stat_rows_for(N)).  Which
partial rows a launch writes, and which sums land in them, depends on the family and on its grid, so the statistics digest moves with
a host-side change that the output digest alone would not see.  The rows are the smallest shapes on both sides of every hand-over of
launch_nt (csrc/pwconv.hip, host side: sw -> swg -> st -> small -> ws -> generic).  Also in the table: the answers of
atomnas_expand_bwd_supported and atomnas_project_bwd_dp_supported, the output digests of ops.expand_bwd on both sides of its
streaming hand-over (again with ATOMNAS_XB_STREAM=0) and of ops.project_bwd for every accumulator width; the gemm_nt rows carry a
second pair of digests taken with ATOMNAS_NT_SW=0 ATOMNAS_NT_SWG=0 ATOMNAS_NT_ST=0.

tests/test_pw_dispatch_gpu.py asserts the library under test against the table, so the table PINS a dispatch: generate it from the
library whose behaviour is to be kept (ATOMNAS_HIP_LIB=<that build>), never from the code under change, on a whole MI355X (256 CUs:
the grids are sized from the CU count).  The library reads its switches once per process, so every setting runs in a child
interpreter with the caller's ATOMNAS_NT_* / ATOMNAS_XB_* variables stripped.

    python tools/make_pw_dispatch.py [out.json]      (GPU box; run it twice and keep the file only if both runs agree)
    python tools/make_pw_dispatch.py --emit MODE     (what a child prints: MODE = default | off | xs0)
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRO_NONE, PRO_BNRELU, PRO_BNBWD = 0, 1, 2
STAT_SQ, STAT_Z = 1, 2
MODES = {"default": {}, "off": {"ATOMNAS_NT_SW": "0", "ATOMNAS_NT_SWG": "0", "ATOMNAS_NT_ST": "0"}, "xs0": {"ATOMNAS_XB_STREAM": "0"}}


def _nt(family, M, N, K, **kw):
    r = dict(family=family, M=M, N=N, K=K, dt=1, a_mode=PRO_NONE, a="plain", c="plain", out_f32=0, add=0, bias=0, z=None, mask=0,
             stat_mode=STAT_SQ)
    r.update(kw)
    return r


def nt_rows():
    """the gemm_nt rows, in table order (the row index seeds the inputs)"""
    rows = []
    # sw: narrow output of a wide slab-major input (N <= 48 in steps of 8, 97 <= K <= 448, M >= 16384)
    for s in [(16384, 24, 432), (16383, 24, 432), (16384, 24, 96), (16384, 48, 448), (16384, 48, 456), (16384, 56, 432), (16384, 20, 432)]:
        rows.append(_nt("sw", *s, a_mode=PRO_BNRELU, a="slab"))
    # swg: the late stages (N <= 320 in steps of 8, K >= 256 in steps of 4, 8192 <= M <= 262144), the wide-stage edge, the row limit
    for s in [(8192, 80, 1440), (8191, 80, 1440), (8192, 64, 1440), (8192, 40, 256), (8192, 40, 252), (8192, 96, 1440), (8192, 192, 1440),
              (8192, 320, 1440), (32768, 80, 256), (32640, 80, 256), (262144, 40, 256), (262208, 40, 256)]:
        rows.append(_nt("swg", *s, a_mode=PRO_BNRELU, a="slab"))
    # st: column-stationary streaming (no prologue, K <= 192 in steps of 8, N >= 2 K, N >= 96, M >= 1024), the shared-burst choice
    for s in [(1024, 96, 24), (1023, 96, 24), (1024, 88, 24), (1024, 96, 20), (1024, 96, 48), (1024, 192, 96), (1024, 256, 128),
              (1024, 384, 192), (1024, 392, 200), (1024, 1472, 24), (1024, 320, 24)]:
        rows.append(_nt("st", *s, c="slab"))
        rows.append(_nt("st", *s, c="slab", z="slab", mask=1, stat_mode=STAT_Z))
    # small: N <= 64, K <= 64, M >= 65536; the 4-channel lane tiles (N % 4 == 0, bf16 output) and the 16-channel form
    for s in [(65536, 16, 16), (65535, 16, 16), (65536, 32, 48), (65536, 64, 64), (65536, 20, 16), (65536, 18, 16)]:
        rows.append(_nt("small", *s))
    rows.append(_nt("small", 65536, 16, 16, out_f32=1))
    rows.append(_nt("small", 65536, 16, 16, a_mode=PRO_BNRELU))
    rows.append(_nt("small", 65536, 16, 16, a_mode=PRO_BNBWD))
    # ws: weights in LDS (K >= 97, M >= 4096), one or two chunks, two subtiles with the BN-backward prologue from M = 100000
    for s in [(4096, 64, 97), (4095, 64, 97), (4096, 64, 96), (4096, 65, 97)]:
        rows.append(_nt("ws", *s, a_mode=PRO_BNRELU))
    for s in [(100000, 24, 128), (99999, 24, 128)]:
        rows.append(_nt("ws", *s, a_mode=PRO_BNBWD))
    # generic: fp32 storage, and a bias + residual epilogue
    rows.append(_nt("generic", 1000, 72, 40, dt=0, a_mode=PRO_BNRELU))
    rows.append(_nt("generic", 1000, 136, 72, add=1, bias=1))
    return rows


def xb_query_rows():
    return [dict(inp=i, hid=h, dt=dt) for dt in (0, 1) for i in (8, 16, 24, 32, 40, 48, 56) for h in (64, 320, 448, 720, 768, 800)]


def pb_query_rows():
    return [dict(M=M, oup=o, hid=h, lay=lay, dt=dt) for dt in (0, 1) for M in (1024, 70000) for lay in ("slab", "plain")
            for o in (8, 16, 32, 48, 64, 72) for h in (96, 200, 203)]


def xb_rows():
    return [dict(M=M, inp=i, hid=h) for (M, i, h) in [(64, 16, 192), (64, 16, 128), (63, 16, 192), (4096, 24, 432)]]


def pb_rows():
    return [dict(M=4096, oup=o, hid=432) for o in (16, 32, 48, 64)]


def pad(c, a):
    return (c + a - 1) // a * a


class Maker:
    """inputs of one row: drawn on the CPU from the row's own generator, rounded to the storage type, then copied to the GPU"""

    def __init__(self, seed, dt):
        import numpy
        import torch
        from atomnas_amd import ops
        self.torch, self.ops = torch, ops
        self.rng = numpy.random.default_rng(seed)
        self.T = torch.bfloat16 if dt == 1 else torch.float32

    def randn(self, *s, scale=1.0):
        return self.torch.from_numpy(self.rng.standard_normal(s, dtype="float32")) * scale

    def act(self, M, C, lay, scale=1.0):
        buf = self.torch.zeros(M, pad(C, 16 if lay == "slab" else 8), dtype=self.T)
        buf[:, :C] = self.randn(M, C, scale=scale).to(self.T)
        buf = buf.cuda()
        return self.ops.Slab.from_plain(buf, C) if lay == "slab" else buf

    def out(self, M, C, lay, T=None):
        T = T or self.T
        if lay == "slab":
            s = self.ops.Slab(M, C, T, "cuda")
            s.t.fill_(float("nan"))
            return s
        buf = self.torch.zeros(M, pad(C, 8), dtype=T, device="cuda")
        buf[:, :C] = float("nan")
        return buf

    def cvec(self, n, scale=1.0, shift=0.0):
        v = self.torch.zeros(pad(n, 8) + 8, dtype=self.torch.float32)
        v[:n] = self.randn(n, scale=scale) + shift
        return v.cuda()

    def weights(self, n, k, scale):
        """packed [n padded to 64][k padded to 32] in the storage type, padding zero"""
        buf = self.torch.zeros(pad(n, 64), pad(k, 32), dtype=self.T)
        buf[:n, :k] = self.randn(n, k, scale=scale).to(self.T)
        return buf.cuda()

    def stats(self, N):
        rows = self.ops.stat_rows_for(N)
        return self.torch.full((rows, 2, N), float("nan"), dtype=self.torch.float32, device="cuda"), rows


def sha(t):
    t = t.t if hasattr(t, "to_plain") else t
    import torch
    return hashlib.sha1(t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run_nt(i, r):
    m = Maker(i, r["dt"])
    torch, ops = m.torch, m.ops
    M, N, K = r["M"], r["N"], r["K"]
    a = m.act(M, K, r["a"])
    wp = m.weights(N, K, K ** -0.5)
    kw = {}
    if r["a_mode"] == PRO_BNRELU:
        kw.update(a_mode=PRO_BNRELU, ac1=m.cvec(K, 0.2, 1.0), ac2=m.cvec(K, 0.3), a_relu=1)
    elif r["a_mode"] == PRO_BNBWD:
        kw.update(a_mode=PRO_BNBWD, a2=m.act(M, K, r["a"]), ac1=m.cvec(K, 0.2, 1.0), ac2=m.cvec(K, 0.2), ac3=m.cvec(K, 0.2))
    if r["bias"]:
        kw["bias"] = m.cvec(N)
    if r["add"]:
        kw["add"] = m.act(M, N, "plain")
    if r["z"]:
        kw.update(z=m.act(M, N, r["z"]), zscale=m.cvec(N, 0.2, 1.0), zshift=m.cvec(N, 0.3), mask=r["mask"])
    c = m.out(M, N, r["c"], torch.float32 if r["out_f32"] else None)
    st, rows = m.stats(N)
    ops.gemm_nt(a, wp, c, M, N, K, stats=st, stat_mode=r["stat_mode"], stat_rows=rows, **kw)
    torch.cuda.synchronize()
    return [sha(c), sha(st)]


def run_xb(i, r):
    m = Maker(1000 + i, 1)
    torch, ops = m.torch, m.ops
    M, inp, hid = r["M"], r["inp"], r["hid"]
    h = m.act(M, hid, "slab")
    x = m.act(M, inp, "plain")
    wt = m.weights(inp, hid, hid ** -0.5)
    c1 = m.cvec(hid, 0.2, 1.0)
    gx = m.out(M, inp, "plain")
    dwe = torch.full((hid * inp,), 0.25, dtype=torch.float32, device="cuda")
    ops.expand_bwd(h, c1, x, wt, None, gx, dwe, M, inp, hid)
    torch.cuda.synchronize()
    return [sha(gx), sha(dwe)]


def run_pb(i, r):
    m = Maker(2000 + i, 1)
    torch, ops = m.torch, m.ops
    M, oup, hid = r["M"], r["oup"], r["hid"]
    g = m.act(M, oup, "plain")
    wpt = m.weights(hid, oup, oup ** -0.5)
    z = m.act(M, hid, "slab")
    zs, zh = m.cvec(hid, 0.2, 1.0), m.cvec(hid, 0.3)
    gh = m.out(M, hid, "slab")
    st, rows = m.stats(hid)
    dwp = torch.full((oup * hid,), 0.25, dtype=torch.float32, device="cuda")
    ops.project_bwd(g, wpt, z, zs, zh, 1, gh, st, dwp, hid, 1, M, oup, hid, stat_rows=rows)
    torch.cuda.synchronize()
    return [sha(gh), sha(st), sha(dwp)]


def emit(mode):
    """what the library in this process (its switches are the process's environment) answers: {section: [answer per row]}"""
    from atomnas_amd import _lib, ops
    lib = _lib.load()
    out = {}
    if mode in ("default", "off"):
        out["gemm_nt"] = [run_nt(i, r) for i, r in enumerate(nt_rows())]
    if mode in ("default", "xs0"):
        out["expand_bwd"] = [run_xb(i, r) for i, r in enumerate(xb_rows())]
    if mode == "default":
        out["project_bwd"] = [run_pb(i, r) for i, r in enumerate(pb_rows())]
        out["expand_bwd_supported"] = [int(lib.atomnas_expand_bwd_supported(r["inp"], r["hid"], r["dt"])) for r in xb_query_rows()]
        q = []
        for r in pb_query_rows():
            slab = r["lay"] == "slab"
            ld, ss = (16, r["M"] * 16) if slab else (pad(r["hid"], 8), 0)
            q.append(int(lib.atomnas_project_bwd_dp_supported(r["M"], r["oup"], r["hid"], pad(r["oup"], 8), ld, ss, ld, ss,
                                                              ops.stat_rows_for(r["hid"]), r["dt"])))
        out["project_bwd_dp_supported"] = q
    return out


def in_child(mode, script=__file__, modes=MODES, strip=("ATOMNAS_NT_", "ATOMNAS_XB_")):
    """emit(mode) of a fresh interpreter: the caller's ATOMNAS_NT_* / ATOMNAS_XB_* switches are stripped, only the mode's are set
    (tools/make_tn_dispatch.py passes its own script, modes and prefixes)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith(strip)}
    env.update(modes[mode])
    r = subprocess.run([sys.executable, os.path.abspath(script), "--emit", mode], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def table(answers):
    """the table's sections from the answers of the three modes: every row is its specification plus what was recorded for it"""
    d, off, xs0 = answers["default"], answers["off"], answers["xs0"]
    return {
        "gemm_nt": [dict(r, out=a[0], stats=a[1], out_off=b[0], stats_off=b[1]) for r, a, b in zip(nt_rows(), d["gemm_nt"], off["gemm_nt"])],
        "expand_bwd_supported": [dict(r, ok=a) for r, a in zip(xb_query_rows(), d["expand_bwd_supported"])],
        "project_bwd_dp_supported": [dict(r, ok=a) for r, a in zip(pb_query_rows(), d["project_bwd_dp_supported"])],
        "expand_bwd": [dict(r, gx=a[0], dwe=a[1], gx_xs0=b[0], dwe_xs0=b[1]) for r, a, b in zip(xb_rows(), d["expand_bwd"], xs0["expand_bwd"])],
        "project_bwd": [dict(r, gh=a[0], stats=a[1], dwp=a[2]) for r, a in zip(pb_rows(), d["project_bwd"])],
    }


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--emit":
        print(json.dumps(emit(sys.argv[2])))
        return
    import torch
    from atomnas_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == 256, "the table is for a whole MI355X (256 CUs), this device has %d" % cus
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "pw_dispatch.json")
    t = table({mode: in_child(mode) for mode in MODES})
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join('"%s": [\n' % k + ",\n".join(json.dumps(r, sort_keys=True) for r in v) + "\n]" for k, v in t.items()) + "\n}\n")
    print("%s from %s -> %s" % (", ".join("%d %s" % (len(v), k) for k, v in t.items()), _lib.LIB_PATH, out))


if __name__ == "__main__":
    main()
