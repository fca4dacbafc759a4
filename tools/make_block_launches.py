#!/usr/bin/env python
"""Writes tests/golden/block_launches.json: what the executors of atomnas_amd/functional.py launch, case by case, and what comes out.

Every case builds one module (an atomic block, a fused block, the tiny network, a stand-alone SqueezeAndExcitation), fills parameters,
buffers and inputs from CPU generators with fixed seeds and runs forward (+ backward) once with both recorders on.  Recorded per case:
  "calls"    the ordered entry-point names of every library call (_lib.PROFILE: SE, fold, fill and BatchNorm entries included),
  "rows"     the ordered rows of the launch recorder (ops.RECORD: sizes, prologue / epilogue / statistics modes, layouts),
  "digests"  the SHA-1 of the bytes of the output, the input gradient, every parameter gradient and every buffer.
The kernels use no floating-point atomics, so equal launches on equal data give equal bits: the digests are an equality.  The cases
are the smallest shapes at which block_backward takes each form of the projection backward (fused / dp / prologue) and of the expand
backward (noe_fused / noe_segments / noe_gemms / e); the form a case took is read back from its rows (forms_of) and asserted
against the case list, so a table that misses a form cannot be written.

tests/test_block_launches_gpu.py asserts the code under test against the table, so the table PINS the executors: generate it from the
functional.py whose behaviour is to be kept, never from the code under change.  The grids of several kernels are sized from the CU
count, so the digests hold for the device in the header; calls and rows hold everywhere.  Only interfaces that a restructuring of
functional.py leaves alone are used: the model classes, ops.RECORD, _lib.PROFILE, functional._FUSED_WG_BATCH.  Every run happens in
a child interpreter whose environment has every ATOMNAS_* variable stripped except ATOMNAS_HIP_LIB.

    python tools/make_block_launches.py [out.json]      (GPU box; runs the cases twice and writes the file only if both runs agree)
    python tools/make_block_launches.py --emit          (what a child prints: one JSON line)
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROJECT_FORMS = ("fused", "dp", "prologue")
EXPAND_FORMS = ("noe_fused", "noe_segments", "noe_gemms", "e")
# the network of tests/test_block_gpu.py (stem, 1x1 and depthwise ConvBNReLU, eleven blocks, the tail)
TINY = dict(num_classes=10, input_size=64, input_channel=16, last_channel=64, width_mult=1.0, dropout_ratio=0.0,
            batch_norm_momentum=0.01, batch_norm_epsilon=1e-3, active_fn="nn.ReLU",
            inverted_residual_setting=[[1, 8, 1, 1, [3]], [6, 16, 2, 2, [3, 5, 7]], [6, 24, 2, 2, [3, 5, 7]], [6, 32, 1, 2, [3, 5, 7]],
                                       [6, 40, 1, 2, [3, 5, 7]]])


def _block(name, inp, oup, stride, channels, ks, N, H, dt, project, expand, expand_flag=True, **kw):
    return dict(name=name, kind="block", inp=inp, oup=oup, stride=stride, channels=channels, ks=ks, expand=expand_flag, N=N, H=H, dt=dt,
                project=project, expand_form=expand, **kw)


def cases():
    """the case list, in table order.  project / expand_form: the form block_backward is expected to take (None: no such step)"""
    out = []
    for dt in (1, 0):
        sfx = "_bf16" if dt else "_fp32"
        pro = (lambda f: f) if dt else (lambda f: "prologue")
        noe = (lambda f: f) if dt else (lambda f: "e")
        out.append(_block("single_16_24_s2" + sfx, 16, 24, 2, [96], [5], 3, 14, dt, pro("fused"), noe("noe_fused")))
        out.append(_block("residual_8_8" + sfx, 8, 8, 1, [16, 16, 16], [3, 5, 7], 3, 14, dt, pro("dp"), noe("noe_fused")))
        if dt:
            out.append(_block("ragged_8_16_s2" + sfx, 8, 16, 2, [12, 20, 7], [3, 5, 7], 3, 14, dt, "dp", "noe_fused"))
            out.append(_block("segments_40_40" + sfx, 40, 40, 1, [240, 240, 240], [3, 5, 7], 2, 14, dt, "fused", "noe_segments"))
            out.append(_block("gemms_40_40" + sfx, 40, 40, 1, [720], [3], 2, 14, dt, "fused", "noe_gemms"))
        out.append(_block("late_80_80" + sfx, 80, 80, 1, [96, 96, 96], [3, 5, 7], 2, 7, dt, pro("dp"), "e"))
        if dt:
            out.append(_block("first_16_8" + sfx, 16, 8, 1, [16], [3], 3, 14, dt, "dp", None, expand_flag=False))
    for se in (0.5, None):
        for dt in (1, 0):
            for batch in (True, False):
                out.append(dict(name="fused_%s_%s_%s" % ("se" if se else "nose", "bf16" if dt else "fp32", "batch" if batch else "segs"),
                                kind="fused", inp=24, oup=24, stride=1, channels=[30, 50, 13], ks=[3, 5, 7], expand=True, se_ratio=se, N=6,
                                H=14, dt=dt, wg_batch=batch, project="dp" if dt else "prologue", expand_form="e"))
    out.append(dict(name="tiny_network_bf16", kind="model", N=6, H=64, dt=1))
    out.append(dict(name="standalone_se_bf16", kind="se", C=24, hid=12, N=4, H=7, dt=1))
    out.append(_block("residual_8_8_eval_bf16", 8, 8, 1, [16, 16, 16], [3, 5, 7], 3, 14, 1, None, None, eval=True))
    return out


def forms_of(rows, backward_blocks=1):
    """(projection form, expand form) of a one-block case, read from its recorder rows"""
    ent = [r["entry"] for r in rows]
    if "bn_finalize_bwd" not in ent:
        return None, None
    project = "fused" if "project_bwd" in ent else "dp" if "bnbwd_apply" in ent else "prologue"
    nx = ent.count("expand_bwd")
    expanding = ent.count("bn_finalize_bwd") // backward_blocks == 3
    expand = ("noe_fused" if nx == 1 else "noe_segments") if nx else "noe_gemms" if "gram" in ent else "e" if expanding else None
    return project, expand


def _randomize(module, seed):
    """parameters and running statistics from a CPU generator (as tests/test_block_gpu.py does)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.dim() == 1 and "bias" not in n:      # BN gamma
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            else:
                p.copy_(torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5)
        for n, b in module.named_buffers():
            if "running_mean" in n:
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
            elif "running_var" in n:
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)


def sha(t):
    import torch
    return hashlib.sha1(t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(c):
    import torch
    from atomnas_amd import _lib, ops
    from atomnas_amd import functional as Fn
    from atomnas_amd.models import mobilenet_base as mb
    T = torch.bfloat16 if c["dt"] else torch.float32
    bn_kw = {"momentum": 0.01, "eps": 1e-3}
    g = torch.Generator().manual_seed(11)
    N, H = c["N"], c["H"]
    y = None
    if c["kind"] == "block":
        mod = mb.InvertedResidualChannels(c["inp"], c["oup"], c["stride"], c["channels"], c["ks"], c["expand"],
                                          active_fn=mb.get_active_fn("nn.ReLU"), batch_norm_kwargs=bn_kw)
    elif c["kind"] == "fused":
        mod = mb.InvertedResidualChannelsFused(c["inp"], c["oup"], c["stride"], c["channels"], c["ks"], c["expand"],
                                               active_fn=mb.get_active_fn("nn.Swish"), batch_norm_kwargs=bn_kw, se_ratio=c["se_ratio"])
    elif c["kind"] == "se":
        mod = mb.SqueezeAndExcitation(c["C"], c["hid"], active_fn=mb.get_active_fn("nn.Swish"))
    else:
        from atomnas_amd.models import mobilenet_supernet as ms
        mod = ms.Model(**TINY)
    if c["kind"] == "model":
        mod.set_compute_dtype(T)
        x = torch.randn(N, 3, H, H, generator=g)
        y = torch.randint(0, 10, (N,), generator=g).cuda()
    else:
        mod.compute_dtype = T
        cin = c["C"] if c["kind"] == "se" else c["inp"]
        cout = c["C"] if c["kind"] == "se" else c["oup"]
        Ho = (H - 1) // c.get("stride", 1) + 1
        x = torch.randn(N, cin, H, H, generator=g).to(T)
        gout = torch.randn(N, cout, Ho, Ho, generator=g).to(T).cuda()
    _randomize(mod, 7)
    mod.cuda()
    old = Fn._FUSED_WG_BATCH
    Fn._FUSED_WG_BATCH = c.get("wg_batch", old)
    ops.RECORD, _lib.PROFILE = [], []
    try:
        if c.get("eval"):
            mod.eval()
            with torch.no_grad():
                out = mod(x.cuda())
            xg = None
        else:
            mod.train()
            xg = x.cuda().requires_grad_(c["kind"] != "model")
            if c["kind"] == "model":
                from atomnas_amd.utils import optim as aopt
                out = mod(xg)
                aopt.CrossEntropyLabelSmooth(10, 0.1, reduction="none")(out, y).mean().backward()
            else:
                for _ in range(2 if c["kind"] == "fused" else 1):   # the fused block's gradients accumulate over two backward passes
                    out = mod(xg)
                    out.backward(gout)
        torch.cuda.synchronize()
        rows, calls = ops.RECORD, [p[0] for p in _lib.PROFILE]
    finally:
        ops.RECORD, _lib.PROFILE, Fn._FUSED_WG_BATCH = None, None, old
    dig = {"out": sha(out)}
    if xg is not None and xg.grad is not None:
        dig["dx"] = sha(xg.grad)
    if not c.get("eval"):
        for n, p in mod.named_parameters():
            dig["grad " + n] = sha(p.grad)
    for n, b in mod.named_buffers():
        dig["buf " + n] = sha(b)
    return dict(name=c["name"], calls=calls, rows=rows, digests=dig)


def check(table):
    """what a table must show before it may be written or trusted: every case, and every form where the case list says it is"""
    by = {r["name"]: r for r in table}
    cs = cases()
    assert [r["name"] for r in table] == [c["name"] for c in cs], "the table's cases are not the generator's"
    for c in cs:
        if c["kind"] in ("block", "fused"):
            got = forms_of(by[c["name"]]["rows"], 2 if c["kind"] == "fused" else 1)
            assert got == (c["project"], c["expand_form"]), "%s took %s, listed as %s" % (c["name"], got, (c["project"], c["expand_form"]))
    ent = lambda n: [r["entry"] for r in by[n]["rows"]]
    nt = lambda n: [r for r in by[n]["rows"] if r["entry"] == "pw_gemm_nt"]
    assert "project_bwd" in ent("single_16_24_s2_bf16")
    rows = by["residual_8_8_bf16"]["rows"]
    i = [r["entry"] for r in rows].index("bnbwd_apply")
    nxt = next(r for r in rows[i + 1:] if r["entry"] == "pw_gemm_nt")
    assert nxt["a_mode"] == 0 and nxt["mask"] and nxt["z"] is not None, "bnbwd_apply is not followed by an unprologued masked pw_gemm_nt"
    assert any(r["a_mode"] == 2 and r["mask"] for r in nt("residual_8_8_fp32")), "no PRO_BNBWD masked pw_gemm_nt"
    assert ent("single_16_24_s2_bf16").count("expand_bwd") == 1 and ent("segments_40_40_bf16").count("expand_bwd") == 3
    assert "gram" in ent("gemms_40_40_bf16") and "expand_bwd" not in ent("gemms_40_40_bf16")
    assert "gram" not in ent("late_80_80_bf16")
    seen = {f for c in cs for f in (c.get("project"), c.get("expand_form")) if f}
    assert seen == set(PROJECT_FORMS + EXPAND_FORMS), seen
    for name in ("fused_se_bf16_batch", "standalone_se_bf16"):
        assert "atomnas_se_bwd_gate" in by[name]["calls"] and "atomnas_se_mlp_fwd" in by[name]["calls"]
    assert "atomnas_fold_jobs" in by["fused_se_bf16_batch"]["calls"] and "atomnas_fold_jobs" not in by["fused_se_bf16_segs"]["calls"]


def emit():
    import torch
    prop = torch.cuda.get_device_properties(0)
    return dict(header=dict(device=prop.name, cus=prop.multi_processor_count), cases=[run_case(c) for c in cases()])


def in_child(timeout=300):
    """emit() of a fresh interpreter with every ATOMNAS_* variable of the caller stripped except the library override"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ATOMNAS_") or k == "ATOMNAS_HIP_LIB"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit"], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def load(path=os.path.join(ROOT, "tests", "golden", "block_launches.json")):
    """(header, [case]) of a written table: the header line, then one compact line per case"""
    lines = [json.loads(l) for l in open(path) if l.strip()]
    return lines[0], lines[1:]


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--emit":
        print(json.dumps(emit()))
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "block_launches.json")
    a, b = in_child(), in_child()
    assert a == b, "two runs disagree: %s" % [x["name"] for x, y in zip(a["cases"], b["cases"]) if x != y]
    check(a["cases"])
    with open(out, "w") as f:
        f.write(json.dumps(a["header"], sort_keys=True) + "\n")
        for r in a["cases"]:
            f.write(json.dumps(r, sort_keys=True, separators=(",", ":")) + "\n")
    print("%d cases, %d calls, %d rows on %s (%d CUs) -> %s" % (len(a["cases"]), sum(len(r["calls"]) for r in a["cases"]),
                                                                sum(len(r["rows"]) for r in a["cases"]), a["header"]["device"],
                                                                a["header"]["cus"], out))


if __name__ == "__main__":
    main()
