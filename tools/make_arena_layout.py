#!/usr/bin/env python
"""Writes tests/golden/arena_layout.json: what atomnas_amd/runtime.py (ArenaManager.materialize) lays out, case by case.

Every case builds one module tree (the tiny network with and without an optimizer and EMA, with changed blocks, after a real shrink; a
tiny searched network of fused blocks with and without SE; stand-alone modules; the three full-size models of configs.py), materialises
its arenas and records
  "nP", "nS", "sizes"     the arena sizes (elements) of P / S and of CNT, packT, packF, FW,
  "exists"                which of SQ / BUF / EMA / SEMA were allocated,
  "param_slots", "buffer_slots", "reg_slots"   as the manager holds them,
  "jobsT", "jobsF"        the decoded rows of the two pack-job tables,
  "fold"                  the fold jobs as offsets from the bases of FW and G, and fold_blk0,
  "plans"                 per plan, in `plans` order: every int / bool / list / str attribute; for every tensor attribute the arena it
                          points into, its element offset from that arena's base, shape, stride and dtype; the bn* dicts the same way
                          (with C, Cpad and the names of their BatchNorm modules); the contents of cmap.
The full-size models keep one SHA-1 per list and per plan instead (digest()); "sha_layout" leaves out what only the bind step knows
(BIND_ONLY), so that a walk that never touches a device can be held against it.

tests/test_arena_layout.py (CPU, through runtime.arena_layout) and tests/test_arena_layout_gpu.py (the materialised arenas) assert the
code under test against the table, so the table PINS the layout: generate it from the runtime.py whose behaviour is to be kept, never
from the code under change.  Only attributes that a restructuring of runtime.py leaves alone are read.  Every run happens in a child
interpreter whose environment has every ATOMNAS_* variable stripped except ATOMNAS_HIP_LIB.

    python tools/make_arena_layout.py [out.json]      (GPU box; runs the cases twice and writes the file only if both runs agree)
    python tools/make_arena_layout.py --emit          (what a child prints: one JSON line)
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from make_block_launches import TINY  # noqa: E402  (the network of tests/test_block_gpu.py)

GOLDEN = os.path.join(ROOT, "tests", "golden", "arena_layout.json")
ARENAS = ("P", "G", "S", "SQ", "BUF", "EMA", "SEMA", "CNT", "packT", "packF", "FW")
BIND_ONLY = ("valid", "act", "se_act")   # plan attributes set from the activation modules while the views are built, not by the layout
SHRINK_THRESHOLD = 1e-3
# tiny searched network (rows [c, n, s, ks, hiddens, expand]): a non-expanding first block, ragged widths, a single branch
FUSED = dict(num_classes=10, input_size=64, input_channel=16, last_channel=64, dropout_ratio=0.0, batch_norm_momentum=0.01,
             batch_norm_epsilon=1e-3, active_fn="nn.Swish", block="InvertedResidualChannelsFused",
             inverted_residual_setting=[[8, 1, 1, [3], [16], False], [16, 1, 2, [3, 5, 7], [30, 50, 13], True],
                                        [16, 1, 1, [3, 5], [21, 4], True], [24, 1, 2, [5], [37], True]])
# features index -> (channels, kernel sizes) of the blocks the "changed" case rebuilds: ragged, all pruned (a residual block), one branch
CHANGED = {2: ([12, 20, 7], [3, 5, 7]), 5: ([], []), 7: ([5], [7])}


def cases():
    """the case list, in table order.  full: written as digests"""
    out = [dict(name="tiny", kind="tiny"),
           dict(name="tiny_rmsprop_ema", kind="tiny", opt="rmsprop", ema=True),
           dict(name="tiny_sgd0", kind="tiny", opt="sgd0"),
           dict(name="tiny_changed", kind="tiny", changed=True),
           dict(name="fused_se", kind="fused", se_ratio=0.5),
           dict(name="fused_nose", kind="fused", se_ratio=None),
           dict(name="alone_block", kind="block"),
           dict(name="alone_convbn_dense", kind="convbn", groups=1),
           dict(name="alone_convbn_dw", kind="convbn", groups=24),
           dict(name="alone_se", kind="se")]
    out += [dict(name=n, kind="config", full=True) for n in ("atomnas_a_supernet", "atomnas_c", "atomnas_c_plus")]
    out.append(dict(name="tiny_shrunk", kind="tiny", opt="rmsprop", ema=True, shrink=True))
    return out


def rebuild_block(model, index, channels, ks):
    """replaces model.features[index] by a block of the same kind with these branch widths / kernel sizes"""
    from atomnas_amd.models import mobilenet_base as mb
    old = model.features[index]
    model.features[index] = mb.InvertedResidualChannels(old.input_dim, old.output_dim, old.stride, list(channels), list(ks), old.expand,
                                                        active_fn=old.active_fn, batch_norm_kwargs=old.batch_norm_kwargs)


def build_model(c, shrunk_to=None):
    """the CPU module tree of a case.  shrunk_to ({features index: (channels, kernel sizes)}): the blocks of a `shrink` case as its
    shrink left them, for a walk without the shrink itself"""
    from atomnas_amd import configs
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.models import searched_network as sn
    bn_kw = {"momentum": 0.01, "eps": 1e-3}
    relu = mb.get_active_fn("nn.ReLU")
    if c["kind"] == "tiny":
        model = ms.Model(**TINY)
        for i, (ch, ks) in sorted((CHANGED if c.get("changed") else shrunk_to or {}).items()):
            rebuild_block(model, i, ch, ks)
        return model
    if c["kind"] == "fused":
        return sn.Model(se_ratio=c["se_ratio"], **FUSED)
    if c["kind"] == "block":
        return mb.InvertedResidualChannels(24, 40, 2, [30, 50, 13], [3, 5, 7], True, active_fn=relu, batch_norm_kwargs=bn_kw)
    if c["kind"] == "convbn":
        g = c["groups"]
        return mb.ConvBNReLU(24, 24 if g > 1 else 37, kernel_size=5 if g > 1 else 1, groups=g, active_fn=relu, batch_norm_kwargs=bn_kw)
    if c["kind"] == "se":
        return mb.SqueezeAndExcitation(24, 12, active_fn=mb.get_active_fn("nn.Swish"))
    if c["name"] == "atomnas_a_supernet":
        return ms.Model(input_size=224, **configs.model_kwparams(c["name"]))
    return sn.Model(input_size=224, **configs.searched_kwparams(c["name"]))


def kill_atoms(model):
    """depthwise-BN gammas of the expanding blocks, before the shrink: ragged survivors, one branch gone, one residual block all gone"""
    import torch
    with torch.no_grad():
        for b, (name, blk) in enumerate(model.get_named_block_list().items()):
            if not blk.expand:
                continue
            for j, bn in enumerate(blk.get_depthwise_bn()):
                c = torch.arange(bn.weight.numel())
                dead = (c * 7 + 3 * j + b) % 5 < 2
                if b == 4 or (b == 6 and j == 1):
                    dead = torch.ones_like(dead)
                bn.weight.copy_(torch.where(dead, torch.zeros(()), 0.5 + 0.01 * c))


def materialize(c):
    """(model, manager) of a case with its arenas built on the GPU, as training would have them"""
    import torch
    from atomnas_amd import runtime
    from atomnas_amd.utils import optim as aopt, rmsprop, sgd
    torch.manual_seed(3)
    model = build_model(c)
    if c.get("shrink"):
        from atomnas_amd.utils import model_profiling as mp
        kill_atoms(model)
        mp.model_profiling(model, 64, 64, verbose=False)
    model.cuda().train()
    mgr = runtime.manager_of(model)
    opt = ema = None
    if c.get("opt") == "rmsprop":
        opt = rmsprop.RMSprop(model.parameters(), lr=0.002, alpha=0.9, momentum=0.9, eps=1e-3, eps_inside_sqrt=True)
    elif c.get("opt") == "sgd0":
        opt = sgd.SGD(model.parameters(), lr=0.1, momentum=0)
    if opt is not None:
        mgr.attach_optimizer(opt)
        opt._mgr = mgr
    if c.get("ema"):
        ema = aopt.ExponentialMovingAverage(0.99)
        for n, p in model.named_parameters():
            ema.register(n, p)
        for n, b in model.named_buffers():
            if "running" in n:
                ema.register(n, b)
        ema.attach(mgr)
    mgr.ensure()
    if c.get("shrink"):
        import train as T   # the project's shrink entry
        from atomnas_amd.utils import config, prune as aprune

        class F(dict):
            __getattr__ = dict.__getitem__
        config.FLAGS.bind(F(image_size=64, use_distributed=False))
        pinfo = aprune.get_bn_to_prune(model, {"bn_prune_filter": "expansion_only_skip_expand1"}, verbose=False)
        wrapper = torch.nn.Module()
        wrapper.module = model
        before = [list(b.channels) for b in model.get_named_block_list().values()]
        T.shrink_model(wrapper, ema, opt, pinfo, SHRINK_THRESHOLD, ema_only=False)
        assert [list(b.channels) for b in model.get_named_block_list().values()] != before, "the shrink removed nothing"
        mgr.ensure()
    torch.cuda.synchronize()
    return model, mgr


def _rows(table, fields):
    """rows of a device job table (bytes of a C struct array) as lists of ints"""
    import numpy as np
    if table is None:
        return []
    a = np.frombuffer(table.cpu().numpy().tobytes(), dtype=np.dtype(fields))
    return [[int(r[n]) for n, _ in fields] for r in a]


PACK_JOB = [("src_off", "<i8"), ("dst_off", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("src_ld", "<i4"), ("dst_ld", "<i4"),
            ("c_off", "<i4"), ("mode", "<i4")]
FOLD_JOB = [("src", "<u8"), ("dst", "<u8"), ("src_ld", "<i8"), ("dst_ld", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("blk0", "<u4"),
            ("pad_", "<i4")]


def record(model, mgr):
    """the whole layout of a materialised manager as plain JSON data"""
    import torch
    arenas = [(n, getattr(mgr, n)) for n in ARENAS if getattr(mgr, n, None) is not None]
    names = {id(m): n for n, m in model.named_modules()}

    def enc(v):
        if isinstance(v, torch.Tensor):
            for n, a in arenas:
                d = v.data_ptr() - a.data_ptr()
                if v.numel() and 0 <= d < a.numel() * a.element_size():
                    return [n, d // a.element_size(), list(v.shape), list(v.stride()), str(v.dtype)]
            return ["own", v.cpu().tolist(), str(v.dtype)]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, (list, tuple)):
            return [enc(x) for x in v]
        if isinstance(v, dict):
            return {k: enc(x) for k, x in v.items() if k != "mgr"}
        if isinstance(v, torch.nn.Module):
            return names[id(v)]
        if callable(v):
            return "fn:" + v.__name__
        raise TypeError(type(v))

    fold = _rows(mgr.fold_table, FOLD_JOB)
    for r in fold:
        r[0], r[1] = (r[0] - mgr.FW.data_ptr()) // 4, (r[1] - mgr.G.data_ptr()) // 4
    return dict(nP=mgr.nP, nS=mgr.nS, sizes={n: getattr(mgr, n).numel() for n in ("CNT", "packT", "packF", "FW")},
                exists={n: getattr(mgr, n) is not None for n in ("SQ", "BUF", "EMA", "SEMA")},
                param_slots=[[n, o, list(s), None if st is None else list(st)] for n, (o, s, st) in mgr.param_slots.items()],
                buffer_slots=[[n, a, o, list(s)] for n, (a, o, s) in mgr.buffer_slots.items()],
                reg_slots=[list(r) for r in mgr.reg_slots],
                jobsT=_rows(mgr.jobsT, PACK_JOB), jobsF=_rows(mgr.jobsF, PACK_JOB), njobs=[mgr.njobsT, mgr.njobsF],
                fold=dict(jobs=fold, blk0=list(mgr.fold_blk0)),
                plans=[[n, {k: enc(v) for k, v in sorted(vars(pl).items()) if k != "mgr"}] for n, pl in mgr.plans.items()])


def sha(x):
    return hashlib.sha1(json.dumps(x, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def digest(rec):
    """a full-size record with every list replaced by its SHA-1 and every plan by two: the whole plan and its layout part"""
    out = {k: (sha(v) if k in ("param_slots", "buffer_slots", "reg_slots", "jobsT", "jobsF", "fold") else v) for k, v in rec.items()}
    out["plans"] = [[n, dict(sha=sha(p), sha_layout=sha({k: v for k, v in p.items() if k not in BIND_ONLY}))] for n, p in rec["plans"]]
    return out


def run_case(c):
    model, mgr = materialize(c)
    rec = record(model, mgr)
    return dict(name=c["name"], **(digest(rec) if c.get("full") else rec))


def emit():
    import torch
    return dict(header=dict(device=torch.cuda.get_device_properties(0).name, align=256), cases=[run_case(c) for c in cases()])


def in_child(timeout=600):
    """emit() of a fresh interpreter with every ATOMNAS_* variable of the caller stripped except the library override"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ATOMNAS_") or k == "ATOMNAS_HIP_LIB"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--emit"], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def load(path=GOLDEN):
    """(header, {name: case}) of a written table: the header line, then one compact line per case"""
    lines = [json.loads(l) for l in open(path) if l.strip()]
    return lines[0], {r["name"]: r for r in lines[1:]}


def shrunk_blocks(rec):
    """{features index: (channels, kernel sizes)} of every block plan of a recorded tiny network"""
    return {int(n.split(".")[1]): (p["hid"], p["ks"]) for n, p in rec["plans"] if "hid" in p}


def check(table):
    """what a table must show before it may be written: every case, and every branch of the walk where the case list says it is"""
    by = {r["name"]: r for r in table}
    assert [r["name"] for r in table] == [c["name"] for c in cases()], "the table's cases are not the generator's"
    plans = lambda n: [p for _, p in by[n]["plans"]]
    assert by["tiny"]["exists"] == dict(SQ=False, BUF=False, EMA=False, SEMA=False)
    assert by["tiny_rmsprop_ema"]["exists"] == dict(SQ=True, BUF=True, EMA=True, SEMA=True)
    assert by["tiny_sgd0"]["exists"] == dict(SQ=False, BUF=False, EMA=False, SEMA=False)
    assert any(p.get("nb") == 0 for p in plans("tiny_changed")) and any(p.get("hid") == [12, 20, 7] for p in plans("tiny_changed"))
    for n in ("tiny_changed", "tiny_shrunk"):
        assert any(p.get("nb") == 0 for p in plans(n)) and any(p.get("nb") in (1, 2) for p in plans(n)), n
        assert any(h % 16 for p in plans(n) for h in p.get("hid", [])), n
    assert any(p.get("se") for p in plans("fused_se")) and not any(p.get("se") for p in plans("fused_nose"))
    assert any(p.get("fused") and not p["expand"] for p in plans("fused_se")) and by["fused_se"]["fold"]["jobs"]
    assert not by["alone_se"]["plans"] and len(by["alone_se"]["param_slots"]) == 4
    assert "taps" in plans("alone_convbn_dw")[0] and "W_pack" in plans("alone_convbn_dense")[0]


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--emit":
        print(json.dumps(emit()))
        return
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    a, b = in_child(), in_child()
    assert a == b, "two runs disagree: %s" % [x["name"] for x, y in zip(a["cases"], b["cases"]) if x != y]
    check(a["cases"])
    with open(out, "w") as f:
        f.write(json.dumps(a["header"], sort_keys=True) + "\n")
        for r in a["cases"]:
            f.write(json.dumps(r, sort_keys=True, separators=(",", ":")) + "\n")
    print("%d cases, %d plans on %s -> %s (%d bytes)" % (len(a["cases"]), sum(len(r["plans"]) for r in a["cases"]), a["header"]["device"],
                                                        out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
