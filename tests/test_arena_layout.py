"""Arena layout (CPU): runtime.arena_layout against tests/golden/arena_layout.json.

The table (tools/make_arena_layout.py) was read back from materialised arenas on the GPU, from the runtime.py BEFORE the layout became a
walk of its own.  Here every case is built on the CPU, walked by arena_layout, and everything the layout determines is held against
the table: arena sizes, parameter / buffer / regulariser slots, the rows of both pack-job tables, the fold jobs, and per plan every
scalar field and the arena, offset, shape and stride of every view, which expected_plan() derives from the plan's slot and pack offsets
independently of the manager's bind step.  What only the bind step knows (gen.BIND_ONLY) and which optimizer arenas exist is left to
tests/test_arena_layout_gpu.py.  The shrunk network is rebuilt from the channel lists the table recorded after the real shrink.
"""
import os
import sys

import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_arena_layout as gen  # noqa: E402

HEADER, TABLE = gen.load()
CASES = gen.cases()
LISTS = ("param_slots", "buffer_slots", "reg_slots", "jobsT", "jobsF", "fold")


def _t(arena, off, shape, dtype=torch.float32):
    """what gen.record writes for a contiguous view"""
    strides = [1] * len(shape)
    for i in range(len(shape) - 2, -1, -1):
        strides[i] = strides[i + 1] * shape[i + 1]
    return [arena, off, list(shape), strides, str(dtype)]


def expected_plan(m, pl, info, T, names):
    """the record of one plan from its layout description: scalar fields as they stand, views from the slot / pack offsets"""
    from atomnas_amd import runtime as rt
    rec = {k: ("fn:" + v.__name__ if callable(v) else v) for k, v in vars(pl).items() if k not in gen.BIND_ONLY and k != "module"}
    rec["module"] = names[id(pl.module)]
    if not info:
        return rec
    so, pk = info["so"], info["pk"]
    pack = lambda t: _t("packT", t[0], [t[1], t[2]], T)
    taps = lambda t: _t("packF", t[0], [t[1], t[2]])

    def bn(sl, n, C, mods, **extra):
        d = dict(gamma=_t("P", sl["g"], [n]), beta=_t("P", sl["b"], [n]), dgamma=_t("G", sl["g"], [n]), dbeta=_t("G", sl["b"], [n]),
                 rm=_t("S", sl["rm"], [n]), rv=_t("S", sl["rv"], [n]), C=C, mods=[names[id(x)] for x in mods])
        return dict(d, **extra)

    if isinstance(m, nn.Linear):
        has_bias = m.bias is not None
        rec.update(W_grad=_t("G", so["W"], [pl.cout * pl.cin]), W_pack=pack(pk["W"]), WT_pack=pack(pk["WT"]),
                   bias=_t("P", so["b"], [rt.pad8(pl.cout)]) if has_bias else None, bias_grad=_t("G", so["b"], [pl.cout]) if has_bias else None)
    elif isinstance(pl, rt.SimplePlan):
        rec.update(bn=bn(so["bn"], rt.pad8(pl.cout), pl.cout, info["mods"]["bn"]), W_grad=_t("G", so["W"], [m[0].weight.numel()]))
        if "W" in pk:
            rec.update(W_pack=pack(pk["W"]), WT_pack=pack(pk["WT"]))
        else:
            rec.update(taps=taps(pk["taps"]))
    else:
        HT, mods = pl.HT, info["mods"]
        wide, extra = HT, {}
        if pl.fused:
            cmap = [-1] * HT
            for sg, st, h in zip(pl.seg, pl.start, pl.hid):
                cmap[sg:sg + h] = range(st, st + h)
            rec["cmap"] = ["own", cmap, "torch.int32"]
            wide, extra = pl.total, dict(cmap=rec["cmap"], Cpad=HT)
        if pl.expand:
            rec.update(We_grad=_t("G", so["We"], [wide * pl.inp]), bne=bn(so["bne"], wide, wide, mods["bne"], **extra),
                       We_pack=pack(pk["We"]), WeT_pack=pack(pk["WeT"]))
        rec.update(Wd_grad=[_t("G", o, [pl.segpad(h) * k * k]) for o, h, k in zip(so["Wd"], pl.hid, pl.ks)],
                   bnd=bn(so["bnd"], HT, HT, mods["bnd"]), Wp_grad=_t("G", so["Wp"], [pl.oup * wide]),
                   bnp=bn(so["bnp"], pl.oup, pl.oup, mods["bnp"]), Wp_pack=pack(pk["Wp"]), WpT_pack=pack(pk["WpT"]),
                   taps=[taps(t) for t in pk["taps"]])
        if pl.se:
            nh, total = pl.se_hid, pl.total
            for a, d in (("P", ""), ("G", "d")):
                rec["se_%sw1" % d], rec["se_%sb1" % d] = _t(a, so["se1w"], [nh * total]), _t(a, so["se1b"], [nh])
                rec["se_%sw2" % d], rec["se_%sb2" % d] = _t(a, so["se2w"], [total * nh]), _t(a, so["se2b"], [total])
            o1, o2, o3 = pk["se"]
            rec.update(se_w1p=_t("packF", o1, [nh * HT]), se_w2t=_t("packF", o2, [nh * HT]), se_b2p=_t("packF", o3, [HT]))
    return rec


def expected(model, lay):
    """the part of gen.record that the layout determines"""
    names = {id(m): n for n, m in model.named_modules()}
    name_of = {id(p): n for n, p in model.named_parameters()}
    name_of.update({id(b): n for n, b in model.named_buffers()})
    sizes = lay.sizes
    params, buffers = [], []
    for arena, mod, attr, off, shape, strides in lay.binds:
        if arena == "P":
            params.append([name_of[id(mod._parameters[attr])], off, list(shape), None if strides is None else list(strides)])
        else:
            buffers.append([name_of[id(mod._buffers[attr])], arena, off, list(shape)])
    blk0, fold = [0], []
    for so, do, sld, dld, r, c in lay.fold_jobs:
        fold.append([so, do, sld, dld, r, c, blk0[-1], 0])
        blk0.append(blk0[-1] + (r * c + 255) // 256)
    return dict(nP=sizes["P"], nS=sizes["S"], sizes={k: sizes[k] for k in ("CNT", "packT", "packF", "FW")}, param_slots=params,
                buffer_slots=buffers, reg_slots=[list(r) for r in lay.reg_slots], jobsT=[list(j) for j in lay.jobsT],
                jobsF=[list(j) for j in lay.jobsF], njobs=[len(lay.jobsT), len(lay.jobsF)], fold=dict(jobs=fold, blk0=blk0),
                plans=[[pl.name, expected_plan(m, pl, info, lay.compute_dtype, names)] for m, pl, info in lay.plans])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_layout_matches_table(case):
    from atomnas_amd import runtime
    want = TABLE[case["name"]]
    model = gen.build_model(case, shrunk_to=gen.shrunk_blocks(want) if case.get("shrink") else None)
    assert next(model.parameters()).device.type == "cpu"
    got = expected(model, runtime.arena_layout(model, torch.bfloat16))
    for key in ("nP", "nS", "sizes", "njobs"):
        assert got[key] == want[key], key
    assert [n for n, _ in got["plans"]] == [n for n, _ in want["plans"]]
    if case.get("full"):
        for key in LISTS:
            assert gen.sha(got[key]) == want[key], key
        for (name, g), (_, w) in zip(got["plans"], want["plans"]):
            assert gen.sha(g) == w["sha_layout"], name
        return
    for key in LISTS:
        assert got[key] == want[key], key
    for (name, g), (_, w) in zip(got["plans"], want["plans"]):
        w = {k: v for k, v in w.items() if k not in gen.BIND_ONLY}
        assert sorted(g) == sorted(w), (name, sorted(set(g) ^ set(w)))
        for k in w:
            assert g[k] == w[k], (name, k, g[k], w[k])


def test_layout_needs_no_device_and_materialize_still_refuses_the_cpu():
    from atomnas_amd import _lib, runtime
    model = gen.build_model(CASES[0])
    lay = runtime.arena_layout(model, torch.float32)
    assert all(p.device.type == "cpu" and not hasattr(p, "_atomnas_off") for p in model.parameters())   # nothing was re-pointed
    assert lay.sizes["P"] == TABLE["tiny"]["nP"]
    with pytest.raises(_lib.AtomnasHipError):
        runtime.manager_of(model).materialize()
