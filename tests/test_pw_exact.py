"""The exact-integer cases of the pointwise kernels (tests/exact_ref.py) hold their preconditions -- for the reference alone, no GPU.

Every case of every table is built and checked:
 (a) per output element the sum of |terms| is below 2^24; per statistics channel the sums over all rows of c^2, |c| and |c z| are; per
     weight-gradient element the sum of |u v| plus |pre-fill| is: fp32 then holds every partial sum of any summation order exactly;
 (b) every k has a non-zero weight in some output column, every row and every operand channel a non-zero effective value;
 (c) every input read through an activation prologue or a mask has at least 5 % of its pre-activations exactly 0, 5 % on each side of
     0 and, in mode 2, 5 % exactly 6 and 5 % above 6;
 (d) padding channels and pad rows of every buffer are zero, outputs are poisoned, statistics buffers are NaN at stat_rows_for(N) rows.
Swish twins are not exact: they are held to (b), (c), (d).

Cases per entry point and family at the time of writing (exact / Swish twins; `python tests/exact_ref.py --count` prints them):
    gemm_nt      generic 112 / 47, small 37 / 12, st 22 / 11, sw 12 / 6, swg 21 / 21, ws 28 / 10
    gemm_tn      dma 48 / 16, generic 9 / 6, slab 111 / 57
    expand_bwd   stream 21, k_expand_bwd 18 (the cases with the x M + v term also run gram and xb_coeffs)
    project_bwd  38 / 34, and 4 layout queries answered "no"
Every case with an activation has its twin; cases that differ in the code 1 / 2 alone share one.
"""
import json
import os

import pytest
import torch

import exact_ref as X

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = X.CAP


def _below(t, what):
    assert float(t.abs().max()) < CAP, "%s reaches %.0f" % (what, float(t.abs().max()))


def _ints(c, *tensors):
    for i, t in enumerate(tensors):
        if t is not None:
            X.check_integer(t, "tensor %d" % i)


def _operand_ok(o, name, exact):
    X.check_coverage(o.eff, name)
    if exact:
        _ints(None, o.a, o.a2, o.c1, o.c2, o.c3, o.eff)


def _nt_case_ok(r):
    c = X.build_nt(r)
    M, N, K = r["M"], r["N"], r["K"]
    _operand_ok(c.A, "A", c.exact)
    assert bool((c.W != 0).any(0).all()) and bool((c.W != 0).any(1).all()), "a k or an output column without a weight"
    X.check_activation_mix(c)
    if c.exact:
        _ints(c, c.W, c.bias, c.add, c.Z.a if c.Z is not None else None)
        _below(c.mag, "sum |terms| of an output")
        for t, what in ((c.out.abs().sum(0), "sum |c|"), ((c.out * c.out).sum(0), "sum c^2"), (c.second.abs().sum(0), "sum |second|")):
            _below(t, what)
        assert bool((c.out == c.out.round()).all())
    b = X.nt_buffers(c, "cpu")
    X.check_padding(b.a, K)
    X.check_packed(b.wp, N, K)
    X.check_padding(b.c, N, poisoned=True)
    X.check_stats_buf(b.stats, N)
    for k, C in (("a2", K), ("add", N), ("z", N)):
        if b.kw.get(k) is not None:
            X.check_padding(b.kw[k], C)
    for k, C in (("ac1", K), ("ac2", K), ("ac3", K), ("zscale", N), ("zshift", N), ("bias", N)):
        if b.kw.get(k) is not None:
            assert b.kw[k].numel() % 8 == 0 and float(b.kw[k][C:].abs().sum()) == 0.0


def _tn_case_ok(r):
    c = X.build_tn(r)
    _operand_ok(c.U, "U", c.exact)
    _operand_ok(c.V, "V", c.exact)
    X.check_activation_mix(c)
    if c.exact:
        _ints(c, c.prefill)
        _below(c.mag, "sum |u v| + |pre-fill|")
        assert bool((c.prod != 0).any()), "nothing to accumulate"
    b = X.tn_buffers(c, "cpu")
    X.check_padding(b.u, r["NU"])
    X.check_padding(b.v, r["NV"])
    for k, C in (("u2", r["NU"]), ("v2", r["NV"])):
        if b.kw.get(k) is not None:
            X.check_padding(b.kw[k], C)


def _xb_case_ok(r):
    c = X.build_xb(r)
    M, inp, hid = r["M"], r["inp"], r["hid"]
    assert X.xb_supported(inp, hid)
    _operand_ok(c.H, "h", True)
    _operand_ok(c.X, "x", True)
    assert bool((c.Wt != 0).any(0).all()) and bool((c.Wt != 0).any(1).all())
    _ints(c, c.Wt, c.c1, c.c2, c.c3, c.add, c.prefill, c.vb)
    X.check_integer(c.mp, "mp", bound=CAP)
    for t, what in ((c.mag, "sum |terms| of gx"), (c.dwe_mag, "sum |terms| of dWe"), (c.dwe1_mag, "sum |terms| of the corrections"),
                    (c.gram, "Gram matrix"), (c.Wt.abs() @ (c.c2.abs().view(-1, 1) * c.Wt.abs().t()), "sum |terms| of M")):
        _below(t, what)
    b = X.xb_buffers(c, "cpu")
    X.check_padding(b.h, hid)
    X.check_padding(b.x, inp)
    X.check_packed(b.wt, inp, hid)
    X.check_packed(b.wexp, hid, inp)
    X.check_padding(b.gx, inp, poisoned=True)
    if b.add is not None:
        X.check_padding(b.add, inp)
    assert float(b.mp.float().abs().max()) == 0.0 and bool(torch.isnan(b.gram).all()) and bool(torch.isnan(b.sx).all())


def _pb_case_ok(r):
    c = X.build_pb(r)
    M, oup, hid = r["M"], r["oup"], r["hid"]
    assert X.pb_expected(r)
    _operand_ok(c.G, "dP", c.exact)
    _operand_ok(c.Z, "z", c.exact)
    assert bool((c.Wt != 0).any(0).all()) and bool((c.Wt != 0).any(1).all())
    X.check_activation_mix(c)
    if c.exact:
        _ints(c, c.Wt, c.prefill)
        for t, what in ((c.mag, "sum |terms| of gh"), (c.dwp_mag, "sum |terms| of dWp"), (c.gh.abs().sum(0), "sum |gh|"),
                        (c.second.abs().sum(0), "sum |gh z|")):
            _below(t, what)
    b = X.pb_buffers(c, "cpu")
    X.check_padding(b.g, oup)
    X.check_padding(b.z, hid)
    X.check_packed(b.wpt, hid, oup)
    X.check_padding(b.gh, hid, poisoned=True)
    X.check_stats_buf(b.stats, hid)


@pytest.mark.parametrize("table,check", [(X.nt_cases, _nt_case_ok), (X.nt_twins, _nt_case_ok), (X.tn_cases, _tn_case_ok),
                                         (X.tn_twins, _tn_case_ok), (X.xb_cases, _xb_case_ok), (X.pb_cases, _pb_case_ok),
                                         (X.pb_twins, _pb_case_ok)], ids=lambda f: getattr(f, "__name__", None))
def test_every_case_holds_its_preconditions(table, check):
    rows = table()
    assert rows, "empty table"
    for r in rows:
        try:
            check(r)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (X.name_of(r), e))


def test_tables_cover_the_families_and_both_answers_of_the_queries():
    pinned = json.load(open(os.path.join(HERE, "golden", "pw_dispatch.json")))
    assert {r["family"] for r in pinned["gemm_nt"]} <= {X.nt_family(r) for r in X.nt_cases()}
    # with the streaming families off, their shapes run ws / generic and the expand cases k_expand_bwd
    assert {X.nt_family(r, off=True) for r in X.nt_cases() if X.nt_family(r) in ("sw", "swg", "st")} == {"ws", "generic"}
    assert {X.xb_family(r) for r in X.xb_cases()} == {"stream", "k_expand_bwd"} and {X.xb_family(r, off=True) for r in X.xb_cases()} == {"k_expand_bwd"}
    assert {X.tn_family(r) for r in X.tn_cases()} == {"dma", "slab", "generic"}
    # gemm_tn instances (tn_plan, 256 CUs).  dma: every U width, and per NU the cross of V's prologue, activation code and layout
    dma = [r for r in X.tn_cases() if X.tn_family(r) == "dma"]
    assert {X.tn_plan(r)["utt"] for r in dma} == {4, 6, 12, 10}
    for NU in {r["NU"] for r in dma}:
        assert {(r["v_mode"], r["v_act"], r["v"]) for r in dma if r["NU"] == NU} == {
            (m, a, lay) for m, a in ((X.PRO_NONE, 0), (X.PRO_BNRELU, 1), (X.PRO_BNRELU, 2)) for lay in ("plain", "slab")}, NU
    # slab: with a workspace reduction every width in the narrow form, widths 4 .. 12 in the wide form, each with every prologue pair
    slab = [(r, X.tn_plan(r)) for r in X.tn_cases() if X.tn_family(r) == "slab"]
    forms = {(u, False) for u in (2, 4, 6, 12, 10, 20)} | {(u, True) for u in (4, 6, 12, 10)}
    for pair in X.TN_PAIRS:
        assert {(p["utt"], p["wide"]) for r, p in slab if p["chunks"] > 1 and (r["u_mode"], r["v_mode"]) == pair} == forms, pair
    assert {(r["u_mode"], r["v_mode"]) for r, p in slab if p["narrowed"]} == set(X.TN_PAIRS)
    assert any(p["narrowed"] and p["utt"] == 2 for r, p in slab) and any(p["narrowed"] and p["utt"] > 2 for r, p in slab)
    assert any(p["xcd"] and p["wide"] for r, p in slab) and any(p["xcd"] and not p["wide"] for r, p in slab)
    assert any(p["chunks"] == 1 and not r["ws"] and r["M"] >= 512 for r, p in slab)
    # generic gemm_nt: one and two live 64-channel chunks in both storage types
    for dt in (0, 1):
        assert {X.nt_generic_chunks(r) for r in X.nt_cases() if X.nt_family(r) == "generic" and r["dt"] == dt} == {1, 2}, dt
    assert {ok for _, _, ok in X.XB_QUERIES} == {0, 1} and all(X.xb_supported(i, h) == bool(ok) for i, h, ok in X.XB_QUERIES)
    assert all(X.pb_expected(r) for r in X.pb_cases()) and not any(X.pb_expected(r) for r in X.PB_QUERIES_NO)
    assert {(r["z"], r["tr"]) for r in X.pb_cases()} == {("slab", 0), ("slab", 1), ("plain", 0), ("plain", 1)}
    # twins are the tables' own cases with code 3
    assert all(r["act"] == 3 or r["mask"] == 3 for r in X.nt_twins()) and all(r["act"] == 3 for r in X.pb_twins())
    assert all(3 in (r["u_act"], r["v_act"]) for r in X.tn_twins())
    # activation codes 1 and 2 reach the prologue and the mask of every gemm_nt family that takes them
    for fam in ("small", "ws", "generic"):
        rows = [r for r in X.nt_cases() if X.nt_family(r) == fam]
        assert {r["act"] for r in rows} >= {1, 2} and {r["mask"] for r in rows} >= {1, 2}, fam
    assert {r["mask"] for r in X.nt_cases() if X.nt_family(r) == "st"} >= {0, 1, 2}
