"""The small launches of the training step whose memory access or launch geometry was reworked (GPU): the tiled weight pack
(csrc/optim.hip k_pack), the fixed-order reduction of partial weight gradients with 16-byte loads (csrc/reduce.hip) and the GEMMs at the
classifier's shapes (M = the batch: the small-M rules of nt_generic_plan and tn_slab_plan); and the masked-gradient + statistics pass
(csrc/bn.hip k_act_bwd_stats) at the block-output widths whose channel-group count is no power of two, which was measured and left as it
was (profiles/stragglers_bench.txt): its cases pin the row layout any later change of that geometry has to keep.

The reduction has no entry point of its own: it is reached through the weight-gradient GEMM, whose fp32 form makes exactly `parts` row
chunks when it is given M = 256 * parts rows and a workspace of parts * NU * NV floats (csrc/pwconv_tn.hip tn_generic_plan), with
n = NU * NV elements per partial and part_stride = n (so n = 1, 31, 1000 / 36 / 32 cover unaligned rows, aligned rows with a ragged last
lane, and whole 16-byte rows).  parts = 1 runs without a reduction at all; it is kept as the base case of the same comparison.

Bounds: a fixed-order fp32 sum of n terms is within (n + 8) u sum |terms| of the float64 sum (tests/glue_util.py), u = 2^-24.
"""
import numpy as np
import pytest
import torch

import glue_ref as R
import glue_util as G
from glue_util import U, pad8
from kutil import assert_close, tol

pytestmark = pytest.mark.gpu

PACK_DT = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("src_ld", "<i4"), ("dst_ld", "<i4"),
                    ("c_off", "<i4"), ("mode", "<i4")])
PACK_SHAPES = [(1, 1), (5, 7), (33, 65), (64, 64), (130, 24), (49, 144)]


def _table(dt, rows):
    tab = np.zeros(len(rows), dtype=dt)
    for i, r in enumerate(rows):
        tab[i] = r
    return torch.from_numpy(tab.view(np.uint8).copy()).cuda()


# ---------------------------------------------------------------------------------------------------------------- weight packing
def _pack_jobs(mode, shapes, variant):
    """jobs of one mode laid out back to back in one destination; variant 0: everything aligned and tight, 1: odd source / destination
    offsets, src_ld > cols, c_off != 0 and dst_ld wider than the logical width.  Returns (jobs, source elements, destination elements)."""
    jobs, so, do = [], 0, 0
    for i, (rows, cols) in enumerate(shapes):
        odd = variant == 1
        c_off = (3 + i) if odd else 0
        src_ld = cols + (5 if odd else 0)
        so += (1 + i) if odd else (-so) % 4
        if mode == 0:
            dst_ld, drows = c_off + cols + (6 if odd else 0), rows
        elif mode == 1:
            dst_ld, drows = rows + (7 if odd else 0), c_off + cols
        else:
            dst_ld, drows = c_off + rows + (9 if odd else 0), cols
        do += (1 + 2 * i) if odd else (-do) % 4
        jobs.append(dict(src_off=so, dst_off=do, rows=rows, cols=cols, src_ld=src_ld, dst_ld=dst_ld, c_off=c_off, mode=mode))
        so += rows * src_ld
        do += drows * dst_ld
    return jobs, so + 8, do + 8


def _pack_expect(arena, jobs, n_dst, dtype):
    """plain torch indexing: the sentinel everywhere but on the jobs' elements"""
    want = torch.full((n_dst,), G.NAN, dtype=dtype)
    for jb in jobs:
        r, c = jb["rows"], jb["cols"]
        src = torch.as_strided(arena, (r, c), (jb["src_ld"], 1), jb["src_off"])
        if jb["mode"] == 0:
            dst = torch.as_strided(want, (r, c), (jb["dst_ld"], 1), jb["dst_off"] + jb["c_off"])
        elif jb["mode"] == 1:
            dst = torch.as_strided(want, (r, c), (1, jb["dst_ld"]), jb["dst_off"] + jb["c_off"] * jb["dst_ld"])
        else:
            dst = torch.as_strided(want, (r, c), (1, jb["dst_ld"]), jb["dst_off"] + jb["c_off"])
        dst.copy_(src.to(dtype))
    return want


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", G.DTYPES)
def test_pack_tiles_every_mode_and_edge(gpu_lib, dt, mode, variant):
    """all six job shapes in ONE launch (single elements, ragged tiles, whole tiles, several tiles in either direction, the depthwise tap
    table), aligned and with odd offsets / c_off / padded pitches: the packed bytes equal torch's `.to(dtype)` of the indexed source, and
    every element no job owns keeps its sentinel.  Mode 2 stores fp32 whatever the storage type."""
    from atomnas_amd import ops
    dtype = G.T(dt)
    out_dtype = torch.float32 if mode == 2 else dtype
    jobs, n_src, n_dst = _pack_jobs(mode, PACK_SHAPES, variant)
    arena = torch.randn(n_src, generator=torch.Generator().manual_seed(17 + mode))
    want = _pack_expect(arena, jobs, n_dst, out_dtype)
    buf = torch.full((n_dst,), G.NAN, dtype=out_dtype, device="cuda")
    tab = _table(PACK_DT, [tuple(jb[k] for k in PACK_DT.names) for jb in jobs])
    ops.pack_weights(arena.cuda(), buf, tab, len(jobs), dtype)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf.cpu()), _bits(want)), "packed bytes differ (values or a write outside the jobs)"
    # two jobs alone in a launch, the later one first
    buf2 =torch.full((n_dst,), G.NAN, dtype=out_dtype, device="cuda")
    two = [jobs[4], jobs[2]]
    ops.pack_weights(arena.cuda(), buf2, _table(PACK_DT, [tuple(jb[k] for k in PACK_DT.names) for jb in two]), 2, dtype)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf2.cpu()), _bits(_pack_expect(arena, two, n_dst, out_dtype)))


# ---------------------------------------------------------------------------------------------------------------- reduction
RED_N = {1: (1, 1), 31: (31, 1), 32: (4, 8), 36: (6, 6), 1000: (25, 40)}   # n -> (NU, NV)
_RED_IN = {}


def _red_inputs(parts, n):
    """U, V of the weight-gradient GEMM that makes `parts` partials of n elements, and the float64 result with its bound; made once"""
    if (parts, n) not in _RED_IN:
        NU, NV = RED_N[n]
        M = 256 * parts
        g = torch.Generator().manual_seed(1000 * parts + n)
        Uc, Vc = torch.randn(M, NU, generator=g), torch.randn(M, NV, generator=g)
        pad = lambda t, c: torch.cat([t, torch.zeros(M, pad8(c) - c)], 1).cuda()
        ref = Uc.double().t() @ Vc.double()
        # every product is rounded once (or fused), then M terms are added in a fixed order, then the sum is added to `out`
        bound = G.sum_bound(M + 2, Uc.double().abs().t() @ Vc.double().abs())
        _RED_IN[(parts, n)] = (pad(Uc, NU), pad(Vc, NV), ref, bound, M)
    return _RED_IN[(parts, n)]


def _red_out(NU, NV, layout):
    """prefilled output and (si, sj, view of the [NU][NV] result)"""
    if layout == "contig":
        o = torch.full((NU, NV), 0.5, device="cuda")
        return o, NV, 1, o
    if layout == "padded":                                 # inner = NV < n elements per row, rows NV + 3 apart
        o = torch.full((NU, NV + 3), 0.5, device="cuda")
        return o, NV + 3, 1, o[:, :NV]
    o = torch.full((NV, NU + 2), 0.5, device="cuda")       # transposed: s_inner = NU + 2, s_outer = 1
    return o, 1, NU + 2, o[:, :NU].t()


@pytest.mark.parametrize("n", [1, 31, 32, 36, 1000])
@pytest.mark.parametrize("parts", [1, 7, 8, 9, 33, 64])
def test_reduce_vector_loads_keep_the_sums(gpu_lib, parts, n):
    """`parts` partial outputs of n elements: the immediate reduction (k_reduce_parts) and the deferred, batched one (k_reduce_batch, two
    jobs of different layouts in one flush) give the same bits, accumulate into a prefilled output in its contiguous, padded and
    transposed layouts, write nothing beside it, and lie within the fixed-order bound of the float64 sums."""
    from atomnas_amd import ops
    NU, NV = RED_N[n]
    Ub, Vb, ref, bound, M = _red_inputs(parts, n)
    ws_floats = max(parts, 1) * NU * NV
    got = {}
    for defer in (False, True):
        outs = [_red_out(NU, NV, lay) for lay in ("contig", "padded", "transposed")]
        wss = [G.Vec(ws_floats) for _ in outs]
        if defer:
            ops.reduce_defer(True)
        try:
            for (o, si, sj, _), ws in zip(outs, wss):
                ops.gemm_tn(Ub, NU, Vb, NV, o, si, sj, M, ws=ws.v if parts > 1 else False)
            if defer:
                ops.reduce_flush()
        finally:
            if defer:
                ops.reduce_defer(False)
        torch.cuda.synchronize()
        for ws in wss:
            ws.check("partial workspace")
        got[defer] = [o.clone() for o, _, _, _ in outs]
        for (o, si, sj, view), lay in zip(outs, ("contig", "padded", "transposed")):
            G.assert_within("%s parts%d n%d" % (lay, parts, n), view, 0.5 + ref, bound + 8 * U * (0.5 + ref.abs()))
            assert torch.equal(view, outs[0][3]), "the output layout changed the sums"
            if lay == "padded":
                assert bool((o[:, NV:] == 0.5).all()), "a write between the rows"
            if lay == "transposed":
                assert bool((o[:, NU:] == 0.5).all()), "a write between the rows"
    for a, b in zip(got[False], got[True]):
        assert torch.equal(a, b), "deferred and immediate reductions differ"


# ---------------------------------------------------------------------------------------------------------------- act_bwd_stats
def _used_rows(M, C, stat_rows):
    """workgroup columns of the launch (csrc/bn.hip stat_geom): one statistics row each"""
    ncg, lcg = (C + 7) // 8, 0
    while (1 << lcg) < ncg and lcg < 5:
        lcg += 1
    pl = 256 >> lcg
    return min((M + pl - 1) // pl, 2048, stat_rows)


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("C", [8, 16, 24, 40, 80, 96, 320])
def test_act_bwd_stats_real_group_counts(gpu_lib, C, dt):
    """the block-output widths (3, 5, 10, 12 and 2 x 20 channel groups among them) at pitch C + 8, M in {1, 63, 257, 4099} (no full trip
    of the unrolled loop, a ragged one, several), stat_rows as ops.stat_rows_for gives it and 3 (a grid far smaller than the pixels ask
    for): every activation code and the unmasked form, with and without g.  The rows sum to the float64 sums of the stored g within the
    bound tests/test_bn_kernels_gpu.py uses, rows beyond the launch's workgroup columns are zero, and a second run gives the same bits."""
    from atomnas_amd import ops
    from test_bn_kernels_gpu import SWISH_BWD_K, swish_bound
    dtype = G.T(dt)
    gen = torch.Generator().manual_seed(7 * C + 1)
    ld = C + 8
    k = 0
    for M in (1, 63, 257, 4099):
        for srows in (ops.stat_rows_for(C), 3):
            k += 1
            act = (None, 1, 2, 3, 0)[k % 5]                # None: unmasked (scale == NULL)
            want_g = k % 3 != 0
            if act is None:
                sc = sh = None
                zs = torch.randn(M, C, generator=gen).to(dtype).double()
                pre = zs
            else:
                sc = ((torch.rand(C, generator=gen) + 0.5) * torch.where(torch.rand(C, generator=gen) > 0.3, 1.0, -1.0)).float().double()
                sh = (torch.randn(C, generator=gen) * 0.5).float().double()
                zs = G.margin_input(gen, M, C, sc, sh, act, dtype) if act in (1, 2) else torch.randn(M, C, generator=gen).to(dtype).double()
                pre = zs * sc + sh
            Z, DY = G.Act(M, C, ld, dtype, zs), G.Act(M, C, ld, dtype, torch.randn(M, C, generator=gen))
            dys = DY.stored()
            g_ref = R.act_grad_ref(pre, act or 0, dys)
            scv, shv = (G.cvec(sc, C), G.cvec(sh, C)) if sc is not None else (None, None)
            runs = []
            for _ in range(2):
                Gt = G.Act(M, C, ld, dtype) if want_g else None
                sv, sview = G.stats_buf(srows, C)
                ops.act_bwd_stats(DY.t, Z.t, scv.v if scv else None, shv.v if shv else None, act or 0, Gt.t if Gt else None, sview, M, C,
                                  stat_rows=srows)
                runs.append((Gt, sv, sview))
            torch.cuda.synchronize()
            tag = "C%d M%d rows%d act%s" % (C, M, srows, act)
            (Gt, sv, sview), (Gt2, _, sview2) = runs
            assert torch.equal(sview, sview2) and (not want_g or torch.equal(Gt.t[:, :C], Gt2.t[:, :C])), tag + ": two runs differ"
            base = 8 * U * g_ref.abs()
            if act == 3:
                base = base + 0.5 * dys.abs() * 8 * U * ((zs * sc).abs() + sh.abs())
            g_sum_ref = g_ref
            if want_g:
                got = Gt.read(tag + " g")
                bound = swish_bound("bwd", base, g_ref, got, dtype) if act == 3 else base + (2.0 ** -8 * g_ref.abs() if dtype == torch.bfloat16 else 0.0)
                G.assert_within(tag + " g", got, g_ref, bound)
                if not (act == 3 and dtype == torch.bfloat16):
                    g_sum_ref = got                        # the stored values (swish in bf16 sums the unrounded gradient)
            tot = G.stats_total(sv, sview, tag + " statistics")
            used = _used_rows(M, C, srows)
            assert bool((sview[used:] == 0).all()), tag + ": rows beyond the launch's workgroup columns are not zero"
            e_el = torch.zeros_like(g_ref) if g_sum_ref is not g_ref or act != 3 else torch.minimum(SWISH_BWD_K * base, base + 2.0 ** -8 * g_ref.abs())
            for pl, terms, name in ((0, g_sum_ref, "sum g"), (1, g_sum_ref * zs, "sum g z")):
                eterm = e_el if pl == 0 else e_el * zs.abs()
                G.assert_within("%s %s" % (tag, name), tot[pl], terms.sum(0), G.sum_bound(M, terms.abs().sum(0)) + eterm.sum(0))


# ---------------------------------------------------------------------------------------------------------------- classifier shapes
def _pack_w(w, dtype):
    n, k = w.shape
    buf = torch.zeros((n + 63) // 64 * 64, (k + 31) // 32 * 32, dtype=dtype, device="cuda")
    buf[:n, :k] = w.to(dtype).cuda()
    return buf


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("K", [72, 1280])
@pytest.mark.parametrize("N", [40, 1000])
@pytest.mark.parametrize("M", [1, 37, 256])
def test_gemm_nt_batch_sized_m(gpu_lib, M, N, K, dt):
    """C = A W^T with M = a batch of pooled rows (the classifier and its input gradient), no prologue: torch on the rounded operands,
    an output that arrived as NaN, two launches with equal bits"""
    from atomnas_amd import ops
    dtype = G.T(dt)
    g = torch.Generator().manual_seed(M + 3 * N + 5 * K)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    Ab = torch.cat([A.to(dtype), torch.zeros(M, pad8(K) - K, dtype=dtype)], 1).cuda()
    ref = A.to(dtype).double() @ W.to(dtype).double().t()
    outs = []
    for _ in range(2):
        Cb = torch.zeros(M, pad8(N), dtype=dtype, device="cuda")
        Cb[:, :N] = G.NAN
        ops.gemm_nt(Ab, _pack_w(W, dtype), Cb, M, N, K)
        outs.append(Cb)
    torch.cuda.synchronize()
    t = tol(dtype)
    assert_close("C", outs[0][:, :N], ref, t["rtol"], t["atol"] * max(1.0, float(ref.abs().max())))
    assert torch.equal(_bits(outs[0].cpu()), _bits(outs[1].cpu()))
    if pad8(N) > N:
        assert float(outs[0][:, N:].abs().max()) == 0.0


@pytest.mark.parametrize("dt", G.DTYPES)
@pytest.mark.parametrize("NV", [40, 1280])
@pytest.mark.parametrize("NU", [24, 1000])
@pytest.mark.parametrize("M", [37, 256])
def test_gemm_tn_batch_sized_m(gpu_lib, M, NU, NV, dt):
    """out += U^T V over M = a batch of rows (the classifier's weight gradient): torch on the rounded operands, an accumulator that
    starts at zero inside a NaN allocation, two launches with equal bits"""
    from atomnas_amd import ops
    dtype = G.T(dt)
    g = torch.Generator().manual_seed(M + 3 * NU + 5 * NV)
    Uc, Vc = torch.randn(M, NU, generator=g), torch.randn(M, NV, generator=g)
    pad = lambda t, c: torch.cat([t.to(dtype), torch.zeros(M, pad8(c) - c, dtype=dtype)], 1).cuda()
    ref = Uc.to(dtype).double().t() @ Vc.to(dtype).double()
    outs = []
    for _ in range(2):
        o = G.Vec(NU * NV, fill=0.0)
        ops.gemm_tn(pad(Uc, NU), NU, pad(Vc, NV), NV, o.v, NV, 1, M)
        outs.append(o)
    torch.cuda.synchronize()
    a, b = (o.check("out").view(NU, NV) for o in outs)
    t = tol(dtype)
    assert_close("out", a, ref, t["rtol"], t["atol"] * max(1.0, float(ref.abs().max())))
    assert torch.equal(a, b)
