"""csrc/shrink.hip at kernel level (GPU): the alive masks with their ascending kept-channel indices across the 256-element scan boundary,
and the index-packed gathers, single and as one launch over a job table.  Integer and copy results: compared exactly with
tests/glue_ref.py (torch.nonzero, plain indexing), outputs inside sentinel-filled allocations.

Single-line change to csrc/shrink.hip seen to be caught (scratch build): `>= thr` for `> thr` in k_gamma_mask -> test_gamma_mask...[0], [1].
"""
import numpy as np
import pytest
import torch

import glue_ref as R
import glue_util as G

pytestmark = pytest.mark.gpu

MASK_DT = np.dtype([("off", "<i8"), ("count", "<i4"), ("out_off", "<i4")])
THR = 0.25      # exact in fp32: values AT the threshold are dead (the comparison is strict)


def _mask_case():
    gen = torch.Generator().manual_seed(21)
    counts = [1, 255, 256, 257, 600, 300, 300, 1]        # the last three: all dead, all alive, a single dead channel
    jobs, off, out_off = [], 19, 5
    for c in counts:
        jobs.append((off, c, out_off))
        off += c + 13
        out_off += c + 3                                   # gaps in the outputs keep their sentinel
    n = off + 7
    p = torch.rand(n, generator=gen) - 0.5                 # |.| <= 0.5: about half alive
    e = torch.rand(n, generator=gen) - 0.5
    for t in (p, e):
        t[::5] = THR
        t[2::11] = -THR
    o, c, _ = jobs[5]
    p[o:o + c] = 0.125
    e[o:o + c] = -THR
    o, c, _ = jobs[6]
    p[o:o + c] = -0.5
    e[o:o + c] = 0.375
    o, c, _ = jobs[7]
    p[o], e[o] = THR, -THR
    o, c, _ = jobs[0]
    p[o], e[o] = 0.3, 0.1
    # channel 255 and 256 of the 257- and 600-channel jobs alive: the scan hands its base across the chunk boundary
    for j in (3, 4):
        o = jobs[j][0]
        p[o + 255], p[o + 256], e[o + 255], e[o + 256] = 0.4, -0.4, -0.3, 0.3
    return jobs, n, p, e, out_off


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gamma_mask_counts_index_and_threshold(gpu_lib, mode):
    """mask, ascending index and kept count of every job equal alive_ref's bit for bit; the index occupies out_off + [0, kept) and the rest
    of the slot (and every gap) keeps its sentinel; a value equal to the threshold is dead"""
    from atomnas_amd import ops
    jobs, n, p, e, nout = _mask_case()
    tab = torch.from_numpy(np.array(jobs, dtype=MASK_DT).view(np.uint8).copy()).cuda()
    mask, index, kept = G.Vec(nout, torch.uint8), G.Vec(nout, torch.int32, marker=-7), G.Vec(len(jobs), torch.int32, marker=-7)
    want_mask, want_index, want_kept = (torch.full((nout,), 113, dtype=torch.uint8), torch.full((nout,), -7, dtype=torch.int32), [])
    for off, cnt, oo in jobs:
        m, idx, k = R.alive_ref(p[off:off + cnt], e[off:off + cnt], THR, mode)
        want_mask[oo:oo + cnt] = m.to(torch.uint8)
        want_index[oo:oo + k] = idx.to(torch.int32)
        want_kept.append(k)
    assert want_kept[5] == 0 and want_kept[6] == 300 and want_kept[7] == 0 and 0 < want_kept[4] < 600
    ops.gamma_mask(p.cuda(), e.cuda() if mode != 0 else None, tab, len(jobs), THR, mode, mask.v, index.v, kept.v)
    torch.cuda.synchronize()
    assert kept.check("kept").tolist() == want_kept
    assert torch.equal(mask.check("mask").cpu(), want_mask)
    assert torch.equal(index.check("index").cpu(), want_index)


@pytest.mark.parametrize("count", [1, 255, 256, 257, 600])
def test_mask_index_single(gpu_lib, count):
    """atomnas_mask_index through gather_by_mask's undeferred path is covered below; here the raw entry point on one mask"""
    from atomnas_amd import _lib, ops
    gen = torch.Generator().manual_seed(count)
    m = (torch.rand(count, generator=gen) > 0.4).to(torch.uint8)
    m[-1] = 1
    m8, index, kept = G.Vec(count, torch.uint8, fill=m), G.Vec(count, torch.int32, marker=-7), G.Vec(1, torch.int32, marker=-7)
    _lib.call("atomnas_mask_index", ops._p(m8.v), count, ops._p(index.v), ops._p(kept.v), ops._stream())
    torch.cuda.synchronize()
    idx = torch.nonzero(m).flatten().to(torch.int32)
    assert kept.check().tolist() == [idx.numel()]
    assert torch.equal(index.check("index", upto=idx.numel()).cpu(), idx)


def _nan_like(shape):
    full = torch.full((int(np.prod(shape)) + 64,), G.NAN, dtype=torch.float32, device="cuda")
    return full, full[32:32 + int(np.prod(shape))].view(shape)


def _same_bytes(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def test_gather_by_mask_undeferred(gpu_lib):
    """dst <- src[mask] (dim 0), src[:, mask] contiguous with an inner extent, and src[:, mask] of a strided band, exactly; 300 channels
    (the index crosses the scan's 256 boundary); nothing written around the destination"""
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(33)
    n = 300
    mask = torch.rand(n, generator=gen) > 0.35
    mask[255], mask[256] = True, True
    k = int(mask.sum())
    md = mask.cuda()
    # dim 0
    src = torch.randn(n, 3, 5, generator=gen)
    full, dst = _nan_like((k, 3, 5))
    ops.gather_by_mask(dst, src.cuda(), md, 0)
    torch.cuda.synchronize()
    assert _same_bytes(dst, R.gather_ref(src, mask, 0)) and bool(torch.isnan(full[:32]).all()) and bool(torch.isnan(full[32 + dst.numel():]).all())
    # dim 1, contiguous, inner = 9
    src = torch.randn(7, n, 3, 3, generator=gen)
    full, dst = _nan_like((7, k, 3, 3))
    ops.gather_by_mask(dst, src.cuda(), md, 1)
    torch.cuda.synchronize()
    assert _same_bytes(dst, R.gather_ref(src, mask, 1)) and bool(torch.isnan(full[:32]).all()) and bool(torch.isnan(full[32 + dst.numel():]).all())
    # dim 1, a band [11][n] of a wider matrix into a band [11][k] of a wider matrix: everything else of the destination stays NaN
    wide = torch.randn(11, n + 40, generator=gen)
    full, dwide = _nan_like((11, k + 24))
    ops.gather_by_mask(dwide[:, 8:8 + k], wide.cuda()[:, 17:17 + n], md, 1)
    torch.cuda.synchronize()
    want = torch.full((11, k + 24), G.NAN)
    want[:, 8:8 + k] = wide[:, 17:17 + n][:, mask]
    assert _same_bytes(dwide, want) and bool(torch.isnan(full[:32]).all()) and bool(torch.isnan(full[32 + dwide.numel():]).all())


def test_gather_jobs_table_of_300(gpu_lib):
    """one launch over 300 recorded jobs of 1..700 elements -- far more jobs than elements per workgroup, so most workgroups sit at a job
    boundary of the binary search: masked dim-0 gathers, identity copies (copy_job) of contiguous tensors and of bands; every
    destination lies in one NaN-filled arena, which must equal the arena built with plain indexing, byte for byte"""
    from atomnas_amd import ops
    gen = torch.Generator().manual_seed(44)
    arena = torch.full((300 * 800,), G.NAN, dtype=torch.float32, device="cuda")
    want = torch.full((300 * 800,), G.NAN, dtype=torch.float32)
    keep = []
    ops.gather_defer(True)
    try:
        for j in range(300):
            base = j * 800 + (j % 7)
            kind = j % 3
            if kind == 0:      # masked rows of [n][inner]
                inner = 1 + j % 5
                n = 1 + (j * 37) % (700 // inner)
                mask = torch.rand(n, generator=gen) > 0.3
                mask[(j * 5) % n] = True
                k = int(mask.sum())
                src = torch.randn(n, inner, generator=gen)
                dst = arena[base:base + k * inner].view(k, inner)
                md, sd = mask.cuda(), src.cuda()
                keep.append((md, sd))
                ops.gather_by_mask(dst, sd, md, 0)
                want[base:base + k * inner] = src[mask].reshape(-1)
            elif kind == 1:    # identity, contiguous
                n = 1 + (j * 53) % 700
                src = torch.randn(n, generator=gen)
                assert ops.copy_job(arena[base:base + n], src.cuda())
                want[base:base + n] = src
            else:              # identity into a band [rows][cols] of a matrix with pitch cols + 3
                rows, cols = 1 + j % 9, 1 + (j * 11) % 60
                src = torch.randn(rows, cols, generator=gen)
                dst = torch.as_strided(arena, (rows, cols), (cols + 3, 1), base)
                assert ops.copy_job(dst, src.cuda())
                torch.as_strided(want, (rows, cols), (cols + 3, 1), base).copy_(src)
        assert ops.gather_flush() == 300
    finally:
        ops.gather_defer(False)
    torch.cuda.synchronize()
    assert _same_bytes(arena, want)
