"""Kernel-level parity (GPU) of the Squeeze-and-Excitation entry points of csrc/se.hip (se_squeeze, se_mlp_fwd, se_scale, se_bwd_gate,
se_bwd_apply) per block activation (none, ReLU, ReLU6, Swish), storage type (fp32, bf16), activation layout (plain, slab-major) and
call form, in the manner of tests/test_dwconv_family_gpu.py.  tests/test_se_gpu.py keeps the wide AtomNAS-C+ shapes in Swish.

Reference: kutil.se_reference, float64 on the CPU with every derivative written out (cross-checked against autograd by
tests/test_se_reference.py, which needs no GPU).  The block's pre-activations come from glue_util.margin_input: at least 2^-6 from 0
(and from 6 in mode 2) after the rounding to the storage type, so no fp32 pre-activation lands on the other side of a bound and NO
outliers are allowed; a mode-2 case has at least 5 % of them above 6 and 5 % below 0 (asserted by the helper).

Shapes (CASES): the smallest that reach each path of the kernels.  Every case asserts ops.se_pool_parts against the value in its row:
a change of se_pool_parts fails the case instead of letting it check another path.  The gate activation alternates between ReLU
and Swish over the rows; every row runs in all four block modes.

Bounds.  Everything fp32 -- pooled, hpre, gate, dz2, dz1, dpooled in either storage type, S in fp32 -- rtol 1e-4, atol 1e-5 and g in fp32
rtol 1e-4, atol 2e-5, as tests/test_se_gpu.py.  The weight gradients, as the increment over non-zero base values: rtol 1e-3,
atol 2e-5 max(1, |ref|_max) sqrt(N HW), as that file.  S and g stored as bf16 are ONE round-to-nearest of an fp32 value: half an ulp,
which is 2^-9 |v| just below a power of two and 2^-8 |v| just above one.  Their bound is 2^-8 |ref| plus that file's absolute floors
(1e-3 for S, 2e-3 for g), which take the fp32 error of the value that is rounded -- against that file's rtol 2e-2.
The statistics rows: against the float64 sums of the kernel's own stored g with that file's bound, and against the reference's sums
within the sum of g's element bounds.
Largest observed error / bound on an MI355X (printed with -s), fp32 / bf16 storage:
    S 0.0085 / 0.96    g 0.017 / 0.79    pooled 0.0073 / 0.0091    hpre 0.035 / 0.026    gate 0.0068 / 0.0036    dz2 0.28 / 0.27
    dz1 0.41 / 0.17    dpooled 0.35 / 0.23    dw1 0.0053 / 0.0020    db1 0.0035 / 0.0009    dw2 0.0025 / 0.0012    db2 0.0012 / 0.0009
The bf16 figures of S and g are elements just above a power of two, where half an ulp IS 2^-8 |v|: they cannot pass 1 while the fp32
error stays below the floor.  dz2, dz1 and dpooled are sums with cancellation held to an absolute 1e-5.

Wrong arithmetic these tests were seen to catch (scratch builds of the library with se.hip alone recompiled, never committed):
  ReLU6's upper bound 5 in act_of                       -> the 36 mode-2 cases of test_se_parity, the 4 mode-2 cases of test_se_exact_boundaries
  `a < m.hi` dropped from act_pass                      -> the same 40
  `a > m.lo` turned into `a >= m.lo`                    -> all 8 cases of test_se_exact_boundaries (nothing else holds a pre-activation of 0)
  the 1 / HW factor dropped from k_se_bwd_apply         -> 128 of test_se_parity (all but HW = 1), the 3 of test_se_mlp_narrow
  the last plane left out by k_se_mlp's select          -> the 64 cases of test_se_parity with parts 2, 4, 8, 16
  1 / (HW + 1) in k_se_pool                             -> all 144 of test_se_parity, the 3 of test_se_mlp_narrow
  Swish in k_se_scale whatever the mode                 -> the 108 cases of test_se_parity in modes 0, 1, 2, all 8 of test_se_exact_boundaries
The first three pass every test of tests/test_se_gpu.py.

Exact forms (test_se_forms): plain against slab-major, a rerun into fresh buffers, plain operands that are column views of wider
NaN-filled buffers (ld = HT + 16, first column 8), stats2 = None, stat_rows = 3 and ops.stat_rows_for(HT): bit-identical outputs
(the same kernel instance with the same thread-to-element map; fixed summation order, no atomics).

Exact boundaries (test_se_exact_boundaries): D in {-1, 0, 0.5, 5.5, 6, 6.5}, scale = 1, shift = 0, dS = 0.75, modes 1 and 2.  The
pre-activation is D itself, so S must be fl(act(D) * gate) of the kernel's own gate (one product, then one rounding to the storage type:
within 1 ulp, and 0 where D <= 0) and g must be exactly 0 at D in {-1, 0} and, in mode 2, at D in {6, 6.5}, non-zero elsewhere:
the strict inequalities of act_pass (csrc/common.h).

The narrow k_se_mlp instances (test_se_mlp_narrow): launch_se_mlp takes the largest G in {8, 4, 2, 1} images per workgroup whose
LDS, G (HT + hid + (1024 if HT <= 512)) * 4 bytes, fits the device's limit per workgroup (160 KiB = 163840 bytes on gfx950, common.h):
    HT  5200, hid 16:   8 * 20864 = 166912 > 163840,   4 * 20864 =  83456   -> G = 4
    HT 10400, hid  8:   4 * 41632 = 166528 > 163840,   2 * 41632 =  83264   -> G = 2
    HT 20608, hid  8:   2 * 82464 = 164928 > 163840,   1 * 82464            -> G = 1    (all three above 64 KiB: the opt-in path)
G = 8 fits while HT + hid <= 5120.  The test cannot observe which instance ran: it rests on this arithmetic and on the device limit.
N = 3 leaves a partial image group for G = 4 and G = 2.
"""
import functools
import types

import pytest
import torch

from kutil import act64, assert_close, se_layout, se_pack, se_reference

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
RELU, SWISH = 1, 3
ROWS = 64          # the default number of statistics rows of these tests, as tests/test_se_gpu.py
WIDE, WIDE_OFF = 16, 8
RATIO = {}

CASES = [
    # N, HW, branch widths, hid, HT, parts                reaches
    (3, 400, [3], 4, 16, 1),                    # cgb 2, PL 128; 13 dead channels in the only group pair
    (3, 301, [15, 23, 13], 5, 64, 2),           # parts 2 (plane clamp of k_se_mlp), ragged share 151 / 150, odd hid
    (3, 529, [15, 23, 13], 8, 64, 4),           # parts 4, shares 133 / 130
    (2, 1100, [15, 23, 13], 8, 64, 8),          # parts 8, shares 138 / 134
    (2, 784, [300], 24, 304, 16),               # parts 16 with cgb 32; JP 3 (threads 960..1023 idle in phase 2)
    (5, 25, [100, 90, 120], 33, 336, 1),        # JP 2; hid 33: the second k_se_wgrad row block holds one unit
    (3, 16, [200, 150, 150], 24, 528, 1),       # first HT past the JP split (one-group form); several k_se_pool channel blocks
    (6, 36, [5, 40], 7, 64, 1),                 # N no multiple of 8 with odd hid; padding inside and after the segments
    (64, 1, [15, 23, 13], 8, 64, 1),            # N exactly one k_se_wgrad image chunk, HW 1
]
NARROW = [
    # branch widths, hid, HT, G
    ([2600, 2590], 16, 5200, 4),
    ([5200, 5190], 8, 10400, 2),
    ([10300, 10290], 8, 20608, 1),
]


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    if RATIO:
        print("\nse: largest error / bound:", {k: round(v, 4) for k, v in sorted(RATIO.items())})


def _ops():
    from atomnas_amd import ops
    return ops


def _name(dtype):
    return "fp32" if dtype == F32 else "bf16"


@functools.lru_cache(maxsize=8)
def case(i, act, dtype):
    N, HW, widths, hid, HT, parts = CASES[i]
    c = se_reference(N, HW, widths, hid, act, RELU if i % 2 == 0 else SWISH, dtype, seed=i)
    assert c.HT == HT
    c.parts = parts
    return c


# ---- operands in the three forms: "plain" [M, HT], "slab" (ops.Slab), "wide" (columns 8 .. 8 + HT of a NaN-filled [M, HT + 16] buffer)
def _operand(x, layout):
    if layout == "slab":
        return _ops().Slab.from_plain(x)
    if layout == "wide":
        buf = torch.full((x.shape[0], x.shape[1] + WIDE), float("nan"), dtype=x.dtype, device=x.device)
        v = buf[:, WIDE_OFF:WIDE_OFF + x.shape[1]]
        v.copy_(x)
        return v
    return x


def _output(M, HT, dtype, layout):
    """an output operand whose every element is poisoned (7.0): the kernels write the whole [M, HT], zeros on padding"""
    if layout == "slab":
        s = _ops().Slab(M, HT, dtype, "cuda")
        s.t.fill_(7.0)
        return s
    return _operand(torch.full((M, HT), 7.0, dtype=dtype, device="cuda"), layout)


def _plain(t, layout, name):
    if layout == "slab":
        return t.to_plain().clone()
    if layout == "wide":
        frame = torch.cat([t._base[:, :WIDE_OFF], t._base[:, WIDE_OFF + t.shape[1]:]], 1)
        assert bool(torch.isnan(frame).all()), "%s: a write outside the columns of the view" % name
        return t.clone()
    return t


def _apply(e, stat_rows, layout="plain"):
    """se_bwd_apply on the buffers of run `e` into a fresh poisoned g -> (g plain, statistics rows or None)"""
    c = e.c
    st2 = None if stat_rows is None else torch.full((stat_rows, 2, c.HT), float("nan"), device="cuda")
    gd = _output(c.M, c.HT, e.dtype, layout)
    _ops().se_bwd_apply(e.dSd, e.Dd, e.sc, e.sh, c.act, e.gate, e.dpooled, gd, st2, c.M, c.HW, c.HT, stat_rows=stat_rows)
    return _plain(gd, layout, "g"), st2


OUTPUTS = ("pooled", "hpre", "gate", "S", "dz2", "dz1", "dpooled", "g", "st2", "dw1", "db1", "dw2", "db2")


def run(c, dtype, layout):
    """the whole sequence as the fused block issues it, every output poisoned beforehand; -> the outputs (activations as plain tensors)"""
    ops = _ops()
    N, HW, M, HT, hid, total = c.N, c.HW, c.M, c.HT, c.hid, c.total
    dev = "cuda"
    e = types.SimpleNamespace(c=c, dtype=dtype)
    e.Dd, e.dSd = _operand(c.D.to(dtype).to(dev), layout), _operand(c.dS.to(dtype).to(dev), layout)
    e.sc, e.sh, cm = c.scale.to(dev), c.shift.to(dev), c.cmap.to(dev)
    w1p, w2t, b2p = (t.to(dev) for t in se_pack(c.w1, c.w2, c.b2, c.cmap, HT))
    parts = ops.se_pool_parts(N, HW, HT)
    f = lambda *s: torch.full(s, 7.0, device=dev)
    e.pooled, e.gate, e.hpre, pparts = f(N, HT), f(N, HT), f(N, hid), f(parts, N, HT)
    ops.se_squeeze(e.Dd, e.sc, e.sh, c.act, pparts, N, HW, HT)
    ops.se_mlp_fwd(pparts, e.pooled, cm, w1p, c.b1.to(dev), w2t, b2p, c.se_act, e.hpre, e.gate, N, HT, hid)
    Sd = _output(M, HT, dtype, layout)
    ops.se_scale(e.Dd, e.sc, e.sh, c.act, e.gate, Sd, M, HW, HT)
    e.S = _plain(Sd, layout, "S")
    e.dz2, e.dpooled, e.dz1, dgate = f(N, HT), f(N, HT), f(N, hid), f(parts, N, HT)
    e.dw1, e.db1, e.dw2, e.db2 = (t.clone().to(dev) for t in c.base)   # the kernels accumulate into the gradient arena
    ops.se_bwd_gate(e.dSd, e.Dd, e.sc, e.sh, c.act, e.gate, e.pooled, cm, w1p, w2t, e.hpre, dgate, e.dz2, e.dz1, e.dpooled, e.dw1, e.db1,
                    e.dw2, e.db2, N, HW, HT, total, hid, se_act=c.se_act)
    e.g, e.st2 = _apply(e, ROWS, layout)
    torch.cuda.synchronize()
    return e


def _close(name, dtype, got, ref, rtol, atol):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    key = "%s %s" % (name, _name(dtype))
    RATIO[key] = max(RATIO.get(key, 0.0), float(((got - ref).abs() / (atol + rtol * ref.abs())).max()))
    assert_close(name, got, ref, rtol, atol)


def _stats(name, st2, g, D):
    """statistics rows against the float64 sums over the STORED g (bound of tests/test_se_gpu.py); no row left unwritten"""
    assert bool(torch.isfinite(st2).all()), "%s: statistics rows left unwritten" % name
    gq, Dq = g.double(), D.double()
    for k, ref in ((0, gq.sum(0)), (1, (gq * Dq).sum(0))):
        mag = (gq if k == 0 else gq * Dq).abs().sum(0)
        assert_close("%s row %d" % (name, k), st2[:, k].sum(0).double(), ref, 1e-4, 1e-4 * max(1.0, float(mag.max())))


def check(c, e, dtype):
    """every output of run `e` against the float64 reference of case `c`"""
    r = c.ref
    idx, pad = c.idx.cuda(), (~c.valid).cuda()
    for name in ("pooled", "gate", "S", "g"):
        assert not bool(getattr(e, name)[:, pad].any()), "%s: padded channels are not exactly zero" % name
    for name in ("pooled", "gate", "dz2", "dpooled"):
        _close(name, dtype, getattr(e, name)[:, idx], getattr(r, name), 1e-4, 1e-5)
    for name in ("hpre", "dz1"):
        _close(name, dtype, getattr(e, name), getattr(r, name), 1e-4, 1e-5)
    rt_s, at_s, rt_g, at_g = (1e-4, 1e-5, 1e-4, 2e-5) if dtype == F32 else (2.0 ** -8, 1e-3, 2.0 ** -8, 2e-3)
    _close("S", dtype, e.S[:, idx], r.S, rt_s, at_s)
    _close("g", dtype, e.g[:, idx], r.g, rt_g, at_g)
    Dd = c.D.to(dtype).cuda()
    _stats("stats2", e.st2, e.g, Dd)
    assert not bool(e.st2[:, :, pad].any()), "statistics of padded channels are not zero"
    # ... and against the reference's sums over ITS stored g: the element bounds of g add up, plus the bound of the fp32 sums above
    gb = at_g + rt_g * r.g.abs() + (r.g_stored - r.g).abs()
    Dr = c.D[:, c.idx].abs()
    got = e.st2.double().sum(0).cpu()[:, c.idx]
    for k, w in ((0, torch.ones_like(Dr)), (1, Dr)):
        bound = (gb * w).sum(0) + 1e-4 * max(1.0, float((r.g_stored.abs() * w).sum(0).max()))
        err = (got[k] - r.stats[k]).abs()
        assert bool((err <= bound).all()), "statistics row %d against the reference: max err %.4g, bound %.4g" % (k, float(err.max()),
                                                                                                               float(bound.min()))
    for name, got, b in (("dw1", e.dw1, c.base[0]), ("db1", e.db1, c.base[1]), ("dw2", e.dw2, c.base[2]), ("db2", e.db2, c.base[3])):
        ref = getattr(r, name).reshape(-1)
        _close(name, dtype, got.double().cpu() - b.double(), ref, 1e-3, 2e-5 * max(1.0, float(ref.abs().max())) * (c.N * c.HW) ** 0.5)


def _same(what, a, b):
    for name in OUTPUTS:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and torch.equal(x, y), "%s: %s differs (%d elements)" % (what, name, int((x != y).sum()))


@pytest.mark.parametrize("layout", ["plain", "slab"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("i", range(len(CASES)), ids=["n%d_hw%d_ht%d" % (t[0], t[1], t[4]) for t in CASES])
def test_se_parity(gpu_lib, i, act, dtype, layout):
    c = case(i, act, dtype)
    assert _ops().se_pool_parts(c.N, c.HW, c.HT) == c.parts
    check(c, run(c, dtype, layout), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("i", range(len(CASES)), ids=["n%d_hw%d_ht%d" % (t[0], t[1], t[4]) for t in CASES])
def test_se_forms(gpu_lib, i, act, dtype):
    """the forms of one case give the same BITS in every output, the statistics rows and the weight gradients included"""
    c = case(i, act, dtype)
    a = run(c, dtype, "plain")
    _same("slab-major against plain", a, run(c, dtype, "slab"))
    _same("second run", a, run(c, dtype, "plain"))
    _same("column views of wider buffers", a, run(c, dtype, "wide"))
    g, _ = _apply(a, None)
    assert torch.equal(g, a.g), "g changes without statistics"
    Dd = c.D.to(dtype).cuda()
    for rows in (3, _ops().stat_rows_for(c.HT)):   # fewer rows than workgroups (the grid is clamped); more (the tail rows are zeroed)
        g, st2 = _apply(a, rows)
        assert torch.equal(g, a.g), "g changes with stat_rows = %d" % rows
        _stats("stat_rows = %d" % rows, st2, g, Dd)


@pytest.mark.parametrize("layout", ["plain", "slab"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("act", [1, 2])
def test_se_exact_boundaries(gpu_lib, act, dtype, layout):
    N, HW, widths, hid = 2, 49, [29], 4
    HT, total, cmap, _ = se_layout(widths)
    assert HT == 32
    gen = torch.Generator().manual_seed(29 + act)
    vals = torch.tensor([-1.0, 0.0, 0.5, 5.5, 6.0, 6.5], dtype=torch.float64)
    c = types.SimpleNamespace(N=N, HW=HW, M=N * HW, hid=hid, act=act, se_act=RELU, HT=HT, total=total, cmap=cmap)
    c.D, c.dS = torch.zeros(c.M, HT, dtype=torch.float64), torch.zeros(c.M, HT, dtype=torch.float64)
    c.D[:, :total] = vals[torch.randint(0, len(vals), (c.M, total), generator=gen)]
    c.dS[:, :total] = 0.75
    c.scale, c.shift = torch.zeros(HT), torch.zeros(HT)
    c.scale[:total] = 1.0
    c.w1, c.b1 = torch.randn(hid, total, generator=gen) / total ** 0.5, torch.randn(hid, generator=gen) * 0.1
    c.w2, c.b2 = torch.randn(total, hid, generator=gen) / hid ** 0.5, torch.randn(total, generator=gen) * 0.1
    c.base = [torch.zeros(hid * total), torch.zeros(hid), torch.zeros(total * hid), torch.zeros(total)]
    e = run(c, dtype, layout)
    D = c.D[:, :total]
    assert all(bool((D == v).any()) for v in vals)
    S, g, gate = e.S[:, :total].cpu(), e.g[:, :total].cpu(), e.gate[:, :total].cpu()
    assert bool(((gate > 0) & (gate < 1)).all())
    # S: one fp32 product of the clamp (exact) with the kernel's own gate, rounded once to the storage type
    want = (act64(D, act).float() * gate.repeat_interleave(HW, 0)).to(dtype)
    assert bool((S[D <= 0] == 0).all()), "S is not exactly 0 where D <= 0"
    it = torch.int32 if dtype == F32 else torch.int16
    pos = D > 0
    assert bool((S[pos] > 0).all())
    ulps = (S[pos].view(it).long() - want[pos].view(it).long()).abs()   # positive values: the bit patterns are ordered
    assert int(ulps.max()) <= 1, "S is %d ulp from act(D) * gate" % int(ulps.max())
    zero = (D <= 0) | (D >= 6) if act == 2 else (D <= 0)
    assert bool((g[zero] == 0).all()), "g is not exactly 0 where the derivative of the activation is 0 (bounds included)"
    assert bool((g[~zero] != 0).all()), "g is 0 where the activation passes the gradient"
    assert not bool(e.S[:, total:].any()) and not bool(e.g[:, total:].any())


@pytest.mark.parametrize("widths,hid,HT,G", NARROW, ids=["G%d" % t[3] for t in NARROW])
def test_se_mlp_narrow(gpu_lib, widths, hid, HT, G):
    """k_se_mlp with fewer than 8 images per workgroup (see the arithmetic at the top of the file; which G ran is not observable)"""
    per_g = (HT + hid + (1024 if HT <= 512 else 0)) * 4
    assert 2 * G * per_g > 160 * 1024 >= G * per_g       # the instance the row is written for, at 160 KiB of LDS per workgroup
    c = se_reference(3, 2, widths, hid, SWISH, SWISH, F32, seed=HT)
    assert c.HT == HT and _ops().se_pool_parts(c.N, c.HW, c.HT) == 1
    check(c, run(c, F32, "plain"), F32)
