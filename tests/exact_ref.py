"""Exact-integer cases of the pointwise kernels (csrc/pwconv.hip, pwconv_tn.hip, xbwd.hip): tables, builder, float64 reference, checks.

The MFMA kernels accumulate in fp32 and bf16 holds every integer of magnitude up to 256.  A case here has small integers for every
operand, coefficient, residual, bias and pre-filled output, and activation codes 0, 1 or 2 only.  Every product, partial sum, partial
row of the statistics and workspace partial is then an integer below 2^24, which fp32 represents exactly: the kernel's result equals the
float64 reference with tolerance ZERO whatever the order of summation (where the storage type rounds the output, the reference is
rounded once to it).  A lost, doubled or misplaced term shows as a difference of at least 1, and so does a mask decided with `>=`
where the contract is `>` (kutil.act_grad64).  Swish (code 3) is not exact: the "twin" of a case carries code 3 instead of 1 / 2 and
keeps the project's rounding bound.

This module needs no GPU to build a case (tests/test_pw_exact.py asserts the preconditions on the CPU); the run_* functions launch the
kernels and return a list of mismatches (tests/test_pw_exact_gpu.py; `python exact_ref.py --child` is the same for a child interpreter
whose environment switches kernel families off).

nt_family / nt_generic_chunks / tn_family / tn_plan / xb_family / pb_expected are Python transcriptions of the plan functions of
csrc/pwconv.hip and csrc/pwconv_tn.hip (no query of the library names the kernel it takes): they label the cases and let the CPU test
assert that every family, instance and form is reached.  KEEP THEM IN STEP with the plan functions when those change.

Cases per entry point and family: tests/test_pw_exact.py lists them, `python tests/exact_ref.py --count` prints them.
"""
import json
import os
import sys
import types

import torch

import kutil

PRO_NONE, PRO_BNRELU, PRO_BNBWD = 0, 1, 2
STAT_SQ, STAT_Z = 1, 2
CAP = float(1 << 24)
BF, F32 = torch.bfloat16, torch.float32

# value tables (drawn uniformly): targets of the EFFECTIVE value / the pre-activation of an element
_T0 = [0] * 6 + [1, -1] * 4 + [2, -2] * 3                                   # no activation: {-2..2}, 30 % zeros
_T1 = [0] * 5 + [-1] * 2 + [-2] * 2 + [1] * 4 + [2] * 4 + [3] * 3            # ReLU / Swish: both sides of 0
_T2 = [0] * 5 + [-1] * 2 + [-2] + [6] * 3 + [7] * 2 + [8] + [1, 2, 3] * 2    # ReLU6: 0, both sides of 0, exactly 6, above 6
_TABLE = {0: _T0, 1: _T1, 2: _T2, 3: _T1}


def _dtype(dt):
    return BF if dt == 1 else F32


def _pad(c, a):
    return (c + a - 1) // a * a


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + hash(k if not isinstance(k, str) else sum(map(ord, k)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _draw(gen, table, *shape):
    t = torch.tensor(table, dtype=torch.float64)
    return t[torch.randint(0, len(table), shape, generator=gen)]


def _pick(gen, values, n):
    return _draw(gen, list(values), n)


# ------------------------------------------------------------------------------------------------ operands
def _mix_ok(pre, act):
    """condition (c) of an input read through an activation: 5 % exactly 0, 5 % on each side of 0; mode 2: 5 % exactly 6, 5 % above 6"""
    frac = lambda m: float(m.double().mean())
    ok = frac(pre == 0) >= 0.05 and frac(pre > 0) >= 0.05 and frac(pre < 0) >= 0.05
    return ok and (act != 2 or (frac(pre == 6) >= 0.05 and frac(pre > 6) >= 0.05))


def operand(gen, M, C, mode, act, dtype):
    """_operand, drawn again (few channels: the coefficients of a channel may keep its pre-activations off 0) until (c) holds"""
    for attempt in range(32):
        o = _operand(gen, M, C, mode, act, dtype)
        if o.pre is None or not o.act or _mix_ok(o.pre, o.act):
            return o
    raise AssertionError("no draw meets the activation mix")


def _operand(gen, M, C, mode, act, dtype):
    """One operand [M, C] read through prologue `mode` (activation code `act` for BNRELU).  Integer raw streams and coefficients are
    derived from a drawn target so that the pre-activation hits 0 and 6 exactly; a row m without a target >= 2 gets one in column m % C.
    -> namespace: a, a2 (raw streams), c1..c3, pre (what the activation sees; None without one), eff (what the MFMA sees)"""
    o = types.SimpleNamespace(mode=mode, act=act if mode == PRO_BNRELU else 0, a2=None, c1=None, c2=None, c3=None, pre=None)
    t = _draw(gen, _TABLE[o.act], M, C)
    r = torch.nonzero(~(t >= 2).any(1)).flatten()      # rows that could end up without a non-zero effective value
    t[r, r % C] = 2.0
    if mode == PRO_NONE:
        o.a = o.eff = t
    elif mode == PRO_BNRELU:
        o.c1, o.c2 = _pick(gen, (1, 2), C), _pick(gen, (-1, 0, 1), C)
        o.a = torch.floor((t - o.c2) / o.c1)
        o.pre = o.a * o.c1 + o.c2
        o.eff = kutil.act64(o.pre, o.act)
        if o.act == 3:
            o.eff = o.eff.to(dtype).double()      # the prologue's result is rounded to the MFMA operand type
    else:
        o.c1, o.c2, o.c3 = _pick(gen, (1, 2, -1), C), _pick(gen, (1, 2, -1), C), _pick(gen, (-1, 0, 1), C)
        o.a2 = _draw(gen, _T0, M, C)
        o.a = torch.floor((t - o.c2 * o.a2 - o.c3) / o.c1)
        o.eff = o.c1 * o.a + o.c2 * o.a2 + o.c3
    return o


def banded(gen, N, K, unit=False):
    """weights [N, K]: every k has a non-zero weight in column k % N, every column at least three; few terms per output so that wide
    K stays inside the caps (`unit`: +-1 only, for the row counts whose statistics would otherwise pass 2^24)"""
    w = torch.zeros(N, K, dtype=torch.float64)
    vals = (-2, -1, 1, 2) if K <= 8 * N and not unit else (-1, 1)
    k = torch.arange(K)
    w[k % N, k] = _pick(gen, vals, K)
    n = torch.arange(N)
    for j in range(3):
        kk = (n * 7 + j * max(1, K // 3) + j) % K
        w[n, kk] = _pick(gen, vals, N)
    return w


def _act2d(x, dtype, lay, device):
    """[M, C] float64 -> the activation buffer: kutil.to_act (padding channels zero), slab-major through ops.Slab.from_plain"""
    from atomnas_amd import ops
    M, C = x.shape
    buf = kutil.to_act(x.t().reshape(1, C, M, 1), dtype, device=device)
    return ops.Slab.from_plain(buf, C) if lay == "slab" else buf


def pack_w(w, dtype, device):
    """[N, K] -> packed [N padded to 64][K padded to 32] in the storage type, padding zero (atomnas_pack_weights mode 0)"""
    n, k = w.shape
    buf = torch.zeros(_pad(n, 64), _pad(k, 32), dtype=dtype, device=device)
    buf[:n, :k] = w.to(dtype).to(device)
    return buf


def fresh(M, C, dtype, lay, device):
    """kutil.fresh (padding zero) with the valid region poisoned with NaN: an integer poison could equal a reference value"""
    from atomnas_amd import ops
    b = kutil.fresh(M, C, dtype, poison=float("nan"), device=device)
    return ops.Slab.from_plain(b, C) if lay == "slab" else b


def stats_buf(N, device):
    from atomnas_amd import ops
    return torch.full((ops.stat_rows_for(N), 2, N), float("nan"), dtype=F32, device=device)


def _cv(v, device):
    return None if v is None else kutil.cvec(v, device=device)


def plain(t):
    return t.to_plain() if hasattr(t, "to_plain") else t


def _operand_kw(o, prefix, dtype, lay, C, device, relu_name):
    kw = {}
    if o.mode != PRO_NONE:
        kw.update({prefix + "_mode": o.mode, prefix + "c1": _cv(o.c1, device), prefix + "c2": _cv(o.c2, device)})
    if o.mode == PRO_BNRELU:
        kw[relu_name] = o.act
    if o.mode == PRO_BNBWD:
        kw.update({prefix + "c3": _cv(o.c3, device), prefix + "2": _act2d(o.a2, dtype, lay, device)})
    return kw


# ------------------------------------------------------------------------------------------------ gemm_nt
def _nt(M, N, K, **kw):
    r = dict(M=M, N=N, K=K, dt=1, a_mode=PRO_NONE, act=0, a="plain", c="plain", out_f32=0, add=0, bias=0, z=None, mask=0, stat_mode=STAT_SQ,
             whole_chip=0)
    r.update(kw)
    return r


def nt_family(r, off=False):
    """the family launch_nt (csrc/pwconv.hip) takes for the case (`off`: with the sw / swg / st families switched off); the LDS and
    2 GB limits of the plans cannot bind at these sizes"""
    M, N, K = r["M"], r["N"], r["K"]
    if r["dt"] == 0:
        return "generic"
    epi = r["out_f32"] or r["add"] or r["bias"]
    proj = (r["a_mode"] == PRO_BNRELU and r["a"] == "slab" and r["c"] == "plain" and N % 8 == 0 and not epi and not r["z"]
            and r["stat_mode"] == STAT_SQ)
    if not off:
        if proj and N <= 48 and 97 <= K <= 448 and M >= 16384:
            return "sw"
        if proj and N <= 320 and K >= 256 and K % 4 == 0 and 8192 <= M <= 262144 and (N + 15) // 16 in (3, 5, 6, 12, 20):
            return "swg"
        lay_ok = lambda lay: lay == "slab" or N % 8 == 0
        if (K <= 192 and N >= 2 * K and N >= 96 and M >= 1024 and r["a_mode"] == PRO_NONE and K % 8 == 0 and not epi and lay_ok(r["c"])
                and ((not r["z"] and r["stat_mode"] == STAT_SQ) or (r["z"] and r["mask"] and r["stat_mode"] == STAT_Z and lay_ok(r["z"])))):
            return "st"
    if N <= 64 and K <= 64 and M >= 65536:
        return "small"
    if K >= 97 and M >= 4096:
        return "ws"
    return "generic"


def _nt_epilogues(M, N, K, dt):
    """residual add, bias with fp32 output, mask + z with STAT_Z (z plain and slab), each with activation codes 1 and 2 in the prologue
    and, separately, in the mask"""
    rows = []
    for act in (1, 2):
        rows.append(_nt(M, N, K, dt=dt, a_mode=PRO_BNRELU, act=act, add=1))
        rows.append(_nt(M, N, K, dt=dt, a_mode=PRO_BNRELU, act=act, bias=1, out_f32=dt))
        for z in (("plain", "slab") if dt == 1 else ("plain",)):
            rows.append(_nt(M, N, K, dt=dt, a_mode=PRO_BNBWD, z=z, mask=act, stat_mode=STAT_Z))
    rows.append(_nt(M, N, K, dt=dt, a_mode=PRO_BNBWD, z="plain", add=1, stat_mode=STAT_Z))     # z for the statistics alone
    return rows


def _pro(i):
    """the three prologues in turn, the activation codes 1 and 2 alternating"""
    return [dict(a_mode=PRO_NONE), dict(a_mode=PRO_BNRELU, act=1 + i % 2), dict(a_mode=PRO_BNBWD)]


def nt_cases():
    rows = []
    # sw (BNRELU, slab A, STAT_SQ): UT 1..3, NCH 5 and 7
    for M in (16384, 16385):
        for N, K in ((8, 97), (24, 432), (48, 448)):
            for act in (1, 2):
                rows.append(_nt(M, N, K, a_mode=PRO_BNRELU, a="slab", act=act))
    # swg: UT 3, 5, 6, 12, 20; K % 64 == 0 and a ragged last chunk; the eight-wave form needs the whole chip's 256 CUs
    i = 0
    for M in (8192, 8191 + 64):
        for K in (256, 260):
            for N in (40, 80, 96, 192, 320):
                rows.append(_nt(M, N, K, a_mode=PRO_BNRELU, a="slab", act=1 + i % 2))
                i += 1
    rows.append(_nt(32768, 80, 256, a_mode=PRO_BNRELU, a="slab", act=2, whole_chip=1))
    # st (FWD and MASK kinds): 1 / 2 / 3 / 6 k-steps, ragged N, both layouts of c and z; 1023 rows are below the family's threshold
    for M in (1024, 1023):
        for N, K in ((96, 24), (96, 48), (192, 96), (384, 192), (104, 40)):
            for lay in ("slab", "plain"):
                rows.append(_nt(M, N, K, c=lay))
                mask = 1 + (len(rows) // 2) % 2
                rows.append(_nt(M, N, K, c=lay, z=lay, mask=mask, stat_mode=STAT_Z))
    rows.append(_nt(1024, 1472, 24, c="slab"))                                     # 23 chunks: the shared-burst form
    rows.append(_nt(1024, 1472, 24, c="slab", z="slab", mask=2, stat_mode=STAT_Z))
    # small: one / two k-steps, 1 / 2 / 4 column tiles, the 16-channel form (N % 4 != 0, fp32 output)
    for M in (65536, 65537):
        for j, (N, K) in enumerate(((16, 16), (32, 48), (64, 64), (20, 16))):
            for p in _pro(j + M):
                rows.append(_nt(M, N, K, **p))
        rows.append(_nt(M, 18, 16, out_f32=1))
        rows.append(_nt(M, 18, 16))
    rows += _nt_epilogues(65537, 32, 48, 1)
    # ws: one / two 64-channel chunks, ragged N and K; two subtiles per wave with the BN-backward prologue from M = 100000
    for M in (4096, 4097):
        for j, N in enumerate((64, 65, 136)):
            for p in _pro(j + M):
                rows.append(_nt(M, N, 97, **p))
    rows.append(_nt(100000, 24, 128, a_mode=PRO_BNBWD))
    rows += _nt_epilogues(4097, 65, 97, 1)
    # generic, both storage types: K below, at and above the k-step, N below / above 64, the small-M single-chunk plan (all of these
    # run one 64-channel chunk per item: nt_generic_chunks), and two live chunks from 128 row blocks x 2 channel groups on
    for dt in (0, 1):
        for j, (M, N, K) in enumerate(((50, 7, 3), (1000, 72, 40), (1000, 136, 72), (1000, 72, 31), (1000, 72, 33), (37, 1000, 72))):
            for p in _pro(j + dt):
                rows.append(_nt(M, N, K, dt=dt, **p))
        rows += _nt_epilogues(1000, 136, 72, dt)
        rows += _nt_epilogues(37, 1000, 72, dt)
        for p in _pro(dt):
            rows.append(_nt(8129, 136, 72, dt=dt, **p))
        rows.append(_nt(8128, 136, 72, dt=dt, a_mode=PRO_BNRELU, act=2 - dt))
        rows += _nt_epilogues(8129, 136, 72, dt)
    return rows


def nt_generic_chunks(r, cus=256):
    """64-channel chunks that stay live per item of k_gemm_nt (nt_generic_plan, for a device of `cus` CUs)"""
    M, N = r["M"], r["N"]
    return 1 if N <= 64 or (M + 63) // 64 * ((N + 127) // 128) < cus else 2


def twin(r, keys):
    """the Swish twin of a case (None when the case has no activation): every activation code 1 / 2 becomes 3"""
    if not any(r.get(k) for k in keys):
        return None
    t = dict(r)
    for k in keys:
        if t.get(k):
            t[k] = 3
    return t


def _dedup(rows):
    seen, out = set(), []
    for r in rows:
        k = json.dumps(r, sort_keys=True)
        if k not in seen:
            seen.add(k)
            out.append(r)
    return out


def nt_twins():
    """the Swish twin of every case that has an activation (cases that differ in the code 1 / 2 alone share one)"""
    return _dedup([t for t in (twin(r, ("act", "mask")) for r in nt_cases()) if t is not None])


def build_nt(r):
    """integer inputs and the float64 reference of one gemm_nt case (no GPU)"""
    M, N, K, dtype = r["M"], r["N"], r["K"], _dtype(r["dt"])
    gen = _gen("nt", *[r[k] if r[k] is not None else -1 for k in sorted(r)])
    c = types.SimpleNamespace(r=r, dtype=dtype, out_dtype=F32 if r["out_f32"] else dtype, exact=r["act"] != 3 and r["mask"] != 3)
    c.A = operand(gen, M, K, r["a_mode"], r["act"], dtype)
    c.W = banded(gen, N, K, unit=M >= 16384)
    acc = c.A.eff @ c.W.t()
    mag = c.A.eff.abs() @ c.W.abs().t()
    c.bias = c.add = c.Z = None
    if r["bias"]:
        c.bias = _pick(gen, (-1, 0, 1, 2), N)
        acc, mag = acc + c.bias, mag + c.bias.abs()
    if r["add"]:
        c.add = _draw(gen, _T0, M, N)
        acc, mag = acc + c.add, mag + c.add.abs()
    if r["z"]:
        c.Z = operand(gen, M, N, PRO_BNRELU, r["mask"] or 1, dtype)      # z = Z.a, zscale = Z.c1, zshift = Z.c2
        if r["mask"]:
            acc = acc * kutil.act_grad64(c.Z.pre, r["mask"])
    c.acc, c.mag = acc, mag
    c.out = acc.to(c.out_dtype).double()                                 # the storage type rounds once
    c.second = c.out * c.out if r["stat_mode"] == STAT_SQ else c.out * c.Z.a
    c.stats = torch.stack([c.out.sum(0), c.second.sum(0)])
    return c


def nt_buffers(c, device):
    from atomnas_amd import ops
    r, dtype = c.r, c.dtype
    b = types.SimpleNamespace()
    b.a = _act2d(c.A.a, dtype, r["a"], device)
    b.wp = pack_w(c.W, dtype, device)
    b.c = fresh(r["M"], r["N"], c.out_dtype, r["c"], device)
    b.stats = stats_buf(r["N"], device)
    kw = _operand_kw(c.A, "a", dtype, r["a"], r["K"], device, "a_relu")
    if c.bias is not None:
        kw["bias"] = _cv(c.bias, device)
    if c.add is not None:
        kw["add"] = _act2d(c.add, dtype, "plain", device)
    if c.Z is not None:
        kw.update(z=_act2d(c.Z.a, dtype, r["z"], device), zscale=_cv(c.Z.c1, device), zshift=_cv(c.Z.c2, device), mask=r["mask"])
    kw.update(stats=b.stats, stat_mode=r["stat_mode"], stat_rows=ops.stat_rows_for(r["N"]))
    b.kw = kw
    return b


# ------------------------------------------------------------------------------------------------ comparisons
def first_diff(name, got, ref):
    """[] when got == ref element for element, else one message naming the first differing index (as kutil.assert_close does)"""
    got, ref = got.double().cpu(), ref.double().cpu()
    if got.shape != ref.shape:
        return ["%s: shape %s, reference %s" % (name, tuple(got.shape), tuple(ref.shape))]
    if torch.equal(got, ref):
        return []
    bad = ~(got == ref)
    idx = torch.nonzero(bad)[0].tolist()
    return ["%s: %d/%d differ, first at %s got %.9g ref %.9g" % (name, int(bad.sum()), bad.numel(), idx, float(got[tuple(idx)]),
                                                                float(ref[tuple(idx)]))]


def close(name, got, ref, rtol, atol):
    try:
        kutil.assert_close(name, got, ref, rtol, atol)
    except AssertionError as e:
        return [str(e)]
    return []


def _pad_zero(name, buf2d, C):
    if buf2d.shape[1] > C and float(buf2d[:, C:].float().abs().max()) != 0.0:
        return ["%s: non-zero padding columns" % name]
    return []


def twin_tol(dtype, scale):
    """the project's bound for one output rounding (kutil.tol), the absolute part scaled by the largest output as test_gemm_nt does"""
    t = kutil.tol(dtype)
    return dict(rtol=t["rtol"], atol=t["atol"] * max(1.0, scale))


def stats_floor(M, terms):
    """fp32 summation floor of a Swish twin's statistics: M * 2^-24 * max|term| per channel"""
    return M * 2.0 ** -24 * float(terms.abs().max())


def check_stats(name, st, first, second, exact, M):
    """statistics summed over the partial rows in float64 against [sum first, sum second] of the stored output"""
    if bool(torch.isnan(st).any()):
        return ["%s: NaN left in %d statistics rows" % (name, int(torch.isnan(st).flatten(1).any(1).sum()))]
    s = st.double().sum(0).cpu()
    if exact:
        return first_diff(name + " sum", s[0], first.sum(0)) + first_diff(name + " second", s[1], second.sum(0))
    return (close(name + " sum", s[0], first.sum(0), 1e-5, stats_floor(M, first)) +
            close(name + " second", s[1], second.sum(0), 1e-5, stats_floor(M, second)))


def name_of(r):
    return " ".join("%s=%s" % (k, r[k]) for k in sorted(r) if r[k] not in (0, None, "plain") or k in ("M", "N", "K"))


def run_nt(r, device="cuda"):
    """one ops.gemm_nt launch of the case -> list of mismatches"""
    from atomnas_amd import ops
    c = build_nt(r)
    b = nt_buffers(c, device)
    M, N, K = r["M"], r["N"], r["K"]
    ops.gemm_nt(b.a, b.wp, b.c, M, N, K, **b.kw)
    torch.cuda.synchronize()
    cp = plain(b.c)
    got = cp[:, :N].double().cpu()
    who = "gemm_nt[%s]" % name_of(r)
    if c.exact:
        bad = first_diff(who + " C", got, c.out)
        first, second = c.out, c.second
    else:
        bad = close(who + " C", got, c.acc, **twin_tol(c.dtype, float(c.acc.abs().max())))
        first, second = got, (got * got if r["stat_mode"] == STAT_SQ else got * c.Z.a)     # sums of the STORED output
    return bad + _pad_zero(who, cp, N) + check_stats(who, b.stats, first, second, c.exact, M)


# ------------------------------------------------------------------------------------------------ gemm_tn
def _tn(M, NU, NV, **kw):
    r = dict(M=M, NU=NU, NV=NV, dt=1, u_mode=PRO_NONE, u_act=0, v_mode=PRO_NONE, v_act=0, u="plain", v="plain", ws=1)
    r.update(kw)
    return r


TN_PAIRS = [(PRO_NONE, PRO_NONE), (PRO_NONE, PRO_BNBWD), (PRO_BNBWD, PRO_BNRELU), (PRO_BNRELU, PRO_BNBWD), (PRO_BNBWD, PRO_NONE),
            (PRO_NONE, PRO_BNRELU)]      # csrc/pwconv_tn.hip for_pair


def _tn_ws_cap(r):
    """partial outputs that fit the workspace ops.gemm_tn allocates (ops.tn_workspace; ws=0: none)"""
    nn = r["NU"] * r["NV"]
    return max(2 * nn, min(256 * nn, 64 << 18)) // nn if r["ws"] else 1


def tn_family(r):
    """launch_tn (csrc/pwconv_tn.hip): dma needs at least 8 row chunks of 128 rows or more, each with a partial in the workspace"""
    if r["dt"] == 0:
        return "generic"
    if (r["u_mode"] == PRO_NONE and r["v_mode"] in (PRO_NONE, PRO_BNRELU) and r["ws"] and r["NV"] >= 256 and 32 <= r["NU"] <= 320
            and r["M"] >= 1024 and min(r["M"] // 128, _tn_ws_cap(r)) >= 8):
        return "dma"
    return "slab"


def tn_utt(NU, dma):
    ut = (NU + 15) // 16
    return (4 if dma else 2) if ut <= 2 else 4 if ut <= 4 else 6 if ut <= 6 else 12 if ut <= 12 else 10 if ut <= 20 else 20


def tn_plan(r, cus=256):
    """the instance and form of a bf16 case: tn_dma_plan / tn_slab_plan for a device of `cus` CUs with at least one resident workgroup
    per CU (the cap of one round of resident workgroups, cus * occupancy / tiles, then binds at none of these sizes)
    -> dict(family, utt, and for slab: wide (128-column V tiles on 64-row slabs), chunks, xcd, narrowed)"""
    fam = tn_family(r)
    M, NU, NV = r["M"], r["NU"], r["NV"]
    if fam != "slab":
        return dict(family=fam, utt=tn_utt(NU, True) if fam == "dma" else 0)

    def plan_as(utt, allow_wide):
        wide = allow_wide and 4 <= utt <= 12 and NV >= 256
        rows, vw = (64, 128) if wide else (128, 64)
        want = min(M // (2 * rows), _tn_ws_cap(r))
        xcd = want >= 8
        want = max(want // 8 * 8 if xcd else want, 1)
        per = (M + want - 1) // want
        return dict(family="slab", utt=utt, wide=wide, vt=(NV + vw - 1) // vw, uz=(NU + 16 * utt - 1) // (16 * utt),
                    chunks=(M + per - 1) // per, xcd=xcd, narrowed=False)

    p = plan_as(tn_utt(NU, False), True)
    if M < 512 and p["chunks"] == 1:
        first = (p["utt"], p["wide"])
        for utt in (12, 10, 6, 4, 2):
            if p["vt"] * p["uz"] >= cus:
                break
            if utt < p["utt"]:
                p = plan_as(utt, False)
        p["narrowed"] = (p["utt"], p["wide"]) != first
    return p


def _pair(um, vm, i):
    kw = dict(u_mode=um, v_mode=vm)
    if um == PRO_BNRELU:
        kw["u_act"] = 1 + i % 2
    if vm == PRO_BNRELU:
        kw["v_act"] = 1 + i % 2
    return kw


def tn_cases():
    rows = []
    # dma: one NU per U-tile width it instantiates (4, 6, 12, 10 accumulator tiles), whole and ragged M / NV, and per NU the full cross
    # of V's prologue (none, BNRELU with code 1, with code 2) and V's layout
    for NU in (40, 88, 136, 200):
        for M, NV in ((1024, 256), (1061, 264)):
            for vm, act in ((PRO_NONE, 0), (PRO_BNRELU, 1), (PRO_BNRELU, 2)):
                for lay in ("plain", "slab"):
                    rows.append(_tn(M, NU, NV, v=lay, u_mode=PRO_NONE, v_mode=vm, v_act=act))
    # slab with a workspace reduction (several row chunks; fewer than 1024 rows keep the dma family out): every accumulator width
    # (2, 4, 6, 12, 10, 20) x the wide form (NV >= 256, widths 4 .. 12) and the narrow one x every prologue pair
    lay = ("plain", "slab")
    for i, NU in enumerate((24, 40, 88, 136, 200, 328)):
        for j, NV in enumerate((264, 72)):
            for k, (um, vm) in enumerate(TN_PAIRS):
                rows.append(_tn(777, NU, NV, u=lay[(i + k) % 2], v=lay[(j + k) % 2], **_pair(um, vm, i + j + k)))
    # ... eight or more chunks (equal work per XCD)
    rows.append(_tn(2100, 88, 264, v="slab", **_pair(PRO_NONE, PRO_BNBWD, 0)))
    rows.append(_tn(2100, 40, 72, **_pair(PRO_BNBWD, PRO_BNRELU, 1)))
    rows.append(_tn(2100, 328, 264, u="slab", **_pair(PRO_BNRELU, PRO_BNBWD, 0)))
    # ... 2 * slab_rows + 1 rows: a single chunk below 512 rows, where tn_slab_plan narrows U (at these widths down to 2 tiles)
    for i, NU in enumerate((24, 40, 88, 136, 200, 328)):
        um, vm = TN_PAIRS[i]
        rows.append(_tn(129, NU, 264, v="slab", **_pair(um, vm, i)))
        rows.append(_tn(257, NU, 72, u="slab" if i % 2 else "plain", **_pair(um, vm, i + 1)))
    # ... every prologue pair on the narrowed plan and above it; the classifier's widths, where narrowing stops at 4 tiles
    for i, (um, vm) in enumerate(TN_PAIRS):
        rows.append(_tn(37, 328, 264, **_pair(um, vm, i)))
        rows.append(_tn(300, 1000, 72, v="slab", **_pair(um, vm, i + 1)))
        rows.append(_tn(1061, 24, 264, u="slab", v="slab", **_pair(um, vm, i)))
    rows.append(_tn(37, 1000, 1280, **_pair(PRO_NONE, PRO_NONE, 0)))
    rows.append(_tn(37, 1000, 1280, v="slab", **_pair(PRO_NONE, PRO_BNRELU, 1)))
    # ... the dma shapes without a workspace, and a wide single chunk
    for i, NU in enumerate((40, 200)):
        rows.append(_tn(1061, NU, 264, ws=0, **_pair(PRO_NONE, PRO_BNRELU, i)))
    rows.append(_tn(257, 88, 72, ws=0, **_pair(PRO_BNBWD, PRO_BNRELU, 1)))
    rows.append(_tn(129, 136, 264, ws=0, **_pair(PRO_NONE, PRO_BNBWD, 0)))
    # generic fp32
    for i, (M, NU, NV) in enumerate(((50, 3, 7), (257, 700, 40), (8 * 32 + 1, 24, 72))):
        for um, vm in (TN_PAIRS[i], TN_PAIRS[i + 3]):
            rows.append(_tn(M, NU, NV, dt=0, **_pair(um, vm, i)))
    rows.append(_tn(257, 24, 72, dt=0, ws=0, **_pair(PRO_BNBWD, PRO_BNRELU, 1)))
    rows.append(_tn(600, 40, 136, dt=0, **_pair(PRO_NONE, PRO_BNRELU, 0)))
    rows.append(_tn(600, 40, 136, dt=0, **_pair(PRO_BNRELU, PRO_BNBWD, 1)))
    return _dedup(rows)


def tn_twins():
    """the Swish twin of every case that has an activation"""
    return _dedup([t for t in (twin(r, ("u_act", "v_act")) for r in tn_cases()) if t is not None])


def build_tn(r):
    M, NU, NV, dtype = r["M"], r["NU"], r["NV"], _dtype(r["dt"])
    gen = _gen("tn", *[r[k] for k in sorted(r)])
    c = types.SimpleNamespace(r=r, dtype=dtype, exact=r["u_act"] != 3 and r["v_act"] != 3)
    c.U = operand(gen, M, NU, r["u_mode"], r["u_act"], dtype)
    c.V = operand(gen, M, NV, r["v_mode"], r["v_act"], dtype)
    c.prefill = _draw(gen, [-3, -2, -1, 0, 1, 2, 3], NU, NV)
    c.prod = c.U.eff.t() @ c.V.eff
    c.mag = c.U.eff.abs().t() @ c.V.eff.abs() + c.prefill.abs()
    c.out = c.prefill + c.prod
    return c


def tn_buffers(c, device):
    r, dtype = c.r, c.dtype
    b = types.SimpleNamespace()
    b.u = _act2d(c.U.a, dtype, r["u"], device)
    b.v = _act2d(c.V.a, dtype, r["v"], device)
    b.kw = dict(_operand_kw(c.U, "u", dtype, r["u"], r["NU"], device, "u_relu"), **_operand_kw(c.V, "v", dtype, r["v"], r["NV"], device, "v_relu"))
    if not r["ws"]:
        b.kw["ws"] = False
    return b


def run_tn(r, device="cuda"):
    """ops.gemm_tn into a pre-filled output, both orientations (si, sj) -> list of mismatches"""
    from atomnas_amd import ops
    c = build_tn(r)
    b = tn_buffers(c, device)
    M, NU, NV = r["M"], r["NU"], r["NV"]
    bad = []
    for si, sj in ((NV, 1), (1, NU)):
        pre = c.prefill if sj == 1 else c.prefill.t()
        out = pre.float().contiguous().to(device)
        ops.gemm_tn(b.u, NU, b.v, NV, out, si, sj, M, **b.kw)
        torch.cuda.synchronize()
        got = out if sj == 1 else out.t()
        who = "gemm_tn[%s si=%d sj=%d]" % (name_of(r), si, sj)
        if c.exact:
            bad += first_diff(who, got, c.out)
        else:
            bad += close(who, got, c.out, **twin_tol(c.dtype, float(c.out.abs().max())))
    return bad


# ------------------------------------------------------------------------------------------------ gram, xb_coeffs, expand_bwd
XB_INSTANCES = [(1, 5), (1, 7), (1, 12), (2, 5), (2, 7), (3, 5)]      # csrc/pwconv.hip: inp <= 16 UT, hid <= 64 NCH


def xb_supported(inp, hid):
    n = (hid + 63) // 64
    nch = 5 if n <= 5 else 7 if n <= 7 else 12 if n <= 12 else 0
    return ((inp + 15) // 16, nch) in XB_INSTANCES


def xb_family(r, off=False):
    return "stream" if (not off and r["h"] == "slab" and r["M"] >= 64 and (r["hid"] + 63) // 64 >= 3) else "k_expand_bwd"


# the three (mp, add) combinations of tests/test_xbwd_gpu.py
XB_FORMS = [(0, 1), (1, 1), (1, 0)]


def xb_cases():
    rows = []
    # one shape per entry of XB_INSTANCES, the streaming kernel (slab-major h) at M = 64, 130 and 4097
    for i, (inp, hid) in enumerate(((16, 320), (8, 448), (16, 768), (32, 304), (24, 448), (40, 320))):
        for j, M in enumerate((64, 130, 4097)):
            mp, add = XB_FORMS[(i + j) % 3]
            rows.append(dict(M=M, inp=inp, hid=hid, h="slab", mp=mp, add=add))
    for mp, add in XB_FORMS:
        rows.append(dict(M=130, inp=24, hid=200, h="slab", mp=mp, add=add))
    # k_expand_bwd: plain h, hid <= 128 (one and two chunks), 63 rows
    for mp, add in XB_FORMS:
        rows.append(dict(M=130, inp=16, hid=320, h="plain", mp=mp, add=add))
        rows.append(dict(M=63, inp=40, hid=320, h="slab", mp=mp, add=add))
        rows.append(dict(M=4097, inp=8, hid=48, h="slab", mp=mp, add=add))
        rows.append(dict(M=130, inp=32, hid=128, h="slab", mp=mp, add=add))
        rows.append(dict(M=63, inp=24, hid=448, h="plain", mp=mp, add=add))
        rows.append(dict(M=4097, inp=16, hid=768, h="plain", mp=mp, add=add))
    return rows


XB_QUERIES = [(16, 320, 1), (16, 768, 1), (32, 448, 1), (48, 320, 1), (40, 720, 0), (16, 800, 0), (48, 448, 0), (56, 64, 0)]


def build_xb(r):
    M, inp, hid = r["M"], r["inp"], r["hid"]
    gen = _gen("xb", *[r[k] for k in sorted(r)])
    c = types.SimpleNamespace(r=r, dtype=BF, exact=True)
    c.H = operand(gen, M, hid, PRO_NONE, 0, BF)                       # masked hidden gradient h
    c.X = operand(gen, M, inp, PRO_NONE, 0, BF)                       # block input x
    c.Wt = banded(gen, inp, hid)                                      # We^T [inp, hid]
    c.c1, c.c2, c.c3 = _pick(gen, (1, 2), hid), _pick(gen, (1, 2, -1), hid), _pick(gen, (-1, 0, 1), hid)
    c.add = _draw(gen, _T0, M, inp) if r["add"] else None
    c.prefill = _draw(gen, [-3, -2, -1, 0, 1, 2, 3], hid, inp)
    We, x, h = c.Wt.t(), c.X.eff, c.H.eff
    c.gram, c.sx = x.t() @ x, x.sum(0)
    c.mm = We.t() @ (c.c2.view(-1, 1) * We)                           # M = We^T diag(c2) We
    c.mp = c.mm.to(BF).double()                                       # rounded once to the weight type
    c.vb = c.c3 @ We
    c.dwe1 = c.prefill + c.c2.view(-1, 1) * (We @ c.gram) + c.c3.view(-1, 1) * c.sx.view(1, -1)      # after xb_coeffs
    c.dwe1_mag = c.prefill.abs() + (We.abs() @ c.gram.abs()) * c.c2.abs().view(-1, 1) + c.sx.abs().view(1, -1) * c.c3.abs().view(-1, 1)
    dE = c.c1 * h
    acc, mag = dE @ We, dE.abs() @ We.abs()
    if r["mp"]:
        acc, mag = acc + x @ c.mp.t() + c.vb, mag + x.abs() @ c.mp.abs().t() + c.vb.abs()
    if c.add is not None:
        acc, mag = acc + c.add, mag + c.add.abs()
    c.acc, c.mag = acc, mag
    c.gx = acc.to(BF).double()
    base = c.dwe1 if r["mp"] else c.prefill
    c.dwe = base + dE.t() @ x
    c.dwe_mag = (c.dwe1_mag if r["mp"] else c.prefill.abs()) + dE.abs().t() @ x.abs()
    return c


def xb_buffers(c, device):
    r = c.r
    M, inp, hid = r["M"], r["inp"], r["hid"]
    b = types.SimpleNamespace()
    b.h = _act2d(c.H.a, BF, r["h"], device)
    b.x = _act2d(c.X.a, BF, "plain", device)
    b.wt = pack_w(c.Wt, BF, device)                 # We^T packed [inp padded to 64][hid padded to 32]
    b.wexp = pack_w(c.Wt.t(), BF, device)           # We packed [hid padded to 64][inp padded to 32]
    b.c1, b.c2, b.c3 = _cv(c.c1, device), _cv(c.c2, device), _cv(c.c3, device)
    b.add = _act2d(c.add, BF, "plain", device) if c.add is not None else None
    b.gx = fresh(M, inp, BF, "plain", device)
    b.dwe = c.prefill.float().contiguous().to(device)
    b.gram = torch.full((inp, inp), float("nan"), dtype=F32, device=device)
    b.sx = torch.full((inp,), float("nan"), dtype=F32, device=device)
    b.mp = torch.zeros(_pad(inp, 64), _pad(inp, 32), dtype=BF, device=device)
    b.vb = torch.full((kutil.pad8(inp),), float("nan"), dtype=F32, device=device)
    return b


def run_xb(r, device="cuda"):
    """gram -> xb_coeffs -> expand_bwd of one case (the first two only where the case has the x M + v term) -> list of mismatches"""
    from atomnas_amd import ops
    c = build_xb(r)
    b = xb_buffers(c, device)
    M, inp, hid = r["M"], r["inp"], r["hid"]
    who = "expand_bwd[%s]" % name_of(r)
    bad = []
    if not ops.expand_bwd_supported(inp, hid, BF):
        return [who + ": atomnas_expand_bwd_supported says no"]
    if r["mp"]:
        ops.gram(b.x, M, inp, b.gram, b.sx)
        torch.cuda.synchronize()
        bad += first_diff(who + " gram", b.gram, c.gram) + first_diff(who + " sx", b.sx, c.sx)
        ops.xb_coeffs(b.c2, b.c3, b.wexp, b.gram, b.sx, inp, hid, b.mp, b.vb, b.dwe)
        torch.cuda.synchronize()
        bad += first_diff(who + " mp", b.mp[:inp, :inp], c.mp) + first_diff(who + " vb", b.vb[:inp], c.vb)
        inside = torch.zeros_like(b.mp, dtype=torch.bool)
        inside[:inp, :inp] = True
        if bool((b.mp.float()[~inside] != 0).any()):
            bad.append(who + " mp: non-zero padding")
        bad += first_diff(who + " dwe after xb_coeffs", b.dwe, c.dwe1)
    ops.expand_bwd(b.h, b.c1, b.x, b.wt, b.add, b.gx, b.dwe.view(-1), M, inp, hid, mp=b.mp if r["mp"] else None, vb=b.vb if r["mp"] else None)
    torch.cuda.synchronize()
    bad += first_diff(who + " gx", b.gx[:, :inp], c.gx) + _pad_zero(who + " gx", b.gx, inp)
    bad += first_diff(who + " dwe", b.dwe, c.dwe)
    return bad


# ------------------------------------------------------------------------------------------------ project_bwd
def pb_cases():
    """oup 8 / 24 / 64 and every accumulator width (1..4 tiles of 16: oup 16, 32, 48, 64, as tools/make_pw_dispatch.py pb_rows), hid
    with whole and ragged 64-channel chunks, activation codes 1 / 2, z plain and slab-major, both strides of dWp"""
    rows = []
    i = 0
    for oup, hid in ((8, 96), (16, 432), (24, 200), (32, 432), (48, 432), (64, 136), (64, 432), (24, 203)):
        for M in (1031, 4100):
            for act in (1, 2):
                lay = "slab" if (hid % 8 or i % 2) else "plain"
                rows.append(dict(M=M, oup=oup, hid=hid, act=act, z=lay, tr=(i // 2) % 2))
                i += 1
    for oup, hid in ((8, 96), (64, 432)):           # the layouts / strides the alternation above left out
        for lay, tr in (("slab", 0), ("slab", 1), ("plain", 0), ("plain", 1)):
            rows.append(dict(M=1031, oup=oup, hid=hid, act=1 + tr, z=lay, tr=tr))
    return _dedup(rows)


def pb_twins():
    """the Swish twin of every case"""
    return _dedup([twin(r, ("act",)) for r in pb_cases()])


# atomnas_project_bwd_dp_supported answers no: plain hidden tensors whose width is no multiple of 8, unsupported widths
PB_QUERIES_NO = [dict(M=1031, oup=24, hid=203, z="plain"), dict(M=4100, oup=8, hid=100, z="plain"), dict(M=1031, oup=72, hid=432, z="slab"),
                 dict(M=1031, oup=64, hid=120, z="slab")]


def pb_query(r):
    """arguments of atomnas_project_bwd_dp_supported for a case: (M, oup, hid, ldg, ldz, z_ss, ldgh, gh_ss, stat_rows, dtype)"""
    from atomnas_amd import ops
    slab = r["z"] == "slab"
    ld, ss = (16, r["M"] * 16) if slab else (kutil.pad8(r["hid"]), 0)
    return (r["M"], r["oup"], r["hid"], kutil.pad8(r["oup"]), ld, ss, ld, ss, ops.stat_rows_for(r["hid"]), 1)


def pb_expected(r):
    """what the query must answer (csrc/pwconv.hip atomnas_project_bwd_supported, nt_st_kind)"""
    oup, hid = r["oup"], r["hid"]
    return bool(8 <= oup <= 64 and oup % 8 == 0 and hid >= 96 and hid >= 2 * oup and (r["z"] == "slab" or hid % 8 == 0))


def build_pb(r):
    M, oup, hid, act = r["M"], r["oup"], r["hid"], r["act"]
    gen = _gen("pb", *[r[k] for k in sorted(r)])
    c = types.SimpleNamespace(r=r, dtype=BF, exact=act != 3)
    c.G = operand(gen, M, oup, PRO_NONE, 0, BF)                       # dP
    c.Z = operand(gen, M, hid, PRO_BNRELU, act, BF)                   # z, zscale, zshift
    c.Wt = banded(gen, hid, oup)                                      # Wp^T [hid, oup]
    c.prefill = _draw(gen, [-3, -2, -1, 0, 1, 2, 3], oup, hid)
    c.acc = (c.G.eff @ c.Wt.t()) * kutil.act_grad64(c.Z.pre, act)
    c.mag = c.G.eff.abs() @ c.Wt.abs().t()
    c.gh = c.acc.to(BF).double()
    c.second = c.gh * c.Z.a
    c.prod = c.G.eff.t() @ c.Z.eff
    c.dwp = c.prefill + c.prod
    c.dwp_mag = c.prefill.abs() + c.G.eff.abs().t() @ c.Z.eff.abs()
    return c


def pb_buffers(c, device):
    r = c.r
    M, oup, hid = r["M"], r["oup"], r["hid"]
    b = types.SimpleNamespace()
    b.g = _act2d(c.G.a, BF, "plain", device)
    b.wpt = pack_w(c.Wt, BF, device)
    b.z = _act2d(c.Z.a, BF, r["z"], device)
    b.zs, b.zh = _cv(c.Z.c1, device), _cv(c.Z.c2, device)
    b.gh = fresh(M, hid, BF, r["z"], device)
    b.stats = stats_buf(hid, device)
    b.dwp = (c.prefill.t() if r["tr"] else c.prefill).float().contiguous().to(device)
    return b


def run_pb(r, device="cuda"):
    from atomnas_amd import ops
    c = build_pb(r)
    b = pb_buffers(c, device)
    M, oup, hid = r["M"], r["oup"], r["hid"]
    who = "project_bwd[%s]" % name_of(r)
    rows = ops.stat_rows_for(hid)
    if not ops.project_bwd_dp_supported(M, oup, hid, b.g, b.z, b.gh, rows):
        return [who + ": atomnas_project_bwd_dp_supported says no"]
    si, sj = (1, oup) if r["tr"] else (hid, 1)
    ops.project_bwd(b.g, b.wpt, b.z, b.zs, b.zh, r["act"], b.gh, b.stats, b.dwp.view(-1), si, sj, M, oup, hid, stat_rows=rows)
    torch.cuda.synchronize()
    ghp = plain(b.gh)
    got = ghp[:, :hid].double().cpu()
    dwp = b.dwp.t() if r["tr"] else b.dwp
    if c.exact:
        bad = first_diff(who + " gh", got, c.gh) + first_diff(who + " dwp", dwp, c.dwp)
        first, second = c.gh, c.second
    else:
        bad = close(who + " gh", got, c.acc, **twin_tol(BF, float(c.acc.abs().max())))
        bad += close(who + " dwp", dwp, c.dwp, **twin_tol(BF, float(c.dwp.abs().max())))
        first, second = got, got * c.Z.a
    return bad + _pad_zero(who + " gh", ghp, hid) + check_stats(who, b.stats, first, second, c.exact, M)


# ------------------------------------------------------------------------------------------------ preconditions (tests/test_pw_exact.py)
def masked_inputs(c):
    """[(name, pre-activation, activation code)] of every input a case reads through an activation prologue or a mask"""
    out = []
    for name in ("A", "U", "V", "Z"):
        o = getattr(c, name, None)
        if o is not None and o.pre is not None and o.act:
            out.append((name, o.pre, o.act))
    return out


def check_activation_mix(c):
    """(c): at least 5 % of the pre-activations exactly 0, 5 % on each side of 0, in mode 2 also 5 % exactly 6 and 5 % above 6"""
    for name, pre, act in masked_inputs(c):
        assert _mix_ok(pre, act), (name, "zero / sign / ReLU6 bound mix")


def check_coverage(eff, name):
    """(b) for one operand: every row and every channel has a non-zero effective value somewhere"""
    nz = eff != 0
    assert bool(nz.any(1).all()), name + ": a row of zeros"
    assert bool(nz.any(0).all()), name + ": a channel of zeros"


def check_integer(t, name, bound=256.0):
    assert bool((t == t.round()).all()) and float(t.abs().max()) <= bound, name + ": not a small integer"


def check_padding(buf, C, poisoned=False):
    """(d) for one activation buffer (plain or slab-major): padding channels zero; an output's valid region is poisoned"""
    p = plain(buf)
    assert p.shape[1] == C or float(p[:, C:].float().abs().max()) == 0.0, "non-zero padding channels"
    if poisoned:
        assert bool(torch.isnan(p[:, :C].float()).all()), "output not poisoned"


def check_packed(wp, n, k):
    """(d) for packed weights: pad rows and pad columns zero"""
    assert wp.shape[0] % 64 == 0 and wp.shape[1] % 32 == 0
    assert float(wp[n:].float().abs().max() if wp.shape[0] > n else 0) == 0.0 and float(wp[:, k:].float().abs().max() if wp.shape[1] > k else 0) == 0.0


def check_stats_buf(st, N):
    from atomnas_amd import ops
    assert tuple(st.shape) == (ops.stat_rows_for(N), 2, N) and bool(torch.isnan(st).all())


# ------------------------------------------------------------------------------------------------ child interpreter
def child_main(what):
    """runs the named tables in THIS interpreter (its environment carries the switches) and prints the mismatches as a JSON list"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bad = []
    if "nt" in what:
        for r in nt_cases():
            if not r["whole_chip"] or cus == 256:
                bad += run_nt(r)
    if "xb" in what:
        for r in xb_cases():
            bad += run_xb(r)
    print(json.dumps(bad))


def counts():
    from collections import Counter
    out = {"gemm_nt": Counter(nt_family(r) for r in nt_cases()), "gemm_nt twins": Counter(nt_family(r) for r in nt_twins()),
           "gemm_tn": Counter(tn_family(r) for r in tn_cases()), "gemm_tn twins": Counter(tn_family(r) for r in tn_twins()),
           "expand_bwd": Counter(xb_family(r) for r in xb_cases()),
           "project_bwd": Counter({"exact": len(pb_cases()), "twins": len(pb_twins()), "queries answered no": len(PB_QUERIES_NO)})}
    return {k: dict(sorted(v.items())) for k, v in out.items()}


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child_main(sys.argv[2].split(","))
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        print(json.dumps(counts(), indent=1))
