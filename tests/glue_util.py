"""Helpers of the kernel-level GPU tests of csrc/bn.hip, head.hip, optim.hip and shrink.hip: outputs inside NaN-filled allocations,
and the error bounds those tests use.

Bounds (u = 2^-24):
  * fp32 result of a short per-element expression:   |got - ref| <= 8 u * sum |terms entering the last addition|
  * stored as bf16:                                   + 2^-8 |ref|   (half an ulp is 2^-9; the margin covers a value the fp32 error
                                                                      moved across a rounding boundary)
  * fixed-order fp32 sum of n terms:                  (n + 8) u * sum |terms|
No outlier allowances: masked inputs are built with a margin (margin_pre), so that not one element may differ.
"""
import torch

U = 2.0 ** -24
GUARD = 3     # sentinel rows in front of and behind an activation tensor
NAN = float("nan")


def pad8(c):
    return (c + 7) // 8 * 8


def T(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


DTYPES = ["fp32", "bf16"]


TINY = 2.0 ** -126   # below the smallest normal fp32 number a result may be flushed to zero


def elem_bound(terms, ref=None, dtype=torch.float32):
    b = 8 * U * terms.double() + TINY
    if dtype == torch.bfloat16:
        b = b + 2.0 ** -8 * ref.double().abs()
    return b


def sum_bound(n, terms_abs_sum):
    return (n + 8) * U * terms_abs_sum.double()


def assert_within(name, got, ref, bound):
    got, ref, bound = got.double().cpu(), ref.double().cpu(), bound.double().cpu() if torch.is_tensor(bound) else bound
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite values (unwritten or corrupted elements)" % name
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(torch.nonzero(bad)[0].tolist())
        b = bound[i] if torch.is_tensor(bound) and bound.dim() else bound
        raise AssertionError("%s: %d of %d elements beyond the bound, first at %s: got %.9g ref %.9g bound %.3g (max err %.3g)" % (
            name, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]), float(b), float(err.max())))
    return float(err.max())


# ---- vectors ------------------------------------------------------------------------------------------------------------------
class Vec:
    """n elements inside a larger sentinel-filled allocation (NaN for floats, a marker value for integers); .v is the slice a kernel
    gets (16-byte aligned), check() asserts that nothing around it changed"""

    def __init__(self, n, dtype=torch.float32, fill=None, pad=16, marker=None):
        self.n, self.pad = n, pad
        self.marker = marker if marker is not None else (NAN if dtype.is_floating_point else 113)
        self.full = torch.full((n + 2 * pad,), self.marker, dtype=dtype, device="cuda")
        self.v = self.full[pad:pad + n]
        if fill is not None:
            self.v.copy_(fill.to(dtype) if torch.is_tensor(fill) else torch.full((n,), fill, dtype=dtype))

    def check(self, name="vector", upto=None):
        """everything outside [0, upto or n) still holds the sentinel"""
        n = self.n if upto is None else upto
        out = torch.cat([self.full[:self.pad], self.full[self.pad + n:]])
        ok = torch.isnan(out).all() if self.full.dtype.is_floating_point else (out == self.marker).all()
        assert bool(ok), "%s: a write outside [0, %d)" % (name, n)
        return self.v[:n]


def cvec(vals, C=None, extra=0.0):
    """per-channel fp32 INPUT vector of pad8(C) elements, channels C.. = `extra`, inside a NaN allocation"""
    C = vals.numel() if C is None else C
    v = Vec(pad8(C), fill=extra)
    v.v[:vals.numel()] = vals.float().cuda()
    return v


# ---- activations --------------------------------------------------------------------------------------------------------------
class Act:
    """[M, C] activation with pitch ld inside a NaN-filled allocation of GUARD rows on either side.  Inputs: columns C..pad8(C)-1 zero
    (the layout's contract), pad8(C)..ld-1 NaN (never to be read).  Outputs: all NaN before the launch; read() asserts afterwards that
    the guard rows and columns pad8(C)..ld-1 are still NaN and that columns C..pad8(C)-1 are zero."""

    def __init__(self, M, C, ld, dtype, values=None):
        assert ld % 8 == 0 and ld >= pad8(C)
        self.M, self.C, self.ld, self.dtype = M, C, ld, dtype
        self.full = torch.full((M + 2 * GUARD, ld), NAN, dtype=dtype, device="cuda")
        self.t = self.full[GUARD:GUARD + M]
        if values is not None:
            self.t[:, :pad8(C)] = 0
            self.t[:, :C] = values.to(dtype).cuda()

    def stored(self):
        """the values as stored, float64 on the CPU"""
        return self.t[:, :self.C].double().cpu()

    def read(self, name="output"):
        C, Cp = self.C, pad8(self.C)
        assert bool(torch.isnan(self.full[:GUARD]).all()) and bool(torch.isnan(self.full[GUARD + self.M:]).all()), "%s: a write outside the rows" % name
        if self.ld > Cp:
            assert bool(torch.isnan(self.t[:, Cp:]).all()), "%s: a write into columns pad8(C)..ld-1" % name
        if Cp > C:
            assert bool((self.t[:, C:Cp].float() == 0).all()), "%s: columns C..pad8(C)-1 are not zero" % name
        got = self.t[:, :C]
        assert bool(torch.isfinite(got.float()).all()), "%s: non-finite or unwritten elements" % name
        return got.double().cpu()


def stats_buf(rows, pitch):
    """statistics rows [rows][2][pitch], NaN before the launch, inside a NaN allocation"""
    v = Vec(rows * 2 * pitch)
    return v, v.v.view(rows, 2, pitch)


def stats_total(vec, view, name="statistics"):
    vec.check(name)
    assert bool(torch.isfinite(view).all()), "%s: rows left unwritten" % name
    return view.double().sum(0).cpu()


def margin_pre(gen, M, C, act, amp=2.0, gap=2.0 ** -5):
    """float64 pre-activations [M, C] at least `gap` away from 0 (and from 6 for ReLU6, whose range they straddle)"""
    t = torch.randn(M, C, generator=gen, dtype=torch.float64) * amp
    if act == 2:
        t = t + 3.0 * (torch.rand(M, C, generator=gen, dtype=torch.float64) > 0.5)
    t = torch.where(t >= 0, t + gap, t - gap)
    if act == 2:
        t = torch.where((t - 6).abs() < gap, torch.where(t >= 6, t + gap, t - gap), t)
    return t


def margin_input(gen, M, C, scale, shift, act, dtype, min_gap=2.0 ** -6, amp=2.0):
    """raw tensor z [M, C], rounded to the storage type, whose pre-activation z*scale + shift stays min_gap away from 0 and 6 in float64
    AFTER the rounding; returns z as float64.  (Built with twice the gap; elements the rounding moved too close are pushed out again.)
    `amp`: margin_pre's spread of the pre-activations."""
    pre = margin_pre(gen, M, C, act, amp=amp)
    z = ((pre - shift.double()) / scale.double()).to(dtype).double()
    for _ in range(4):
        p = z * scale.double() + shift.double()
        near = (p.abs() < min_gap) | ((act == 2) & ((p - 6).abs() < min_gap))
        if not bool(near.any()):
            break
        q = torch.full_like(p, 0.25)
        push = torch.where(p >= 6, q, torch.where(p >= 3, -q, torch.where(p >= 0, q, -q)))
        z = torch.where(near, ((p + push - shift.double()) / scale.double()).to(dtype).double(), z)
    p = z * scale.double() + shift.double()
    assert float(p.abs().min()) >= min_gap and (act != 2 or float((p - 6).abs().min()) >= min_gap)
    return z
