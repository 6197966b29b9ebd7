"""Preconditions of tests/test_gpu_ray_edges.py, on the CPU: every ray class of ray_edge_cases.py contains what it is named after
(so the GPU comparison cannot pass on empty classes), and a model of the Markstein divide in exact arithmetic pins where its
domain ends.  Each test prints its counts (pytest -s shows them)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ray_edge_cases as rc
from helpers import bits
from oracle import binding as ob

F = np.float32
HITS_AND_MISSES = [(c, s) for c, s in rc.CASE_IDS if c not in ("tmax_edges", "on_plane")] + [(c, "far16") for c in rc.FAR16_CLASSES]


def _finite(rays):
    return np.isfinite(rays["o"]).all() and np.isfinite(rc.normalize32(rays["d"])).all() and not np.isnan(rays["tmax"]).any()


@pytest.mark.parametrize("cls,scn", HITS_AND_MISSES)
def test_class_hits_and_misses(cls, scn):
    desc, rays = rc.case(cls, scn)
    assert _finite(rays)
    oh, _ = rc.oracle_scene(desc).intersect(rays)
    n, hits = len(rays), int(oh["hit"].sum())
    print("%s on %s: %d rays, %d hits, %d misses" % (cls, scn, n, hits, n - hits))
    assert 2000 <= n <= 40000
    assert not np.isnan(oh["t"]).any()      # (a NaN has no defined bit pattern to compare)
    assert hits >= 0.05 * n and n - hits >= 0.05 * n


@pytest.mark.parametrize("cls", ["tmax_edges", "on_plane"])
def test_exempt_classes_still_hit(cls):
    for scn in rc.SCENES:
        desc, rays = rc.case(cls, scn)
        assert _finite(rays)
        oh, _ = rc.oracle_scene(desc).intersect(rays)
        print("%s on %s: %d rays, %d hits" % (cls, scn, len(rays), int(oh["hit"].sum())))
        assert oh["hit"].sum() >= 200 and (oh["hit"] == 0).sum() >= 200


def test_domain_edge_rays_hit():
    for name, desc, rays in rc.domain_edge():
        assert _finite(rays)
        oh, _ = rc.oracle_scene(desc).intersect(rays)
        print("domain_edge %s: %d rays, %d hits" % (name, len(rays), int(oh["hit"].sum())))
        assert oh["hit"].sum() >= 500
    # what the three cases are named after, on the normalised directions
    (_, tiny, r0), (_, far, r1), (_, spike, r2) = rc.domain_edge()
    lo, hi = rc.mesh_root_box(tiny)
    a = np.abs(hi[1] - r0["o"][:, 1])
    assert ((a > 0) & (a <= F(2.0 ** -107))).sum() >= 1000
    with np.errstate(over="ignore"):
        for desc, rays in ((far, r1), (spike, r2)):
            lo, hi = rc.mesh_root_box(desc)
            dy = rc.normalize32(rays["d"])[:, 1]
            fast = np.abs(dy) >= rc.LIM             # only these take the Markstein divide
            q = np.maximum(np.abs((hi[1] - rays["o"][:, 1]) / dy), np.abs((lo[1] - rays["o"][:, 1]) / dy))
            print("  |D.y| >= 2^-40: %d rays, of them %d with an overflowing root-box quotient" % (fast.sum(), np.isinf(q[fast]).sum()))
            assert np.isinf(q[fast]).sum() >= 500 and np.isfinite(q[fast]).sum() >= 100


def test_threshold_values_reach_the_traversal():
    """Each threshold value arrives bit for bit (after the normalisation) on at least 20 rays per sign, and both sides of 2^-40 occur
    on every axis."""
    desc, rays = rc.case("threshold", "grid1")
    d = rc.normalize32(rays["d"])
    for v in rc.THRESHOLD_VALUES:
        for s in (F(1), F(-1)):
            n = int((d == s * v).any(axis=1).sum())
            print("threshold %-14r sign %+d: %d rays" % (float(v), int(s), n))
            assert n >= 20
    for a in range(3):
        assert (np.abs(d[:, a]) >= rc.LIM).sum() > 500 and ((np.abs(d[:, a]) < rc.LIM) & (d[:, a] != 0)).sum() > 200


def test_on_plane_quotients():
    """(b - O) / D over the height field's root box in fp32: 0/0 = NaN on the zero-component half, +-0 on the other."""
    desc, rays = rc.case("on_plane", "grid1")
    lo, hi = rc.mesh_root_box(desc, 0)
    d = rc.normalize32(rays["d"])
    with np.errstate(all="ignore"):
        q = np.concatenate([(lo - rays["o"]) / d, (hi - rays["o"]) / d], axis=1)
    nan = int(np.isnan(q).any(axis=1).sum())
    zero = int(((q == 0) & ~np.isnan(q)).any(axis=1).sum())
    flat = int(((rays["o"][:, 1] == 0) & (d[:, 1] == 0)).sum())
    print("on_plane: %d rays with a NaN quotient, %d with a +-0 quotient, %d in the plane of the flat mesh" % (nan, zero, flat))
    assert nan >= 200 and zero >= 200 and flat >= 100
    for a in range(3):
        z = d[:, a] == 0
        assert (np.signbit(d[:, a]) & z).sum() >= 50 and (~np.signbit(d[:, a]) & z).sum() >= 50


def test_signed_zero_both_signs_on_every_axis():
    """Both signs of zero occur on every axis.  The count of rays for which Bounds::Intersect on the height field's root box answers
    differently for +0.0 and -0.0 is printed, not asserted: no ray can make it differ.  With D[a] = +-0 the axis' quotients are
      origin inside the slab    (-inf, +inf) in either order, the same t0 = -inf and t1 = +inf for both signs;
      origin outside the slab   (+inf, +inf) or (-inf, -inf): one sign makes tmin = +inf, the other tmax = -inf, and as D has a
                                non-zero component (a zero vector cannot be normalised) another axis makes tmax finite, before or
                                after: tmax * 1.00000024f < tmin rejects for both signs, also with ray.t = +inf;
      origin on the lower face  (NaN, +-inf): the comparator min/max return their second argument, t0 = t1 = +-inf, rejected as above;
      origin on the upper face  (+-inf, NaN): t0 = t1 = NaN, which the comparator max/min against tmin/tmax drop for both signs.
    The class still matters on the GPU: 1/D = -inf flips the slab order, and the hardware min/max differ from the comparator form
    exactly on these NaNs."""
    desc, rays = rc.case("signed_zero", "grid1")
    d = rays["d"]
    for a in range(3):
        z = d[:, a] == 0
        neg, pos = int((np.signbit(d[:, a]) & z).sum()), int((~np.signbit(d[:, a]) & z).sum())
        print("signed_zero axis %d: %d rays with -0.0, %d with +0.0" % (a, neg, pos))
        assert neg >= 200 and pos >= 200
    lo, hi = rc.mesh_root_box(desc, 0)
    differ = nan = 0
    for r in rays:
        f = r.copy()
        f["d"] = np.where(f["d"] == 0, -f["d"], f["d"])
        differ += ob.bounds_intersect(lo, hi, r)[0] != ob.bounds_intersect(lo, hi, f)[0]
    with np.errstate(all="ignore"):
        nan = int(np.isnan(np.concatenate([(lo - rays["o"]) / d, (hi - rays["o"]) / d], axis=1)).any(axis=1).sum())
    print("signed_zero: the root-box answer depends on the sign of zero for %d of %d rays; %d rays have a NaN quotient" % (differ, len(rays), nan))
    assert nan >= 100


FIELDS_SAME = ("hit", "prim", "tri", "b1", "b2")


def scaled_relation_holds(h0, hk, k):
    """The records of scaled(k) against those of scaled(0): same hit/prim/tri/b1/b2 bits and t * 2^k exactly.  (The Ray constructor
    normalises D, so a D scaled by 2^k reaches the traversal bit for bit as the unscaled one: the relation is t * 2^k for both
    variants, and the scaled-D variant checks the normalisation's own scaling.)"""
    same = all(np.array_equal(h0[f].view(np.uint32), hk[f].view(np.uint32)) for f in FIELDS_SAME)
    return same and np.array_equal(bits(h0["t"] * F(2.0 ** k)), bits(hk["t"]))


@pytest.mark.parametrize("scale_d", [False, True])
def test_scaled_oracle_records(scale_d):
    """At k = +-20 the oracle's own records obey the relation (the builder makes the same splits).  At k = +-40 they do not: at
    2^-40 the triangle test's determinant products and the sphere's r^2 leave the normal range, so only the oracle comparison is
    made there (test_gpu_ray_edges.py)."""
    d0, r0 = rc.scaled(0, scale_d)
    h0, _ = rc.oracle_scene(d0).intersect(r0)
    assert h0["hit"].sum() >= 0.05 * len(r0) and (h0["hit"] == 0).sum() >= 0.05 * len(r0)
    for k in rc.SCALED_K:
        dk, rk = rc.scaled(k, scale_d)
        assert _finite(rk)
        hk, _ = rc.oracle_scene(dk).intersect(rk)
        ok = scaled_relation_holds(h0, hk, k)
        print("scaled(%d, D scaled: %s): %d hits, relation to k = 0 holds: %s" % (k, scale_d, int(hk["hit"].sum()), ok))
        assert hk["hit"].sum() >= 0.05 * len(rk) and (hk["hit"] == 0).sum() >= 0.05 * len(rk)
        if abs(k) <= 20:
            assert ok


# ---- the Markstein divide in exact arithmetic --------------------------------------------------------------------------------
def rn32(x):
    """Round a Fraction to the nearest fp32 value, ties to even, denormals included; +-inf beyond the range."""
    if x == 0:
        return Fraction(0)
    s, x = (-1, -x) if x < 0 else (1, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n = x / ulp
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (fl & 1)):
        fl += 1
    r = fl * ulp
    return s * math.inf if r >= Fraction(2) ** 128 else s * r


def mdiv_model(a, b):
    """agpt_trace.h: mdiv with r = RN(1/b): q = RN(a*r); e = RN(a - b*q); RN(e*r + q), each one IEEE operation.  An infinite q
    makes e the opposite infinity and the last fma inf - inf."""
    r = rn32(1 / b)
    q = rn32(a * r)
    if isinstance(q, float):
        return math.nan
    e = rn32(a - b * q)
    return rn32(e * r + q)


def _operands(rng, n, lo_exp, hi_exp):
    e = rng.randint(lo_exp, hi_exp + 1, size=n)
    m = rng.randint(2 ** 23, 2 ** 24, size=n)
    s = rng.choice([-1, 1], size=n)
    out = []
    for ei, mi, si in zip(e, m, s):
        if ei < -126:                                   # a denormal: a multiple of 2^-149 below 2^(ei+1)
            mi = max(1, int(mi) >> (-126 - int(ei)))
            ei = -126
        out.append(int(si) * Fraction(int(mi), 2 ** 23) * Fraction(2) ** int(ei))
    return out


def _count_differing(rng, n, a_exp, b_exp, keep=None):
    differ = total = 0
    for a, b in zip(_operands(rng, n, *a_exp), _operands(rng, n, *b_exp)):
        want = rn32(a / b)
        if keep is not None and not keep(want):
            continue
        got = mdiv_model(a, b)
        total += 1
        differ += not (got == want)          # a NaN differs from everything
    return differ, total


def test_mdiv_model_pins_the_domain():
    """Inside |a| in 2^[-100, 87], |b| in 2^[-40, 100] (and on the two other regions measured equal) the three-operation divide is
    the fp32 division; for |a| <= 2^-107 the correction term underflows and some quotients differ; where the quotient overflows the
    result is a NaN instead of an infinity.  This is data about the arithmetic, not the definition of the kernel: the kernel is
    judged by the oracle (test_gpu_ray_edges.py).  (Values are compared, so the sign of a zero quotient is not modelled.)"""
    rng = np.random.RandomState(40)
    for a_exp, b_exp in (((-100, 87), (-40, 100)), ((-20, 20), (-40, 20)), ((-10, 10), (40, 127))):
        differ, total = _count_differing(rng, 3000, a_exp, b_exp)
        print("mdiv model, |a| in 2^%s, |b| in 2^%s: %d of %d differ" % (a_exp, b_exp, differ, total))
        assert differ == 0 and total == 3000
    differ, total = _count_differing(rng, 4000, (-149, -107), (-40, -10))
    print("mdiv model, |a| < 2^-106, |b| in 2^[-40, -10]: %d of %d differ" % (differ, total))
    assert differ >= 1
    differ, total = _count_differing(rng, 3000, (89, 127), (-40, 0), keep=lambda w: isinstance(w, float))
    print("mdiv model, overflowing quotients: %d of %d differ" % (differ, total))
    assert total >= 500 and differ == total
