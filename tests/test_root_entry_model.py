"""Why a fast ray may enter a mesh at its root's child pair (k_trace_fast: pick_next): Bounds::Intersect
(bvhtrimesh.h:18-36) is monotone under box containment as long as every quotient is a finite number -- a box inside a rejected box is
rejected.  A float32 numpy model of the reference's test (true division, fminf / fmaxf, the 1.00000024f factor) is run on random
(ray, parent box, contained child box) triples whose direction components are all at least 2^-40 in magnitude, the fast path's
condition, and must never accept the child of a rejected parent.  A second group has a zero direction component: there the 0/0 of an
origin on a face plane is dropped by fminf / fmaxf on one box and not on the other, the implication fails, and slow rays therefore
keep the root-box step."""
import numpy as np

F = np.float32
FLT_MAX = F(3.402823466e+38)
C = F(1.00000024)


def bounds_intersect(lo, hi, o, d, rayt):
    """Bounds::Intersect for n (box, ray) pairs in float32, operation by operation; True where the box is accepted"""
    with np.errstate(all="ignore"):
        tmin = np.zeros(len(o), F)
        tmax = rayt.astype(F).copy()
        ok = np.ones(len(o), bool)
        for a in range(3):
            q0 = ((lo[:, a] - o[:, a]).astype(F) / d[:, a]).astype(F)
            q1 = ((hi[:, a] - o[:, a]).astype(F) / d[:, a]).astype(F)
            t0, t1 = np.fmin(q0, q1), np.fmax(q0, q1)
            tmin = np.fmax(t0, tmin)
            tmax = np.fmin(t1, tmax)
            ok &= ~((tmax * C).astype(F) < tmin)
    return ok


def triples(n, seed, grid=None):
    """n parent boxes, child boxes inside them and rays.  A third of the child faces lie on the parent's face, a fifth of all box
    axes have zero thickness, a quarter of the origin coordinates lie on a face plane of either box; rayt is FLT_MAX for half of the
    rays, and the others end around the boxes.  grid: coordinates rounded to multiples of it (exact ties between planes)."""
    rs = np.random.RandomState(seed)
    snap = (lambda x: x) if grid is None else (lambda x: np.round(x / grid) * grid)
    a, b = snap(rs.uniform(-4, 4, (n, 3))), snap(rs.uniform(-4, 4, (n, 3)))
    plo, phi = np.minimum(a, b).astype(F), np.maximum(a, b).astype(F)
    flat = rs.uniform(size=(n, 3)) < 0.2
    phi = np.where(flat & (rs.uniform(size=(n, 3)) < 0.5), plo, phi)
    u, v = rs.uniform(size=(n, 3)), rs.uniform(size=(n, 3))
    clo = snap(plo + np.minimum(u, v) * (phi - plo)).astype(F)
    chi = snap(plo + np.maximum(u, v) * (phi - plo)).astype(F)
    clo = np.where(rs.uniform(size=(n, 3)) < 1 / 3, plo, clo)
    chi = np.where(rs.uniform(size=(n, 3)) < 1 / 3, phi, chi)
    chi = np.where(flat, clo, chi)
    clo, chi = np.clip(clo, plo, phi), np.clip(chi, plo, phi)
    chi = np.maximum(clo, chi)
    assert (plo <= clo).all() and (clo <= chi).all() and (chi <= phi).all()
    # rays: towards a point near the child box (half) or anywhere; origins inside, outside and on face planes
    o = snap(rs.uniform(-6, 6, (n, 3))).astype(F)
    inside = rs.uniform(size=n) < 0.2
    o[inside] = (plo + rs.uniform(size=(n, 3)) * (phi - plo)).astype(F)[inside]
    planes = np.stack([plo, phi, clo, chi], 0)
    on_face = rs.uniform(size=(n, 3)) < 0.25
    pick = rs.randint(4, size=(n, 3))
    o = np.where(on_face, np.take_along_axis(planes, pick[None], 0)[0], o).astype(F)
    tgt = clo + rs.uniform(-0.2, 1.2, (n, 3)) * (chi - clo) + rs.normal(0, 0.05, (n, 3))
    d = np.where((rs.uniform(size=n) < 0.6)[:, None], tgt - o, rs.normal(size=(n, 3)))
    tiny = rs.uniform(size=(n, 3)) < 0.1
    d = np.where(tiny, 2.0 ** rs.uniform(-40, -20, (n, 3)) * rs.choice([-1.0, 1.0], (n, 3)), d)
    d = np.where(np.abs(d) < 2.0 ** -40, np.where(d < 0, -1.0, 1.0) * 2.0 ** -40, d).astype(F)
    rayt = np.where(rs.uniform(size=n) < 0.5, FLT_MAX, rs.uniform(0, 12, n)).astype(F)
    return plo, phi, clo, chi, o, d, rayt


def test_a_box_inside_a_rejected_box_is_rejected():
    """>= 10^5 triples with every |D| component >= 2^-40: child accepted => parent accepted"""
    total = accepted = rejected_parents = 0
    for seed, grid in ((1, None), (2, None), (3, 0.125), (4, 0.5)):
        plo, phi, clo, chi, o, d, rayt = triples(60000, seed, grid)
        assert (np.abs(d) >= F(2.0 ** -40)).all()
        assert ((chi == clo).any(1)).sum() > 5000 and ((clo == plo) | (chi == phi)).any(1).sum() > 20000
        assert (rayt == FLT_MAX).sum() > 20000 and (rayt < FLT_MAX).sum() > 20000
        assert ((o == plo) | (o == phi) | (o == clo) | (o == chi)).any(1).sum() > 20000
        parent, child = bounds_intersect(plo, phi, o, d, rayt), bounds_intersect(clo, chi, o, d, rayt)
        bad = child & ~parent
        assert not bad.any(), (int(bad.sum()), plo[bad][:2], phi[bad][:2], clo[bad][:2], chi[bad][:2], o[bad][:2], d[bad][:2], rayt[bad][:2])
        total += len(o)
        accepted += int(child.sum())
        rejected_parents += int((~parent).sum())
    print("triples %d, child accepted %d, parent rejected %d" % (total, accepted, rejected_parents))
    assert total >= 100000 and accepted > 20000 and rejected_parents > 20000


def test_a_zero_direction_component_breaks_the_implication():
    """A zero-thickness child on its parent's face and an origin in that plane, D = 0 on the axis: both child quotients are 0/0, which
    fminf / fmaxf drop (the axis passes); the parent's are 0/0 and an infinity, which survives (tmin = +inf or tmax = -inf: rejected)."""
    plo, phi = F([[-1, 0, -1]]), F([[1, 2, 1]])
    clo, chi = F([[-1, 0, -1]]), F([[1, 0, 1]])          # the floor of the room
    o, d, rayt = F([[-3, 0, 0.25]]), F([[1, 0, 0]]), F([FLT_MAX])
    assert bounds_intersect(clo, chi, o, d, rayt)[0] and not bounds_intersect(plo, phi, o, d, rayt)[0]
    # and among random triples with one zero component (either sign) on an axis where the origin lies on a face plane
    plo, phi, clo, chi, o, d, rayt = triples(60000, 5, 0.125)
    rs = np.random.RandomState(6)
    axis = rs.randint(3, size=len(o))
    rows = np.arange(len(o))
    d[rows, axis] = np.where(rs.uniform(size=len(o)) < 0.5, F(-0.0), F(0.0))
    o[rows, axis] = np.where(rs.uniform(size=len(o)) < 0.5, clo[rows, axis], chi[rows, axis])
    parent, child = bounds_intersect(plo, phi, o, d, rayt), bounds_intersect(clo, chi, o, d, rayt)
    print("zero-component triples %d: child accepted under a rejected parent %d" % (len(o), int((child & ~parent).sum())))
    assert (child & ~parent).sum() >= 1
