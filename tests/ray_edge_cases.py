"""Scenes and ray classes at the numeric edges of the traversal arithmetic (no GPU needed to build them).

The trace kernels leave the reference's plain (b - O) / D in three places: the Markstein divide of the fast slab test (all
|D| >= 2^-40), the true-division path for the other rays, and the conservative prefilters in front of the exact root-box tests.
helpers.random_rays reaches the edge of none of them; the classes here do.  tests/test_ray_edges.py checks on the CPU that every
class really contains what it is named after, tests/test_gpu_ray_edges.py compares the kernels with the oracle on them.

Both the oracle and the kernels normalise D as the reference's Ray constructor does (D * (1 / sqrt(dot(D, D)))), so a direction
component keeps a chosen bit pattern only when that factor is exactly 1: the builders below use directions whose other components
have an fp32 norm of exactly 1 (normalize32() is the fp32 model of that step), next to ordinary ones that move the component by
a factor near 1.  Every direction has at least one component of ordinary magnitude and every origin, direction and tmax is finite
except for tmax = +inf where a class says so: no ray here has a NaN or an infinite O or D.
"""
import numpy as np

import ag_pathtracer_amd as ag
from oracle import binding as ob

F = np.float32
FLT_MAX = F(3.402823466e+38)
FLT_MIN = F(2.0 ** -126)
DENORM_MIN = F(2.0 ** -149)
LIM = F(2.0 ** -40)          # agpt_trace.h: the fast slab test is taken when every |D| component is >= LIM


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def _idx(tris):
    t = np.asarray(tris, np.int32).reshape(-1)
    return np.stack([t, t, t], axis=1)


def _quads(nx, nz):
    a = (np.arange(nz)[:, None] * (nx + 1) + np.arange(nx)[None, :]).reshape(-1)
    b, c, d = a + 1, a + nx + 1, a + nx + 2
    return np.stack([a, c, b, b, c, d], axis=1).reshape(-1, 3)


def grid_heightfield():
    """16 x 16 cells over [-2, 2]^2, heights in [0.5, 1.5]; every coordinate is a multiple of 1/8."""
    n = 16
    x = -2.0 + 0.25 * np.arange(n + 1)
    X, Z = np.meshgrid(x, x, indexing="xy")
    Y = 1.0 + np.round(4.0 * np.sin(1.7 * X + 0.3) * np.cos(1.3 * Z)) / 8.0
    v = np.stack([X, Y, Z], axis=-1).reshape(-1, 3).astype(F)
    assert np.all(v * 8 == np.round(v * 8))
    return v, _idx(_quads(n, n))


def flat_quads(y=0.0, half=2.5, n=4):
    """n x n quads in the plane y: the root box and every inner box have zero thickness."""
    x = np.linspace(-half, half, n + 1)
    X, Z = np.meshgrid(x, x, indexing="xy")
    v = np.stack([X, np.full_like(X, y), Z], axis=-1).reshape(-1, 3).astype(F)
    return v, _idx(_quads(n, n))


def _tetra(c, h):
    v = np.asarray(c, np.float64) + h * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    return v.astype(F), _idx([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def grid(leaf=1):
    d = ag.SceneDesc("grid-leaf%d" % leaf)
    m = d.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
    v, idx = grid_heightfield()
    d.add_mesh(v, None, None, idx, m, leaf)
    v, idx = flat_quads()
    d.add_mesh(v, None, None, idx, m, leaf)
    d.add_sphere([0.5, 2.5, -0.25], 0.5, m)
    d.add_plane([0.0, -0.5, 0.0], [6.0, 6.0], m)
    return d


def grid_long():
    """grid plus small meshes and spheres to 70 primitives: the same rays through k_candidates and k_trace_fast<LIST>."""
    d = grid(1)
    d.name = "grid-long"
    rng = np.random.RandomState(70)
    m = 0
    while d.n_prims < 70:
        c = np.round(rng.uniform([-3, 0.5, -3], [3, 3.5, 3]) * 8) / 8
        if d.n_prims % 4 == 0:
            d.add_sphere(c, 0.25, m)
        else:
            v, idx = _tetra(c, 0.25)
            d.add_mesh(v, None, None, idx, m, 1)
    return d


def far16():
    """70 primitives in three groups: mesh centres around +-7e4 and +-1e5 (beyond the fp16 range: the packed top-level boxes
    carry infinities), around 1e-6 (below the smallest normal half) and at ordinary coordinates.  The spheres all have ordinary
    coordinates."""
    d = ag.SceneDesc("far16")
    m = d.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
    rng = np.random.RandomState(16)
    for i in range(24):
        s = rng.choice([-1.0, 1.0], 3)
        c = s * rng.choice([7e4, 1e5], 3) + rng.uniform(-4e3, 4e3, 3)
        if i % 3 == 0:
            c[rng.randint(3)] = rng.uniform(-100, 100)   # a box that straddles 0 on one axis and is out of range on the others
        v, idx = _tetra(c, 2.5e3)
        d.add_mesh(v, None, None, idx, m, 1)
    for i in range(22):
        v, idx = _tetra(rng.uniform(-3e-6, 3e-6, 3), 1e-6)
        d.add_mesh(v, None, None, idx, m, 1)
    for i in range(16):
        v, idx = _tetra(rng.uniform(-6, 6, 3), 0.75)
        d.add_mesh(v, None, None, idx, m, 1)
    for i in range(8):
        d.add_sphere(rng.uniform(-6, 6, 3), 0.75, m)
    assert d.n_prims == 70
    return d


def mesh_root_box(desc, which=0):
    v = [op[1] for op in desc.ops if op[0] == "mesh"][which]
    return v.min(0), v.max(0)


# ---- shared pieces -------------------------------------------------------------------------------------------------------
def normalize32(d):
    """The Ray constructor's normalize in fp32, operation by operation (oracle_math.h: f3_normalize)."""
    d = np.ascontiguousarray(d, F)
    with np.errstate(all="ignore"):
        dot = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inv = F(1.0) / np.sqrt(dot)
        return d * inv[:, None]


def _bounds(desc):
    lo = np.full(3, np.inf)
    hi = np.full(3, -np.inf)
    for op in desc.ops:
        if op[0] == "mesh":
            lo, hi = np.minimum(lo, op[1].min(0)), np.maximum(hi, op[1].max(0))
        elif op[0] == "sphere":
            lo, hi = np.minimum(lo, op[1] - op[2]), np.maximum(hi, op[1] + op[2])
    return lo, hi


def _tris(desc):
    return np.concatenate([op[1].astype(np.float64)[op[4][:, 0].reshape(-1, 3)] for op in desc.ops if op[0] == "mesh"])


def _targets(desc, rng, n, miss=0.3):
    """n points to aim at and a mask of the ones meant to miss: points inside triangles, exact vertices, points inside spheres;
    the missing ones lie above everything in the scene."""
    tri = _tris(desc)
    k = rng.randint(len(tri), size=n)
    w = rng.dirichlet([1, 1, 1], n)
    p = (tri[k] * w[:, :, None]).sum(1)
    vtx = rng.uniform(size=n) < 0.25
    p[vtx] = tri[k, rng.randint(3, size=n)][vtx]
    sph = [(op[1].astype(np.float64), op[2]) for op in desc.ops if op[0] == "sphere"]
    if sph:
        on = rng.uniform(size=n) < 0.15
        j = rng.randint(len(sph), size=n)
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        q = np.array([sph[i][0] for i in j]) + 0.5 * np.array([sph[i][1] for i in j])[:, None] * u
        p[on] = q[on]
    lo, hi = _bounds(desc)
    missing = rng.uniform(size=n) < miss
    up = p.copy()
    up[:, 1] = hi[1] + (hi[1] - lo[1]) * rng.uniform(0.5, 2.0, n)
    p[missing] = up[missing]
    return p, missing


def _rays_towards(desc, rng, d, tmax_short=0.25):
    """Rays with the given directions (float64 [n, 3], written to the rays unchanged) through _targets(): O = T - s * unit(D).
    A ray meant to miss starts at its target above the scene and does not point down."""
    n = len(d)
    p, missing = _targets(desc, rng, n)
    d = d.copy()
    down = missing & (d[:, 1] < 0)
    d[down] = -d[down]
    with np.errstate(all="ignore"):
        u = d / np.linalg.norm(d, axis=1, keepdims=True)
    s = rng.uniform(0.5, 8.0, n) * np.maximum(0.5 * np.abs(p).max(1), 1e-5)
    s[missing] = 0.0
    rays = np.zeros(n, ag.RAY_DTYPE)
    rays["o"] = (p - s[:, None] * u).astype(F)
    rays["d"] = d.astype(F)
    t = np.full(n, FLT_MAX, F)
    short = rng.uniform(size=n) < tmax_short
    t[short] = (s * rng.uniform(0.5, 1.5, n)).astype(F)[short]
    rays["tmax"] = t
    return rays


# pairs (x, y) whose fp32 squares sum to exactly 1: with a third component below 2^-39 the normalisation factor is exactly 1
def _unit_pairs():
    out = [(1.0, 0.0)]
    for a, b, c in ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29), (9, 40, 41), (12, 35, 37)):
        x, y = F(a) / F(c), F(b) / F(c)
        if x * x + y * y == F(1.0):
            out.append((float(x), float(y)))
    return out


UNIT_PAIRS = _unit_pairs()


def _fill_ordinary(rng, d, special):
    """Give the components of d[n, 3] that are not `special` ordinary values: half of the rays get a unit pair or a single +-1 (the
    special components then survive the normalisation bit for bit), the others random components."""
    n = len(d)
    for i in range(n):
        free = np.nonzero(~special[i])[0]
        if rng.uniform() < 0.5:
            if len(free) == 1:
                d[i, free[0]] = rng.choice([-1.0, 1.0])
            else:
                x, y = UNIT_PAIRS[rng.randint(len(UNIT_PAIRS))]
                if rng.uniform() < 0.5:
                    x, y = y, x
                two = rng.permutation(free)[:2]
                d[i, two[0]] = x * rng.choice([-1.0, 1.0])
                d[i, two[1]] = y * rng.choice([-1.0, 1.0])
                for a in free:
                    if a not in two:
                        d[i, a] = 0.0
        else:
            d[i, free] = rng.normal(size=len(free)) + np.sign(rng.normal(size=len(free))) * 0.05
    return d


# ---- ray classes -------------------------------------------------------------------------------------------------------------
THRESHOLD_VALUES = np.array([LIM, np.nextafter(LIM, F(0)), F(2.0 ** -39), F(2.0 ** -41), F(2.0 ** -60), FLT_MIN,
                             F(2.0 ** -127), F(3 * 2.0 ** -140), DENORM_MIN], F)


def aimed(desc, n=3000, seed=1):
    """Ordinary rays (no special component anywhere): the base set of tmax_edges and scaled."""
    rng = np.random.RandomState(seed)
    d = rng.normal(size=(n, 3))
    return _rays_towards(desc, rng, d)


def threshold(desc, n=4000, seed=2):
    """One or two direction components from THRESHOLD_VALUES (both signs) around the 2^-40 switch between the Markstein and the
    true-division slab test, the others ordinary."""
    rng = np.random.RandomState(seed)
    d = np.zeros((n, 3))
    special = np.zeros((n, 3), bool)
    for i in range(n):
        k = 1 if rng.uniform() < 0.7 else 2
        special[i, rng.permutation(3)[:k]] = True
    vals = THRESHOLD_VALUES[rng.randint(len(THRESHOLD_VALUES), size=(n, 3))].astype(np.float64) * rng.choice([-1.0, 1.0], (n, 3))
    d[special] = vals[special]
    _fill_ordinary(rng, d, special)
    return _rays_towards(desc, rng, d)


def signed_zero(desc, n=4000, seed=3):
    """One or two zero direction components, each +0.0 or -0.0 independently.  On a zero axis the origin coordinate is that of the
    target (inside the slab), beyond the scene box (outside) or exactly a face of a mesh's root box (0/0); the other axes start
    inside or outside as the distance to the target falls.  A fifth of the rays has tmax = +inf."""
    rng = np.random.RandomState(seed)
    d = np.zeros((n, 3))
    special = np.zeros((n, 3), bool)
    for i in range(n):
        k = 1 if rng.uniform() < 0.6 else 2
        special[i, rng.permutation(3)[:k]] = True
    d[special] = np.where(rng.uniform(size=(n, 3)) < 0.5, -0.0, 0.0)[special]
    _fill_ordinary(rng, d, special)
    rays = _rays_towards(desc, rng, d)
    lo, hi = _bounds(desc)
    meshes = [op[1] for op in desc.ops if op[0] == "mesh"]
    o = rays["o"]
    mode = rng.uniform(size=n)
    for i in range(n):
        a = np.nonzero(special[i])[0][0]
        if mode[i] < 0.25:
            o[i, a] = F(lo[a] - rng.uniform(0.125, 2.0)) if rng.uniform() < 0.5 else F(hi[a] + rng.uniform(0.125, 2.0))
        elif mode[i] < 0.40:
            v = meshes[rng.randint(len(meshes))]
            o[i, a] = v[:, a].min() if rng.uniform() < 0.5 else v[:, a].max()
    rays["o"] = o
    rays["tmax"][rng.uniform(size=n) < 0.2] = np.inf
    return rays


def on_plane(desc, n=1500, seed=4):
    """grid scenes only.  A +-0.0 direction component on an axis where the origin coordinate is a vertex coordinate of grid (a
    multiple of 1/8; a third of them a face of the height field's root box, a sixth y = 0, the plane of the flat mesh): (b - O)/D
    is 0/0 at every box plane there.  The second half repeats the origins with a non-zero component on that axis (quotient +-0)."""
    rng = np.random.RandomState(seed)
    lo, hi = mesh_root_box(desc, 0)
    rays = np.zeros(2 * n, ag.RAY_DTYPE)
    d = rng.normal(size=(n, 3))
    axis = rng.randint(3, size=n)
    t = rng.uniform(lo - 0.5, hi + 0.5, (n, 3))
    kind = rng.uniform(size=n)
    for i in range(n):
        a = axis[i]
        if kind[i] < 1 / 3:
            t[i, a] = lo[a] if rng.uniform() < 0.5 else hi[a]
        elif kind[i] < 1 / 2:
            a = axis[i] = 1
            t[i, a] = 0.0
            t[i, [0, 2]] = rng.uniform(-3, 3, 2)
        else:
            step = 0.125 if a == 1 else 0.25
            t[i, a] = lo[a] + step * rng.randint(int(round((hi[a] - lo[a]) / step)) + 1)
        d[i, a] = -0.0 if rng.uniform() < 0.5 else 0.0
    s = rng.uniform(0.0, 5.0, n)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    o = t - s[:, None] * u
    o[np.arange(n), axis] = t[np.arange(n), axis]
    rays["o"][:n] = o.astype(F)
    rays["d"][:n] = d.astype(F)
    d2 = d.copy()
    d2[np.arange(n), axis] = rng.normal(size=n)
    rays["o"][n:] = rays["o"][:n]
    rays["d"][n:] = d2.astype(F)
    rays["tmax"] = FLT_MAX
    rays["tmax"][rng.uniform(size=2 * n) < 0.2] = np.inf
    return rays


def tmax_edges(desc, n_base=1500, seed=5):
    """Rays the oracle hits at t*, each repeated with tmax in {t*, nextafter up, nextafter down, 0, -0.0, the smallest denormal,
    +inf, -1}: TriangleIntersect rejects t >= ray.t, Sphere::Intersect rejects ray.t < root."""
    base = aimed(desc, n_base, seed)
    base["tmax"] = FLT_MAX
    oh, _ = oracle_scene(desc).intersect(base)
    hit = base[oh["hit"] == 1]
    ts = oh["t"][oh["hit"] == 1]
    variants = [ts, np.nextafter(ts, F(np.inf)), np.nextafter(ts, F(-np.inf)), np.zeros_like(ts), np.full_like(ts, -0.0),
                np.full_like(ts, DENORM_MIN), np.full_like(ts, np.inf), np.full_like(ts, -1.0)]
    out = np.tile(hit, len(variants))
    out["tmax"] = np.concatenate(variants).astype(F)
    return out


def far_origin(desc, n=4000, seed=6):
    """Origins 2^10 ... 2^60 scene sizes away (less where the scene is large, see k_max) along random directions, aimed at vertices, sphere tangent points and root-box
    corners; D is the fp64 unit vector from the rounded origin to the target times 2^j, j in {0, -60, -10, 10, 30, 60}.  (An origin
    carries 24 bits: beyond about 2^24 scene sizes the aim at a triangle is lost, every b - O is -O, every box passes within the
    test's two ulps and the sphere test's discriminant is rounding noise of either sign -- the reference reports many such rays
    as sphere hits, and the oracle with it; half of the distances stay below 2^22.)"""
    rng = np.random.RandomState(seed)
    lo, hi = _bounds(desc)
    size = float(np.linalg.norm(hi - lo))
    tri = _tris(desc)
    tgt = tri[rng.randint(len(tri), size=n), rng.randint(3, size=n)]
    boxes = [(op[1].min(0), op[1].max(0)) for op in desc.ops if op[0] == "mesh"]
    sph = [(op[1].astype(np.float64), op[2]) for op in desc.ops if op[0] == "sphere"]
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    kind = rng.uniform(size=n)
    for i in range(n):
        if kind[i] < 0.25:
            b = boxes[rng.randint(len(boxes))]
            tgt[i] = np.where(rng.uniform(size=3) < 0.5, b[0], b[1])
        elif kind[i] < 0.45 and sph:
            c, r = sph[rng.randint(len(sph))]
            w = np.cross(u[i], rng.normal(size=3))
            tgt[i] = c + r * w / np.linalg.norm(w)          # the ray along u touches the sphere there
    # (|O| stays below 2^62: beyond 2^64 the sphere test's |O|^2 overflows and the reference reports hits at t = NaN, whose bit
    # pattern no standard fixes -- far16, 2^18 across, stops at 2^44 scene sizes)
    k_max = min(60.0, 62.0 - np.log2(size + np.abs(np.concatenate([lo, hi])).max()))
    k = np.where(rng.uniform(size=n) < 0.5, rng.uniform(10, 22, n), rng.uniform(22, k_max, n))
    # meant to miss: a tenth aims a scene size above the scene from no further than 2^20 sizes, a tenth points away from it
    lifted = rng.uniform(size=n) < 0.1
    tgt[lifted, 1] = hi[1] + size * rng.uniform(1.0, 2.0, n)[lifted]
    k[lifted] = rng.uniform(10, 20, n)[lifted]
    o = (tgt - u * (size * 2.0 ** k)[:, None]).astype(F)
    d = tgt - o.astype(np.float64)
    away = rng.uniform(size=n) < 0.1
    d[away] = -d[away]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= (2.0 ** rng.choice([0, 0, 0, -60, -10, 10, 30, 60], n))[:, None]
    rays = np.zeros(n, ag.RAY_DTYPE)
    rays["o"] = o
    rays["d"] = d.astype(F)
    rays["tmax"] = FLT_MAX
    return rays


SCALED_K = (-40, -20, 0, 20, 40)


def scaled(k, scale_d, leaf=1):
    """(scene, rays): grid and a fixed ray set with vertices, sphere centre and radius, plane, origins and finite tmax times 2^k;
    scale_d multiplies D by 2^k too.  Powers of two commute with every rounding as long as nothing leaves the normal range."""
    f = F(2.0 ** k)
    base = grid(leaf)
    d = ag.SceneDesc("grid-2^%d" % k)
    for op in base.ops:
        if op[0] == "material":
            d.add_material(op[1], op[2], op[3], op[4])
        elif op[0] == "mesh":
            d.add_mesh(op[1] * f, None, None, op[4], op[5], op[6])
        elif op[0] == "sphere":
            d.add_sphere(op[1] * f, float(F(op[2]) * f), op[3])
        elif op[0] == "plane":
            d.add_plane(op[1] * f, op[2] * f, op[3])
    rays = np.concatenate([aimed(base, 2000, 7), signed_zero(base, 1000, 8)])
    rays["tmax"][np.isinf(rays["tmax"])] = FLT_MAX
    rays["o"] *= f
    finite = rays["tmax"] < FLT_MAX
    rays["tmax"][finite] *= f
    if scale_d:
        rays["d"] *= f
    return d, rays


def domain_edge():
    """[(name, scene, rays)] that push a = b_box - O of the Markstein divide to the two measured limits of its domain while the
    oracle still reports hits.
      tiny-floor   a floor whose heights are m * 2^-125 with random mantissas m, under rays that start at y = 0 or at another such
                   height (|a| <= 2^-107 on the y axis: the correction term of the divide underflows) and rays from above;
      far-origin-y origins with y near 2^88 and D.y near +-2^-39 (normalisation factor exactly 1), each inside one of four spheres
                   centred at such a height, over the grid height field: the quotients of the mesh boxes overflow;
      spike        the height field with one vertex lifted to y = 2^90, under near-horizontal rays with D.y near +-2^-39 that hit
                   its ordinary triangles: the quotient of the root box's upper plane overflows on a box the ray does enter."""
    out = []
    m = 0
    # -- tiny floor
    rng = np.random.RandomState(9)
    d = ag.SceneDesc("tiny-floor")
    d.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
    v, idx = flat_quads(0.0, 2.0, 8)
    tiny = lambda n: (rng.uniform(1.0, 2.0, n).astype(F) * F(2.0 ** -125)).astype(F)
    v[:, 1] = tiny(len(v))
    d.add_mesh(v, None, None, idx, m, 1)
    d.add_sphere([0.5, 2.5, -0.25], 0.5, m)
    n = 3000
    dirs = rng.normal(size=(n, 3))
    dirs[:, 1] = np.abs(dirs[:, 1]) + 0.05
    special = np.zeros((n, 3), bool)
    special[: n // 3, 1] = True
    dirs[: n // 3, 1] = (2.0 ** -39) * rng.uniform(0.5, 4.0, n // 3)
    _fill_ordinary(rng, dirs[: n // 3], special[: n // 3])
    rays = np.zeros(n, ag.RAY_DTYPE)
    rays["o"] = rng.uniform(-1.9, 1.9, (n, 3)).astype(F)
    oy = np.where(rng.uniform(size=n) < 0.5, F(0), tiny(n))
    above = rng.uniform(size=n) < 0.25
    oy[above] = rng.uniform(0.5, 3.0, n).astype(F)[above]
    dirs[above, 1] = -dirs[above, 1]
    rays["o"][:, 1] = oy
    rays["d"] = dirs.astype(F)
    rays["tmax"] = FLT_MAX
    out.append(("tiny-floor", d, rays))
    # -- far origin on y
    rng = np.random.RandomState(10)
    d = ag.SceneDesc("far-origin-y")
    d.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
    v, idx = grid_heightfield()
    d.add_mesh(v, None, None, idx, m, 1)
    heights = [F(1.5 * 2.0 ** 86), F(1.25 * 2.0 ** 88), F(1.75 * 2.0 ** 89), F(2.0 ** 91)]
    for h in heights:
        d.add_sphere([0.0, h, 0.0], 4.0, m)
    n = 2000
    dirs = np.zeros((n, 3))
    special = np.zeros((n, 3), bool)
    special[:, 1] = True
    dirs[:, 1] = (2.0 ** -39) * rng.uniform(0.25, 4.0, n) * rng.choice([-1.0, 1.0], n)
    _fill_ordinary(rng, dirs, special)
    rays = np.zeros(n, ag.RAY_DTYPE)
    rays["o"] = rng.uniform(-1.9, 1.9, (n, 3)).astype(F)
    rays["o"][:, 1] = np.array(heights, F)[rng.randint(4, size=n)]
    rays["d"] = dirs.astype(F)
    rays["tmax"] = FLT_MAX
    out.append(("far-origin-y", d, rays))
    # -- spike
    rng = np.random.RandomState(11)
    d = ag.SceneDesc("spike")
    d.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
    v, idx = grid_heightfield()
    v[8 * 17 + 8, 1] = F(2.0 ** 90)
    d.add_mesh(v, None, None, idx, m, 1)
    n = 2000
    dirs = np.zeros((n, 3))
    special = np.zeros((n, 3), bool)
    special[:, 1] = True
    dirs[:, 1] = (2.0 ** -39) * rng.uniform(0.25, 4.0, n) * rng.choice([-1.0, 1.0], n)
    _fill_ordinary(rng, dirs, special)
    u = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    tgt = rng.uniform([-2, 0.5, -2], [2, 1.5, 2], (n, 3))
    rays = np.zeros(n, ag.RAY_DTYPE)
    rays["o"] = (tgt - rng.uniform(0.5, 6.0, n)[:, None] * u).astype(F)
    rays["d"] = dirs.astype(F)
    rays["tmax"] = FLT_MAX
    out.append(("spike", d, rays))
    return out


def oracle_scene(desc):
    return desc.instantiate(ob.OracleScene())


# class name -> builder(desc), for the scenes every class runs on
CLASSES = {"threshold": threshold, "signed_zero": signed_zero, "on_plane": on_plane, "tmax_edges": tmax_edges, "far_origin": far_origin}
SCENES = {"grid1": lambda: grid(1), "grid4": lambda: grid(4), "grid_long": grid_long}
CASE_IDS = [(c, s) for c in CLASSES for s in SCENES]
FAR16_CLASSES = ("far_origin", "signed_zero", "random")
_CACHE = {}


def case(cls, scn):
    """(scene, rays) of one class on one scene; built once per process and shared (do not modify the arrays)."""
    if (cls, scn) not in _CACHE:
        desc = far16() if scn == "far16" else SCENES[scn]()
        if cls == "random":
            from helpers import random_rays
            rays = random_rays(desc, 4000, seed=31)
        else:
            rays = CLASSES[cls](desc)
        rays.setflags(write=False)
        _CACHE[(cls, scn)] = (desc, rays)
    return _CACHE[(cls, scn)]
