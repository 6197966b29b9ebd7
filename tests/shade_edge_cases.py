"""Scenes and ray classes on the rarely-taken branches of surface and light sampling (no GPU needed to build them): the shading
counterpart of ray_edge_cases.py.

agpt_shade.h and agpt_records.h restate a dozen branches the reference takes only at degenerate geometry: a reference point inside
a sphere light (Sphere::Sample(ref) and Sphere::Pdf), the two sides of its small-cone threshold, an interpolated normal of zero
length, a shading tangent parallel to the normal, a degenerate uv mapping (CoordinateSystem(ng) instead of dpdu / dpdv), a zero-area
triangle rejected after its t test, a sphere hit on its z axis, and an environment map read along the coordinate axes.  Camera rays
of C1 enter none of them but the cone threshold (tests/test_shade_edges.py records that).  Every scene here is a
handful of primitives -- one 8 x 8 quad of two triangles at y = 0, at most one unit sphere, lights -- and every case has at most 2000
rays with one xorshift32 stream each; oracle_li_tally (oracle/agpt_oracle.h) counts how often the oracle enters each branch.
tests/test_shade_edges.py checks on the CPU that every class really contains what it is named after,
tests/test_gpu_shade_edges.py compares the kernels with the oracle on them.

`light_sample_rejected` (AreaLight::Sample_Li: the sample is the reference point) is reached from outside the light, by the
reference points of inside_light that lie within a few ulps of its surface (inside_light_rim).  Not reached: `inside_pdf_inf`, an
infinite converted pdf inside the light.  It needs normalize(pObj) of the uniform sphere sample to be exactly perpendicular to the
direction to it; no construction is known, and search_unreached() below found none among 2 * 10^6 streams (three quarters of a
minute of the oracle).  No class here claims it.
"""
import numpy as np

import ag_pathtracer_amd as ag
from oracle import binding as ob
from ray_edge_cases import normalize32

F = np.float32
FLT_MAX = F(3.402823466e+38)
TALLY = {n: i for i, n in enumerate(ob.TALLY_NAMES)}
DEPTHS = (1, 5)
SHIFT = np.array([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 0.25], [0, 0, 0, 1]], F)   # the translation of the records-rebuilt test

# the sphere lights every class without lights of its own is lit by: one near (wide cone), one far (small cone)
SPHERE_LIGHTS = (((1.5, 3.0, 0.5), 1.0, (6.0, 6.0, 6.0)), ((-2.0, 40.0, 1.0), 1.0, (900.0, 900.0, 900.0)))
# sphere_poles: the sphere's poles (0, 1, -+1) face along z; a light on the axis at either end (the pole rays start between light and
# sphere, so a mirror sends them back into it), and the far one
POLE_LIGHTS = (((0.0, 1.0, -8.0), 1.0, (6.0, 6.0, 6.0)), ((0.0, 1.0, 8.0), 1.0, (6.0, 6.0, 6.0)), SPHERE_LIGHTS[1])
LIGHT_C, LIGHT_R = np.array([0.0, 0.5, 0.0], F), F(1.0)                              # inside_light's straddling light
CONE_LIGHT_Y = 38.1   # cone_threshold: r / sqrt(0.00068523) = 38.2017 is the distance of floor points 2.79 from the axis


class Case:
    """One scene with its rays.  need = {tally counter: minimum over the case at depth 5}; meshes = the mesh primitives whose
    records the GPU test rebuilds (update_mesh / transform_mesh); cls = the class the FAST shares are pooled by."""

    def __init__(self, name, cls, desc, rays, seed, need, meshes=(0,)):
        rays["tmax"] = FLT_MAX
        rays.setflags(write=False)
        states = np.random.RandomState(seed).randint(1, 2 ** 31 - 1, len(rays)).astype(np.uint32)
        states.setflags(write=False)
        assert len(rays) <= 2000
        self.name, self.cls, self.desc, self.rays, self.states, self.need, self.meshes = name, cls, desc, rays, states, need, meshes


# ---- scenes ------------------------------------------------------------------------------------------------------------------
# The quad: v1 - v0 is dpdu under the default uvs (+x on the first triangle, -x on the second), and dpdu x dpdv points up on both
QUAD_V = np.array([[-4, 0, 4], [4, 0, 4], [4, 0, -4], [-4, 0, -4]], F)
QUAD_TRIS = np.array([[0, 1, 2], [2, 3, 0]], np.int32)


def _indices(tris, n=None, t=None):
    """(vertex, normal, texcoord) index triplets; n / t = None: index 0 (arrays of one entry, or none at all)"""
    v = np.asarray(tris, np.int32).reshape(-1)
    z = np.zeros_like(v)
    return np.stack([v, z if n is None else np.asarray(n, np.int32).reshape(-1), z if t is None else np.asarray(t, np.int32).reshape(-1)], 1)


FLOOR = (ag.MAT_DISNEY, [.7, .7, .7], 0.5, 0.0)
MATERIALS = {"black": (ag.MAT_DISNEY, [0, 0, 0], 0.5, 0.0), "rough0": (ag.MAT_DISNEY, [.7, .7, .7], 0.0, 0.0),
             "metal1": (ag.MAT_DISNEY, [.7, .7, .7], 0.5, 1.0), "metal05": (ag.MAT_DISNEY, [.7, .7, .7], 0.5, 0.5)}


def _light(desc, lights, sphere=True):
    if sphere:                                    # something for the floor's bounces to reach: paths longer than one vertex
        desc.add_sphere([2, 1, -1], 1.0, 0)
    if lights == "env":
        desc.add_infinite_area_light(ag.scenes.synthetic_hdr(16, 8))
    else:
        for c, r, L in lights:
            desc.add_area_light(c, r, L)
    return desc


def quad_scene(name, normals=None, uvs=None, indices=None, verts=QUAD_V, floor=FLOOR, lights=SPHERE_LIGHTS, sphere=True):
    d = ag.SceneDesc(name)
    d.add_material(*floor)
    d.add_mesh(verts, normals, uvs, _indices(QUAD_TRIS) if indices is None else indices, 0, 1)
    return _light(d, lights, sphere)


def sphere_scene(name, material, lights=POLE_LIGHTS):
    d = ag.SceneDesc(name)
    d.add_material(*FLOOR)
    d.add_material(*material)
    d.add_mesh(QUAD_V, None, None, _indices(QUAD_TRIS), 0, 1)
    d.add_sphere([0, 1, 0], 1.0, 1)
    return _light(d, lights, False)


def uv_threshold_values():
    """(below, above): adjacent fp32 values s with fl(s * s) on either side of the reference's (double)fabsf(det) < 1e-8; with the
    texture coordinates (0, 0) (s, 0) (s, s) the determinant is fl(s * s) - 0"""
    s = F(1e-4)
    while float(s * s) < 1e-8:
        s = np.nextafter(s, F(1))
    while float(s * s) >= 1e-8:
        s = np.nextafter(s, F(0))
    return s, np.nextafter(s, F(1))


def uv_threshold_scene(lights):
    """two meshes, one triangle of the quad each: the first with a uv determinant just below 1e-8, the second just above"""
    d = ag.SceneDesc("uv-threshold")
    d.add_material(*FLOOR)
    for tri, s in zip(QUAD_TRIS, uv_threshold_values()):
        d.add_mesh(QUAD_V, None, np.array([[0, 0], [s, 0], [s, s]], F), _indices([tri], t=[0, 1, 2]), 0, 1)
    return _light(d, lights)


TINY, TINY_Y = F(2.0 ** -40), F(2.0 ** -10)


def zero_area_scene(lights):
    """the quad plus a horizontal triangle with edges of 2^-40, 2^-10 above the floor's centre: det = e1 . (D x e2) is 2^-80 for a
    ray straight down, sqrlen(cross(e2, e1)) = 2^-160 underflows to 0 -- the hit passes every test up to t (it is nearer than the
    floor) and is then rejected"""
    v = np.concatenate([QUAD_V, np.array([[0, TINY_Y, 0], [TINY, TINY_Y, 0], [0, TINY_Y, TINY]], F)])
    tris = np.concatenate([QUAD_TRIS, [[4, 5, 6]]])
    return quad_scene("zero-area", verts=v, indices=_indices(tris), lights=lights)


def embed_long(desc):
    """desc plus small tetrahedra and spheres above the action to 70 primitives: the same rays through the candidates path and
    k_trace_fast<LIST>"""
    from ray_edge_cases import _tetra
    rng = np.random.RandomState(70)
    while desc.n_prims < 70:
        c = np.round(rng.uniform([-3.5, 4.5, -3.5], [3.5, 7.5, 3.5]) * 8) / 8
        if desc.n_prims % 4 == 0:
            desc.add_sphere(c, 0.125, 0)
        else:
            v, idx = _tetra(c, 0.125)
            desc.add_mesh(v, None, None, idx, 0, 1)
    desc.name += "-long"
    return desc


# ---- rays --------------------------------------------------------------------------------------------------------------------
def _rays(o, tgt):
    """rays from o through tgt (float64 [n, 3] each)"""
    rays = np.zeros(len(o), ag.RAY_DTYPE)
    rays["o"] = np.asarray(o, np.float64).astype(F)
    rays["d"] = (np.asarray(tgt, np.float64) - rays["o"].astype(np.float64)).astype(F)
    return rays


def _disc(rng, n, radius):
    r, a = radius * np.sqrt(rng.uniform(size=n)), rng.uniform(0, 2 * np.pi, n)
    return np.stack([r * np.cos(a), np.zeros(n), r * np.sin(a)], 1)


def floor_rays(n, seed, half=3.9, tgt=None):
    """rays from above onto the quad"""
    rng = np.random.RandomState(seed)
    if tgt is None:
        tgt = np.stack([rng.uniform(-half, half, n), np.zeros(n), rng.uniform(-half, half, n)], 1)
    o = tgt + np.stack([rng.uniform(-2, 2, n), rng.uniform(1, 4, n), rng.uniform(-2, 2, n)], 1)
    return _rays(o, tgt)


def hit_points(desc, rays):
    """(oracle hit records, p = O + t D in fp32 as ray_at computes it)"""
    oh, _ = desc.instantiate(ob.OracleScene()).intersect(rays)
    return oh, (rays["o"] + normalize32(rays["d"]) * oh["t"][:, None]).astype(F)


def sqrlen32(v):
    v = np.ascontiguousarray(v, F)
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def inside_light_scene():
    d = ag.SceneDesc("inside-light")
    d.add_material(*FLOOR)
    d.add_mesh(QUAD_V, None, None, _indices(QUAD_TRIS), 0, 1)
    d.add_area_light(LIGHT_C, float(LIGHT_R), [4, 4, 4])
    d.add_area_light([0, 400, 0], 1.0, [40000, 40000, 40000])
    return d


def inside_light_rim(desc, n_inside=250, n_outside=450, seed=22):
    """rays from inside and from outside the light to the circle where it cuts the floor, kept where the fp32 hit point lies within 4 ulps of
    |p - c|^2 == r^2: n_inside with sqrlen(p - c) <= r2 (inside, the reference's test) and n_outside beyond it.  From a point that
    close outside, the cone sample of Sphere::Sample(ref) is the point itself: on about one in seven of them it has the same bits,
    and AreaLight::Sample_Li rejects the sample (light_sample_rejected)."""
    rng = np.random.RandomState(seed)
    n = 12000
    a = rng.uniform(0, 2 * np.pi, n)
    out = np.arange(n) % 2 == 1
    rim = np.sqrt(float(LIGHT_R) ** 2 - float(LIGHT_C[1]) ** 2) + np.where(out, 1e-7, 0.0)    # (an ulp of the coordinates is 6e-8)
    tgt = np.stack([rim * np.cos(a), np.zeros(n), rim * np.sin(a)], 1)
    o = LIGHT_C.astype(np.float64) + rng.uniform(-0.3, 0.3, (n, 3))
    # (a ray from inside reaches a floor point beyond the light only after the light's own surface: the other half comes from outside)
    o[out] = (tgt * (1 + rng.uniform(0.5, 2.0, (n, 1))) + np.stack([np.zeros(n), rng.uniform(0.2, 0.7, n), np.zeros(n)], 1))[out]
    rays = _rays(o, tgt)
    rays["tmax"] = FLT_MAX
    oh, p = hit_points(desc, rays)
    sq = sqrlen32(p - LIGHT_C)
    r2 = LIGHT_R * LIGHT_R
    near = (oh["hit"] == 1) & (oh["prim"] == 0) & (np.abs(sq.astype(np.float64) - float(r2)) <= 4 * 2.0 ** -23)
    inside, outside = np.nonzero(near & (sq <= r2))[0][:n_inside], np.nonzero(near & (sq > r2))[0][:n_outside]
    assert len(inside) == n_inside and len(outside) == n_outside, (len(inside), len(outside))
    return rays[np.concatenate([inside, outside])]


def inside_light_case():
    desc = inside_light_scene()
    rng = np.random.RandomState(21)
    n = 900
    # origins inside the light and above the floor, targets on the floor inside the light
    u = rng.normal(size=(n, 3))
    o = LIGHT_C + 0.85 * u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0, 1, (n, 1)) ** (1 / 3)
    o[:, 1] = np.maximum(o[:, 1], 0.05)
    to_floor = _rays(o, _disc(rng, n, 0.8))
    # ... and rays that end on the inside of the light's own surface: the emitter seen from within, then the pass-through recast
    m = 300
    u = rng.normal(size=(m, 3))
    u[:, 1] = np.abs(u[:, 1]) + 0.2
    o = LIGHT_C + rng.uniform(-0.3, 0.3, (m, 3))
    to_shell = _rays(o, o + u)
    rays = np.concatenate([to_floor, to_shell, inside_light_rim(desc)])
    return Case("inside_light", "inside_light", desc, rays, 210, {"inside_sample": 100, "inside_pdf": 100, "light_sample_rejected": 30})


def cone_threshold_case():
    d = ag.SceneDesc("cone-threshold")
    d.add_material(*FLOOR)
    d.add_mesh(QUAD_V, None, None, _indices(QUAD_TRIS), 0, 1)
    d.add_area_light([0, CONE_LIGHT_Y, 0], 1.0, [2000, 2000, 2000])
    rng = np.random.RandomState(23)
    n = 1000
    tgt = np.stack([rng.uniform(-3.9, 3.9, n), np.zeros(n), rng.uniform(-3.9, 3.9, n)], 1)
    # half of them within a few 1e-4 of the circle where sinThetaMax2 crosses 0.00068523f
    ring = np.sqrt(1.0 / 0.00068523 - CONE_LIGHT_Y ** 2) * (1 + rng.uniform(-3e-4, 3e-4, n // 2))
    a = rng.uniform(0, 2 * np.pi, n // 2)
    tgt[: n // 2] = np.stack([ring * np.cos(a), np.zeros(n // 2), ring * np.sin(a)], 1)
    return Case("cone_threshold", "cone_threshold", d, floor_rays(n, 24, tgt=tgt), 230, {"small_cone": 100, "wide_cone": 100})


def pole_rays(seed):
    """the unit sphere at (0, 1, 0): rays along +-z through its centre (the hit has pHit.x == 0 && pHit.y == 0), interleaved with
    rays offset in x by 1e-12 ... 1e-3"""
    rng = np.random.RandomState(seed)
    n = 128
    sign = np.where(np.arange(n) % 4 < 2, 1.0, -1.0)
    o = np.stack([np.zeros(n), np.ones(n), -sign * rng.uniform(2, 6, n)], 1)
    off = 10.0 ** -rng.randint(3, 13, n) * rng.choice([-1.0, 1.0], n)
    o[1::2, 0] = off[1::2]
    rays = np.zeros(n, ag.RAY_DTYPE)
    rays["o"] = o.astype(F)
    rays["d"] = np.stack([np.zeros(n), np.zeros(n), sign], 1).astype(F)
    return rays


def axis_rays(seed):
    """from (0, 1, 0): the six axis directions with every combination of signed zeros in the other two components, ten times over
    (the streams differ), and 200 rays down onto the floor that bounce into the environment"""
    axes = []
    for a in range(3):
        for s in (1.0, -1.0):
            for z0 in (0.0, -0.0):
                for z1 in (0.0, -0.0):
                    d = [z0, z1]
                    d.insert(a, s)
                    axes.append(d)
    axes = np.array(axes * 10, F)
    rays = np.zeros(len(axes), ag.RAY_DTYPE)
    rays["o"] = [0, 1, 0]
    rays["d"] = axes
    return np.concatenate([rays, floor_rays(200, seed)])


ZERO_N = np.zeros((1, 3), F)
ALONG_DPDU = np.array([[1, 0, 0]], F)


def _build():
    cases = [inside_light_case(), cone_threshold_case()]
    cases.append(Case("zero_normals", "zero_normals", quad_scene("zero-normals", normals=ZERO_N), floor_rays(1000, 31), 310, {"ns_zero": 100}))
    cases.append(Case("normals_along_dpdu", "normals_along_dpdu", quad_scene("normals-along-dpdu", normals=ALONG_DPDU),
                      floor_rays(1000, 32), 320, {"ts_zero": 100}))
    down = np.zeros(300, ag.RAY_DTYPE)      # straight down through the tiny triangle: b1 = i / 16, b2 = j / 16 exactly
    rng = np.random.RandomState(33)
    i, j = rng.randint(0, 8, 300), rng.randint(0, 8, 300)
    down["o"] = np.stack([i / 16 * float(TINY), rng.randint(1, 64, 300) / 8.0, j / 16 * float(TINY)], 1).astype(F)   # (O - v0 is exact)
    down["d"] = [0, -1, 0]
    for tag, lights in (("", SPHERE_LIGHTS), ("/env", "env")):
        cases.append(Case("flat_uv/one_texcoord" + tag, "flat_uv", quad_scene("flat-uv", uvs=np.array([[0.3, 0.7]], F), lights=lights),
                          floor_rays(1000, 34), 340, {"degenerate_frame": 100}))
        cases.append(Case("flat_uv/uv_threshold" + tag, "flat_uv", uv_threshold_scene(lights), floor_rays(1000, 35), 350,
                          {"degenerate_frame": 30}, meshes=(0, 1)))
        cases.append(Case("flat_uv/zero_area" + tag, "flat_uv", zero_area_scene(lights), np.concatenate([down, floor_rays(500, 36)]), 360,
                          {"zero_area_reject": 100}))
    cases.append(Case("flat_uv/long", "flat_uv", embed_long(quad_scene("flat-uv", uvs=np.array([[0.3, 0.7]], F))), floor_rays(1000, 34), 340,
                      {"degenerate_frame": 100}))
    for tag, mat in (("disney", FLOOR), ("diffuse", (ag.MAT_DIFFUSE_ONLY, [.6, .6, .6], 0.5, 0.0)), ("mirror", (ag.MAT_MIRROR, [.9, .9, .9], 0.5, 0.0))):
        cases.append(Case("sphere_poles/" + tag, "sphere_poles", sphere_scene("poles-" + tag, mat), pole_rays(41), 410, {"sphere_pole": 30},
                          meshes=()))
    cases.append(Case("env_axes/disney", "env_axes", quad_scene("env-axes", lights="env", sphere=False), axis_rays(51), 510, {"shaded": 30}, meshes=()))
    cases.append(Case("env_axes/mirror", "env_axes", quad_scene("env-axes-mirror", floor=(ag.MAT_MIRROR, [.9, .9, .9], 0.5, 0.0), lights="env", sphere=False),
                      axis_rays(51), 510, {"shaded": 30}, meshes=()))
    for tag, mat in MATERIALS.items():
        cases.append(Case("materials/zero_normals/" + tag, "materials", quad_scene("zero-normals-" + tag, normals=ZERO_N, floor=mat),
                          floor_rays(1000, 31), 310, {"ns_zero": 100}))
        cases.append(Case("materials/sphere_poles/" + tag, "materials", sphere_scene("poles-" + tag, mat), pole_rays(41), 410,
                          {"sphere_pole": 30}, meshes=()))
    return {c.name: c for c in cases}


_CASES = None
_REF = {}


def cases():
    """{name: Case}, built once per process and shared (the arrays are read-only)"""
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def case_names():
    return list(cases())


def oracle_li(desc, rays, states, depth):
    """The oracle's Li on every ray in TRIG_CORRECTLY_ROUNDED, what the kernels compute: (radiance [n, 3], stream states after the
    paths, closest + any-hit rays traced, summed branch tally)"""
    o = desc.instantiate(ob.OracleScene())
    o.set_max_depth(depth)
    n = len(rays)
    want, after, total, tally = np.zeros((n, 3), F), np.zeros(n, np.uint32), 0, np.zeros(len(ob.TALLY_NAMES), np.int64)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        for i in range(n):
            want[i], after[i], st, counts = o.li(rays[i], int(states[i]), tally=True)
            total += st.rays
            tally += counts
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    return want, after, total, tally


def reference(name, depth):
    """oracle_li of a case, computed once per process and shared (do not modify the arrays)"""
    if (name, depth) not in _REF:
        c = cases()[name]
        _REF[(name, depth)] = oracle_li(c.desc, c.rays, c.states, depth)
    return _REF[(name, depth)]


def moved(case, prims=None):
    """(scene, rays) of the case with its meshes `prims` (default: case.meshes) translated by SHIFT as Scene.transform_mesh places
    them, and the ray origins moved along"""
    d = ag.SceneDesc(case.desc.name + "-moved")
    prim = 0
    for op in case.desc.ops:
        if op[0] == "mesh" and prim in (case.meshes if prims is None else prims):
            v, n = ag.transform_arrays(SHIFT, op[1], op[2])
            op = ("mesh", v, n) + op[3:]
        d.ops.append(op)
        prim += op[0] in ("mesh", "sphere", "plane", "area_light")
    d.n_prims, d.n_materials, d.n_lights = case.desc.n_prims, case.desc.n_materials, case.desc.n_lights
    rays = case.rays.copy()
    rays["o"] = rays["o"] + SHIFT[:3, 3]
    return d, rays


def search_unreached(n=2000000, seed=99):
    """Streams on the inside_light scene that enter light_sample_rejected or inside_pdf_inf (see the module docstring): the number of
    either found among n single-bounce paths from one floor point inside the light."""
    o = inside_light_scene().instantiate(ob.OracleScene())
    o.set_max_depth(1)
    ray = np.zeros(1, ag.RAY_DTYPE)
    ray["o"], ray["d"], ray["tmax"] = [0.1, 0.6, 0.2], [0.05, -1, 0.1], FLT_MAX
    found = np.zeros(2, np.int64)
    for s in np.random.RandomState(seed).randint(1, 2 ** 31 - 1, n):
        counts = o.li(ray[0], int(s), tally=True)[3]
        found += counts[[TALLY["light_sample_rejected"], TALLY["inside_pdf_inf"]]]
    return found
