"""The vote loop of the production trace kernel (k_trace_fast): every round the wave runs the one body most of
its lanes wait for -- interior step, leaf step or list step -- and that body updates the lane's cur / sp / mask (and rayt and the hit
record at a leaf) for the lanes that took part, while the others keep theirs.  The CPU oracle walks each ray alone and knows no votes:
a lane whose state a round updates wrongly, or a round that touches a lane that did not take part, shows as a hit record, an occlusion
flag, a radiance or a film that differs from the oracle's, and everything here is compared with it bit for bit.

The scene is the smallest that reaches every way out of a body: two overlapping tessellated meshes one behind the other (both
children hit with a push and a later pop, one child hit, a dead end with an empty and with a non-empty stack), a grid whose leaves
hold two triangles, stacks of nine triangles that share a box (big leaves, the side table), a sphere with a material, a plane, and an
emitter sphere between the camera and the rest (the re-cast).  The rays: 4,096 from eight origins in seeded random directions -- far
more than a wave, with early misses beside long walks, so every wave refills in flight, at the closest-hit and at the any-hit
threshold --, 64 with a zero direction component (the true-division slab test) and 64 that start inside a mesh's root box."""
import functools

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import bits, gpu_scene, oracle_render, oracle_scene, scene_bounds, signed_zero_grid
from oracle import binding as ob

pytestmark = pytest.mark.gpu
F = np.float32
DEPTH = 5
FLT_MAX = F(3.402823466e+38)
BLOB_FRONT, BLOB_BACK, GRID, STACKS, SPHERE, PLANE, EMITTER = range(7)   # list positions in scene()
FRONT, BACK = (3, (-0.2, 1.0, 0.2), 0.7), (11, (0.15, 1.1, 0.9), 0.85)   # the two blobs: (seed, centre, radius)


def corners(tris):
    t = np.asarray(tris, np.int32).reshape(-1)
    return np.stack([t, t, t], axis=1)


def blob(seed, center, radius):
    """2 * 12 * 8 = 192 triangles"""
    v, _, _, idx = ag.scenes.blob_mesh(12, 9, center=center, radius=radius, seed=seed)
    return np.ascontiguousarray(v, F), corners(idx[:, 0])


def stacks(clusters=2, copies=9, at=(-2.2, 0.4, 1.2)):
    """`clusters` stacks of `copies` triangles that share their box, hence their centroid: no split separates them, each stack is one
    leaf of nine triangles"""
    tris = []
    for c in range(clusters):
        for k in range(copies):
            quad = F([[0, 0, 0], [1, 0, 0], [0, 1, 0]] if k % 2 == 0 else [[1, 1, 0], [0, 1, 0], [1, 0, 0]])
            tris.append(quad + F([1.5 * c, 0, 0]) + F(at))
    v = np.concatenate(tris).astype(F)
    return v, corners(np.arange(len(v)).reshape(-1, 3))


def deep27():
    """28 triangles, 8^-27 to 1 across, from the origin along x in the plane z = 0 (the small ones need the coordinates near zero): a
    27-level tree, deeper than the 23 stack entries the kernels keep in LDS (the SPILL instantiations)"""
    v, tris, x = [], [], 0.0
    for i in range(28):
        w = 8.0 ** (i - 27)
        v += [[x, 0, 0], [x + w, 0, 0], [x, w, 0]]
        tris.append([3 * i, 3 * i + 1, 3 * i + 2])
        x += w * 1.5
    return np.array(v, F), corners(tris)


def scene(extra=None):
    """extra: None, "list70" (63 more primitives: 70 in all, more than the 64 of a short list) or "deep" (the 27-level mesh)"""
    d = ag.SceneDesc("vote-loop" + ("-" + extra if extra else ""))
    grey = d.add_material(ag.MAT_DISNEY, [.7, .7, .65], 0.8, 0.0)
    red = d.add_material(ag.MAT_DISNEY, [.8, .3, .25], 0.4, 0.3)
    v, idx = blob(*FRONT)
    d.add_mesh(v, None, None, idx, red, 1)
    v, idx = blob(*BACK)
    d.add_mesh(v, None, None, idx, grey, 1)
    v, idx = signed_zero_grid(4)
    d.add_mesh(v * F([2.5, 1, 2.5]) + F([0, 0.05, 0.5]), None, None, idx, grey, 4)
    v, idx = stacks()
    d.add_mesh(v, None, None, idx, red, 1)
    d.add_sphere([1.3, 0.7, 0.3], 0.5, grey)
    d.add_plane([0, -0.4, 0], [9, 9], grey)
    d.add_area_light([0.1, 1.25, -2.6], 0.3, [30., 28., 25.])
    if extra == "list70":
        rng = np.random.RandomState(70)
        for i in range(63):
            c = rng.uniform([-2.5, 0.1, -1.5], [2.5, 2.4, 2.0])
            if i % 3 == 0:
                d.add_sphere(c, float(rng.uniform(0.05, 0.2)), red)
            else:
                v, _, _, idx = ag.scenes.blob_mesh(4, 3, center=tuple(c), radius=float(rng.uniform(0.1, 0.3)), seed=i)
                d.add_mesh(np.ascontiguousarray(v, F), None, None, corners(idx[:, 0]), grey, 1)
        assert d.n_prims == 70
    if extra == "deep":
        v, idx = deep27()
        d.add_mesh(v, None, None, idx, grey, 1)
    d.add_uniform_infinite_light([.3, .35, .4])
    d.set_camera([0.2, 1.4, -5.0], [0, 1.1, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    return d


@functools.lru_cache(maxsize=None)
def query_rays():
    """the three ray sets of the module's docstring on scene(); read-only, shared by the tests"""
    d = scene()
    rng = np.random.RandomState(2024)
    lo, hi = scene_bounds(d)
    verts = np.concatenate([op[1] for op in d.ops if op[0] == "mesh"])
    # 4,096 rays from eight origins: random directions, a third of them aimed near a vertex so that walks of every length sit in one
    # wave; a quarter are short (shadow-like)
    origins = F([[0.2, 1.4, -5.0], [-3.5, 2.5, -2.0], [3.5, 0.3, -1.0], [0.0, 4.0, 0.5], [0.1, 1.0, 3.5], [-0.2, 1.0, 0.2], [2.8, 2.8, 2.8],
                 [-1.5, 0.2, 0.9]])
    n = 4096
    a = np.zeros(n, ag.RAY_DTYPE)
    a["o"] = origins[np.arange(n) % 8]
    dirs = rng.normal(size=(n, 3))
    aim = rng.uniform(size=n) < 0.35
    dirs[aim] = (verts[rng.randint(len(verts), size=n)] + rng.normal(0, 0.02, (n, 3)) - a["o"])[aim]
    a["d"] = dirs.astype(F)
    a["tmax"] = FLT_MAX
    short = rng.uniform(size=n) < 0.25
    a["tmax"][short] = rng.uniform(0.5, 6.0, n).astype(F)[short]
    # 64 rays with one direction component exactly zero, towards the meshes
    b = np.zeros(64, ag.RAY_DTYPE)
    b["o"] = rng.uniform(lo - 1.0, hi + 1.0, (64, 3)).astype(F)
    tgt = verts[rng.randint(len(verts), size=64)]
    b["d"] = (tgt - b["o"]).astype(F)
    b["d"][np.arange(64), np.arange(64) % 3] = 0.0
    b["tmax"] = FLT_MAX
    # 64 rays that start inside the root box of the front blob
    blo, bhi = blob(*FRONT)[0].min(0), blob(*FRONT)[0].max(0)
    c = np.zeros(64, ag.RAY_DTYPE)
    c["o"] = rng.uniform(blo, bhi, (64, 3)).astype(F)
    c["d"] = rng.normal(size=(64, 3)).astype(F)
    c["tmax"] = FLT_MAX
    rays = np.concatenate([a, b, c])
    assert not np.any(np.all(rays["d"] == 0, axis=1))
    rays.setflags(write=False)
    return rays


def same_hits(a, b):
    assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["tri"], b["tri"])
    m = b["hit"] == 1
    for f in ("t", "b1", "b2"):
        assert np.array_equal(bits(a[f][m]), bits(b[f][m])), f


def test_the_scene_has_what_the_tails_need():
    """(no GPU work: the trees the builder makes of the scene's meshes)"""
    nodes = ag.bvh_build(*stacks(), 1)[0]
    assert np.count_nonzero(nodes["count"] > 8) == 2          # big leaves: the side table
    v, idx = signed_zero_grid(4)
    nodes = ag.bvh_build(v * F([2.5, 1, 2.5]) + F([0, 0.05, 0.5]), idx, 4)[0]
    assert np.count_nonzero((nodes["count"] > 1) & (nodes["count"] <= 8)) > 0   # leaves of more than one triangle, counted inline
    assert ag.bvh_build(*deep27(), 1)[2] == 27
    assert 180 <= len(blob(*FRONT)[1]) // 3 <= 220   # (one index row per corner)
    lo_a, hi_a = [f(blob(*FRONT)[0], axis=0) for f in (np.min, np.max)]
    lo_b, hi_b = [f(blob(*BACK)[0], axis=0) for f in (np.min, np.max)]
    assert np.all(np.maximum(lo_a, lo_b) < np.minimum(hi_a, hi_b))   # the two blobs' boxes overlap


@pytest.mark.parametrize("extra", [None, "list70", "deep"])
def test_ray_queries(extra):
    """closest hit and any hit on the short list, on 70 primitives (LIST) and with the 27-level mesh (SPILL)"""
    d = scene(extra)
    rays = query_rays()
    o = oracle_scene(d)
    want, wantp = o.intersect(rays)[0], o.intersect(rays, any_hit=True)[0]
    g = gpu_scene(d)
    got, gotp = g.Intersect(rays)[0], g.IntersectP(rays)[0]
    g.close()
    print(extra, "rays %d, hits %d, occluded %d" % (len(rays), int(got["hit"].sum()), int(gotp["hit"].sum())))
    same_hits(got, want)
    assert np.array_equal(gotp["hit"], wantp["hit"])
    if extra is None:
        hit = got[got["hit"] == 1]
        assert {BLOB_FRONT, BLOB_BACK, GRID, STACKS, SPHERE, PLANE, EMITTER} <= set(hit["prim"].tolist())
        assert 0.2 < got["hit"].mean() < 0.9   # early misses beside long walks in every wave


@pytest.mark.parametrize("extra", [None, "list70", "deep"])
def test_li(extra):
    """agpt_li_batch: closest hits, shadow rays and the MIS queries towards the sphere light and towards the sky, re-casts included"""
    d = scene(extra)
    o = oracle_scene(d, DEPTH)
    n = 768
    rng = np.random.RandomState(5)
    rays = np.zeros(n, ag.RAY_DTYPE)
    states = np.zeros(n, np.uint32)
    for i in range(n):
        rays[i], states[i] = o.camera_ray(float(rng.uniform()), float(rng.uniform()), rng=int(rng.randint(1, 2 ** 31 - 1)))
    want = np.zeros((n, 3), F)
    after = np.zeros(n, np.uint32)
    total = 0
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        for i in range(n):
            want[i], after[i], st = o.li(rays[i], int(states[i]))
            total += st.rays
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    g = gpu_scene(d)
    got, got_after, st = ag.PathTracer(DEPTH).Li(g, rays, states)
    g.close()
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(got_after, after)
    assert st.rays == total and st.samples == n


@pytest.mark.parametrize("spp", [64, 3])
def test_films(monkeypatch, spp):
    """16 x 16 at 64 spp -- the first launch of the batch is the coherent one (COH) -- and at 3 spp, the ordinary kernel; both in the
    small-batch (PEEK) form, with camera rays that pass through the emitter (the re-cast).  Equal to the oracle's film and to the run
    with AGPT_NO_COHERENT=1."""
    d = scene()
    g = gpu_scene(d)
    pt = ag.PathTracer(DEPTH)
    a, sa = pt.render_to_host(g, 16, 16, spp)
    monkeypatch.setenv("AGPT_NO_COHERENT", "1")
    b, sb = pt.render_to_host(g, 16, 16, spp)
    monkeypatch.delenv("AGPT_NO_COHERENT")
    g.close()
    oacc, ost = oracle_render(d, 16, 16, spp, DEPTH)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(bits(a[..., :3]), bits(oacc[..., :3]))
    for s in (sa, sb):
        assert (s.closest_rays, s.anyhit_rays, s.outliers) == (ost.closest_rays, ost.anyhit_rays, ost.outliers)


def test_counting_instantiation(monkeypatch):
    """counters=2, the production kernels counting their own work (COUNT): the film and the ray totals of the plain run and of the
    oracle; a mesh's first record counts as its root test whichever record it is, so the run that enters every mesh at its root pair
    (AGPT_ROOT_STEP=1) counts the same root tests and triangle tests and no fewer record fetches.  (The oracle counts the reference's
    recursion, which visits the nodes the prefilter spares the kernel: it has no count of the kernel's fetches to compare with.)"""
    d = scene()
    g = gpu_scene(d)
    pt = ag.PathTracer(DEPTH)
    plain, sp = pt.render_to_host(g, 32, 24, 2)
    a, sa = pt.render_to_host(g, 32, 24, 2, counters=2)
    monkeypatch.setenv("AGPT_ROOT_STEP", "1")
    b, sb = pt.render_to_host(g, 32, 24, 2, counters=2)
    monkeypatch.delenv("AGPT_ROOT_STEP")
    g.close()
    oacc, ost = oracle_render(d, 32, 24, 2, DEPTH)
    print("interior %d roots %d tris %d;  root step: interior %d roots %d tris %d;  oracle: interior %d tris %d" % (
        sa.interior_visits, sa.root_tests, sa.tri_tests, sb.interior_visits, sb.root_tests, sb.tri_tests, ost.interior_visits, ost.tri_tests))
    assert plain.tobytes() == a.tobytes() == b.tobytes()
    assert np.array_equal(bits(a[..., :3]), bits(oacc[..., :3]))
    for s in (sp, sa, sb):
        assert (s.closest_rays, s.anyhit_rays, s.outliers) == (ost.closest_rays, ost.anyhit_rays, ost.outliers)
    assert sa.root_tests == sb.root_tests > 0 and sa.tri_tests == sb.tri_tests > 0
    assert 0 < sa.interior_visits + sa.root_tests <= sb.interior_visits + sb.root_tests
