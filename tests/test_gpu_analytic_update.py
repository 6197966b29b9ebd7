"""Spheres, planes and lights of a committed scene moved in place (agpt_scene_update_sphere, _plane, the two radiance calls,
agpt_scene_update_spheres_device) and their motion vectors, on the GPU: after every call the scene is, byte for byte, a scene freshly
built from a description with the new values -- renders (against the CPU oracle too), Li, ray queries, feature buffers, DbgLi --; the
emitter re-cast and the long-list kernels see the moved records; the device batch at sizes around the wave and the block, its refusals
and the host mirror; agpt_render_features_motion against tests/analytic_motion_model.py bit for bit; temporal history that follows a
moved ball; every new entry point on a caller's non-blocking stream."""
import copy
import ctypes as C

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import analytic_motion_model as am
import motion_model as mm
from helpers import bits, gpu_context, gpu_scene, oracle_render, render

pytestmark = pytest.mark.gpu
F = np.float32
CW, CH = mm.CARD_W, mm.CARD_H
PT = ag.PathTracer(5)
PRIM_OPS = ("mesh", "sphere", "plane", "area_light")
LIGHT_OPS = ("area_light", "infinite_light", "env_light")


# ---- descriptions with new values -----------------------------------------------------------------------------------------------
def op_of(desc, kinds, k):
    return [i for i, op in enumerate(desc.ops) if op[0] in kinds][k]


def with_sphere(desc, prim, center, radius):
    d = copy.deepcopy(desc)
    i = op_of(d, PRIM_OPS, prim)
    op = d.ops[i]
    assert op[0] in ("sphere", "area_light")
    d.ops[i] = (op[0], np.asarray(center, F).copy(), float(radius), op[3])
    return d


def with_plane(desc, prim, o, size):
    d = copy.deepcopy(desc)
    i = op_of(d, PRIM_OPS, prim)
    assert d.ops[i][0] == "plane"
    d.ops[i] = ("plane", np.asarray(o, F).copy(), np.asarray(size, F).copy(), d.ops[i][3])
    return d


def with_area_radiance(desc, prim, L):
    d = copy.deepcopy(desc)
    i = op_of(d, PRIM_OPS, prim)
    op = d.ops[i]
    assert op[0] == "area_light"
    d.ops[i] = (op[0], op[1], op[2], np.asarray(L, F).copy())
    return d


def with_infinite_radiance(desc, light, L):
    d = copy.deepcopy(desc)
    i = op_of(d, LIGHT_OPS, light)
    assert d.ops[i][0] == "infinite_light"
    d.ops[i] = ("infinite_light", np.asarray(L, F).copy())
    return d


def three_spheres():
    """a plane, a Disney sphere, a mirror sphere, a diffuse sphere, one area light and a uniform sky: no triangle anywhere"""
    d = ag.SceneDesc("three-spheres")
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.6, 0.6, 0.6))
    dis = d.add_material(ag.MAT_DISNEY, (0.8, 0.3, 0.2), 0.4, 0.2)
    mir = d.add_material(ag.MAT_MIRROR, (0.9, 0.9, 0.9))
    d.add_plane((0.0, 0.0, 0.0), (8.0, 8.0), grey)           # primitive 0
    d.add_sphere((-0.9, 0.5, 0.2), 0.5, dis)                 # 1
    d.add_sphere((0.9, 0.6, 0.4), 0.6, mir)                  # 2
    d.add_sphere((0.1, 0.3, -1.0), 0.3, grey)                # 3
    d.add_area_light((0.5, 2.4, -0.5), 0.4, (30.0, 28.0, 25.0))   # 4, light 0
    d.add_uniform_infinite_light((0.3, 0.35, 0.4))           # light 1
    d.set_camera(*mm.CARD_CAMERA)
    return d


def aimed_rays(desc, n, seed):
    """rays from around the camera side of the scene, most aimed near a primitive's centre, a third of them short"""
    rng = np.random.RandomState(seed)
    centres = np.array([op[1] if op[0] != "mesh" else op[1].mean(0) for op in desc.ops if op[0] in PRIM_OPS], np.float64)
    rays = np.zeros(n, ag.RAY_DTYPE)
    o = rng.uniform(-3, 3, (n, 3)) + np.array([0.0, 1.5, -2.0])
    d = centres[rng.randint(len(centres), size=n)] + rng.normal(0, 0.25, (n, 3)) - o
    wild = rng.uniform(size=n) < 0.2
    d[wild] = rng.normal(size=(int(wild.sum()), 3))
    rays["o"], rays["d"] = o.astype(F), d.astype(F)
    t = np.full(n, mm.FLT_MAX, F)
    short = rng.uniform(size=n) < 0.3
    t[short] = rng.uniform(0.5, 4.0, n).astype(F)[short]
    rays["tmax"] = t
    return rays


def totals(st):
    return (st.rays, st.closest_rays, st.anyhit_rays)


def assert_same_scene(g, desc, W, H, spp, what, oracle=True, seed=5):
    """g is, for every reader, a scene freshly built from desc"""
    f = gpu_scene(desc)
    try:
        for arith in ("exact", "fast"):
            a, sa = render(g, W, H, spp, arith=arith)
            b, sb = render(f, W, H, spp, arith=arith)
            assert a.tobytes() == b.tobytes() and totals(sa) == totals(sb), (what, arith)
            if arith == "exact" and oracle:
                oacc, ost = oracle_render(desc, W, H, spp)
                assert np.array_equal(bits(a[..., :3]), bits(oacc[..., :3])), what
                assert totals(sa) == (ost.rays, ost.closest_rays, ost.anyhit_rays), what
        g.set_shading_arith("exact")
        f.set_shading_arith("exact")
        rays = aimed_rays(desc, 3000, seed)
        states = (np.arange(len(rays), dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)) | np.uint32(1)
        la, ra, _ = PT.Li(g, rays, states)
        lb, rb, _ = PT.Li(f, rays, states)
        assert la.tobytes() == lb.tobytes() and ra.tobytes() == rb.tobytes(), what
        ha, hb = g.Intersect(rays)[0], f.Intersect(rays)[0]
        assert ha.tobytes() == hb.tobytes() and ha["hit"].sum() > 500, what
        assert g.IntersectP(rays)[0].tobytes() == f.IntersectP(rays)[0].tobytes(), what
        for x, y in zip(PT.render_features_to_host(g, W, H), PT.render_features_to_host(f, W, H)):
            assert x.tobytes() == y.tobytes(), what
        assert PT.DbgLi(g, rays).tobytes() == PT.DbgLi(f, rays).tobytes(), what
    finally:
        f.close()


# ---- 1. parity after every call -----------------------------------------------------------------------------------------------------
def test_card_scene_is_a_fresh_scene_after_every_call():
    desc = mm.card_scene()
    g = gpu_scene(desc)
    try:
        before, _ = render(g, CW, CH, 2)
        g.update_sphere(2, (0.9, 1.7, -0.4), 0.45)                 # the light: nearer, larger
        desc = with_sphere(desc, 2, (0.9, 1.7, -0.4), 0.45)
        assert_same_scene(g, desc, CW, CH, 2, "update_sphere")
        assert render(g, CW, CH, 2)[0].tobytes() != before.tobytes()
        g.set_area_light_radiance(2, (5.0, 12.0, 0.0))
        desc = with_area_radiance(desc, 2, (5.0, 12.0, 0.0))
        assert_same_scene(g, desc, CW, CH, 2, "set_area_light_radiance")
    finally:
        g.close()


def test_three_sphere_scene_is_a_fresh_scene_after_every_call():
    desc = three_spheres()
    g = gpu_scene(desc)
    try:
        g.update_sphere(1, (-0.7, 0.65, -0.3), 0.65)               # the Disney sphere
        desc = with_sphere(desc, 1, (-0.7, 0.65, -0.3), 0.65)
        assert_same_scene(g, desc, CW, CH, 2, "update_sphere")
        g.update_plane(0, (0.5, -0.1, 0.25), (5.0, 9.0))
        desc = with_plane(desc, 0, (0.5, -0.1, 0.25), (5.0, 9.0))
        assert_same_scene(g, desc, CW, CH, 2, "update_plane")
        g.set_area_light_radiance(4, (0.0, 45.0, -2.0))            # zero and negative are values like any other
        desc = with_area_radiance(desc, 4, (0.0, 45.0, -2.0))
        assert_same_scene(g, desc, CW, CH, 2, "set_area_light_radiance")
        g.set_infinite_light_radiance(1, (0.9, 0.1, 0.05))
        desc = with_infinite_radiance(desc, 1, (0.9, 0.1, 0.05))
        assert_same_scene(g, desc, CW, CH, 2, "set_infinite_light_radiance")
        g.update_sphere(2, (1.1, 0.4, 0.0), 0.4)                   # the mirror sphere, and the light's own sphere
        g.update_sphere(4, (-0.5, 2.0, -1.0), 0.25)
        desc = with_sphere(with_sphere(desc, 2, (1.1, 0.4, 0.0), 0.4), 4, (-0.5, 2.0, -1.0), 0.25)
        assert_same_scene(g, desc, CW, CH, 2, "two spheres")
    finally:
        g.close()


def refused(fn, *args, word=None):
    with pytest.raises(ag.AgptError):
        fn(*args)
    if word is not None:
        assert word in ag.lib().agpt_last_error(), ag.lib().agpt_last_error()


def test_refusals_leave_the_scene_alone():
    desc = three_spheres()
    g = gpu_scene(desc)
    h = ag.Scene(gpu_context())
    try:
        before, _ = render(g, 32, 24, 2)
        nan, inf = float("nan"), float("inf")
        for c, r in (((nan, 0, 0), 0.5), ((0, inf, 0), 0.5), ((0, 0, 0), nan), ((0, 0, 0), inf), ((0, 0, 0), 0.0), ((0, 0, 0), -1.0)):
            refused(g.update_sphere, 1, c, r, word=b"finite")
        for prim in (-1, 0, 5, 99):                                 # out of range, a plane
            refused(g.update_sphere, prim, (0, 0, 0), 0.5, word=b"not a sphere")
        for o, size in (((nan, 0, 0), (1, 1)), ((0, 0, 0), (inf, 1)), ((0, 0, 0), (1, nan)), ((0, 0, 0), (0.0, 1)), ((0, 0, 0), (1, -2.0))):
            refused(g.update_plane, 0, o, size)
        for prim in (-1, 1, 4, 5):
            refused(g.update_plane, prim, (0, 0, 0), (1, 1), word=b"not a plane")
        refused(g.set_area_light_radiance, 1, (1, 1, 1), word=b"no area light")
        refused(g.set_area_light_radiance, 0, (1, 1, 1), word=b"not a sphere")
        refused(g.set_area_light_radiance, 4, (1, nan, 1), word=b"finite")
        refused(g.set_infinite_light_radiance, 0, (1, 1, 1), word=b"not a uniform infinite light")   # the area light
        refused(g.set_infinite_light_radiance, 2, (1, 1, 1), word=b"not a uniform infinite light")
        refused(g.set_infinite_light_radiance, 1, (inf, 1, 1), word=b"finite")
        assert render(g, 32, 24, 2)[0].tobytes() == before.tobytes()
        # a scene that is not committed
        desc.instantiate(h)
        h.add_sphere((0, 5, 0), 0.1, 0)
        for fn, args in ((h.update_sphere, (1, (0, 0, 0), 0.5)), (h.update_plane, (0, (0, 0, 0), (1, 1))), (h.set_area_light_radiance, (4, (1, 1, 1))),
                         (h.set_infinite_light_radiance, (1, (1, 1, 1))), (h.update_spheres, ([1], np.ones((1, 4), F)))):
            refused(fn, *args, word=b"not committed")
    finally:
        g.close()
        h.close()


# ---- 2. absolute, not cumulative ---------------------------------------------------------------------------------------------------
def test_two_updates_in_a_row_and_back_again():
    desc = three_spheres()
    g = gpu_scene(desc)
    try:
        untouched, st0 = render(g, CW, CH, 2)
        g.update_sphere(3, (0.4, 0.9, -1.2), 0.2)
        g.update_sphere(3, (-0.3, 0.5, -0.8), 0.5)
        g.update_plane(0, (0, 0.1, 0), (3, 3))
        g.set_area_light_radiance(4, (1, 2, 3))
        g.set_infinite_light_radiance(1, (0, 0, 0))
        moved = with_infinite_radiance(with_area_radiance(with_plane(with_sphere(desc, 3, (-0.3, 0.5, -0.8), 0.5), 0, (0, 0.1, 0), (3, 3)), 4, (1, 2, 3)),
                                       1, (0, 0, 0))
        assert_same_scene(g, moved, CW, CH, 2, "the last values only", oracle=False)
        g.update_sphere(3, (0.1, 0.3, -1.0), 0.3)
        g.update_plane(0, (0.0, 0.0, 0.0), (8.0, 8.0))
        g.set_area_light_radiance(4, (30.0, 28.0, 25.0))
        g.set_infinite_light_radiance(1, (0.3, 0.35, 0.4))
        again, st1 = render(g, CW, CH, 2)
        assert again.tobytes() == untouched.tobytes() and totals(st0) == totals(st1)
    finally:
        g.close()


# ---- 3. emitter paths ----------------------------------------------------------------------------------------------------------------
EMITTERS = (([1.6, -0.2, 0.4], 0.7), ([2.2, -0.1, 0.9], 0.6), ([-1.8, -0.3, 0.8], 0.6), ([0.2, -0.4, -1.9], 0.5), ([0.0, 1.9, 0.3], 0.5),
            ([-0.6, -0.5, 2.4], 0.45))


def emitter_gauntlet():
    """C1's geometry with six emitter spheres hovering around the gold sphere, two of them overlapping (test_gpu_render.py)"""
    d = ag.scenes.scene_c1()
    d.name = "emitter-gauntlet-moved"
    first = d.n_prims
    for c, r in EMITTERS:
        d.add_area_light(c, r, ag.scenes.KEY_LIGHT * np.float32(3))
    return d, first


def test_moved_emitters_in_the_recast_and_the_mis_queries():
    desc, first = emitter_gauntlet()
    g = gpu_scene(desc)
    W, H, spp = 80, 60, 4
    try:
        g.update_sphere(first + 1, (1.9, 0.1, 0.2), 0.75)           # now overlaps the first emitter more, and the gold sphere's side
        g.update_sphere(first + 4, (-0.4, 1.4, -0.6), 0.35)
        moved = with_sphere(with_sphere(desc, first + 1, (1.9, 0.1, 0.2), 0.75), first + 4, (-0.4, 1.4, -0.6), 0.35)
        a, sa = render(g, W, H, spp)
        f = gpu_scene(moved)
        b, sb = render(f, W, H, spp)
        f.close()
        oacc, ost = oracle_render(moved, W, H, spp)
        assert np.array_equal(bits(a[..., :3]), bits(oacc[..., :3]))
        assert totals(sa) == (ost.rays, ost.closest_rays, ost.anyhit_rays)
        assert a.tobytes() == b.tobytes() and sa.iterations == sb.iterations and totals(sa) == totals(sb)
    finally:
        g.close()


# ---- 4. long lists ---------------------------------------------------------------------------------------------------------------------
def seventy():
    """70 primitives: small meshes with a sphere at every fifth place, the last one a light, before a sky"""
    d = ag.SceneDesc("analytic-70")
    mats = [d.add_material(ag.MAT_DIFFUSE_ONLY, c) for c in ([.8, .3, .2], [.2, .7, .3], [.3, .4, .8])]
    for k in range(69):
        c = (1.4 * (k % 10) - 6.3, 0.9 * ((k // 10) % 7) - 2.0, 1.1 * (k % 3))
        if k % 5 == 2:
            d.add_sphere(c, 0.4, mats[k % 3])
        else:
            d.add_mesh(*ag.scenes.blob_mesh(5, 4, center=c, radius=0.45, seed=k), mats[k % 3], 1)
    d.add_area_light([0.0, 8.0, -4.0], 0.8, [70, 65, 60])         # primitive 69: in the second chunk
    d.add_uniform_infinite_light([.25, .3, .35])
    d.set_camera([0, 1, -16], [0, 0.5, 0], [0, 1, 0], 4 / 3.0, 50.0, 0.0)
    assert d.n_prims == 70
    return d


SEVENTY_MOVES = ((2, (-3.0, 1.0, -2.0), 0.9), (67, (2.5, -1.0, -1.5), 0.7), (69, (1.0, 6.0, -5.0), 1.1))


def moved_seventy(desc):
    for prim, c, r in SEVENTY_MOVES:
        desc = with_sphere(desc, prim, c, r)
    return desc


def test_seventy_primitives_through_the_candidate_list():
    desc = seventy()
    g = gpu_scene(desc)
    try:
        for prim, c, r in SEVENTY_MOVES:
            g.update_sphere(prim, c, r)
        assert_same_scene(g, moved_seventy(desc), 32, 24, 2, "70 primitives")
    finally:
        g.close()


def test_seventy_primitives_on_the_generic_kernel(monkeypatch):
    desc = seventy()
    moved = moved_seventy(desc)
    monkeypatch.setenv("AGPT_FORCE_GENERIC", "1")
    ctx = ag.Context(0)
    monkeypatch.delenv("AGPT_FORCE_GENERIC")
    g = desc.instantiate(ag.Scene(ctx))
    try:
        for prim, c, r in SEVENTY_MOVES:
            g.update_sphere(prim, c, r)
        a, sa = render(g, 32, 24, 2)
        oacc, ost = oracle_render(moved, 32, 24, 2)
        assert np.array_equal(bits(a[..., :3]), bits(oacc[..., :3])) and sa.rays == ost.rays
        rays = aimed_rays(moved, 3000, 9)
        f = gpu_scene(moved)
        want = f.Intersect(rays)[0]
        f.close()
        assert g.Intersect(rays)[0].tobytes() == want.tobytes()
    finally:
        g.close()
        ctx.close()


# ---- 5. the device batch ---------------------------------------------------------------------------------------------------------------
N_SPHERES = 300


def many_spheres():
    """a floor mesh (primitive 0), a plane (1), 300 spheres on a 20 x 15 grid (2 .. 301), the last ten of them lights"""
    d = ag.SceneDesc("analytic-300")
    mats = [d.add_material(ag.MAT_DIFFUSE_ONLY, c) for c in ([.8, .3, .2], [.2, .7, .3], [.3, .4, .8])]
    d.add_mesh(mm.FLOOR[0], None, None, mm.FLOOR[1], mats[0])
    d.add_plane((0.0, 6.0, 0.0), (2.0, 2.0), mats[1])
    for k in range(N_SPHERES):
        c = (0.5 * (k % 20) - 4.75, 0.5 * (k // 20) + 0.3, 0.2 * (k % 3))
        if k >= N_SPHERES - 10:
            d.add_area_light(c, 0.15, (20.0, 20.0, 20.0))
        else:
            d.add_sphere(c, 0.2, mats[k % 3])
    d.add_uniform_infinite_light([.25, .3, .35])
    d.set_camera([0, 4, -14], [0, 4, 0], [0, 1, 0], 4 / 3.0, 45.0, 0.0)
    assert d.n_prims == N_SPHERES + 2
    return d


def batch(n, order, seed):
    """(ids[n], records[n, 4]): n distinct spheres in `order`, each moved within its grid cell and resized"""
    rng = np.random.RandomState(seed)
    k = np.sort(rng.choice(N_SPHERES, n, replace=False))
    k = k[::-1].copy() if order == "descending" else rng.permutation(k)
    rec = np.zeros((n, 4), F)
    rec[:, 0] = 0.5 * (k % 20) - 4.75 + rng.uniform(-0.1, 0.1, n)
    rec[:, 1] = 0.5 * (k // 20) + 0.3 + rng.uniform(-0.1, 0.1, n)
    rec[:, 2] = -0.5 + rng.uniform(-0.1, 0.1, n)
    rec[:, 3] = rng.uniform(0.1, 0.24, n)
    return (k + 2).astype(np.int32), rec


def with_batch(desc, ids, rec):
    d = copy.deepcopy(desc)
    for prim, r in zip(ids, rec):
        i = op_of(d, PRIM_OPS, int(prim))
        op = d.ops[i]
        d.ops[i] = (op[0], r[:3].copy(), float(r[3]), op[3])
    return d


def centre_rays(desc):
    """one ray through every sphere's centre, from the camera side"""
    c = np.array([op[1] for op in desc.ops if op[0] in ("sphere", "area_light")], F)
    rays = np.zeros(len(c), ag.RAY_DTYPE)
    rays["o"] = c + np.array([0.01, 0.02, -6.0], F)
    rays["d"] = c - rays["o"]
    rays["tmax"] = mm.FLT_MAX
    return rays


@pytest.mark.parametrize("n,order", [(1, "descending"), (64, "shuffled"), (65, "descending"), (257, "shuffled")])
def test_device_batch_is_a_fresh_scene(n, order):
    desc = many_spheres()
    ids, rec = batch(n, order, 100 + n)
    moved = with_batch(desc, ids, rec)
    g, f = gpu_scene(desc), gpu_scene(moved)
    try:
        g.update_spheres(ids, rec)
        rays = centre_rays(moved)
        got, want = g.Intersect(rays)[0], f.Intersect(rays)[0]
        assert got.tobytes() == want.tobytes() and want["hit"].all()
        assert np.isin(ids, want["prim"]).all()                     # every moved sphere is the closest hit of some ray
        a, sa = render(g, 32, 24, 2)
        b, sb = render(f, 32, 24, 2)
        assert a.tobytes() == b.tobytes() and totals(sa) == totals(sb)
        # the mirror is synchronised before DbgLi reads it ...
        assert PT.DbgLi(g, rays).tobytes() == PT.DbgLi(f, rays).tobytes()
        # ... and before a REBUILD's commit flattens the scene again: the moved spheres stay
        g.update_mesh(0, mm.FLOOR[0] - F(0.25), None, "rebuild")
        f.update_mesh(0, mm.FLOOR[0] - F(0.25), None, "rebuild")
        got = g.Intersect(rays)[0]
        assert got.tobytes() == f.Intersect(rays)[0].tobytes()
        assert got.tobytes() == want.tobytes()                      # (the lowered floor is behind every sphere)
        assert render(g, 32, 24, 2)[0].tobytes() == render(f, 32, 24, 2)[0].tobytes()
    finally:
        g.close()
        f.close()


TORCH_CHILD = """
import contextlib
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch                      # before the library touches the GPU (INTEGRATION.md section 3)
import numpy as np
torch.zeros(1, device="cuda")
import ag_pathtracer_amd as ag
import test_gpu_analytic_update as t

ag.lib()
with open("/proc/self/maps") as f:
    runtimes = sorted({ln.split(None, 5)[5].strip() for ln in f if "libamdhip64" in ln and len(ln.split(None, 5)) == 6})
assert len(runtimes) == 1, "torch and libagpt_hip.so are bound to different HIP runtime copies: a torch stream is no handle for the library"

desc = t.many_spheres()
for own_stream, n, order in ((False, 64, "descending"), (True, 65, "shuffled")):
    # own_stream: the context runs on a stream of torch's pool and the tensor is produced on it (no wait in between)
    s = torch.cuda.Stream() if own_stream else None
    ctx = ag.Context(0, stream=s.cuda_stream if own_stream else None)
    with (torch.cuda.stream(s) if own_stream else contextlib.nullcontext()):
        ids, rec = t.batch(n, order, 300 + n)
        moved = t.with_batch(desc, ids, rec)
        a, b = moved.instantiate(ag.Scene(ctx)), desc.instantiate(ag.Scene(ctx))
        tr = torch.from_numpy(rec).cuda() * 1.0          # produced on torch's current stream
        b.update_spheres(ids, tr)
        tr.fill_(1.0)                                    # the call has read the records before it returns
        rays = t.centre_rays(moved)
        want = a.Intersect(rays)[0]
        assert b.Intersect(rays)[0].tobytes() == want.tobytes() and want["hit"].all() and np.isin(ids, want["prim"]).all()
        assert t.render(a, 32, 24, 2)[0].tobytes() == t.render(b, 32, 24, 2)[0].tobytes()
        assert t.PT.DbgLi(a, rays).tobytes() == t.PT.DbgLi(b, rays).tobytes()
        bad = [tr.double(), tr.reshape(-1), tr.t().contiguous(), torch.cat([tr, tr], 1)[:, :4], tr[:-1]]
        for x in bad:
            try:
                b.update_spheres(ids, x)
            except ValueError:
                pass
            else:
                raise AssertionError("accepted %%s %%s" %% (x.dtype, tuple(x.shape)))
        b.update_spheres(ids, torch.from_numpy(rec))       # a CPU tensor: uploaded by the binding
        assert b.Intersect(rays)[0].tobytes() == want.tobytes()
        torch.cuda.current_stream().synchronize()
        a.close(); b.close(); ctx.close()
print("torch-ok")
"""


def test_device_batch_from_torch_tensors():
    """Scene.update_spheres with a torch tensor on the GPU (its data_ptr() handed to agpt_scene_update_spheres_device), at n = 64 and 65, in a
    child process as in test_gpu_mesh_update_device.py: torch must initialise the GPU before the library does."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = TORCH_CHILD % {"root": root, "tests": os.path.join(root, "tests")}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "torch-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_batch_refusals_write_nothing():
    desc = many_spheres()
    g = gpu_scene(desc)
    ctx = gpu_context()
    try:
        before, _ = render(g, 32, 24, 2)
        rays = centre_rays(desc)
        hits = g.Intersect(rays)[0].tobytes()
        ids, rec = batch(65, "shuffled", 7)
        twice = ids.copy()
        twice[-1] = twice[3]
        refused(g.update_spheres, twice, rec, word=b"twice")
        for bad, word in ((0, b"not a sphere"), (1, b"not a sphere"), (-1, b"not a sphere"), (N_SPHERES + 2, b"not a sphere")):   # a mesh, a plane, out of range
            other = ids.copy()
            other[40] = bad
            refused(g.update_spheres, other, rec, word=word)
        ptr = ctx.alloc(rec.nbytes + 16)
        try:
            ctx.upload(ptr, rec)
            refused(g.update_spheres_device, ids, ptr + 4, word=b"aligned")
            L = ag.lib()
            pi = ids.ctypes.data_as(C.POINTER(C.c_int32))
            assert L.agpt_scene_update_spheres_device(g.h, pi, -1, ptr) == -1
            assert L.agpt_scene_update_spheres_device(g.h, pi, 0, ptr) == 0       # n == 0: nothing to do
            assert L.agpt_scene_update_spheres_device(g.h, None, 1, ptr) == -1 and L.agpt_scene_update_spheres_device(g.h, pi, 1, None) == -1
        finally:
            ctx.free(ptr)
        # records the check kernel refuses: nothing is written, whichever lane held the bad one
        for lane, column, value in ((0, 1, np.nan), (64, 3, 0.0), (31, 3, -1.0), (17, 0, np.inf), (63, 3, np.nan)):
            poisoned = rec.copy()
            poisoned[lane, column] = value
            refused(g.update_spheres, ids, poisoned, word=b"non-finite")
            assert g.Intersect(rays)[0].tobytes() == hits
        assert render(g, 32, 24, 2)[0].tobytes() == before.tobytes()
        g.update_spheres(ids, rec)                                   # the same batch without the bad record goes through
        assert g.Intersect(rays)[0].tobytes() != hits
    finally:
        g.close()


# ---- 6. motion vectors -----------------------------------------------------------------------------------------------------------------
MOTION_BASES = {1: 0}      # the card is the only mesh


def motion_scene():
    """a floor PLANE (0), the card (1), a diffuse sphere (2), the sphere light (3), seen by the card scene's camera"""
    d = ag.SceneDesc("analytic-motion")
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.6, 0.6, 0.6))
    red = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.7, 0.2, 0.15))
    d.add_plane((0.0, 0.0, 0.0), (10.0, 10.0), grey)
    v, ix = mm.card_mesh()
    d.add_mesh(v, None, None, ix, red)
    d.add_sphere((-1.1, 0.6, 0.4), 0.5, grey)
    d.add_area_light(mm.LIGHT[0], mm.LIGHT[1], (40.0, 40.0, 40.0))
    d.set_camera(*mm.CARD_CAMERA)
    return d


def model_prev_point(g, cam, W, H, meshes, bases, desc_old, desc_new):
    O, once, D = mm.feature_rays(ag.camera_vectors(cam), W, H)
    rays = np.zeros(W * H, ag.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"] = O, once, mm.FLT_MAX
    hits, _ = g.Intersect(rays)
    rec, prim = am.hit_records(hits, bases)
    (ro, kinds), (rn, _) = am.records(desc_old), am.records(desc_new)
    gen = mm.generation(meshes)
    pp = am.prev_points(rec, prim, O, D, gen, gen, ro, rn, kinds)
    plain = mm.prev_points(rec, O, D, gen, gen)
    return pp.reshape(H, W, 4), plain.reshape(H, W, 4), hits.reshape(H, W)


def check_motion(g, cam, W, H, meshes, bases, desc_old, desc_new, moved_prims):
    """render_features_motion == the model on the full film and on a tile with a pitch; w == 1 exactly on the moved primitives"""
    albedo, nd = PT.render_features_to_host(g, W, H)
    a2, n2, pp = PT.render_features_motion_to_host(g, W, H)
    assert a2.tobytes() == albedo.tobytes() and n2.tobytes() == nd.tobytes()
    model, plain, hits = model_prev_point(g, cam, W, H, meshes, bases, desc_old, desc_new)
    differ = (bits(pp) != bits(model)).any(-1)
    assert not differ.any(), np.argwhere(differ)[:8]
    on_moved = (hits["hit"] == 1) & np.isin(hits["prim"], list(moved_prims))
    assert np.array_equal(pp[..., 3] == 1, on_moved)
    assert set(np.unique(pp[..., 3])) <= {0.0, 1.0, 2.0}
    if not moved_prims:
        assert pp.tobytes() == plain.tobytes()
    else:
        assert on_moved.sum() >= 20 and (pp[on_moved, :3] != plain[on_moved, :3]).any()
    ctx = g.ctx
    x0, y0, w, h = 5, 3, W - 11, H - 9
    pitch, row0 = W + 3, H - y0 - h
    sentinel = np.full((h, pitch, 4), -7.0, F)
    ptrs = [ctx.alloc(sentinel.nbytes) for _ in range(3)]
    try:
        for p in ptrs:
            ctx.upload(p, sentinel)
        PT.render_features_motion(g, W, H, *ptrs, tile=(x0, y0, w, h), accum_pitch=pitch, accum_row0=row0)
        got = [ctx.download(p, (h, pitch, 4)) for p in ptrs]
    finally:
        for p in ptrs:
            ctx.free(p)
    rows = slice(H - y0 - h, H - y0)
    outside = np.ones((h, pitch), bool)
    outside[:, x0:x0 + w] = False
    for t, full in zip(got, (albedo, nd, pp)):
        assert t[:, x0:x0 + w].tobytes() == full[rows, x0:x0 + w].tobytes()
        assert (t[outside] == -7.0).all()
    return pp, hits


MOTION_CASES = {
    "sphere translated": (lambda g: g.update_sphere(2, (-0.8, 0.75, 0.1), 0.5), lambda d: with_sphere(d, 2, (-0.8, 0.75, 0.1), 0.5), [2]),
    "sphere scaled": (lambda g: g.update_sphere(2, (-1.1, 0.6, 0.4), 0.7), lambda d: with_sphere(d, 2, (-1.1, 0.6, 0.4), 0.7), [2]),
    "plane moved and resized": (lambda g: g.update_plane(0, (0.4, 0.1, -0.3), (8.0, 12.0)), lambda d: with_plane(d, 0, (0.4, 0.1, -0.3), (8.0, 12.0)),
                                [0]),
    "light moved": (lambda g: g.update_sphere(3, (1.3, 1.8, 0.6), 0.3), lambda d: with_sphere(d, 3, (1.3, 1.8, 0.6), 0.3), [3]),
    "light moved by the batch call": (lambda g: g.update_spheres([3, 2], np.array([[1.3, 1.8, 0.6, 0.35], [-1.0, 0.6, 0.4, 0.5]], F)),
                                      lambda d: with_sphere(with_sphere(d, 3, (1.3, 1.8, 0.6), 0.35), 2, (-1.0, 0.6, 0.4), 0.5), [2, 3]),
    "radiance only": (lambda g: g.set_area_light_radiance(3, (1.0, 2.0, 3.0)), lambda d: with_area_radiance(d, 3, (1.0, 2.0, 3.0)), []),
    "nothing": (lambda g: None, lambda d: d, []),
}


@pytest.mark.parametrize("case", list(MOTION_CASES))
def test_motion_vectors_of_moved_analytic_primitives(case):
    update, describe, moved_prims = MOTION_CASES[case]
    desc = motion_scene()
    g = gpu_scene(desc)
    try:
        g.snapshot_positions()
        update(g)
        g.snapshot_positions()
        pp, hits = check_motion(g, mm.CARD_CAMERA, CW, CH, [mm.card_mesh()], MOTION_BASES, desc, describe(desc), moved_prims)
        on_card = (hits["hit"] == 1) & (hits["prim"] == 1)
        assert (pp[on_card, 3] == 2).all() and on_card.sum() >= 100 and (pp[..., 3] == 0).any()     # mesh hits and misses: as before
        # a third snapshot: nothing moved between the last two
        g.snapshot_positions()
        check_motion(g, mm.CARD_CAMERA, CW, CH, [mm.card_mesh()], MOTION_BASES, describe(desc), describe(desc), [])
    finally:
        g.close()


def test_snapshot_rules_of_the_analytic_generations():
    # a scene without triangles
    desc = three_spheres()
    g = gpu_scene(desc)
    try:
        g.snapshot_positions()
        check_motion(g, mm.CARD_CAMERA, CW, CH, [], {}, desc, desc, [])           # the first call fills both generations
        g.update_sphere(1, (-0.7, 0.65, -0.3), 0.65)
        g.update_plane(0, (0.0, 0.0, 0.5), (8.0, 6.0))
        g.snapshot_positions()
        moved = with_plane(with_sphere(desc, 1, (-0.7, 0.65, -0.3), 0.65), 0, (0.0, 0.0, 0.5), (8.0, 6.0))
        check_motion(g, mm.CARD_CAMERA, CW, CH, [], {}, desc, moved, [0, 1])
        g.commit()                                                                # drops both generations
        with pytest.raises(ag.AgptError, match="snapshot"):
            PT.render_features_motion_to_host(g, CW, CH)
        g.snapshot_positions()
        check_motion(g, mm.CARD_CAMERA, CW, CH, [], {}, moved, moved, [])
    finally:
        g.close()
    # a REBUILD between the snapshots and the feature pass keeps them
    desc = motion_scene()
    g = gpu_scene(desc)
    try:
        g.snapshot_positions()
        g.update_sphere(2, (-0.8, 0.75, 0.1), 0.5)
        g.snapshot_positions()
        g.update_mesh(1, mm.card_mesh()[0], None, "rebuild")
        check_motion(g, mm.CARD_CAMERA, CW, CH, [mm.card_mesh()], MOTION_BASES, desc, with_sphere(desc, 2, (-0.8, 0.75, 0.1), 0.5), [2])
    finally:
        g.close()


# ---- 7. history follows a moved ball ---------------------------------------------------------------------------------------------------
BALL, BALL_R = (-0.3, 1.0, 0.0), 0.8
BALL_SLIDE = 0.55       # a third of the ball's on-screen diameter of 24 pixels: 8 pixels = 0.55 at the ball's distance of 4


def ball_scene():
    d = ag.SceneDesc("ball")
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.6, 0.6, 0.6))
    red = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.7, 0.2, 0.15))
    d.add_plane((0.0, 0.0, 0.0), (12.0, 12.0), grey)
    d.add_sphere(BALL, BALL_R, red)                          # primitive 1
    d.add_area_light((1.6, 3.2, -1.0), 0.3, (60.0, 60.0, 60.0))
    d.add_uniform_infinite_light((0.3, 0.3, 0.3))
    d.set_camera(*mm.CARD_CAMERA)
    return d


def ball_frame(g, k, motion):
    acc, m2, _, _ = PT.render_adaptive_to_host(g, CW, CH, 4, 4, 4, 0.0, seed_base=k + 1)
    assert (acc[..., 3] == 4).all()
    feats = PT.render_features_motion_to_host(g, CW, CH) if motion else PT.render_features_to_host(g, CW, CH)
    return (acc, m2) + tuple(feats)


def eroded(mask, r):
    out = mask.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            shifted = np.zeros_like(mask)
            ys, yd = slice(max(dy, 0), mask.shape[0] + min(dy, 0)), slice(max(-dy, 0), mask.shape[0] + min(-dy, 0))
            xs, xd = slice(max(dx, 0), mask.shape[1] + min(dx, 0)), slice(max(-dx, 0), mask.shape[1] + min(-dx, 0))
            shifted[yd, xd] = mask[ys, xs]
            out &= shifted
    return out


def test_history_follows_a_moved_ball():
    ctx = gpu_context()
    desc = ball_scene()
    new_c = (BALL[0] + BALL_SLIDE, BALL[1], BALL[2])
    moved = with_sphere(desc, 1, new_c, BALL_R)
    g = gpu_scene(desc)
    try:
        g.snapshot_positions()
        f0 = ball_frame(g, 0, False)
        prev = f0[:4]
        g.update_sphere(1, new_c, BALL_R)
        g.snapshot_positions()
        acc, m2, albedo, nd, pp = ball_frame(g, 1, True)
        model_pp, _, hits = model_prev_point(g, mm.CARD_CAMERA, CW, CH, [], {}, desc, moved)
        assert np.array_equal(bits(pp), bits(model_pp))
        on_ball = (hits["hit"] == 1) & (hits["prim"] == 1)
        assert np.array_equal(pp[..., 3] == 1, on_ball)
        cur = (acc, m2, albedo, nd)
        va = ag.camera_vectors(mm.CARD_CAMERA)
        # the picked set, from the models alone: moved pixels whose four taps lie two pixels inside the ball's previous silhouette --
        # the pixels of the previous normal_depth whose point O + depth * D is on the old sphere
        O, _, D = mm.feature_rays(va, CW, CH)
        p_prev = O + prev[3][..., 3:4] * D.reshape(CH, CW, 3)
        was_ball = (prev[3][..., 3] > 0) & (np.abs(np.linalg.norm(p_prev - np.asarray(BALL, F), axis=-1) - BALL_R) < 1e-3)
        assert 300 <= was_ball.sum() <= 700, was_ball.sum()
        inner = eroded(was_ball, 2)
        pos, is_moved = mm.position(va, va, True, albedo[..., 3], nd[..., 3], model_pp, CW, CH)
        assert np.array_equal(is_moved, on_ball)
        picked = np.zeros((CH, CW), bool)
        for r, c in zip(*np.nonzero(is_moved & pos["found"])):
            taps = [(CH - 1 - (pos["y0"][r, c] + dy), pos["x0"][r, c] + dx) for dy in (0, 1) for dx in (0, 1)]
            picked[r, c] = all(0 <= y < CH and 0 <= x < CW and inner[y, x] for y, x in taps)
        print("ball: %d pixels now, %d before, %d picked" % (on_ball.sum(), was_ball.sum(), picked.sum()))
        assert picked.sum() >= 50
        model = mm.accumulate_motion(va, va, *cur, prev, model_pp, identity=True)
        assert (model[0][picked, 3] > 4).all()
        # the GPU
        got = ctx.temporal_to_host(mm.CARD_CAMERA, mm.CARD_CAMERA, *cur, prev=prev, prev_point=pp)
        assert np.array_equal(bits(got[0]), bits(model[0])) and np.array_equal(bits(got[1]), bits(model[1]))
        assert (got[0][picked, 3] > 4).all()
        # without motion vectors the pixels the ball newly covers find no history
        plain = ctx.temporal_to_host(mm.CARD_CAMERA, mm.CARD_CAMERA, *cur, prev=prev)
        newly = on_ball & ~was_ball
        assert newly.sum() >= 50 and (plain[0][newly, 3] == 4).all()
    finally:
        g.close()


# ---- 8. a caller's stream ----------------------------------------------------------------------------------------------------------------
def test_every_new_entry_point_on_a_callers_stream():
    from test_gpu_streams import Stage
    desc = motion_scene()
    ids = np.array([3, 2], np.int32)
    rec = np.array([[1.3, 1.8, 0.6, 0.35], [-1.0, 0.6, 0.4, 0.5]], F)
    wrong = np.array([[9.0, 9.0, 9.0, 2.0], [-9.0, 3.0, 1.0, 0.25]], F)
    after_batch = with_batch(desc, ids, rec)
    final = with_area_radiance(with_plane(with_sphere(after_batch, 2, (-0.8, 0.75, 0.1), 0.45), 0, (0.4, 0.1, -0.3), (8.0, 12.0)), 3, (9.0, 7.0, 5.0))
    oacc, ost = oracle_render(final, CW, CH, 2)
    with Stage() as st:
        g = st.scene(desc)
        g.snapshot_positions()
        # the batch: its records are staged behind the delay
        b_rec = st.buffer(rec, wrong)
        st.open([b_rec])
        st.call("update_spheres_device", g.update_spheres_device, ids, b_rec.dst)
        st.open()
        st.call("snapshot_positions", g.snapshot_positions)
        albedo, nd, pp = (st.output((CH, CW, 4), -7.0) for _ in range(3))
        st.open([albedo, nd, pp])
        st.call("render_features_motion", PT.render_features_motion, g, CW, CH, albedo.dst, nd.dst, pp.dst)
        got_pp = st.read(pp)
        model, _, hits = model_prev_point(g, mm.CARD_CAMERA, CW, CH, [mm.card_mesh()], MOTION_BASES, desc, after_batch)
        assert np.array_equal(bits(got_pp), bits(model))
        assert np.array_equal(got_pp[..., 3] == 1, (hits["hit"] == 1) & np.isin(hits["prim"], [2, 3]))
        # the host calls, each with the hazard window open
        st.open()
        st.call("update_sphere", g.update_sphere, 2, (-0.8, 0.75, 0.1), 0.45)
        st.open()
        st.call("update_plane", g.update_plane, 0, (0.4, 0.1, -0.3), (8.0, 12.0))
        st.open()
        st.call("set_area_light_radiance", g.set_area_light_radiance, 3, (9.0, 7.0, 5.0))
        film = st.output((CH, CW, 4), -7.0)
        st.open([film])
        stats = st.call("render", PT.render, g, CW, CH, 2, film.dst)
        got = st.read(film)
        assert np.array_equal(bits(got[..., :3]), bits(oacc[..., :3])) and stats.rays == ost.rays
    # the infinite light, on a scene that has one
    desc = three_spheres()
    final = with_infinite_radiance(desc, 1, (0.9, 0.1, 0.05))
    oacc, ost = oracle_render(final, 32, 24, 2)
    with Stage() as st:
        g = st.scene(desc)
        st.open()
        st.call("set_infinite_light_radiance", g.set_infinite_light_radiance, 1, (0.9, 0.1, 0.05))
        film = st.output((24, 32, 4), -7.0)
        st.open([film])
        stats = st.call("render", PT.render, g, 32, 24, 2, film.dst)
        assert np.array_equal(bits(st.read(film)[..., :3]), bits(oacc[..., :3])) and stats.rays == ost.rays
