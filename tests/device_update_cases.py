"""The meshes, scenes and comparisons of the mesh-update tests on the GPU (test_gpu_mesh_update_device.py, test_gpu_transform_mesh.py,
test_gpu_pose_mesh.py, test_gpu_morph_mesh.py, test_gpu_smooth_normals.py, test_gpu_streams.py): the smallest meshes at which the
update kernels can still go wrong, all in ONE scene, the snapshot of a scene that two update paths must leave bit-identical, and the
matrices, bindings and targets that more than one of those files gives a mesh."""
import numpy as np

import ag_pathtracer_amd as ag
from helpers import gpu_context, random_rays
from morph_cases import targets
from skin_cases import JOINTS3, binding, flat_shaded
from transform_cases import MATRICES

F = np.float32
W = H = 32
SPP, DEPTH, N_RAYS = 2, 3, 3000


def _corners(tris, with_normals):
    t = np.asarray(tris, np.int32).reshape(-1)
    return np.stack([t, t if with_normals else np.full_like(t, -1), np.full_like(t, -1)], 1)


def _normals(v, seed):
    n = np.random.RandomState(seed).normal(size=v.shape) + [0, 3, 0]
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)


def one_triangle(with_normals):
    """the root is a leaf"""
    v = np.array([[-0.5, 0.1, 0.2], [0.6, 0.3, -0.1], [0.1, 1.1, 0.4]], F)
    return v, (_normals(v, 1) if with_normals else None), _corners([0, 1, 2], with_normals)


def strip(with_normals):
    """65 vertices, one past a 64-lane block: 63 triangles"""
    k = np.arange(65)
    v = np.stack([0.06 * k - 2.0, 0.5 + 0.35 * (k % 2) + 0.1 * np.sin(0.4 * k), 0.2 * np.cos(0.3 * k)], 1).astype(F)
    tris = [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(63)]
    return v, (_normals(v, 2) if with_normals else None), _corners(tris, with_normals)


def bumpy_grid(with_normals):
    """13 x 13 vertices (x = 0 on the middle column exactly), 288 triangles, and one more vertex that no triangle references"""
    n = 13
    x, z = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing="ij")
    y = 0.25 * np.sin(3.3 * x + 0.4) * np.cos(2.9 * z) + 0.1 * np.sin(9 * x * z)
    v = np.stack([x, y + 0.6, z], -1).reshape(-1, 3)
    v = np.concatenate([v, [[0.3, 5.0, 0.3]]]).astype(F)
    tris = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, i * n + j + 1, (i + 1) * n + j, (i + 1) * n + j + 1
            tris += [(a, b, c), (b, d, c)]
    assert v[6 * n + 3, 0] == 0 and len(tris) == 288
    return v, (_normals(v, 3) if with_normals else None), _corners(tris, with_normals)


UNREFERENCED = 13 * 13       # bumpy_grid's spare vertex
REFERENCED = 6 * 13 + 3      # one of its middle column
# (name, builder of the arrays, with normals, max_prims_in_node, offset in the scene)
ZOO = [("triangle+n", one_triangle, True, 1, (-2.5, 0.0, 1.5)), ("triangle", one_triangle, False, 1, (2.5, 0.0, 1.5)),
       ("strip+n", strip, True, 1, (0.0, 1.2, 2.5)), ("strip", strip, False, 4, (0.0, -0.6, -1.0)),
       ("grid1+n", bumpy_grid, True, 1, (-1.3, 0.0, 0.0)), ("grid1", bumpy_grid, False, 1, (1.3, 0.0, 0.0)),
       ("grid4+n", bumpy_grid, True, 4, (-1.3, 0.0, -2.4)), ("grid4", bumpy_grid, False, 4, (1.3, 0.0, -2.4))]
PRIMS = list(range(1, 1 + len(ZOO)))   # prim 0 is the floor
GRID1_N, GRID1, GRID4_N, GRID4 = 5, 6, 7, 8


def zoo_arrays(prim, pose=0):
    """positions and normals of prim in a pose: 0 = as built, 1 and 2 = smooth deformations (normals turned with them)"""
    _, make, wn, _, off = ZOO[prim - 1]
    v, n, _ = make(wn)
    v = v + np.array(off, F)
    if pose:
        p = v.astype(np.float64)
        p = p + 0.12 * pose * np.stack([np.sin(2.1 * p[:, 1] + pose), np.cos(1.7 * p[:, 0]), np.sin(1.3 * p[:, 2] - pose)], 1)
        v = p.astype(F)
        if n is not None:
            n = np.roll(n, pose, axis=0).copy()
    return v, n


def zoo_scene():
    """a floor and the eight meshes (none has texture coordinates), a sphere light, sky"""
    d = ag.SceneDesc("device-update-zoo")
    floor = d.add_material(ag.MAT_DISNEY, [.6, .62, .45], 1.0, 0.0)
    gold = d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], 0.4, 1.0)
    mirror = d.add_material(ag.MAT_MIRROR, [.9, .9, .9])
    red = d.add_material(ag.MAT_DISNEY, [0.8, 0.1, 0.12], 0.6, 0.0)
    fv = np.array([[-8, -1, -8], [8, -1, -8], [8, -1, 8], [-8, -1, 8]], F)
    d.add_mesh(fv, None, None, _corners([0, 2, 1, 0, 3, 2], False), floor, 1)
    for prim, (_, make, wn, mpn, _) in zip(PRIMS, ZOO):
        v, n = zoo_arrays(prim)
        d.add_mesh(v, n, None, make(wn)[2], [gold, red, mirror][prim % 3], mpn)
    d.add_area_light([0, 9, -3], 1.0, np.array([120, 112, 108], F))
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([0.4, 3.2, -7.5], [0.0, 0.3, 0.0], [0, 1, 0], 1.0, 50.0, 0.0)
    return d


_RAYS = {}


def rays_for(desc):
    if desc.name not in _RAYS:
        r = random_rays(desc, N_RAYS, seed=7)
        r.setflags(write=False)
        _RAYS[desc.name] = r
    return _RAYS[desc.name]


def snapshot(g, desc, prims):
    """everything the two paths must agree on, as bytes: every mesh's BVH, closest- and any-hit records, the render and its ray totals.
    It calls bvh() -- agpt_mesh_get_bvh, which runs sync_mirror(s, false) -- and therefore synchronises the mirror's bounds (and the
    spheres) at every use: after it no mesh has bounds_stale set.  A test that needs a stale flag to survive from one call into the next
    must not observe through it (test_gpu_update_walks.py observes the device only)."""
    out = {}
    for p in prims:
        nodes, order = g.bvh(p)
        out["bvh%d" % p] = nodes.tobytes() + order.tobytes()
    rays = rays_for(desc)
    out["closest"] = g.Intersect(rays)[0].tobytes()
    out["any"] = g.IntersectP(rays)[0].tobytes()
    acc, st = ag.PathTracer(DEPTH).render_to_host(g, W, H, SPP)
    out["render"] = acc.tobytes()
    out["rays"] = (st.rays, st.closest_rays, st.anyhit_rays)
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], k


class DeviceArrays:
    """positions (and normals) in device memory of the context, through agpt_device_alloc / agpt_device_upload"""

    def __init__(self, ctx, v, n=None):
        self.ctx = ctx
        self.v = np.ascontiguousarray(v, F)
        self.n = None if n is None else np.ascontiguousarray(n, F)
        self.pv = ctx.alloc(self.v.nbytes)
        ctx.upload(self.pv, self.v)
        self.pn = None
        if self.n is not None:
            self.pn = ctx.alloc(self.n.nbytes)
            ctx.upload(self.pn, self.n)

    def update(self, g, prim, mode="refit"):
        g.update_mesh_device(prim, self.pv, len(self.v), self.pn, 0 if self.n is None else len(self.n), mode)

    def free(self):
        self.ctx.free(self.pv)
        if self.pn:
            self.ctx.free(self.pn)


def update_through_device(g, prim, v, n, mode="refit"):
    d = DeviceArrays(g.ctx, v, n)
    try:
        d.update(g, prim, mode)
        # the library has copied the arrays: scribbling over them must not change the scene
        g.ctx.memset(d.pv, 0xFF, d.v.nbytes)
    finally:
        d.free()


def pair(builder="host", desc=None):
    """(description, scene A, scene B): two identical scenes of the zoo (or of desc) on the GPU"""
    desc = desc or zoo_scene()
    scenes = []
    for _ in range(2):
        g = ag.Scene(gpu_context())
        g.set_bvh_builder(builder)
        scenes.append(desc.instantiate(g))
    return desc, scenes[0], scenes[1]


def seventy_prims():
    d = ag.SceneDesc("device-update-70")
    mats = [d.add_material(ag.MAT_DIFFUSE_ONLY, c) for c in ([.8, .3, .2], [.2, .7, .3], [.3, .4, .8])]
    for k in range(70):
        c = (1.4 * (k % 10) - 6.3, 0.9 * ((k // 10) % 7) - 2.0, 1.1 * (k % 3))
        d.add_mesh(*ag.scenes.blob_mesh(5, 4, center=c, radius=0.45, seed=k), mats[k % 3], 1)
    d.add_area_light([0.0, 8.0, -4.0], 0.8, [70, 65, 60])
    d.add_uniform_infinite_light([.25, .3, .35])
    d.set_camera([0, 1, -16], [0, 0.5, 0], [0, 1, 0], 1.0, 50.0, 0.0)
    return d


def about(prim, M):
    """M applied about the mesh's place in the zoo (so that it stays in view): T(c) M T(-c), in float32 as given to both paths"""
    c = np.array(ZOO[prim - 1][4], np.float64)
    t0, t1 = np.eye(4), np.eye(4)
    t0[:3, 3], t1[:3, 3] = -c, c
    return (t1 @ M.astype(np.float64) @ t0).astype(F)


def frame_hash(rgb_words):
    """the FNV-1a hash the C++ examples print for a frame"""
    h = np.uint64(1469598103934665603)
    with np.errstate(over="ignore"):
        for w in np.asarray(rgb_words, np.uint32).reshape(-1):
            h = (h ^ np.uint64(w)) * np.uint64(1099511628211)
    return int(h)


def palette(prim, pose):
    """three joints about the mesh's place in the zoo; the two poses move every joint differently"""
    return np.stack([about(prim, JOINTS3[i]) for i in ((0, 1, 2), (1, 2, 0))[pose]])


BIG, FLAT = 10, 11         # the two meshes big_scene() adds to the zoo (prim 9 is the light)
BIG_N = 33                 # 33 x 33 = 1,089 vertices and as many normals: 2,178 items, 8.5 blocks of 256


def big_grid():
    x, z = np.meshgrid(np.linspace(-1, 1, BIG_N), np.linspace(-1, 1, BIG_N), indexing="ij")
    y = 0.2 * np.sin(2.7 * x + 0.3) * np.cos(3.1 * z)
    v = (np.stack([x, y + 0.5, z], -1).reshape(-1, 3) + [3.4, 0.0, -0.6]).astype(F)
    tris = []
    for i in range(BIG_N - 1):
        for j in range(BIG_N - 1):
            a, b, c, d = i * BIG_N + j, i * BIG_N + j + 1, (i + 1) * BIG_N + j, (i + 1) * BIG_N + j + 1
            tris += [(a, b, c), (b, d, c)]
    return v, _normals(v, 9), _corners(tris, True)


def flat_grid():
    """bumpy_grid with one normal per triangle: 170 vertices, 288 normals"""
    v, _, ix = bumpy_grid(False)
    v = (v + np.array([-3.4, 0.0, -0.6], F)).astype(F)
    n = flat_shaded(v, ix[:, 0])
    corners = ix.copy()
    corners[:, 1] = np.repeat(np.arange(len(n), dtype=np.int32), 3)
    return v, n, corners


def big_scene():
    d = zoo_scene()
    d.name = "morph-zoo"
    for k, (v, n, ix) in enumerate((big_grid(), flat_grid())):
        d.add_mesh(v, n, None, ix, k, 4)
    return d


def arrays_of(prim):
    if prim == BIG:
        return big_grid()[:2]
    if prim == FLAT:
        return flat_grid()[:2]
    return zoo_arrays(prim)


def morph_targets(g, prim, T=3, seed=None, normal_deltas=True):
    """seeded targets of mesh prim, set on scene g (if any) -> (dP, dN or None)"""
    v, n = arrays_of(prim)
    seed = 10 * prim + T if seed is None else seed
    dP = targets(len(v), T, seed, extent=2.0)
    dN = targets(len(n), T, seed + 1, extent=5.0) if n is not None and normal_deltas else None
    if g is not None:
        g.set_mesh_morph_targets(prim, dP, dN)
    return dP, dN


def skin_of(g, prim, n_joints=3):
    v, n = arrays_of(prim)
    J, W = binding(len(v), 4, seed=prim)
    nJ, nW = binding(len(n), 4, seed=prim + 50) if n is not None and len(n) != len(v) else (None, None)
    g.set_mesh_skin(prim, J, W, nJ, nW, n_joints=n_joints)
    return J, W, nJ, nW


def joints_of(prim, k):
    """three joint matrices about the mesh's own place: the zoo's palette, or the same matrices about the centre of an added mesh"""
    if prim in PRIMS:
        return palette(prim, k)
    v = arrays_of(prim)[0].astype(np.float64)
    c = 0.5 * (v.min(0) + v.max(0))
    t0, t1 = np.eye(4), np.eye(4)
    t0[:3, 3], t1[:3, 3] = -c, c
    order = ("rotation+translation", "scale+shear", "identity")
    return np.stack([(t1 @ MATRICES[order[(i + k) % 3]].astype(np.float64) @ t0).astype(F) for i in range(3)])
