"""Root entry of the short-list trace kernels (k_trace_fast: pick_next): a fast ray enters a mesh whose root is
interior at the root's child pair and never runs the root-box step.  Nothing may change: every case runs once as is and once with
AGPT_ROOT_STEP=1 (every mesh entered at its root pair) and requires the two results byte for byte equal, and both equal to the CPU
oracle's.  The scene holds what the entry has to get right: a mesh of two zero-thickness planes whose root box is the whole room, a
one-triangle mesh (its root is a leaf and keeps the root step), a mesh that can never be hit, two coincident meshes with a sphere
between them in the list, and an emitter sphere.  (An empty mesh in the list cannot exist: agpt_scene_add_mesh refuses a mesh without
a triangle, as the reference's build does not terminate on one -- test_ray_queries asserts that; the never-hit mesh, one degenerate
triangle, stands in its place in the list.)"""
import functools

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import ray_edge_cases as rec
from helpers import bits, gpu_context, gpu_scene, oracle_render, oracle_scene, random_rays

pytestmark = pytest.mark.gpu
F = np.float32
DEPTH = 5
ROOM, ONE_TRI, NEVER_HIT, BLOB_A, SPHERE, BLOB_B, EMITTER = range(7)   # list positions


def corners(tris):
    t = np.asarray(tris, np.int32).reshape(-1)
    return np.stack([t, t, t], axis=1)


def room():
    """floor (y = 0) and ceiling (y = 3) of 6 x 6 quads each in ONE mesh: both are zero-thickness boxes, the root box is the room"""
    vf, idx = rec.flat_quads(0.0, 3.0, 6)
    vc, _ = rec.flat_quads(3.0, 3.0, 6)
    return np.concatenate([vf, vc]), np.concatenate([idx, idx + len(vf)])


def blob(seed=3, center=(-1.0, 1.0, 0.25), radius=0.6):
    v, _, _, idx = ag.scenes.blob_mesh(10, 7, center=center, radius=radius, seed=seed)
    return np.ascontiguousarray(v, F), corners(idx[:, 0])


def deep27():
    """test_gpu_intersect.deep_mesh's construction with 28 triangles, 8^-27 to 1 across, from the origin along x in the plane z = 0 (the
    small ones need the coordinates near zero): a 27-level tree, deeper than the 23 stack entries the kernels keep in LDS"""
    v, tris, x = [], [], 0.0
    for i in range(28):
        w = 8.0 ** (i - 27)
        v += [[x, 0, 0], [x + w, 0, 0], [x, w, 0]]
        tris.append([3 * i, 3 * i + 1, 3 * i + 2])
        x += w * 1.5
    return np.array(v, F), corners(tris)


def scene(deep=False, blob_b=None):
    """blob_b: the arrays of BLOB_B (default: BLOB_A's, the two meshes coincide)"""
    d = ag.SceneDesc("root-entry" + ("-deep" if deep else ""))
    grey = d.add_material(ag.MAT_DISNEY, [.7, .7, .65], 0.8, 0.0)
    red = d.add_material(ag.MAT_DISNEY, [.8, .3, .25], 0.4, 0.3)
    v, idx = room()
    d.add_mesh(v, None, None, idx, grey, 1)
    d.add_mesh(F([[0.5, 0.2, -1], [1.5, 0.2, -1], [1.0, 1.4, -0.5]]), None, None, corners([0, 1, 2]), red, 1)
    d.add_mesh(F([[0, 1, 1], [1, 1, 1], [2, 1, 1]]), None, None, corners([0, 1, 2]), red, 1)   # zero area: det == 0, never hit
    v, idx = blob()
    d.add_mesh(v, None, None, idx, red, 1)
    d.add_sphere([0.9, 0.7, 0.6], 0.5, grey)
    d.add_mesh(v if blob_b is None else blob_b, None, None, idx, grey, 2)
    d.add_area_light([0.0, 2.4, -0.5], 0.3, [30., 28., 25.])
    if deep:
        v, idx = deep27()
        d.add_mesh(v, None, None, idx, grey, 1)
    d.add_uniform_infinite_light([.3, .35, .4])
    d.set_camera([0.2, 1.4, -5.0], [0, 1.1, 0], [0, 1, 0], 64 / 48, 45.0, 0.0)
    assert d.n_tris <= 2000
    return d


@functools.lru_cache(maxsize=None)
def query_rays():
    """4,000 random rays and every ray class of ray_edge_cases on the scene; read-only, shared by the tests"""
    d = scene()
    sets = [random_rays(d, 4000, seed=41)] + [build(d) for build in rec.CLASSES.values()]
    rays = np.concatenate(sets)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def oracle_queries(key):
    """the oracle's Intersect / IntersectP records for query_rays() on SCENES[key]()"""
    o = oracle_scene(SCENES[key]())
    return o.intersect(query_rays())[0], o.intersect(query_rays(), any_hit=True)[0]


def same_hits(a, b):
    assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["tri"], b["tri"])
    m = b["hit"] == 1
    for f in ("t", "b1", "b2"):
        assert np.array_equal(bits(a[f][m]), bits(b[f][m])), f


def check_queries(monkeypatch, g, key, oracle=True):
    """Intersect and IntersectP of g on query_rays(): entry on == AGPT_ROOT_STEP=1, and both == the oracle on SCENES[key]()"""
    rays = query_rays()
    on, onp = g.Intersect(rays)[0], g.IntersectP(rays)[0]
    monkeypatch.setenv("AGPT_ROOT_STEP", "1")
    off, offp = g.Intersect(rays)[0], g.IntersectP(rays)[0]
    monkeypatch.delenv("AGPT_ROOT_STEP")
    assert on.tobytes() == off.tobytes() and onp.tobytes() == offp.tobytes()
    print(key, "rays %d, hits %d, occluded %d" % (len(rays), int(on["hit"].sum()), int(onp["hit"].sum())))
    if oracle:
        oh, op_ = oracle_queries(key)
        same_hits(on, oh)
        assert np.array_equal(onp["hit"], op_["hit"])
    return on


def totals(st):
    return st.closest_rays, st.anyhit_rays, st.answered_rays, st.outliers


def check_render(monkeypatch, g, desc, W=64, H=48, spp=2, oracle=True):
    pt = ag.PathTracer(DEPTH)
    a, sa = pt.render_to_host(g, W, H, spp)
    monkeypatch.setenv("AGPT_ROOT_STEP", "1")
    b, sb = pt.render_to_host(g, W, H, spp)
    monkeypatch.delenv("AGPT_ROOT_STEP")
    assert a.tobytes() == b.tobytes()
    assert totals(sa) == totals(sb)
    if oracle:
        oacc, ost = oracle_render(desc, W, H, spp, DEPTH)
        assert np.array_equal(bits(a[..., :3]), bits(oacc[..., :3]))
        assert (sa.closest_rays, sa.anyhit_rays, sa.outliers) == (ost.closest_rays, ost.anyhit_rays, ost.outliers)
        assert sa.rays == ost.rays
    return a


def moved_blob():
    """another blob on the same index list: its binned-SAH tree has another topology"""
    return blob(seed=11, center=(-0.6, 1.2, 0.4), radius=0.7)[0]


SCENES = {"base": scene, "deep": lambda: scene(deep=True), "scaled": lambda: scene(blob_b=blob()[0] * F(2)),
          "moved": lambda: scene(blob_b=moved_blob())}


def test_ray_queries(monkeypatch):
    g = gpu_scene(scene())
    with pytest.raises(ag.AgptError):   # (why the scene has no empty mesh)
        ag.Scene(gpu_context()).add_mesh(np.zeros((3, 3), F), None, None, np.zeros((0, 3), np.int32), -1)
    assert len(g.bvh(ONE_TRI)[0]) == 2 and len(g.bvh(ROOM)[0]) > 3   # (nodes + 1: a leaf root, an interior root)
    hits = check_queries(monkeypatch, g, "base")
    g.close()
    hit = hits[hits["hit"] == 1]
    assert {ROOM, ONE_TRI, BLOB_A, SPHERE, EMITTER} <= set(hit["prim"].tolist()) and NEVER_HIT not in set(hit["prim"].tolist())


@pytest.mark.parametrize("case", ["base", "c1", "deep-spill", "group-of-64"])
def test_renders(monkeypatch, case):
    """64 x 48 at 2 spp on the scene and on C1; the scene with a 27-level mesh (the SPILL instantiations); 16 x 12 at 64 spp, where
    the first launch of the batch is the coherent one (COH)"""
    desc = {"c1": ag.scenes.scene_c1, "deep-spill": SCENES["deep"]}.get(case, scene)()
    if case == "deep-spill":
        assert ag.bvh_build(*deep27(), 1)[2] == 27
    g = gpu_scene(desc)
    if case == "group-of-64":
        check_render(monkeypatch, g, desc, 16, 12, 64)
    else:
        check_render(monkeypatch, g, desc)
    g.close()


def test_mesh_updates(monkeypatch):
    """agpt_scene_update_mesh and agpt_scene_pose_mesh on BLOB_B, which starts coincident with BLOB_A.  A refit under an exact scale by
    two leaves the tree the builder would build (test_mesh_update_api.py), and a rebuild builds it: both are compared with the oracle
    on the new arrays.  A refit to another shape keeps the old topology, which the oracle does not have: those are compared with the
    AGPT_ROOT_STEP=1 run only."""
    v0 = blob()[0]
    g = gpu_scene(scene())
    before = g.bvh(BLOB_B)[0].tobytes()
    # REFIT, exact x2
    g.update_mesh(BLOB_B, v0 * F(2), None, "refit")
    check_queries(monkeypatch, g, "scaled")
    check_render(monkeypatch, g, SCENES["scaled"]())
    # REFIT to another shape: the old topology with new boxes
    g.update_mesh(BLOB_B, moved_blob(), None, "refit")
    check_queries(monkeypatch, g, "moved", oracle=False)
    check_render(monkeypatch, g, None, oracle=False)
    # REBUILD of that shape: a new topology
    g.update_mesh(BLOB_B, moved_blob(), None, "rebuild")
    assert g.bvh(BLOB_B)[0].tobytes() != before
    check_queries(monkeypatch, g, "moved")
    check_render(monkeypatch, g, SCENES["moved"]())
    # POSE: one joint with weight 1 that scales by two (exact: the oracle's tree), then three joints that bend the mesh
    g.update_mesh(BLOB_B, v0, None, "rebuild")
    n = len(v0)
    g.set_mesh_skin(BLOB_B, np.zeros((n, 1), np.int32), np.ones((n, 1), F), n_joints=1)
    g.pose_mesh(BLOB_B, np.diag(F([2, 2, 2, 1]))[None])
    check_queries(monkeypatch, g, "scaled")
    check_render(monkeypatch, g, SCENES["scaled"]())
    from skin_cases import JOINTS3, binding
    J, W = binding(n, 4, seed=5)
    g.set_mesh_skin(BLOB_B, J, W, n_joints=3)
    g.pose_mesh(BLOB_B, JOINTS3)
    check_queries(monkeypatch, g, "base", oracle=False)
    check_render(monkeypatch, g, None, oracle=False)
    g.close()


def test_counters(monkeypatch):
    """counters=2, the production kernels counting their own work: a mesh's first record counts as its root test whichever record it
    is, so root_tests is the same in both modes, and the entry saves interior fetches, never adds any"""
    g = gpu_scene(scene())
    pt = ag.PathTracer(DEPTH)
    a, sa = pt.render_to_host(g, 64, 48, 2, counters=2)
    monkeypatch.setenv("AGPT_ROOT_STEP", "1")
    b, sb = pt.render_to_host(g, 64, 48, 2, counters=2)
    monkeypatch.delenv("AGPT_ROOT_STEP")
    plain, sp = pt.render_to_host(g, 64, 48, 2)
    g.close()
    print("entry on: interior %d roots %d tris %d;  root step: interior %d roots %d tris %d" % (
        sa.interior_visits, sa.root_tests, sa.tri_tests, sb.interior_visits, sb.root_tests, sb.tri_tests))
    assert a.tobytes() == b.tobytes() == plain.tobytes()
    assert totals(sa) == totals(sb) == totals(sp)
    assert sa.root_tests == sb.root_tests > 0
    assert sa.interior_visits + sa.root_tests <= sb.interior_visits + sb.root_tests
    assert sa.tri_tests == sb.tri_tests
