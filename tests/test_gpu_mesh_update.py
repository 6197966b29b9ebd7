"""agpt_scene_update_mesh on the GPU.  REBUILD must leave the scene a fresh one would be; REFIT keeps the topology, so it is checked
three ways: against the oracle where the refitted tree IS the built one (unchanged arrays, an exact x2 scale --
test_mesh_update_api.py asserts that premise on the CPU), against the numpy refit model plus a forced host re-commit of the same
scene (scene B: every device-written record against the host flatten's, through renders and all work counters), and against the
oracle's hit records on random rays."""
import ctypes as C
import functools

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import bvh_refit_model as model
import mesh_update_cases as cases
from helpers import bits, build_cpp_example, gpu_context, gpu_scene, oracle_render_on, oracle_scene, random_rays, signed_zero_grid
from oracle import binding as ob

pytestmark = pytest.mark.gpu
F = np.float32
W = H = 48
SPP = 2
COUNTERS = ("closest_rays", "anyhit_rays", "interior_visits", "tri_tests", "shaded_vertices", "samples", "outliers", "iterations",
            "trace_launches", "root_tests", "answered_rays")
BLOBS = (1, 2)   # the primitives of cases.scene that move


def counters(st):
    return {k: getattr(st, k) for k in COUNTERS}


def render(g, counters_mode=0, w=W, h=H):
    return ag.PathTracer(5).render_to_host(g, w, h, SPP, counters=counters_mode)


@functools.lru_cache(maxsize=None)
def oracle_render(pose, scale):
    """the oracle scene of both blobs in `pose` -- kept: the tests query it too -- and its render, once per argument set"""
    o = oracle_scene(cases.scene(pose, pose, scale), 5)
    acc, st = oracle_render_on(o, W, H, SPP)
    acc.setflags(write=False)
    return o, acc, st


def update_blobs(g, target, mode, scale=1.0):
    """both blobs of the scene moved to the arrays of cases.scene(target, target, scale)"""
    d = cases.scene(target, target, scale)
    for prim in BLOBS:
        v, n = cases.blob_arrays(d, prim)
        g.update_mesh(prim, v, n, mode)
    return d


def recommitted(build):
    """scene B: the same scene with the same updates, then a forced full host flatten (an unused material uncommits the scene)"""
    b = build()
    b.add_material(ag.MAT_DIFFUSE_ONLY, [.1, .2, .3])
    b.commit()
    return b


def assert_same_scene(a, b, w=W, h=H):
    for mode in (0, 2):   # production kernels, then the production trace kernel counting its own work
        ra, sa = render(a, mode, w, h)
        rb, sb = render(b, mode, w, h)
        assert ra.tobytes() == rb.tobytes()
        assert counters(sa) == counters(sb)
    for prim in range(3):
        if a.L.agpt_mesh_num_nodes(a.h, prim) > 0:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a.bvh(prim), b.bvh(prim)))


def test_errors_in_the_documented_order():
    g = ag.Scene(gpu_context())
    d = cases.scene(0, 0)
    L, fp = g.L, C.POINTER(C.c_float)
    v, n = cases.blob_arrays(d, 1)
    pv, pn = v.ctypes.data_as(fp), n.ctypes.data_as(fp)

    def refused(what, *args):
        assert L.agpt_scene_update_mesh(*args) == -1
        assert what in L.agpt_last_error(), L.agpt_last_error()
    refused(b"NULL", g.h, 99, None, 0, None, 0, 7)              # NULL vertices first
    refused(b"not committed", g.h, 99, pv, 1, None, 0, 7)       # then the commit state
    d.instantiate(g)
    before = [x.tobytes() for x in g.bvh(1)] + [render(g)[0].tobytes()]
    for prim in (-1, 3, 99):
        refused(b"not a mesh", g.h, prim, pv, 1, None, 0, 7)    # then the primitive (3 is the sphere light)
    refused(b"vertices and", g.h, 1, pv, len(v) - 1, pn, len(n), 7)
    refused(b"vertices and", g.h, 1, pv, len(v), pn, len(n) - 1, 7)
    refused(b"vertices and", g.h, 1, pv, len(v), None, len(n), 7)
    refused(b"vertices and", g.h, 2, pv, len(v), pn, len(n), 7)   # the second blob has no normals
    refused(b"unknown mode", g.h, 1, pv, len(v), pn, len(n), 7)
    assert [x.tobytes() for x in g.bvh(1)] + [render(g)[0].tobytes()] == before   # a refused call changes nothing
    g.close()


@pytest.mark.parametrize("builder", ["host", "device"])
def test_rebuild_equals_a_fresh_scene(builder):
    g = ag.Scene(gpu_context())
    g.set_bvh_builder(builder)
    cases.scene(0, 0).instantiate(g)
    update_blobs(g, 1, "rebuild")
    o, oacc, ost = oracle_render(1, 1.0)
    acc, st = render(g, 1)
    assert acc.tobytes() == oacc.tobytes()
    assert st.rays == ost.rays and st.closest_rays == ost.closest_rays and st.anyhit_rays == ost.anyhit_rays
    for prim in (0,) + BLOBS:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g.bvh(prim), o.bvh(prim)))
    g.close()


def test_refit_with_unchanged_arrays_is_a_no_op():
    g = gpu_scene(cases.scene(0, 0))
    before = [g.bvh(p) for p in BLOBS]
    update_blobs(g, 0, "refit")
    for p, (nodes, order) in zip(BLOBS, before):
        assert g.bvh(p)[0].tobytes() == nodes.tobytes() and g.bvh(p)[1].tobytes() == order.tobytes()
    o, oacc, ost = oracle_render(0, 1.0)
    acc, st = render(g, 1)
    assert acc.tobytes() == oacc.tobytes() and st.rays == ost.rays
    g.close()


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_refit_under_an_exact_scale_by_two_equals_the_oracle(arith):
    """The refitted tree is the built one (asserted on the CPU), so everything is the oracle's: the tree, the render bit for bit,
    the reference-order work counters.  FAST compares against a fresh GPU scene in the same arithmetic."""
    g = gpu_scene(cases.scene(0, 0))
    update_blobs(g, 0, "refit", 2.0)
    o, oacc, ost = oracle_render(0, 2.0)
    for prim in BLOBS:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g.bvh(prim), o.bvh(prim)))
    g.set_shading_arith(arith)
    acc, st = render(g, 1)
    if arith == "exact":
        assert acc.tobytes() == oacc.tobytes()
    else:
        f = gpu_scene(cases.scene(0, 0, 2.0))
        f.set_shading_arith("fast")
        facc, fst = render(f, 1)
        f.close()
        assert acc.tobytes() == facc.tobytes() and counters(st) == counters(fst)
    assert st.rays == ost.rays
    assert st.interior_visits == ost.interior_visits and st.tri_tests == ost.tri_tests
    g.close()


def deformed():
    g = gpu_scene(cases.scene(0, 0))
    update_blobs(g, 1, "refit")
    return g


def test_refit_under_a_general_deformation_equals_the_model_and_the_host_flatten():
    d0 = cases.scene(0, 0)
    a = gpu_scene(d0)
    built = {p: a.bvh(p) for p in BLOBS}
    d1 = update_blobs(a, 1, "refit")
    idx = cases.blob(0)[3]
    for p in BLOBS:
        nodes, order = a.bvh(p)
        assert order.tobytes() == built[p][1].tobytes()
        assert nodes.tobytes() == model.refit(built[p][0], order, cases.blob_arrays(d1, p)[0], idx).tobytes()
    b = recommitted(deformed)
    assert_same_scene(a, b)
    # and a second update of the same meshes (the cached path), back to the build pose: the oracle's scene again
    update_blobs(a, 0, "refit")
    assert render(a, 1)[0].tobytes() == oracle_render(0, 1.0)[1].tobytes()
    a.close()
    b.close()


@pytest.mark.parametrize("mpn", [1, 4])
def test_refit_of_the_signed_zero_grid_equals_a_fresh_commit(mpn):
    """The tie rule of the shared box (tminf / tmaxf keep the later of equal operands: +0 against -0) through the device refit: the
    same arrays, then every coordinate negated and negated back, must leave the tree and a closest-hit batch a fresh commit's."""
    v, idx = signed_zero_grid(12)   # 288 triangles, two per leaf
    d = ag.SceneDesc("signed-zero-grid")
    d.add_mesh(v, None, None, idx, d.add_material(ag.MAT_DIFFUSE_ONLY, [.7, .7, .7]), mpn)
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([0, 2, -4], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    rng = np.random.RandomState(12)
    rays = np.zeros(384, ag.RAY_DTYPE)
    o = rng.uniform(-1.2, 1.2, (384, 3)).astype(F)
    o[:, 1] = np.where(np.arange(384) % 2 == 0, F(2), F(-2))
    target = v[rng.randint(len(v), size=384)].copy()           # exact vertices: shared edges and corners, the x = -0 line
    target[:128] += rng.normal(0, 0.05, (128, 3)).astype(F)
    o[256:, 0], o[256:, 2] = target[256:, 0], target[256:, 2]  # straight down / up onto a vertex: zero direction components
    rays["o"], rays["d"], rays["tmax"] = o, target - o, F(3.402823466e+38)
    fresh, g = gpu_scene(d), gpu_scene(d)
    nodes, order = fresh.bvh(0)
    used = np.arange(len(nodes)) != 1
    assert (nodes["count"][used] > 1).any() and (np.signbit(nodes["bmin"][used]) & (nodes["bmin"][used] == 0)).any()
    hits, _ = fresh.Intersect(rays)
    assert np.count_nonzero(hits["hit"]) > 100

    def same_as_fresh():
        got_nodes, got_order = g.bvh(0)
        for f in ("bmin", "bmax"):
            assert np.array_equal(bits(got_nodes[f][used]), bits(nodes[f][used]))
        assert got_nodes.tobytes() == nodes.tobytes() and got_order.tobytes() == order.tobytes()
        assert g.Intersect(rays)[0].tobytes() == hits.tobytes()
    g.update_mesh(0, v, None, "refit")
    same_as_fresh()
    g.update_mesh(0, -v, None, "refit")
    g.update_mesh(0, -(-v), None, "refit")
    same_as_fresh()
    fresh.close()
    g.close()


def test_refit_still_finds_the_geometry():
    """Closest hit and any hit of 20,000 helpers.random_rays (seed 1) against the oracle built from the new arrays: hit flag and the
    bits of t equal on all rays but at most 2 (the trees differ, and a slab test is not strictly conservative against the triangle
    test at a box corner); where they agree and no other triangle ties at that t, prim and tri agree too.  Checked on the CPU
    beforehand: oracle scenes of the deformed meshes with max_prims_in_node (1, 4) and (4, 1) disagree on 0 of these rays (closest and
    any hit; seeds 1, 2 and 3 alike)."""
    d1 = cases.scene(1, 1)
    rays = random_rays(d1, 20000, seed=1)
    o = oracle_scene(d1)
    swapped = oracle_scene(cases.scene(1, 1, mpn=(4, 1)))
    oh, _ = o.intersect(rays)
    sh, _ = swapped.intersect(rays)
    assert int(((oh["hit"] != sh["hit"]) | ((oh["hit"] == 1) & (bits(oh["t"]) != bits(sh["t"])))).sum()) <= 2
    g = deformed()
    gh, _ = g.Intersect(rays)
    differ = (gh["hit"] != oh["hit"]) | ((oh["hit"] == 1) & (bits(gh["t"]) != bits(oh["t"])))
    print("closest: rays that differ", int(differ.sum()), "hits", int(oh["hit"].sum()))
    assert int(differ.sum()) <= 2
    agree = ~differ & (oh["hit"] == 1)
    other = agree & ((gh["prim"] != oh["prim"]) | (gh["tri"] != oh["tri"]))
    print("same t, another triangle:", int(other.sum()))
    meshes = [op for op in d1.ops if op[0] in ("mesh", "sphere", "area_light")]
    for i in np.nonzero(other)[0]:
        # the GPU's triangle alone, in the oracle: it must hit at the oracle's t (a tie), or the GPU reported the wrong triangle
        op = meshes[gh["prim"][i]]
        assert op[0] == "mesh"
        tri = op[4][gh["tri"][i]:gh["tri"][i] + 3, 0]
        single = ob.OracleScene()
        single.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
        single.add_mesh(op[1][tri], None, None, np.repeat(np.arange(3, dtype=np.int32), 3).reshape(3, 3), 0, 1)
        one, _ = single.intersect(rays[i:i + 1])
        assert one["hit"][0] == 1 and bits(one["t"])[0] == bits(oh["t"])[i], i
    gp, _ = g.IntersectP(rays)
    op_, _ = o.intersect(rays, any_hit=True)
    print("any hit: rays that differ", int((gp["hit"] != op_["hit"]).sum()))
    assert int((gp["hit"] != op_["hit"]).sum()) <= 2
    g.close()


def test_refit_in_a_long_list_rebuilds_the_top_level_tree():
    from test_gpu_long_lists import _many_prims
    d = _many_prims(65, 31, duplicates=False)
    d.add_area_light([0.0, 8.0, 0.0], 0.8, [70, 65, 60])
    d.add_uniform_infinite_light([.25, .3, .35])
    d.set_camera([0, 3, -16], [0, 0, 0], [0, 1, 0], 1.0, 50.0, 0.0)
    prim = 7
    moved = ag.scenes.blob_mesh(5, 4, center=(0.5, 2.0, -9.0), radius=1.5, seed=99)   # well outside its old root box, towards the camera

    def build():
        g = gpu_scene(d)
        g.update_mesh(prim, moved[0], moved[1], "refit")
        return g
    a, b = build(), recommitted(build)
    assert_same_scene(a, b)
    still = gpu_scene(d)
    assert render(still)[0].tobytes() != render(a)[0].tobytes()   # (the film sees the move)
    for s in (a, b, still):
        s.close()


def test_refit_of_a_textured_mesh_with_a_normal_map():
    rng = np.random.RandomState(5)
    d = cases.scene(0, 0)
    tex = d.add_texture(ag.scenes.checker_texture(16, 16, 4))
    nmap = d.add_texture((np.array([.5, .5, 1.0], F) + rng.uniform(-.25, .25, (8, 8, 3)) * [1, 1, 0]).astype(F))
    d.set_material_texture(1, tex)
    d.set_material_normal_texture(1, nmap, 1.0)

    def build():
        g = gpu_scene(d)
        update_blobs(g, 1, "refit")
        return g
    a, b = build(), recommitted(build)
    assert_same_scene(a, b)
    a.close()
    b.close()


def test_update_between_two_adaptive_frames():
    pt = ag.PathTracer(5)
    a = gpu_scene(cases.scene(0, 0))
    first = pt.render_adaptive_to_host(a, W, H, 2, 4, 2, 0.05)
    update_blobs(a, 1, "refit")
    second = pt.render_adaptive_to_host(a, W, H, 2, 4, 2, 0.05)
    b = recommitted(deformed)
    want = pt.render_adaptive_to_host(b, W, H, 2, 4, 2, 0.05)
    assert second[0].tobytes() == want[0].tobytes() and second[1].tobytes() == want[1].tobytes()
    assert second[3].as_dict() == want[3].as_dict()
    assert first[0].tobytes() != second[0].tobytes()
    a.close()
    b.close()


def test_a_non_finite_vertex_takes_the_host_path():
    d1 = cases.scene(1, 1)
    v, n = cases.blob_arrays(d1, 1)
    v = v.copy()
    v[40, 1] = np.inf
    v[41, 0] = np.nan

    def build():
        g = gpu_scene(cases.scene(0, 0))
        g.update_mesh(2, *cases.blob_arrays(d1, 2))   # (a device refit first: its bounds reach the host mirror before the commit)
        g.update_mesh(1, v, n, "refit")
        return g
    a = build()
    built = gpu_scene(cases.scene(0, 0)).bvh(1)
    nodes, order = a.bvh(1)
    assert nodes.tobytes() == model.refit(built[0], order, v, cases.blob(0)[3]).tobytes()
    b = recommitted(build)
    assert_same_scene(a, b)
    a.close()
    b.close()


def test_cpp_animated_example_writes_a_frame_per_pose(tmp_path):
    import subprocess
    exe = build_cpp_example(tmp_path, "animated_scene")
    out = subprocess.run([exe, str(tmp_path / "f"), "3", "32", "24"], check=True, capture_output=True, text=True).stdout
    frames = [(tmp_path / ("f_%03d.png" % k)).read_bytes() for k in range(3)]
    assert out.count("samples=8") == 3
    assert len(set(frames)) == 3 and all(f[:8] == b"\x89PNG\r\n\x1a\n" for f in frames)
