"""agpt_scene_transform_mesh on the GPU against its definition: scene A gets agpt_scene_update_mesh with the arrays of
agpt_transform_arrays(M, rest pose) -- the host twin that test_transform_arrays.py pins to the OBJ loader's arithmetic --, scene B the
transform call; BVH bytes, hit records and renders must be bit-identical (device_update_cases.snapshot)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_update_cases as dc
from device_update_cases import about, frame_hash, pair, seventy_prims
from helpers import build_cpp_example, gpu_context, gpu_scene
from transform_cases import MATRICES

pytestmark = pytest.mark.gpu
F = np.float32
# x and w exchanged: w = x, which is exactly 0 on the middle column of the grids -> Inf / NaN positions from finite input
SWAP_XW = np.array([[0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]], F)


def by_definition(g, prim, M, rest, mode):
    v, n = ag.transform_arrays(M, *rest)
    g.update_mesh(prim, v, n, mode)


@pytest.mark.parametrize("mode,builder", [("refit", "host"), ("rebuild", "host"), ("rebuild", "device")])
def test_transform_equals_update_with_transformed_arrays(mode, builder):
    desc, a, b = pair(builder)
    start = dc.snapshot(b, desc, dc.PRIMS)
    for name in ("rotation+translation", "scale+shear", "projective"):
        for prim in dc.PRIMS:
            M = about(prim, MATRICES[name]) if name != "projective" else MATRICES[name]
            by_definition(a, prim, M, dc.zoo_arrays(prim), mode)
            b.transform_mesh(prim, M, mode)
        sa, sb = dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS)
        dc.assert_same(sa, sb)
        assert sb["render"] != start["render"]
    a.close()
    b.close()


def test_the_transform_is_absolute_and_the_identity_is_the_rest_pose():
    desc, a, b = pair()
    rest = dc.snapshot(a, desc, dc.PRIMS)
    prim = dc.GRID4_N
    M = about(prim, MATRICES["rotation+translation"])
    b.transform_mesh(prim, M)
    once = dc.snapshot(b, desc, dc.PRIMS)
    b.transform_mesh(prim, M)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), once)      # M twice = M once
    assert once["render"] != rest["render"]
    b.transform_mesh(prim, np.eye(4, dtype=F))
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)      # the identity: the rest pose again, not M's
    b.transform_mesh(prim, M, "rebuild")
    b.transform_mesh(prim, np.eye(4, dtype=F), "rebuild")     # (the rest pose outlives the rebuilt tree)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)
    a.close()
    b.close()


@pytest.mark.parametrize("through", ["host", "device"])
def test_an_explicit_update_resets_the_rest_pose(through):
    desc, a, b = pair()
    prim = dc.GRID1_N
    M = about(prim, MATRICES["scale+shear"])
    b.transform_mesh(prim, about(prim, MATRICES["rotation+translation"]))   # a rest pose is on the device already
    v, n = dc.zoo_arrays(prim, 2)
    if through == "host":
        b.update_mesh(prim, v, n)
    else:
        dc.update_through_device(b, prim, v, n)    # the new rest pose exists on the device only: the transform fetches it
    b.transform_mesh(prim, M)
    by_definition(a, prim, M, (v, n), "refit")
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_a_transform_in_a_seventy_primitive_scene_and_a_stale_mirror():
    desc, a, b = pair(desc=seventy_prims())
    prim = 7
    rest = desc.ops[3 + prim][1:3]
    M = np.eye(4, dtype=F)
    M[:3, 3] = [4.5, 3.0, -8.0]
    by_definition(a, prim, M, rest, "refit")
    b.transform_mesh(prim, M)
    dc.assert_same(dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim]))
    # a REBUILD of another mesh re-flattens every mesh from the mirror: the transformed pose must be in it
    w = desc.ops[3 + 20][1] * F(1.25)
    for g in (a, b):
        g.update_mesh(20, w, desc.ops[3 + 20][2], "rebuild")
    dc.assert_same(dc.snapshot(a, desc, [prim, 20]), dc.snapshot(b, desc, [prim, 20]))
    a.close()
    b.close()


def test_non_finite_transformed_positions_take_the_fallback():
    desc, a, b = pair()
    for prim in (dc.GRID1_N, dc.GRID4):
        v, n = dc.zoo_arrays(prim)
        M = SWAP_XW.copy()
        M[3, 3] = -np.float32(dc.ZOO[prim - 1][4][0])   # w = x - the mesh's offset: 0 on its middle column
        tv, _ = ag.transform_arrays(M, v, n)
        assert not np.isfinite(tv).all() and np.isfinite(tv).any()
        by_definition(a, prim, M, (v, n), "refit")
        b.transform_mesh(prim, M)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_refusals_change_nothing():
    ctx = gpu_context()
    g = ag.Scene(ctx)
    desc = dc.zoo_scene()
    L, fp = g.L, C.POINTER(C.c_float)
    eye = np.eye(4, dtype=F).reshape(16)
    pm = eye.ctypes.data_as(fp)

    def refused(what, *args):
        assert L.agpt_scene_transform_mesh(*args) == -1
        assert b"agpt_scene_transform_mesh" in L.agpt_last_error() and what in L.agpt_last_error(), L.agpt_last_error()
    refused(b"NULL", None, 1, pm, 0)
    refused(b"not committed", g.h, 1, None, 7)             # the scene's state before the matrix
    desc.instantiate(g)
    g.transform_mesh(dc.GRID1_N, about(dc.GRID1_N, MATRICES["scale+shear"]))
    before = dc.snapshot(g, desc, dc.PRIMS)
    for prim in (-1, len(dc.PRIMS) + 1, 99):
        refused(b"not a mesh", g.h, prim, None, 7)
    refused(b"unknown mode", g.h, dc.GRID1_N, None, 7)     # the mode before the matrix
    refused(b"NULL matrix", g.h, dc.GRID1_N, None, 0)
    for bad in (np.nan, np.inf):
        m = eye.copy()
        m[6] = bad
        refused(b"non-finite", g.h, dc.GRID1_N, m.ctypes.data_as(fp), 0)
    singular = np.array([[1, 2, 3, 0], [2, 4, 6, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F).reshape(16)
    for mode in (0, 1):
        refused(b"singular", g.h, dc.GRID1_N, singular.ctypes.data_as(fp), mode)
    with pytest.raises(ag.AgptError, match="singular"):
        g.transform_mesh(dc.GRID1_N, np.zeros((4, 4), F))
    dc.assert_same(dc.snapshot(g, desc, dc.PRIMS), before)
    g.close()


def test_cpp_rigid_example_matches_python(tmp_path):
    """examples/rigid_scene.cpp spins an octahedron over a backdrop with Scene::TransformMesh; the FNV-1a hashes it prints for its
    first and last frame are those of the same frames through the Python binding"""
    import re
    exe = build_cpp_example(tmp_path, "rigid_scene")
    frames, w, h, spp = 4, 32, 24, 4
    out = subprocess.run([exe, str(frames), str(w), str(h)], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {int(k): int(x, 16) for k, x in re.findall(r"frame (\d+) hash ([0-9a-f]{16})", out)}
    assert sorted(got) == list(range(frames)) and len(set(got.values())) == frames, out

    d = ag.SceneDesc("rigid")
    gold = d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], .4, 1.)
    floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
    d.add_mesh(*ag.create_backdrop([0, -1.5, 20], [40, 20, 40], 7.5, 8), floor, 1)
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1.5, 0], [0, -1.5, 0], [0, 0, 1], [0, 0, -1]], F)
    tris = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    t = np.asarray(tris, np.int32).reshape(-1)
    d.add_mesh(v, None, None, np.stack([t, t, t], 1), gold, 1)
    d.add_area_light([0, 25, -20], 1.0, [200., np.float32(.941) * np.float32(200), np.float32(.914) * np.float32(200)])
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], np.float32(w) / np.float32(h), 45.0, 0.0)
    g = gpu_scene(d)
    turns = [(1.0, 0.0), (0.8, 0.6), (0.28, 0.96), (-0.352, 0.936)]   # exact-ish (cos, sin) pairs, the literals of the example
    want = {}
    p = g.ctx.alloc(w * h * 16)
    try:
        for k in (0, frames - 1):
            c, s = (F(x) for x in turns[k % 4])
            M = np.array([[c, 0, s, 0], [0, 1, 0, F(0.25) * F(k)], [-s, 0, c, 0], [0, 0, 0, 1]], F)
            g.transform_mesh(1, M)
            acc, _ = ag.PathTracer(5).render_to_host(g, w, h, spp)
            g.ctx.upload(p, acc)
            want[k] = frame_hash(g.ctx.resolve(p, w * h, spp))
    finally:
        g.ctx.free(p)
        g.close()
    assert {k: got[k] for k in want} == want
