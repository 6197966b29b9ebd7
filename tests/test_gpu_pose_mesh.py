"""agpt_scene_pose_mesh on the GPU against its definition: scene A gets agpt_scene_update_mesh with the arrays of
agpt_skin_arrays(palette, rest pose, binding) -- the host twin that test_skin_arrays.py pins to the numpy model --, scene B the binding
and the pose call; BVH bytes, hit records and renders must be bit-identical (device_update_cases.snapshot)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_update_cases as dc
import skin_model
from device_update_cases import about, frame_hash, pair, palette, seventy_prims
from helpers import build_cpp_example, gpu_context, gpu_scene
from skin_cases import JOINTS3, binding, single_slot

pytestmark = pytest.mark.gpu
F = np.float32
EYE = np.eye(4, dtype=F)


def bound(g, prim, K=4, seed=None):
    J, W = binding(len(dc.zoo_arrays(prim)[0]), K, seed=prim if seed is None else seed)
    g.set_mesh_skin(prim, J, W, n_joints=3)
    return J, W


def by_definition(g, prim, mats, rest, J, W, mode="refit"):
    v, n = ag.skin_arrays(mats, rest[0], J, W, rest[1])
    g.update_mesh(prim, v, n, mode)


def pose_all(a, b, mode, pose, bindings):
    for prim in dc.PRIMS:
        by_definition(a, prim, palette(prim, pose), dc.zoo_arrays(prim), *bindings[prim], mode)
        b.pose_mesh(prim, palette(prim, pose), mode)


@pytest.mark.parametrize("mode,builder", [("refit", "host"), ("rebuild", "host"), ("rebuild", "device")])
def test_pose_equals_update_with_skinned_arrays(mode, builder):
    """all eight meshes of the zoo, K = 4, two poses in a row (the second finds rest pose and binding on the device)"""
    desc, a, b = pair(builder)
    start = dc.snapshot(b, desc, dc.PRIMS)
    bindings = {prim: bound(b, prim) for prim in dc.PRIMS}
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), start)        # a binding alone moves nothing
    for pose in (0, 1):
        pose_all(a, b, mode, pose, bindings)
        sa, sb = dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS)
        dc.assert_same(sa, sb)
        assert sb["render"] != start["render"]
        start = sb
    a.close()
    b.close()


def test_the_global_palette_route_writes_the_same_bytes(monkeypatch):
    """the case above (REFIT) with the palette staged in LDS on scene A and read from global memory on scene B"""
    desc, a, b = pair()
    for g in (a, b):
        for prim in dc.PRIMS:
            bound(g, prim)
    for pose in (0, 1):
        for prim in dc.PRIMS:
            a.pose_mesh(prim, palette(prim, pose))
        monkeypatch.setenv("AGPT_SKIN_GLOBAL_PALETTE", "1")
        for prim in dc.PRIMS:
            b.pose_mesh(prim, palette(prim, pose))
        monkeypatch.delenv("AGPT_SKIN_GLOBAL_PALETTE")
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_a_palette_too_large_for_lds():
    """4,096 joints (192 KiB of M alone: more than a CU's LDS), three of them used, at the ends and in the middle"""
    desc, a, b = pair()
    used = np.array([0, 2047, 4095], np.int32)
    for prim in (dc.GRID1_N, dc.GRID4, 3, 2):
        v, n = dc.zoo_arrays(prim)
        J, W = binding(len(v), 4, seed=prim)
        J = used[J]
        mats = np.tile(EYE, (4096, 1, 1))
        mats[used] = palette(prim, 0)
        b.set_mesh_skin(prim, J, W, n_joints=4096)
        b.pose_mesh(prim, mats)
        by_definition(a, prim, mats, (v, n), J, W)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


@pytest.mark.parametrize("prim,n_joints", [(dc.GRID4_N, 487), (dc.GRID4_N, 488), (dc.GRID1, 787), (dc.GRID1, 788)])
def test_palettes_on_either_side_of_the_lds_cap(prim, n_joints):
    """40 KiB: 487 joints of 84 B (a mesh with normals) and 787 of 52 B (one without) are the last that are staged, one more is read
    from global memory; three of the joints used, the first, the last and one between"""
    desc, a, b = pair()
    used = np.array([0, n_joints // 2, n_joints - 1], np.int32)
    v, n = dc.zoo_arrays(prim)
    J, W = binding(len(v), 4, seed=prim)
    J = used[J]
    mats = np.tile(EYE, (n_joints, 1, 1))
    mats[used] = palette(prim, 1)
    b.set_mesh_skin(prim, J, W, n_joints=n_joints)
    b.pose_mesh(prim, mats)
    by_definition(a, prim, mats, (v, n), J, W)
    dc.assert_same(dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim]))
    a.close()
    b.close()


def test_the_pose_is_absolute_and_shares_the_rest_pose_with_the_transform():
    desc, a, b = pair()
    rest = dc.snapshot(a, desc, dc.PRIMS)
    prim = dc.GRID4_N
    nv = len(dc.zoo_arrays(prim)[0])
    # one slot of weight 1 per vertex (any joint): the identity palette is then the rest pose bit for bit
    rs = np.random.RandomState(8)
    J = rs.randint(0, 3, (nv, 4)).astype(np.int32)
    W = np.zeros((nv, 4), F)
    W[np.arange(nv), rs.randint(0, 4, nv)] = 1
    b.set_mesh_skin(prim, J, W, n_joints=3)
    P, I3 = palette(prim, 0), np.stack([EYE] * 3)
    b.pose_mesh(prim, P)
    once = dc.snapshot(b, desc, dc.PRIMS)
    b.pose_mesh(prim, P)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), once)       # P twice = P once
    assert once["render"] != rest["render"]
    b.pose_mesh(prim, I3)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)       # the identity palette: the rest pose again, not P's
    b.transform_mesh(prim, about(prim, JOINTS3[1]))
    b.pose_mesh(prim, I3.reshape(3, 16))                       # (the other accepted shape)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)       # the transform did not become the rest pose
    b.pose_mesh(prim, P)
    b.transform_mesh(prim, EYE)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)       # nor did the pose
    a.close()
    b.close()


@pytest.mark.parametrize("through", ["host", "device"])
def test_an_explicit_update_resets_the_rest_pose_and_keeps_the_binding(through):
    desc, a, b = pair()
    prim = dc.GRID1_N
    J, W = bound(b, prim)
    b.pose_mesh(prim, palette(prim, 0))          # rest pose and binding are on the device already
    v, n = dc.zoo_arrays(prim, 2)
    if through == "host":
        b.update_mesh(prim, v, n)
    else:
        dc.update_through_device(b, prim, v, n)   # the new rest pose exists on the device only: the pose fetches it
    b.pose_mesh(prim, palette(prim, 1))
    by_definition(a, prim, palette(prim, 1), (v, n), J, W)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_a_pose_after_a_rebuild_uploads_the_binding_again():
    desc, a, b = pair()
    for prim in (dc.GRID4_N, 4):
        J, W = bound(b, prim)
        for pose, mode in ((0, "refit"), (1, "rebuild"), (0, "refit"), (1, "refit")):   # the REBUILD destroys the device cache
            b.pose_mesh(prim, palette(prim, pose), mode)
            by_definition(a, prim, palette(prim, pose), dc.zoo_arrays(prim), J, W, mode)
            dc.assert_same(dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim]))
    a.close()
    b.close()


def test_binding_again_replaces_the_binding():
    desc, a, b = pair()
    prim = dc.GRID1_N
    rest = dc.zoo_arrays(prim)
    bound(b, prim)
    b.pose_mesh(prim, palette(prim, 0))
    J, W = bound(b, prim, K=8, seed=77)          # other weights, and another size of the device copies
    b.pose_mesh(prim, palette(prim, 0))
    by_definition(a, prim, palette(prim, 0), rest, J, W)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    b.set_mesh_skin(prim, None, None)             # removed: the mesh stays as posed, and cannot be posed
    with pytest.raises(ag.AgptError, match="has no skin"):
        b.pose_mesh(prim, palette(prim, 1))
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_a_pose_in_a_seventy_primitive_scene_and_a_stale_mirror():
    desc, a, b = pair(desc=seventy_prims())
    prim = 7
    v, n = desc.ops[3 + prim][1:3]
    assert n is not None and len(n) == len(v)
    J, W = binding(len(v), 4, seed=70)
    mats = np.stack([EYE] * 3)
    mats[0, :3, 3] = [4.5, 3.0, -8.0]
    mats[1, :3, 3] = [4.0, 3.5, -8.0]
    mats[2, :3, 3] = [4.5, 2.5, -7.0]
    b.set_mesh_skin(prim, J, W)
    by_definition(a, prim, mats, (v, n), J, W)
    b.pose_mesh(prim, mats)
    dc.assert_same(dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim]))
    # a REBUILD of another mesh re-flattens every mesh from the mirror: the posed arrays must be in it
    w = desc.ops[3 + 20][1] * F(1.25)
    for g in (a, b):
        g.update_mesh(20, w, desc.ops[3 + 20][2], "rebuild")
    dc.assert_same(dc.snapshot(a, desc, [prim, 20]), dc.snapshot(b, desc, [prim, 20]))
    a.close()
    b.close()


def test_non_finite_posed_positions_take_the_fallback():
    """(the two grids of test_gpu_mesh_update_device's NaN case: with ten vertices of GRID1_N or GRID4 at +Inf instead, agpt_render gives
    up on a path that does not terminate -- after the host call as well, it is the scene's doing, not the update's)"""
    desc, a, b = pair()
    T = EYE.copy()
    T[0, 3] = 3e38
    mats = np.stack([EYE, T, T])
    for prim in (dc.GRID4_N, dc.GRID1):
        v, n = dc.zoo_arrays(prim)
        J, W = single_slot(len(v), 2, 0, (0,), 1.0)
        J[10:20], W[10:20] = (1, 2), (1, 1)        # x + 3e38 twice: +Inf, never NaN
        mv, mn = skin_model.skin_arrays(mats, v, J, W, n)
        assert np.isposinf(mv[10:20, 0]).all() and not np.isnan(mv).any() and np.isinf(mv).sum() == 10
        assert np.isfinite(np.delete(mv, np.s_[10:20], 0)).all() and (mn is None or np.isfinite(mn).all())
        tv, tn = ag.skin_arrays(mats, v, J, W, n)
        assert tv.tobytes() == mv.tobytes() and (tn is None or tn.tobytes() == mn.tobytes())
        b.set_mesh_skin(prim, J, W)
        by_definition(a, prim, mats, (v, n), J, W)
        b.pose_mesh(prim, mats)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_refusals_in_their_order_change_nothing():
    ctx = gpu_context()
    g = ag.Scene(ctx)
    desc = dc.zoo_scene()
    L, fp, ip = g.L, C.POINTER(C.c_float), C.POINTER(C.c_int32)
    prim = dc.GRID1_N
    good = palette(prim, 0).reshape(48)
    pm = good.ctypes.data_as(fp)

    def refused(what, *args):
        assert L.agpt_scene_pose_mesh(*args) == -1
        assert b"agpt_scene_pose_mesh" in L.agpt_last_error() and what in L.agpt_last_error(), L.agpt_last_error()
    refused(b"NULL", None, 1, pm, 3, 0)
    refused(b"not committed", g.h, 1, None, 3, 7)            # the scene's state before everything else
    desc.instantiate(g)
    for p in (-1, len(dc.PRIMS) + 1, 99):
        refused(b"not a mesh", g.h, p, None, 3, 7)
    refused(b"unknown mode", g.h, prim, None, 3, 7)          # the mode before the skin
    refused(b"has no skin", g.h, prim, None, 2, 0)           # the skin before the matrices
    J, W = bound(g, prim)
    g.pose_mesh(prim, good.reshape(3, 16))
    before = dc.snapshot(g, desc, dc.PRIMS)
    nan = good.copy()
    nan[16 + 6] = np.nan
    nan[15] = 2                                               # (and a bad last row in joint 0)
    refused(b"NULL joints16", g.h, prim, None, 2, 0)         # NULL before the count
    refused(b"n_joints is 2, the skin was set with 3", g.h, prim, nan.ctypes.data_as(fp), 2, 0)   # the count before the entries
    refused(b"joint 1 has a non-finite entry", g.h, prim, nan.ctypes.data_as(fp), 3, 0)           # non-finite before the last row
    inf = good.copy()
    inf[32 + 3] = np.inf
    refused(b"joint 2 has a non-finite entry", g.h, prim, inf.ctypes.data_as(fp), 3, 0)
    singular = np.array([[1, 2, 3, 0], [2, 4, 6, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F).reshape(16)
    row = good.copy()
    row[0:16] = singular
    row[32 + 12] = 1e-30
    refused(b"the last row of joint 2 is not (0, 0, 0, 1)", g.h, prim, row.ctypes.data_as(fp), 3, 0)   # the last row before the determinant
    sing = good.copy()
    sing[16:32] = singular
    for mode in (0, 1):
        refused(b"joint 1 is singular", g.h, prim, sing.ctypes.data_as(fp), 3, mode)
    with pytest.raises(ag.AgptError, match="joint 0 is singular"):
        g.pose_mesh(prim, np.stack([np.diag([0, 0, 0, 1]).astype(F)] * 3))
    # a refused binding leaves the binding
    def unbound(what, K, n_joints, J, W):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)   # noqa: E731
        assert L.agpt_scene_set_mesh_skin(g.h, prim, K, n_joints, p(J, ip), p(W, fp), None, None) == -1
        assert b"agpt_scene_set_mesh_skin" in L.agpt_last_error() and what in L.agpt_last_error(), L.agpt_last_error()
    unbound(b"outside 1 .. 8", 9, 3, J, W)
    unbound(b"outside 1 .. 65536", 4, 0, J, W)
    unbound(b"NULL vertex_joints", 4, 3, None, W)
    unbound(b"joint index 2 out of range", 4, 2, J, W)
    Wb = W.copy()
    Wb[5, 2] = -1
    unbound(b"negative weight (vertex 5, slot 2)", 4, 3, J, Wb)
    assert L.agpt_scene_set_mesh_skin(None, prim, 4, 3, None, None, None, None) == -1
    assert L.agpt_scene_set_mesh_skin(g.h, len(dc.PRIMS) + 1, 4, 3, J.ctypes.data_as(ip), W.ctypes.data_as(fp), None, None) == -1   # the light
    assert L.agpt_scene_set_mesh_skin(g.h, 99, 4, 3, J.ctypes.data_as(ip), W.ctypes.data_as(fp), None, None) == -1
    dc.assert_same(dc.snapshot(g, desc, dc.PRIMS), before)
    g.pose_mesh(prim, good.reshape(3, 16))                                    # the binding of before
    dc.assert_same(dc.snapshot(g, desc, dc.PRIMS), before)
    g.close()


def test_cpp_skinned_example_matches_python(tmp_path):
    """examples/skinned_scene.cpp bends a two-joint strip over a backdrop with Scene::SetMeshSkin / PoseMesh; the FNV-1a hashes it
    prints for its first and last frame are those of the same frames through the Python binding"""
    exe = build_cpp_example(tmp_path, "skinned_scene")
    frames, w, h, spp = 4, 32, 24, 4
    out = subprocess.run([exe, str(frames), str(w), str(h)], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {int(k): int(x, 16) for k, x in re.findall(r"frame (\d+) hash ([0-9a-f]{16})", out)}
    assert sorted(got) == list(range(frames)) and len(set(got.values())) == frames, out

    d = ag.SceneDesc("skinned")
    red = d.add_material(ag.MAT_DISNEY, [0.8, 0.1, 0.12], .6, 0.)
    floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
    d.add_mesh(*ag.create_backdrop([0, -1.5, 20], [40, 20, 40], 7.5, 8), floor, 1)
    i = np.repeat(np.arange(17), 2)
    v = np.stack([F(0.25) * i.astype(F) - F(2), np.zeros(34, F), np.tile(np.array([-0.5, 0.5], F), 17)], 1).astype(F)
    n = np.tile(np.array([0, 1, 0], F), (34, 1))
    t = (i.astype(F) / F(16)).astype(F)
    J, W = np.tile(np.array([0, 1], np.int32), (34, 1)), np.stack([F(1) - t, t], 1).astype(F)
    corners = np.concatenate([[2 * k, 2 * k + 1, 2 * k + 2, 2 * k + 1, 2 * k + 3, 2 * k + 2] for k in range(16)]).astype(np.int32)
    d.add_mesh(v, n, None, np.stack([corners, corners, np.full_like(corners, -1)], 1), red, 1)
    d.add_area_light([0, 25, -20], 1.0, [200., np.float32(.941) * np.float32(200), np.float32(.914) * np.float32(200)])
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 2.16, -5.64], [0, 0.5, 0], [0, 1, 0], np.float32(w) / np.float32(h), 45.0, 0.0)
    g = gpu_scene(d)
    g.set_mesh_skin(1, J, W)
    turns = [(1.0, 0.0), (0.96, 0.28), (0.8, 0.6), (0.6, 0.8)]   # the literals of the example
    want = {}
    p = g.ctx.alloc(w * h * 16)
    try:
        for k in (0, frames - 1):
            c, s = (F(x) for x in turns[k % 4])
            M = np.array([[c, -s, 0, 0], [s, c, 0, F(0.125) * F(k)], [0, 0, 1, 0], [0, 0, 0, 1]], F)
            g.pose_mesh(1, np.stack([EYE, M]))
            acc, _ = ag.PathTracer(5).render_to_host(g, w, h, spp)
            g.ctx.upload(p, acc)
            want[k] = frame_hash(g.ctx.resolve(p, w * h, spp))
    finally:
        g.ctx.free(p)
        g.close()
    assert {k: got[k] for k in want} == want
