"""agpt_scene_morph_mesh on the GPU against its definition: scene A gets agpt_scene_update_mesh with the arrays of
agpt_morph_arrays(weights, rest pose, targets) -- through agpt_skin_arrays as well when the call brings joints --, the host twins that
test_morph_arrays.py and test_skin_arrays.py pin to the numpy models; scene B gets the targets and the morph call.  BVH bytes, hit
records and renders must be bit-identical (device_update_cases.snapshot)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_update_cases as dc
import morph_model
from device_update_cases import (BIG, FLAT, about, arrays_of, big_scene, frame_hash, joints_of, morph_targets, pair, palette, seventy_prims,
                                 skin_of)
from helpers import build_cpp_example, gpu_context, gpu_scene
from morph_cases import targets, weights
from skin_cases import binding
from test_gpu_streams import MOVED, Stage, assert_rays_through_updated_scene, twin_scene
from transform_cases import MATRICES

pytestmark = pytest.mark.gpu
F = np.float32
EYE = np.eye(4, dtype=F)
def by_definition(g, prim, w, rest, dP, dN, mode="refit", mats=None, skin=None):
    v, n = ag.morph_arrays(w, rest[0], dP, rest[1], dN)
    if mats is not None:
        v, n = ag.skin_arrays(mats, v, *skin[:2], n, *skin[2:])
    g.update_mesh(prim, v, n, mode)


WEIGHT_SETS = ([0, 2], [0, 1, 2])      # the first leaves the all-zero target idle (its weight is -0.0), the second uses it


@pytest.mark.parametrize("mode,builder", [("refit", "host"), ("rebuild", "host"), ("rebuild", "device")])
def test_morph_equals_update_with_morphed_arrays(mode, builder):
    """all eight meshes of the zoo, T = 3, two weight sets in a row (the second finds rest pose and deltas on the device)"""
    desc, a, b = pair(builder)
    start = dc.snapshot(b, desc, dc.PRIMS)
    tg = {prim: morph_targets(b, prim) for prim in dc.PRIMS}
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), start)        # targets alone move nothing
    for k, act in enumerate(WEIGHT_SETS):
        for prim in dc.PRIMS:
            w = weights(3, prim + k, act)
            by_definition(a, prim, w, dc.zoo_arrays(prim), *tg[prim], mode)
            b.morph_mesh(prim, w, mode=mode)
        sa, sb = dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS)
        dc.assert_same(sa, sb)
        assert sb["render"] != start["render"]
        start = sb
    a.close()
    b.close()


@pytest.mark.parametrize("route", ["lds", "global"])
@pytest.mark.parametrize("mode,builder", [("refit", "host"), ("rebuild", "host"), ("rebuild", "device")])
def test_fused_morph_equals_update_with_morphed_and_skinned_arrays(mode, builder, route, monkeypatch):
    """the same with a skin (K = 4, three joints): morph, then skin, the palette staged in LDS or read from global memory"""
    desc, a, b = pair(builder)
    start = dc.snapshot(b, desc, dc.PRIMS)
    tg = {prim: morph_targets(b, prim) for prim in dc.PRIMS}
    skins = {prim: skin_of(b, prim) for prim in dc.PRIMS}
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), start)
    if route == "global":
        monkeypatch.setenv("AGPT_SKIN_GLOBAL_PALETTE", "1")
    for k, act in enumerate(WEIGHT_SETS):
        for prim in dc.PRIMS:
            w = weights(3, prim + k, act)
            by_definition(a, prim, w, dc.zoo_arrays(prim), *tg[prim], mode, palette(prim, k), skins[prim])
            b.morph_mesh(prim, w, palette(prim, k), mode)
        sa, sb = dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS)
        dc.assert_same(sa, sb)
        assert sb["render"] != start["render"]
        start = sb
    a.close()
    b.close()


def test_fused_with_a_palette_just_over_the_staging_cap():
    """488 joints of 84 B for a mesh with normals: one more than the LDS route takes; the first, the last and one between are used"""
    desc, a, b = pair()
    prim, n_joints = dc.GRID4_N, 488
    used = np.array([0, n_joints // 2, n_joints - 1], np.int32)
    v, n = dc.zoo_arrays(prim)
    J, W = binding(len(v), 4, seed=prim)
    J = used[J]
    mats = np.tile(EYE, (n_joints, 1, 1))
    mats[used] = palette(prim, 1)
    dP, dN = morph_targets(b, prim)
    b.set_mesh_skin(prim, J, W, n_joints=n_joints)
    w = weights(3, 5, [0, 2])
    b.morph_mesh(prim, w, mats)
    by_definition(a, prim, w, (v, n), dP, dN, "refit", mats, (J, W, None, None))
    dc.assert_same(dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim]))
    a.close()
    b.close()


@pytest.mark.parametrize("T,act", [(300, [0, 150, 299]), (1, [0])])
def test_the_ends_of_the_delta_buffers(T, act):
    desc, a, b = pair()
    for prim in (dc.GRID1_N, dc.GRID4, 3):
        dP, dN = morph_targets(b, prim, T)
        w = weights(T, prim, act)
        by_definition(a, prim, w, dc.zoo_arrays(prim), dP, dN)
        b.morph_mesh(prim, w)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


@pytest.mark.parametrize("fused", [False, True])
def test_a_capped_grid_walks_the_stride_loop(fused, monkeypatch):
    """AGPT_MORPH_MAX_BLOCKS = 1 and 2 on the 170-vertex grid (2 blocks of items with its normals) and the 1,089-vertex one (8.5
    blocks): the bytes of the uncapped call, which are those of the definition"""
    desc, a, b = pair(desc=big_scene())
    prims = (dc.GRID4_N, BIG)
    tg = {prim: morph_targets(b, prim) for prim in prims}
    skins = {prim: skin_of(b, prim) for prim in prims} if fused else {}
    w = weights(3, 3, [0, 1, 2])
    for prim in prims:
        mats = joints_of(prim, 0) if fused else None
        by_definition(a, prim, w, arrays_of(prim), *tg[prim], "refit", mats, skins.get(prim))
        b.morph_mesh(prim, w, mats)
    want = dc.snapshot(a, desc, prims)
    uncapped = dc.snapshot(b, desc, prims)
    dc.assert_same(want, uncapped)
    for cap in ("1", "2"):
        for prim in prims:
            b.morph_mesh(prim, np.zeros(3, F))                   # (away from the pose, so that the capped call has to write it)
        assert dc.snapshot(b, desc, prims)["render"] != want["render"]
        monkeypatch.setenv("AGPT_MORPH_MAX_BLOCKS", cap)
        for prim in prims:
            b.morph_mesh(prim, w, joints_of(prim, 0) if fused else None)
        monkeypatch.delenv("AGPT_MORPH_MAX_BLOCKS")
        dc.assert_same(dc.snapshot(b, desc, prims), want)
    a.close()
    b.close()


def test_normals_without_normal_deltas_keep_their_rest_values():
    desc, a, b = pair()
    for prim in (dc.GRID1_N, 3):
        dP, dN = morph_targets(b, prim, normal_deltas=False)
        assert dN is None and dc.zoo_arrays(prim)[1] is not None
        w = weights(3, 1, [0, 2])
        by_definition(a, prim, w, dc.zoo_arrays(prim), dP, None)
        b.morph_mesh(prim, w)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


@pytest.mark.parametrize("fused", [False, True])
def test_normals_with_a_count_and_influences_of_their_own(fused):
    desc, a, b = pair(desc=big_scene())
    v, n = arrays_of(FLAT)
    assert len(n) == 288 != len(v) == 170
    dP, dN = morph_targets(b, FLAT)
    skin = skin_of(b, FLAT) if fused else None
    assert not fused or skin[2] is not None
    mats = joints_of(FLAT, 1) if fused else None
    start = dc.snapshot(b, desc, [FLAT])
    for act in WEIGHT_SETS:
        w = weights(3, 2, act)
        by_definition(a, FLAT, w, (v, n), dP, dN, "refit", mats, skin)
        b.morph_mesh(FLAT, w, mats)
        sb = dc.snapshot(b, desc, [FLAT])
        dc.assert_same(dc.snapshot(a, desc, [FLAT]), sb)
        assert sb["render"] != start["render"]
    a.close()
    b.close()


def test_the_morph_is_absolute_and_shares_the_rest_pose():
    desc, a, b = pair()
    rest = dc.snapshot(a, desc, dc.PRIMS)
    prim = dc.GRID4_N
    nv = len(dc.zoo_arrays(prim)[0])
    morph_targets(b, prim)
    w, zero = weights(3, 1, [0, 1, 2]), np.zeros(3, F)
    b.morph_mesh(prim, w)
    once = dc.snapshot(b, desc, dc.PRIMS)
    b.morph_mesh(prim, w)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), once)       # w twice = w once
    assert once["render"] != rest["render"]
    b.morph_mesh(prim, zero)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)       # all weights zero: the rest pose again
    b.transform_mesh(prim, about(prim, MATRICES["rotation+translation"]))
    b.morph_mesh(prim, np.array([0, -0.0, 0], F))
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)       # the transform did not become the rest pose
    J = np.zeros((nv, 4), np.int32)
    W = np.zeros((nv, 4), F)
    W[:, 1] = 1                                                 # one slot of weight 1: the identity palette is the rest pose
    b.set_mesh_skin(prim, J, W, n_joints=3)
    b.morph_mesh(prim, w)
    b.pose_mesh(prim, np.stack([EYE] * 3))
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)       # nor did the morph
    b.morph_mesh(prim, w)
    b.transform_mesh(prim, EYE)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)
    b.morph_mesh(prim, w, np.stack([EYE] * 3))                  # fused with the identity palette: the morph alone
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), once)
    a.close()
    b.close()


@pytest.mark.parametrize("through", ["host", "device"])
def test_an_explicit_update_resets_the_rest_pose_and_keeps_the_targets(through):
    desc, a, b = pair()
    prim = dc.GRID1_N
    dP, dN = morph_targets(b, prim)
    b.morph_mesh(prim, weights(3, 1, [0, 2]))    # rest pose and deltas are on the device already
    v, n = dc.zoo_arrays(prim, 2)
    if through == "host":
        b.update_mesh(prim, v, n)
    else:
        dc.update_through_device(b, prim, v, n)   # the new rest pose exists on the device only: the morph fetches it
    w = weights(3, 2, [0, 1, 2])
    b.morph_mesh(prim, w)
    by_definition(a, prim, w, (v, n), dP, dN)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


@pytest.mark.parametrize("fused", [False, True])
def test_a_morph_after_a_rebuild_uploads_the_deltas_again(fused):
    desc, a, b = pair()
    for prim in (dc.GRID4_N, 4):
        dP, dN = morph_targets(b, prim)
        skin = skin_of(b, prim) if fused else None
        for k, mode in ((0, "refit"), (1, "rebuild"), (2, "refit"), (3, "refit")):   # the REBUILD destroys the device cache
            w = weights(3, k, WEIGHT_SETS[k % 2])
            mats = palette(prim, k % 2) if fused else None
            b.morph_mesh(prim, w, mats, mode)
            by_definition(a, prim, w, dc.zoo_arrays(prim), dP, dN, mode, mats, skin)
            dc.assert_same(dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim]))
    a.close()
    b.close()


def test_setting_targets_again_replaces_them():
    desc, a, b = pair()
    prim = dc.GRID1_N
    rest = dc.zoo_arrays(prim)
    morph_targets(b, prim)
    b.morph_mesh(prim, weights(3, 1, [0, 2]))
    dP, dN = morph_targets(b, prim, T=5, seed=77)          # other deltas, and another size of the device copies
    w = weights(5, 3, [1, 3, 4])
    b.morph_mesh(prim, w)
    by_definition(a, prim, w, rest, dP, dN)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    with pytest.raises(ag.AgptError, match="n_targets is 3, the targets were set with 5"):
        b.morph_mesh(prim, weights(3, 1, [0]))
    b.set_mesh_morph_targets(prim, None)                    # removed: the mesh stays as morphed, and cannot be morphed
    with pytest.raises(ag.AgptError, match="has no morph targets"):
        b.morph_mesh(prim, w)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_a_morph_in_a_seventy_primitive_scene_and_a_stale_mirror():
    desc, a, b = pair(desc=seventy_prims())
    prim = 7
    v, n = desc.ops[3 + prim][1:3]
    assert n is not None and len(n) == len(v)
    dP, dN = targets(len(v), 3, 70, extent=3.0), targets(len(n), 3, 71, extent=5.0)
    b.set_mesh_morph_targets(prim, dP, dN)
    w = weights(3, 7, [0, 2])
    before = dc.snapshot(b, desc, [prim])
    by_definition(a, prim, w, (v, n), dP, dN)
    b.morph_mesh(prim, w)
    sb = dc.snapshot(b, desc, [prim])
    dc.assert_same(dc.snapshot(a, desc, [prim]), sb)
    assert sb["render"] != before["render"]
    # a REBUILD of another mesh re-flattens every mesh from the mirror: the morphed arrays must be in it
    u = desc.ops[3 + 20][1] * F(1.25)
    for g in (a, b):
        g.update_mesh(20, u, desc.ops[3 + 20][2], "rebuild")
    dc.assert_same(dc.snapshot(a, desc, [prim, 20]), dc.snapshot(b, desc, [prim, 20]))
    a.close()
    b.close()


def test_non_finite_morphed_positions_take_the_fallback():
    """(the two grids of test_gpu_pose_mesh's case, for its reason: with +Inf vertices on the nearer grids agpt_render gives up on a path
    that does not terminate, after the host update call as well)"""
    desc, a, b = pair()
    w = np.ones(2, F)
    for prim in (dc.GRID4_N, dc.GRID1):
        v, n = dc.zoo_arrays(prim)
        dP = np.zeros((2, len(v), 3), F)
        dP[:, 10:20, 0] = 3e38                      # x + 3e38 twice: +Inf, never NaN
        dN = None if n is None else np.zeros((2, len(n), 3), F)
        mv, mn = morph_model.morph_arrays(w, v, dP, n, dN)
        assert np.isposinf(mv[10:20, 0]).all() and not np.isnan(mv).any() and np.isinf(mv).sum() == 10
        assert np.isfinite(np.delete(mv, np.s_[10:20], 0)).all() and (mn is None or np.isfinite(mn).all())
        tv, tn = ag.morph_arrays(w, v, dP, n, dN)
        assert tv.tobytes() == mv.tobytes() and (tn is None or tn.tobytes() == mn.tobytes())
        b.set_mesh_morph_targets(prim, dP, dN)
        by_definition(a, prim, w, (v, n), dP, dN)
        b.morph_mesh(prim, w)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_refusals_in_their_order_change_nothing():
    ctx = gpu_context()
    g = ag.Scene(ctx)
    desc = dc.zoo_scene()
    L, fp = g.L, C.POINTER(C.c_float)
    prim = dc.GRID1_N
    w3 = weights(3, 1, [0, 2])
    pw = w3.ctypes.data_as(fp)
    good = palette(prim, 0).reshape(48)
    pm = good.ctypes.data_as(fp)

    def refused(what, *args):
        assert L.agpt_scene_morph_mesh(*args) == -1
        assert b"agpt_scene_morph_mesh" in L.agpt_last_error() and what in L.agpt_last_error(), L.agpt_last_error()
    refused(b"NULL", None, 1, pw, 3, None, 0, 0)
    refused(b"not committed", g.h, 1, None, 2, None, 0, 7)           # the scene's state before everything else
    desc.instantiate(g)
    for p in (-1, len(dc.PRIMS) + 1, 99):
        refused(b"not a mesh", g.h, p, None, 2, None, 0, 7)
    refused(b"unknown mode", g.h, prim, None, 2, None, 0, 7)         # the mode before the targets
    refused(b"has no morph targets", g.h, prim, None, 2, pm, 2, 0)   # the targets before the weights
    dP, dN = morph_targets(g, prim)
    g.morph_mesh(prim, w3)
    before = dc.snapshot(g, desc, dc.PRIMS)
    nan = w3.copy()
    nan[1] = np.nan
    pn = nan.ctypes.data_as(fp)
    refused(b"NULL weights", g.h, prim, None, 2, pm, 2, 0)           # NULL before the count
    refused(b"n_targets is 2, the targets were set with 3", g.h, prim, pn, 2, pm, 2, 0)   # the count before the values
    refused(b"non-finite weight (target 1)", g.h, prim, pn, 3, pm, 2, 0)                  # the weights before the skin
    inf = w3.copy()
    inf[2] = -np.inf
    refused(b"non-finite weight (target 2)", g.h, prim, inf.ctypes.data_as(fp), 3, None, 0, 0)
    # with joints16: agpt_scene_pose_mesh's remaining checks, in its order
    bad = good.copy()
    bad[16 + 6] = np.nan
    bad[15] = 2                                                       # (and a bad last row in joint 0)
    pb = bad.ctypes.data_as(fp)
    refused(b"has no skin", g.h, prim, pw, 3, pb, 2, 0)               # the skin before the matrices
    J, W = binding(len(dc.zoo_arrays(prim)[0]), 4, seed=prim)
    g.set_mesh_skin(prim, J, W, n_joints=3)
    refused(b"n_joints is 2, the skin was set with 3", g.h, prim, pw, 3, pb, 2, 0)       # the count before the entries
    refused(b"joint 1 has a non-finite entry", g.h, prim, pw, 3, pb, 3, 0)               # non-finite before the last row
    singular = np.array([[1, 2, 3, 0], [2, 4, 6, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F).reshape(16)
    row = good.copy()
    row[0:16] = singular
    row[32 + 12] = 1e-30
    refused(b"the last row of joint 2 is not (0, 0, 0, 1)", g.h, prim, pw, 3, row.ctypes.data_as(fp), 3, 0)   # the last row before the determinant
    sing = good.copy()
    sing[16:32] = singular
    for mode in (0, 1):
        refused(b"joint 1 is singular", g.h, prim, pw, 3, sing.ctypes.data_as(fp), 3, mode)
    refused(b"non-finite weight (target 1)", g.h, prim, pn, 3, sing.ctypes.data_as(fp), 3, 0)   # the morph's checks before the skin's
    g.morph_mesh(prim, w3)                                            # joints16 NULL: n_joints is ignored, the skin not asked for
    assert L.agpt_scene_morph_mesh(g.h, prim, pw, 3, None, 99, 0) == 0

    # a refused set leaves the targets
    def unset(what, T, dP, dN=None, scene=g.h, p=prim):
        q = lambda x: None if x is None else x.ctypes.data_as(fp)   # noqa: E731
        assert L.agpt_scene_set_mesh_morph_targets(scene, p, T, q(dP), q(dN)) == -1
        assert b"agpt_scene_set_mesh_morph_targets" in L.agpt_last_error() and what in L.agpt_last_error(), L.agpt_last_error()
    unset(b"NULL scene", 3, dP, scene=None)
    for p in (len(dc.PRIMS) + 1, 99, -1):
        unset(b"is not a mesh", 3, dP, p=p)
    unset(b"n_targets is 4097, outside 1 .. 4096", 4097, dP)
    unset(b"n_targets is -1, outside 1 .. 4096", -1, dP)
    unset(b"NULL position_deltas", 3, None)
    db = dP.copy()
    db[2, 5, 1] = np.inf
    unset(b"non-finite position delta (target 2, vertex 5)", 3, db, dN)
    db = dN.copy()
    db[0, 7, 0] = np.nan
    unset(b"non-finite normal delta (target 0, normal 7)", 3, dP, db)
    dc.assert_same(dc.snapshot(g, desc, dc.PRIMS), before)
    g.morph_mesh(prim, w3)                                            # the targets of before
    dc.assert_same(dc.snapshot(g, desc, dc.PRIMS), before)
    g.close()


def test_morph_mesh_on_a_non_blocking_stream():
    """one morph and one fused morph per mesh on a context bound to a caller's non-blocking stream, behind test_gpu_streams' delay: the
    first call of a mesh uploads rest pose, deltas and (fused) binding, the second finds them"""
    desc = dc.zoo_scene()
    with Stage() as st, twin_scene(desc) as a:
        b = st.scene(desc)
        tg, skins = {}, {}
        for prim in MOVED:
            tg[prim] = morph_targets(b, prim)
            skins[prim] = skin_of(b, prim)
        arrays = {}
        for k, fused in enumerate((False, True)):
            for prim in MOVED:
                w = weights(3, prim + k, WEIGHT_SETS[k])
                mats = palette(prim, k) if fused else None
                rest = dc.zoo_arrays(prim)
                v, n = ag.morph_arrays(w, rest[0], tg[prim][0], rest[1], tg[prim][1])
                if fused:
                    v, n = ag.skin_arrays(mats, v, *skins[prim][:2], n)
                arrays[prim] = (v, n)
                a.update_mesh(prim, v, n, "refit")
                st.open()
                st.call("morph_mesh prim %d fused %d" % (prim, fused), b.morph_mesh, prim, w, mats, "refit")
            dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        assert_rays_through_updated_scene(st, b, arrays, False)


def test_cpp_morphed_example_matches_python(tmp_path):
    """examples/morphed_scene.cpp drives two targets of a two-joint strip over a backdrop with Scene::SetMeshMorphTargets / MorphMesh;
    the FNV-1a hashes it prints for its first frame (morph only) and its last (fused) are those of the same frames through the Python
    binding"""
    exe = build_cpp_example(tmp_path, "morphed_scene")
    frames, w, h, spp = 4, 32, 24, 4
    out = subprocess.run([exe, str(frames), str(w), str(h)], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {int(k): int(x, 16) for k, x in re.findall(r"frame (\d+) hash ([0-9a-f]{16})", out)}
    assert sorted(got) == list(range(frames)) and len(set(got.values())) == frames, out

    d = ag.SceneDesc("morphed")
    red = d.add_material(ag.MAT_DISNEY, [0.8, 0.1, 0.12], .6, 0.)
    floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
    d.add_mesh(*ag.create_backdrop([0, -1.5, 20], [40, 20, 40], 7.5, 8), floor, 1)
    i = np.repeat(np.arange(17), 2)
    side = np.tile(np.array([-1, 1], F), 17)
    v = np.stack([F(0.25) * i.astype(F) - F(2), np.zeros(34, F), F(0.5) * side], 1).astype(F)
    n = np.tile(np.array([0, 1, 0], F), (34, 1))
    t = (i.astype(F) / F(16)).astype(F)
    J, W = np.tile(np.array([0, 1], np.int32), (34, 1)), np.stack([F(1) - t, t], 1).astype(F)
    dP, dN = np.zeros((2, 34, 3), F), np.zeros((2, 34, 3), F)
    dP[0, :, 1] = F(0.75) * (F(1) - np.abs(i - 8).astype(F) / F(8))
    dN[0, :, 0] = F(0.375) * np.sign(i - 8).astype(F)
    dP[1, :, 1] = F(0.5) * side * t
    dN[1, :, 2] = F(-0.5) * t
    corners = np.concatenate([[2 * k, 2 * k + 1, 2 * k + 2, 2 * k + 1, 2 * k + 3, 2 * k + 2] for k in range(16)]).astype(np.int32)
    d.add_mesh(v, n, None, np.stack([corners, corners, np.full_like(corners, -1)], 1), red, 1)
    d.add_area_light([0, 25, -20], 1.0, [200., np.float32(.941) * np.float32(200), np.float32(.914) * np.float32(200)])
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 2.16, -5.64], [0, 0.5, 0], [0, 1, 0], np.float32(w) / np.float32(h), 45.0, 0.0)
    g = gpu_scene(d)
    g.set_mesh_morph_targets(1, dP, dN)
    g.set_mesh_skin(1, J, W)
    morphs = [(0.5, 0.0), (1.0, 0.25), (0.75, 0.5), (-0.25, 1.0)]   # the literals of the example
    turns = [None, None, (0.96, 0.28), (0.8, 0.6)]
    want = {}
    p = g.ctx.alloc(w * h * 16)
    try:
        for k in (0, frames - 1):
            mats = None
            if turns[k]:
                c, s = (F(x) for x in turns[k])
                mats = np.stack([EYE, np.array([[c, -s, 0, 0], [s, c, 0, F(0.125) * F(k)], [0, 0, 1, 0], [0, 0, 0, 1]], F)])
            g.morph_mesh(1, np.array(morphs[k], F), mats)
            acc, _ = ag.PathTracer(5).render_to_host(g, w, h, spp)
            g.ctx.upload(p, acc)
            want[k] = frame_hash(g.ctx.resolve(p, w * h, spp))
    finally:
        g.ctx.free(p)
        g.close()
    assert {k: got[k] for k in want} == want
