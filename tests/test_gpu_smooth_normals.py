"""AGPT_NORMALS_SMOOTH on the GPU against its definition: scene A takes agpt_scene_update_mesh in GIVEN mode with the call's positions V
and N = agpt_vertex_normals_arrays(V, the mesh's indices) -- the host twin that test_vertex_normals_arrays.py pins to the numpy model --;
scene B is in SMOOTH mode and takes the call itself.  BVH bytes, hit records and renders must be bit-identical
(device_update_cases.snapshot)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_update_cases as dc
import normals_cases as nc
from device_update_cases import BIG, FLAT, about, arrays_of, big_scene, frame_hash, joints_of, morph_targets, pair, seventy_prims, skin_of
from helpers import build_cpp_example, gpu_context, gpu_scene, oracle_render
from morph_cases import weights
from test_gpu_streams import Stage, assert_rays_through_updated_scene, posed_zoo, twin_scene
from transform_cases import MATRICES

pytestmark = pytest.mark.gpu
F = np.float32
EYE = np.eye(4, dtype=F)
SMOOTH = nc.ZOO_WITH_NORMALS
FRONT_ENDS = ("update", "device", "transform", "pose", "morph", "fused")
MODES = [("refit", "host"), ("rebuild", "host"), ("rebuild", "device")]
MATS = ("rotation+translation", "scale+shear")


def corners_of(prim):
    if prim == BIG:
        return dc.big_grid()[2]
    if prim == FLAT:
        return dc.flat_grid()[2]
    _, make, wn, _, _ = dc.ZOO[prim - 1]
    return make(wn)[2]


def twin(prim, V):
    return ag.vertex_normals_arrays(V, corners_of(prim), len(arrays_of(prim)[1]))


def smooth(g, prims):
    for prim in prims:
        g.set_mesh_normals_mode(prim, "smooth")


def garbage(prim):
    return np.full((len(arrays_of(prim)[1]), 3), np.nan, F)


class Driver:
    """one front end on scene b: what it binds once, and call k of mesh prim -> the positions V the call stands for"""

    def __init__(self, b, front, prims, normal_deltas=True):
        self.b, self.front = b, front
        self.tg = {p: morph_targets(b, p, normal_deltas=normal_deltas) for p in prims} if front in ("morph", "fused") else {}
        self.skins = {p: skin_of(b, p) for p in prims} if front in ("pose", "fused") else {}

    def positions(self, prim, k):
        front = self.front
        rv, rn = arrays_of(prim)
        if front in ("update", "device"):
            return dc.zoo_arrays(prim, 1 + k)[0]
        if front == "transform":
            return ag.transform_arrays(about(prim, MATRICES[MATS[k]]), rv, rn)[0]
        v, n = rv, rn
        if front in ("morph", "fused"):
            v, n = ag.morph_arrays(weights(3, prim + k, [0, 2] if k == 0 else [0, 1, 2]), rv, self.tg[prim][0], rn, self.tg[prim][1])
        if front in ("pose", "fused"):
            v = ag.skin_arrays(joints_of(prim, k), v, *self.skins[prim][:2], n, *self.skins[prim][2:])[0]
        return v

    def call(self, prim, k, mode, V):
        b, front = self.b, self.front
        if front == "update":
            b.update_mesh(prim, V, garbage(prim) if k else None, mode)          # NULL, then an array that must be ignored
        elif front == "device":
            d = dc.DeviceArrays(b.ctx, V, garbage(prim) if k else None)
            try:
                b.update_mesh_device(prim, d.pv, len(V), d.pn, len(arrays_of(prim)[1]), mode)
            finally:
                d.free()
        elif front == "transform":
            b.transform_mesh(prim, about(prim, MATRICES[MATS[k]]), mode)
        elif front == "pose":
            b.pose_mesh(prim, joints_of(prim, k), mode)
        else:
            w = weights(3, prim + k, [0, 2] if k == 0 else [0, 1, 2])
            b.morph_mesh(prim, w, joints_of(prim, k) if front == "fused" else None, mode)


def both(a, drv, prim, k, mode):
    V = drv.positions(prim, k)
    a.update_mesh(prim, V, twin(prim, V), mode)
    drv.call(prim, k, mode, V)
    return V


@pytest.mark.parametrize("mode,builder", MODES)
@pytest.mark.parametrize("front", FRONT_ENDS)
def test_every_front_end_equals_update_with_the_twins_normals(front, mode, builder):
    """the four zoo meshes with normals, two calls in a row each: the second finds the adjacency on the device (REFIT)"""
    desc, a, b = pair(builder)
    start = dc.snapshot(b, desc, SMOOTH)
    smooth(b, SMOOTH)
    drv = Driver(b, front, SMOOTH)
    dc.assert_same(dc.snapshot(b, desc, SMOOTH), start)          # the mode (and the bindings) alone move nothing
    for k in (0, 1):
        for prim in SMOOTH:
            both(a, drv, prim, k, mode)
        sa, sb = dc.snapshot(a, desc, SMOOTH), dc.snapshot(b, desc, SMOOTH)
        dc.assert_same(sa, sb)
        assert sb["render"] != start["render"]
        start = sb
    a.close()
    b.close()


@pytest.mark.parametrize("prim", [BIG, FLAT])
def test_fused_morph_and_skin_on_the_larger_meshes(prim):
    """33 x 33: 1,089 normal items and 2,048 triangles, several blocks and a ragged tail in both kernels; flat_grid: 288 normals for 170
    vertices, each named by the three corners of one triangle"""
    desc, a, b = pair(desc=big_scene())
    assert len(arrays_of(BIG)[1]) == 1089 and len(arrays_of(FLAT)[1]) == 288 != len(arrays_of(FLAT)[0])
    smooth(b, [prim])
    drv = Driver(b, "fused", [prim])
    start = dc.snapshot(b, desc, [prim])
    for k in (0, 1):
        both(a, drv, prim, k, "refit")
        sb = dc.snapshot(b, desc, [prim])
        dc.assert_same(dc.snapshot(a, desc, [prim]), sb)
        assert sb["render"] != start["render"]
    a.close()
    b.close()


def valence_scene():
    """the zoo plus the 200-fan (prim 10) and the 288-triangle grid whose 864 corners share ONE normal (prim 11)"""
    d = dc.zoo_scene()
    d.name = "normals-zoo"
    out = {}
    for k, (case, off) in enumerate(((nc.fan(200), (3.4, 0.4, -0.6)), (nc.shared_normal(), (-3.4, 0.0, -0.6)))):
        v, ix, nn = case
        v = (v + np.array(off, F)).astype(F)
        out[10 + k] = (v, ix, nn)
        d.add_mesh(v, np.tile(np.array([0, 1, 0], F), (nn, 1)), None, ix, k, 4)
    return d, out


def test_high_valence_items():
    desc, cases = valence_scene()
    _, a, b = pair(desc=desc)
    prims = sorted(cases)
    smooth(b, prims)
    start = dc.snapshot(b, desc, prims)
    for k in (1, 2):
        for prim in prims:
            v, ix, nn = cases[prim]
            p = v.astype(np.float64)
            V = (p + 0.1 * k * np.stack([np.sin(2.1 * p[:, 1] + k), np.cos(1.7 * p[:, 0]), np.sin(1.3 * p[:, 2] - k)], 1)).astype(F)
            N = ag.vertex_normals_arrays(V, ix, nn)
            assert abs(np.linalg.norm(N[0].astype(np.float64)) - 1) < 1e-6
            a.update_mesh(prim, V, N)
            b.update_mesh(prim, V)
        sb = dc.snapshot(b, desc, prims)
        dc.assert_same(dc.snapshot(a, desc, prims), sb)
        assert sb["render"] != start["render"]
    a.close()
    b.close()


def test_smooth_changes_the_picture_of_a_morph_without_normal_deltas():
    desc, a, b = pair()
    prim = dc.GRID1_N
    for g in (a, b):
        morph_targets(g, prim, normal_deltas=False)
    b.set_mesh_normals_mode(prim, "smooth")
    w = weights(3, 1, [0, 2])
    a.morph_mesh(prim, w)                                        # GIVEN: the rest normals
    b.morph_mesh(prim, w)
    sa, sb = dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim])
    assert sa["bvh%d" % prim] == sb["bvh%d" % prim] and sa["closest"] == sb["closest"]   # the same geometry,
    assert sa["render"] != sb["render"]                                                  # lit by other normals
    a.close()
    b.close()


def test_a_smooth_rebuild_equals_the_oracles_fresh_scene():
    arrays = {}
    g = gpu_scene(dc.zoo_scene())
    smooth(g, SMOOTH)
    for prim in SMOOTH:
        V = dc.zoo_arrays(prim, 1)[0]
        g.update_mesh(prim, V, None, "rebuild")
        arrays[prim] = (V, twin(prim, V))
    oacc, ost = oracle_render(posed_zoo(arrays), dc.W, dc.H, dc.SPP, dc.DEPTH)
    acc, st = ag.PathTracer(dc.DEPTH).render_to_host(g, dc.W, dc.H, dc.SPP)
    assert acc.tobytes() == oacc.tobytes()
    assert (st.rays, st.closest_rays, st.anyhit_rays) == (ost.rays, ost.closest_rays, ost.anyhit_rays)
    g.close()


@pytest.mark.parametrize("explicit", [False, True])
def test_back_to_given_the_identity_gives_the_rest_pose(explicit):
    """the rest pose is what the mirror holds after the last explicit update: add_mesh's arrays, or (V, the recomputed N)"""
    desc, a, b = pair()
    prim = dc.GRID4_N
    rest = dc.snapshot(b, desc, dc.PRIMS)
    b.set_mesh_normals_mode(prim, "smooth")
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)         # the mode alone moves nothing
    if explicit:
        V = dc.zoo_arrays(prim, 2)[0]
        b.update_mesh(prim, V)
        a.update_mesh(prim, V, twin(prim, V))
        moved = dc.snapshot(a, desc, dc.PRIMS)
        assert moved["render"] != rest["render"]
        rest = moved
    b.transform_mesh(prim, about(prim, MATRICES["rotation+translation"]))
    assert dc.snapshot(b, desc, dc.PRIMS)["render"] != rest["render"]
    b.set_mesh_normals_mode(prim, "given")
    b.transform_mesh(prim, EYE)
    dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), rest)
    a.close()
    b.close()


def test_a_refit_after_a_rebuild_uploads_the_adjacency_again():
    desc, a, b = pair()
    smooth(b, SMOOTH)
    drv = Driver(b, "transform", SMOOTH)
    for prim in (dc.GRID4_N, 3):
        for k, mode in ((0, "refit"), (1, "rebuild"), (0, "refit"), (1, "refit")):   # the REBUILD destroys the device cache
            both(a, drv, prim, k, mode)
            dc.assert_same(dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim]))
    a.close()
    b.close()


def test_a_stale_mirror_keeps_the_recomputed_normals():
    """after a SMOOTH device REFIT of mesh X its arrays exist on the device only; a REBUILD of mesh Y re-flattens every mesh from the mirror"""
    desc, a, b = pair()
    x, y = dc.GRID1_N, dc.GRID4
    b.set_mesh_normals_mode(x, "smooth")
    V = dc.zoo_arrays(x, 1)[0]
    a.update_mesh(x, V, twin(x, V))
    d = dc.DeviceArrays(b.ctx, V)
    try:
        b.update_mesh_device(x, d.pv, len(V), None, len(arrays_of(x)[1]), "refit")
    finally:
        d.free()
    for g in (a, b):
        g.update_mesh(y, *dc.zoo_arrays(y, 2), "rebuild")
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_a_seventy_primitive_scene():
    desc, a, b = pair(desc=seventy_prims())
    prim = 7
    v, n, _, ix = desc.ops[3 + prim][1:5]
    assert n is not None
    b.set_mesh_normals_mode(prim, "smooth")
    before = dc.snapshot(b, desc, [prim])
    V = (v * F(1.5) + np.array([0.3, 0.2, -0.4], F)).astype(F)   # outside its old root box: the top-level tree is built again
    a.update_mesh(prim, V, ag.vertex_normals_arrays(V, ix, len(n)))
    b.update_mesh(prim, V)
    sb = dc.snapshot(b, desc, [prim])
    dc.assert_same(dc.snapshot(a, desc, [prim]), sb)
    assert sb["render"] != before["render"]
    u = desc.ops[3 + 20][1] * F(1.25)
    for g in (a, b):
        g.update_mesh(20, u, desc.ops[3 + 20][2], "rebuild")
    dc.assert_same(dc.snapshot(a, desc, [prim, 20]), dc.snapshot(b, desc, [prim, 20]))
    a.close()
    b.close()


@pytest.mark.parametrize("front", ["update", "device", "transform"])
def test_a_nan_in_a_referenced_vertex_takes_the_fallback(front):
    """(the two far grids of test_gpu_pose_mesh's case; GRID4_N alone has normals)"""
    desc, a, b = pair()
    prim = dc.GRID4_N
    b.set_mesh_normals_mode(prim, "smooth")
    rv, rn = dc.zoo_arrays(prim)
    if front == "transform":
        bad = rv.copy()
        bad[dc.REFERENCED, 2] = np.nan
        b.update_mesh(prim, bad)                                 # a NaN in the rest pose: every transform of it has one
        M = about(prim, MATRICES["rotation+translation"])
        V = ag.transform_arrays(M, bad, twin(prim, bad))[0]
        a.update_mesh(prim, V, twin(prim, V))
        b.transform_mesh(prim, M)
    else:
        V = dc.zoo_arrays(prim, 1)[0]
        V[dc.REFERENCED, 2] = np.nan
        a.update_mesh(prim, V, twin(prim, V))
        if front == "update":
            b.update_mesh(prim, V)
        else:
            d = dc.DeviceArrays(b.ctx, V)
            try:
                b.update_mesh_device(prim, d.pv, len(V), None, len(rn), "refit")
            finally:
                d.free()
    N = twin(prim, V)
    assert np.isnan(V).any() and np.isfinite(N).all() and (N[dc.REFERENCED] == 0).all()
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_refusals_in_their_order_change_nothing():
    ctx = gpu_context()
    g = ag.Scene(ctx)
    desc = dc.zoo_scene()
    L, fp = g.L, C.POINTER(C.c_float)
    prim, bare = dc.GRID1_N, dc.GRID1
    v, n = dc.zoo_arrays(prim)
    pv, pn = v.ctypes.data_as(fp), n.ctypes.data_as(fp)

    def refused_mode(what, *args):
        assert L.agpt_scene_set_mesh_normals_mode(*args) == -1
        assert b"agpt_scene_set_mesh_normals_mode" in L.agpt_last_error() and what in L.agpt_last_error(), L.agpt_last_error()
    refused_mode(b"NULL scene", None, 99, 7)                              # the scene before everything else
    refused_mode(b"is not a mesh", g.h, 0, 7)                             # (nothing added yet)
    desc.instantiate(g)
    before = dc.snapshot(g, desc, dc.PRIMS)
    for p in (-1, len(dc.PRIMS) + 1, 99):
        refused_mode(b"is not a mesh", g.h, p, 7)                         # the primitive before the mode (9 is the sphere light)
    refused_mode(b"unknown mode 7", g.h, bare, 7)                         # the mode before the mesh's normals
    refused_mode(b"unknown mode -1", g.h, prim, -1)
    refused_mode(b"has no normals", g.h, bare, 1)
    assert L.agpt_scene_set_mesh_normals_mode(g.h, bare, 0) == 0          # GIVEN is fine for a mesh without normals

    def refused(fn, what, *args):
        assert getattr(L, fn)(*args) == -1
        assert fn.encode() in L.agpt_last_error() and what in L.agpt_last_error(), L.agpt_last_error()
    # GIVEN: NULL normals for a mesh that has some are still refused, on both calls
    refused("agpt_scene_update_mesh", b"vertices and", g.h, prim, pv, len(v), None, len(n), 0)
    refused("agpt_scene_update_mesh_device", b"vertices and", g.h, prim, C.c_void_p(1 << 20), len(v), None, len(n), 0)
    g.set_mesh_normals_mode(prim, "smooth")
    g.set_mesh_normals_mode(prim, "given")                                # and again after the mode was set and taken back
    refused("agpt_scene_update_mesh", b"vertices and", g.h, prim, pv, len(v), None, len(n), 0)
    g.set_mesh_normals_mode(prim, "smooth")
    # SMOOTH: every other refusal stays, in its order, with normals NULL or not
    for normals in (None, pn):
        refused("agpt_scene_update_mesh", b"NULL", g.h, prim, None, len(v), normals, len(n), 7)
        refused("agpt_scene_update_mesh", b"not a mesh", g.h, 99, pv, len(v), normals, len(n), 7)
        refused("agpt_scene_update_mesh", b"vertices and", g.h, prim, pv, len(v) - 1, normals, len(n), 7)
        refused("agpt_scene_update_mesh", b"vertices and", g.h, prim, pv, len(v), normals, len(n) - 1, 7)
        refused("agpt_scene_update_mesh", b"vertices and", g.h, prim, pv, len(v), normals, 0, 7)     # the count is still the mesh's
        refused("agpt_scene_update_mesh", b"unknown mode", g.h, prim, pv, len(v), normals, len(n), 7)
        refused("agpt_scene_update_mesh_device", b"vertices and", g.h, prim, C.c_void_p(1 << 20), len(v), None, 0, 0)
        refused("agpt_scene_update_mesh_device", b"unknown mode", g.h, prim, C.c_void_p(1 << 20), len(v), None, len(n), 7)
    refused("agpt_scene_transform_mesh", b"unknown mode", g.h, prim, EYE.ctypes.data_as(fp), 7)
    refused("agpt_scene_transform_mesh", b"NULL matrix", g.h, prim, None, 0)
    refused("agpt_scene_pose_mesh", b"has no skin", g.h, prim, EYE.ctypes.data_as(fp), 1, 0)
    refused("agpt_scene_morph_mesh", b"has no morph targets", g.h, prim, pv, 3, None, 0, 0)
    dc.assert_same(dc.snapshot(g, desc, dc.PRIMS), before)
    with pytest.raises(ValueError, match="unknown mode"):
        g.set_mesh_normals_mode(prim, "flat")
    g.close()


def test_smooth_updates_on_a_non_blocking_stream():
    """the host call, the device call (its positions produced on the stream) and a transform of two meshes in SMOOTH mode on a context
    bound to a caller's non-blocking stream, behind test_gpu_streams' delay: the first call of a mesh uploads the adjacency, the later
    ones find it"""
    desc = dc.zoo_scene()
    moved = (dc.GRID1_N, dc.PRIMS[0])
    with Stage() as st, twin_scene(desc) as a:
        b = st.scene(desc)
        smooth(b, moved)
        arrays = {}
        for pose, wrong in ((1, 2), (2, 1)):
            for prim in moved:
                V, W = dc.zoo_arrays(prim, pose)[0], dc.zoo_arrays(prim, wrong)[0]
                arrays[prim] = (V, twin(prim, V))
                a.update_mesh(prim, *arrays[prim], "refit")
                if pose == 1:
                    st.open()
                    st.call("update_mesh smooth prim %d" % prim, b.update_mesh, prim, V, None, "refit")
                else:
                    bv = st.buffer(V, W)
                    st.open([bv])
                    st.call("update_mesh_device smooth prim %d" % prim, b.update_mesh_device, prim, bv.dst, len(V), None,
                            len(arrays[prim][1]), "refit")
            dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        for prim in moved:
            M = about(prim, MATRICES["scale+shear"])
            V = ag.transform_arrays(M, *arrays[prim])[0]         # the rest pose is the last explicit update's (V, recomputed N)
            arrays[prim] = (V, twin(prim, V))
            a.update_mesh(prim, *arrays[prim], "refit")
            st.open()
            st.call("transform_mesh smooth prim %d" % prim, b.transform_mesh, prim, M, "refit")
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        assert_rays_through_updated_scene(st, b, arrays, False)


TORCH_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch                      # before the library touches the GPU (INTEGRATION.md section 3)
torch.zeros(1, device="cuda")
import ag_pathtracer_amd as ag
import device_update_cases as dc
import normals_cases as nc

desc = dc.zoo_scene()
ctx = ag.Context(0)
a, b = desc.instantiate(ag.Scene(ctx)), desc.instantiate(ag.Scene(ctx))
for prim in (dc.GRID1_N, dc.PRIMS[0]):
    b.set_mesh_normals_mode(prim, "smooth")
    v, ix, nn = nc.zoo_case(prim, 1)
    a.update_mesh(prim, v, ag.vertex_normals_arrays(v, ix, nn))
    tv = torch.from_numpy(v).cuda() * 1.0
    b.update_mesh(prim, tv, None, "refit")          # a device tensor of positions and no normals: NULL goes through
    tv.fill_(float("nan"))
dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
a.set_mesh_normals_mode(dc.GRID1_N, "given")
try:
    a.update_mesh(dc.GRID1_N, torch.from_numpy(v).cuda(), None)   # GIVEN: still refused
except ag.AgptError as e:
    assert "normals may be NULL only without any" in str(e), e
else:
    raise AssertionError("NULL normals were accepted in GIVEN mode")
print("torch-ok")
"""


def test_a_torch_tensor_of_positions_and_no_normals():
    """Scene.update_mesh with a torch tensor on the GPU and normals=None in SMOOTH mode (agpt_scene_update_mesh_device with NULL normals
    and the mesh's own count).  In a child process: torch must initialise the GPU before the library does."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = TORCH_CHILD % {"root": root, "tests": os.path.join(root, "tests")}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "torch-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_cpp_rippled_example_matches_python(tmp_path):
    """examples/rippled_scene.cpp rewrites the heights of a 17 x 17 grid in MeshNormals::Smooth mode every frame; the FNV-1a hashes it
    prints for its first and last frame are those of the same frames through the Python binding"""
    exe = build_cpp_example(tmp_path, "rippled_scene")
    frames, w, h, spp = 3, 32, 24, 4
    out = subprocess.run([exe, str(frames), str(w), str(h)], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {int(k): int(x, 16) for k, x in re.findall(r"frame (\d+) hash ([0-9a-f]{16})", out)}
    assert sorted(got) == list(range(frames)) and len(set(got.values())) == frames, out

    side = 17
    d = ag.SceneDesc("rippled")
    blue = d.add_material(ag.MAT_DISNEY, [0.15, 0.35, 0.8], .3, 0.)
    floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
    d.add_mesh(*ag.create_backdrop([0, -1.5, 20], [40, 20, 40], 7.5, 8), floor, 1)
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    v = np.stack([F(0.25) * i.astype(F) - F(2), np.zeros(side * side, F), F(0.25) * j.astype(F) - F(2)], 1).astype(F)
    tris = []
    for p in range(side - 1):
        for q in range(side - 1):
            a, b = p * side + q, p * side + q + 1
            tris += [a, b, a + side, b, b + side, a + side]
    corners = np.array(tris, np.int32)
    d.add_mesh(v, np.tile(np.array([0, 1, 0], F), (side * side, 1)), None, np.stack([corners, corners, np.full_like(corners, -1)], 1), blue, 4)
    d.add_area_light([0, 25, -20], 1.0, [200., np.float32(.941) * np.float32(200), np.float32(.914) * np.float32(200)])
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 2.16, -5.64], [0, 0.0, 0], [0, 1, 0], np.float32(w) / np.float32(h), 45.0, 0.0)
    g = gpu_scene(d)
    g.set_mesh_normals_mode(1, "smooth")

    def wave(k):
        r = k % 8
        return np.where(r < 4, r, 8 - r)
    want = {}
    p = g.ctx.alloc(w * h * 16)
    try:
        for k in (0, frames - 1):
            u = v.copy()
            u[:, 1] = F(0.0625) * wave(i + 2 * k).astype(F) + F(0.03125) * wave(2 * j + 3 * k).astype(F)
            g.update_mesh(1, u)
            acc, _ = ag.PathTracer(5).render_to_host(g, w, h, spp)
            g.ctx.upload(p, acc)
            want[k] = frame_hash(g.ctx.resolve(p, w * h, spp))
    finally:
        g.ctx.free(p)
        g.close()
    assert {k: got[k] for k in want} == want
