"""agpt_scene_update_mesh_device on the GPU: every case builds two identical scenes, updates A through the host call and B through
the device-pointer call (arrays from agpt_device_alloc / agpt_device_upload), and compares -- bit for bit -- every mesh's
agpt_mesh_get_bvh, closest- and any-hit records on the same rays, and a render with its ray totals (device_update_cases.snapshot).
The host call itself is pinned to the oracle by test_gpu_mesh_update.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_update_cases as dc
from device_update_cases import pair, seventy_prims
from helpers import gpu_context, gpu_scene
from morph_cases import weights
from skin_cases import JOINTS3, binding
from transform_cases import MATRICES

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode,builder", [("refit", "host"), ("refit", "device"), ("rebuild", "host"), ("rebuild", "device")])
def test_device_arrays_equal_host_arrays(mode, builder):
    """all eight meshes of the zoo (1 triangle, 65 vertices, 288 triangles at max_prims_in_node 1 and 4; with and without normals; no
    texture coordinates), then a second update of each (the cached path)"""
    desc, a, b = pair(builder)
    before = dc.snapshot(b, desc, dc.PRIMS)
    for pose in (1, 2):
        for prim in dc.PRIMS:
            v, n = dc.zoo_arrays(prim, pose)
            a.update_mesh(prim, v, n, mode)
            dc.update_through_device(b, prim, v, n, mode)
        sa, sb = dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS)
        dc.assert_same(sa, sb)
        assert sb["render"] != before["render"] and sb["bvh1"] != before["bvh1"]   # (the update shows)
        before = sb
    a.close()
    b.close()


def test_a_stale_mirror_survives_the_rebuild_of_another_mesh():
    """device-REFIT of one mesh, then a host REBUILD of another: the full flatten behind the REBUILD must see the first mesh's NEW
    arrays, which exist only on the device until then"""
    desc, a, b = pair()
    moved, other = dc.GRID1_N, dc.GRID4
    v, n = dc.zoo_arrays(moved, 2)
    a.update_mesh(moved, v, n, "refit")
    dc.update_through_device(b, moved, v, n, "refit")
    still = b.bvh(moved)[0].tobytes()
    w, _ = dc.zoo_arrays(other, 1)
    for g in (a, b):
        g.update_mesh(other, w, None, "rebuild")
    sa, sb = dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS)
    dc.assert_same(sa, sb)
    assert b.bvh(moved)[0].tobytes() == still   # the new pose, in the mirror too
    fresh = gpu_scene(desc)
    assert fresh.bvh(moved)[0].tobytes() != still
    # and the other way round: the fallback's commit (a non-finite update of a third mesh) after a device REFIT
    u, _ = dc.zoo_arrays(dc.GRID1, 1)
    u[dc.REFERENCED, 1] = np.nan
    for g in (a, b):
        g.update_mesh(dc.GRID1, u, None, "refit")
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    for g in (a, b, fresh):
        g.close()


def test_a_seventy_primitive_scene_gets_its_top_level_tree_again():
    desc, a, b = pair(desc=seventy_prims())
    prim = 7
    v, n, _, _ = ag.scenes.blob_mesh(5, 4, center=(0.5, 2.0, -9.0), radius=1.2, seed=7)   # well outside its old root box
    before = dc.snapshot(b, desc, [prim])
    a.update_mesh(prim, v, n, "refit")
    dc.update_through_device(b, prim, v, n, "refit")
    sa, sb = dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim])
    dc.assert_same(sa, sb)
    assert sb["render"] != before["render"] and sb["closest"] != before["closest"]
    a.close()
    b.close()


@pytest.mark.parametrize("vertex", [dc.UNREFERENCED, dc.REFERENCED])
def test_a_non_finite_coordinate_takes_the_fallback(vertex):
    """one NaN, in a vertex no triangle references and in one that several do: the kernel looks at every coordinate (the host
    path's rule), and the result is the host call's"""
    desc, a, b = pair()
    for prim in (dc.GRID4_N, dc.GRID1):
        v, n = dc.zoo_arrays(prim, 1)
        v[vertex, 2] = np.nan
        a.update_mesh(prim, v, n, "refit")
        dc.update_through_device(b, prim, v, n, "refit")
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    # the scene is usable afterwards: a finite device update of the same mesh
    v, n = dc.zoo_arrays(dc.GRID1, 2)
    a.update_mesh(dc.GRID1, v, n, "refit")
    dc.update_through_device(b, dc.GRID1, v, n, "refit")
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_one_mesh_through_every_front_end_in_a_row():
    """the 170-vertex grid with normals and the one without, each through transform, skin + pose, device arrays (the rest pose is
    forgotten, the binding kept), pose, targets + fused morph, a REBUILD morph (the device cache goes), pose, -- the mesh with normals
    only -- SMOOTH mode with a morph and a pose, new targets (T = 2) + morph, a new skin (K = 2, five joints) + pose, GIVEN mode again and
    a host update with a NaN vertex (the fallback), and a transform: after every step scene B equals scene A, which received the host
    twins' arrays through agpt_scene_update_mesh"""
    desc, a, b = pair()
    prims = (dc.GRID4_N, dc.GRID1)
    rest = {p: dc.zoo_arrays(p) for p in prims}
    corners = {p: dc.ZOO[p - 1][1](dc.ZOO[p - 1][2])[2] for p in prims}
    smooth, skins, tg = set(), {}, {}
    assert len(rest[dc.GRID4_N][0]) == 170 == len(rest[dc.GRID4_N][1]) and rest[dc.GRID1][1] is None
    last = [dc.snapshot(b, desc, prims)]

    def step(arrays, call, mode="refit", moves=True):
        """arrays(p) -> the (V, N) the step stands for, call(p): the front end on scene B"""
        for p in prims:
            v, n = arrays(p)
            if p in smooth:
                n = ag.vertex_normals_arrays(v, corners[p], len(rest[p][1]))
            a.update_mesh(p, v, n, mode)
            call(p)
        sa, sb = dc.snapshot(a, desc, prims), dc.snapshot(b, desc, prims)
        dc.assert_same(sa, sb)
        assert not moves or sb["render"] != last[0]["render"]
        last[0] = sb

    def posed(p, mats, v=None, n=None):
        return ag.skin_arrays(mats, rest[p][0] if v is None else v, *skins[p][:2], rest[p][1] if n is None else n, *skins[p][2:])

    def morphed(p, w):
        return ag.morph_arrays(w, rest[p][0], tg[p][0], rest[p][1], tg[p][1])

    M = {p: dc.about(p, MATRICES["rotation+translation"]) for p in prims}
    step(lambda p: ag.transform_arrays(M[p], *rest[p]), lambda p: b.transform_mesh(p, M[p]))                          # 1
    skins.update({p: dc.skin_of(b, p) for p in prims})
    step(lambda p: posed(p, dc.palette(p, 0)), lambda p: b.pose_mesh(p, dc.palette(p, 0)))                            # 2
    rest = {p: dc.zoo_arrays(p, 2) for p in prims}
    step(lambda p: rest[p], lambda p: dc.update_through_device(b, p, *rest[p]))                                       # 3
    step(lambda p: posed(p, dc.palette(p, 1)), lambda p: b.pose_mesh(p, dc.palette(p, 1)))                            # 4: the new rest pose
    tg.update({p: dc.morph_targets(b, p, 3) for p in prims})
    w3 = {p: weights(3, p, [0, 2]) for p in prims}
    step(lambda p: posed(p, dc.palette(p, 0), *morphed(p, w3[p])), lambda p: b.morph_mesh(p, w3[p], dc.palette(p, 0)))   # 5: fused
    w3 = {p: weights(3, p + 1, [0, 1, 2]) for p in prims}
    step(lambda p: morphed(p, w3[p]), lambda p: b.morph_mesh(p, w3[p], mode="rebuild"), "rebuild")                    # 6
    step(lambda p: posed(p, dc.palette(p, 1)), lambda p: b.pose_mesh(p, dc.palette(p, 1), "refit"))                   # 7
    b.set_mesh_normals_mode(dc.GRID4_N, "smooth")                                                                     # 8
    smooth.add(dc.GRID4_N)
    step(lambda p: morphed(p, w3[p]), lambda p: b.morph_mesh(p, w3[p]))
    step(lambda p: posed(p, dc.palette(p, 0)), lambda p: b.pose_mesh(p, dc.palette(p, 0)))
    tg.update({p: dc.morph_targets(b, p, 2) for p in prims})                                                          # 9
    w2 = {p: weights(2, p, [0, 1]) for p in prims}
    step(lambda p: morphed(p, w2[p]), lambda p: b.morph_mesh(p, w2[p]))
    for p in prims:                                                                                                   # 10
        J, W = binding(len(rest[p][0]), 2, seed=p + 7, n_joints=5)
        b.set_mesh_skin(p, J, W, n_joints=5)
        skins[p] = (J, W, None, None)
    five = {p: np.stack([dc.about(p, JOINTS3[i]) for i in (2, 0, 1, 0, 2)]) for p in prims}
    step(lambda p: posed(p, five[p]), lambda p: b.pose_mesh(p, five[p]))
    b.set_mesh_normals_mode(dc.GRID4_N, "given")                                                                      # 11
    smooth.clear()
    rest = {p: dc.zoo_arrays(p, 1) for p in prims}
    for p in prims:
        rest[p][0][dc.REFERENCED, 1] = np.nan
    step(lambda p: rest[p], lambda p: b.update_mesh(p, *rest[p]))
    M = {p: dc.about(p, MATRICES["scale+shear"]) for p in prims}
    step(lambda p: ag.transform_arrays(M[p], *rest[p]), lambda p: b.transform_mesh(p, M[p]))                          # 12
    a.close()
    b.close()


def test_refusals_in_the_documented_order_change_nothing():
    ctx = gpu_context()
    g = ag.Scene(ctx)
    desc = dc.zoo_scene()
    L = g.L
    v, n = dc.zoo_arrays(dc.GRID1_N, 1)
    d = dc.DeviceArrays(ctx, v, n)
    pv, pn = C.c_void_p(d.pv), C.c_void_p(d.pn)

    def refused(what, *args):
        assert L.agpt_scene_update_mesh_device(*args) == -1
        assert b"agpt_scene_update_mesh_device" in L.agpt_last_error() and what in L.agpt_last_error(), L.agpt_last_error()
    refused(b"NULL", None, 99, pv, 1, None, 0, 7)
    refused(b"NULL", g.h, 99, None, 0, None, 0, 7)                       # NULL vertices first
    refused(b"not committed", g.h, 99, pv, 1, None, 0, 7)                # then the commit state
    desc.instantiate(g)
    before = dc.snapshot(g, desc, dc.PRIMS)
    sphere_light = len(dc.PRIMS) + 1
    for prim in (-1, sphere_light, 99):
        refused(b"not a mesh", g.h, prim, pv, 1, None, 0, 7)             # then the primitive
    refused(b"vertices and", g.h, dc.GRID1_N, pv, len(v) - 1, pn, len(n), 7)
    refused(b"vertices and", g.h, dc.GRID1_N, pv, len(v), pn, len(n) - 1, 7)
    refused(b"vertices and", g.h, dc.GRID1_N, pv, len(v), None, len(n), 7)   # NULL normals on a mesh that has them
    refused(b"vertices and", g.h, dc.GRID1, pv, len(v), pn, len(n), 7)       # normals for a mesh that has none
    refused(b"unknown mode", g.h, dc.GRID1_N, pv, len(v), pn, len(n), 7)
    dc.assert_same(dc.snapshot(g, desc, dc.PRIMS), before)
    d.free()
    g.close()


TORCH_CHILD = r"""
import contextlib
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch                      # before the library touches the GPU (INTEGRATION.md section 3)
import numpy as np
torch.zeros(1, device="cuda")
import ag_pathtracer_amd as ag
import device_update_cases as dc

# a stream handle means something only to the HIP runtime copy that made it: torch's streams may reach the library only if torch and
# the library are bound to ONE libamdhip64 (the check comes before the use)
ag.lib()
with open("/proc/self/maps") as f:
    runtimes = sorted({ln.split(None, 5)[5].strip() for ln in f if "libamdhip64" in ln and len(ln.split(None, 5)) == 6})
print("libamdhip64 mapped: %%d %%s" %% (len(runtimes), runtimes))
assert len(runtimes) == 1, "torch and libagpt_hip.so are bound to different HIP runtime copies: a torch stream is no handle for the library"

waits = [0]
stream_synchronize = torch.cuda.Stream.synchronize
def counted(self):
    waits[0] += 1
    return stream_synchronize(self)
torch.cuda.Stream.synchronize = counted

desc = dc.zoo_scene()
for own_stream in (False, True):
    # own_stream: the context runs on a stream of torch's pool (non-blocking, a non-zero handle -- torch's DEFAULT stream is handle 0,
    # the null stream) and the tensors are produced on it, so Scene.update_mesh hands them over without a wait
    s = torch.cuda.Stream() if own_stream else None
    ctx = ag.Context(0, stream=s.cuda_stream if own_stream else None)
    assert (ctx.stream != 0) == own_stream
    with (torch.cuda.stream(s) if own_stream else contextlib.nullcontext()):
        a, b = desc.instantiate(ag.Scene(ctx)), desc.instantiate(ag.Scene(ctx))
        waits[0] = 0
        for prim in (dc.GRID1_N, dc.GRID4, dc.PRIMS[0]):
            v, n = dc.zoo_arrays(prim, 1)
            a.update_mesh(prim, v, n)
            tv = torch.from_numpy(v).cuda() * 1.0          # produced on torch's current stream
            tn = None if n is None else torch.from_numpy(n).cuda()
            b.update_mesh(prim, tv, tn, "refit")
            tv.fill_(float("nan"))
        assert waits[0] == (0 if own_stream else 3), waits   # (the shortcut: no wait when the context runs on that very stream)
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        v, n = dc.zoo_arrays(dc.GRID1_N, 2)
        a.update_mesh(dc.GRID1_N, v, n)
        b.update_mesh(dc.GRID1_N, torch.from_numpy(v), torch.from_numpy(n))   # CPU tensors: the host call
        dc.assert_same(dc.snapshot(a, desc, [dc.GRID1_N]), dc.snapshot(b, desc, [dc.GRID1_N]))
        before = dc.snapshot(b, desc, [dc.GRID1_N])
        tv, tn = torch.from_numpy(v).cuda(), torch.from_numpy(n).cuda()
        bad = [(tv.double(), tn), (tv.half(), tn), (tv.reshape(-1), tn), (tv.t().contiguous(), tn), (torch.cat([tv, tv], 1)[:, :3], tn),
               (tv, tn.double()), (tv, torch.from_numpy(n)), (torch.from_numpy(v), tn), (torch.empty(tv.shape, device="meta"), tn)]
        for x, y in bad:
            try:
                b.update_mesh(dc.GRID1_N, x, y)
            except ValueError as e:
                assert "update_mesh" in str(e)
            else:
                raise AssertionError("accepted %%s %%s %%s" %% (x.dtype, tuple(x.shape), x.device))
        dc.assert_same(dc.snapshot(b, desc, [dc.GRID1_N]), before)
        torch.cuda.current_stream().synchronize()
        a.close(); b.close(); ctx.close()
print("torch-ok")
"""


def test_torch_device_tensors_equal_ndarrays():
    """Scene.update_mesh with torch tensors on the GPU (data_ptr() handed to agpt_scene_update_mesh_device after torch's stream was
    synchronised; and once with the context on a torch.cuda.Stream() that also produces the tensors, which needs no wait) against the
    ndarray call; wrong dtype, shape, layout or device is refused in Python.  In a child process: torch must initialise the GPU before
    the library does, and the child first checks that both are bound to one HIP runtime copy -- only then is torch's stream a handle
    the library may be given."""
    code = TORCH_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "torch-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
