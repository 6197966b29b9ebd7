"""agpt_skin_arrays, CPU side: the host-only twin of agpt_scene_pose_mesh against the numpy model of its definition (skin_model.py),
bit for bit, and against agpt_transform_arrays where the definition reduces to it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_update_cases as dc
import skin_model
from helpers import assert_exported, bits
from skin_cases import ALL_ZERO, JOINTS3, binding, flat_shaded, single_slot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "agpt.h")).read()
F = np.float32
MESHES = {"triangle": dc.one_triangle, "strip": dc.strip, "grid": dc.bumpy_grid}


def same_bits(got, want):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))


def test_symbols_declared_and_exported():
    names = ("agpt_skin_arrays", "agpt_scene_set_mesh_skin", "agpt_scene_pose_mesh")
    assert_exported(names)
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, HEADER), name
        assert name in ag.binding.EXPORTS


@pytest.mark.parametrize("K", [1, 4, 8])
@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_twin_equals_the_model(mesh, with_normals, K):
    v, n, _ = MESHES[mesh](with_normals)
    assert len(v) == {"triangle": 3, "strip": 65, "grid": 170}[mesh]
    J, W = binding(len(v), K, seed=10 * K + len(v))
    got_v, got_n = ag.skin_arrays(JOINTS3, v, J, W, n)
    want_v, want_n = skin_model.skin_arrays(JOINTS3, v, J, W, n)
    same_bits(got_v, want_v)
    same_bits(got_v[ALL_ZERO], v[ALL_ZERO])              # no used slot: the rest position, bit for bit
    if K > 1:
        assert not np.array_equal(bits(got_v), bits(v))
    if with_normals:
        same_bits(got_n, want_n)
        same_bits(got_n[ALL_ZERO], n[ALL_ZERO])
    else:
        assert got_n is None


@pytest.mark.parametrize("joint", [0, 1, 2])
def test_one_slot_of_weight_one_and_two_halves_are_the_transform(joint):
    v, n, _ = dc.bumpy_grid(True)
    want_v, want_n = ag.transform_arrays(JOINTS3[joint], v, n)
    for slots, weight in (((2,), 1.0), ((1, 3), 0.5)):
        J, W = single_slot(len(v), 4, joint, slots, weight)
        got_v, got_n = ag.skin_arrays(JOINTS3, v, J, W, n)
        assert got_v.tobytes() == want_v.tobytes() and got_n.tobytes() == want_n.tobytes()
        mv, mn = skin_model.skin_arrays(JOINTS3, v, J, W, n)
        assert mv.tobytes() == want_v.tobytes() and mn.tobytes() == want_n.tobytes()


def test_normals_with_counts_and_influences_of_their_own():
    v, _, ix = dc.bumpy_grid(False)
    n = flat_shaded(v, ix[:, 0])
    assert len(n) == 288 != len(v)
    J, W = binding(len(v), 4, seed=5)
    nJ, nW = binding(len(n), 4, seed=6)
    got_v, got_n = ag.skin_arrays(JOINTS3, v, J, W, n, nJ, nW)
    want_v, want_n = skin_model.skin_arrays(JOINTS3, v, J, W, n, nJ, nW)
    same_bits(got_v, want_v)
    same_bits(got_n, want_n)
    with pytest.raises(ag.AgptError, match="may be NULL .* only when n_normals == n_vertices"):
        ag.skin_arrays(JOINTS3, v, J, W, n)


def test_in_place():
    v, n, _ = dc.strip(True)
    J, W = binding(len(v), 4, seed=3)
    want_v, want_n = ag.skin_arrays(JOINTS3, v, J, W, n)
    L, fp, ip = ag.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    m = np.ascontiguousarray(JOINTS3).reshape(-1)
    vi, ni = v.copy(), n.copy()
    assert L.agpt_skin_arrays(m.ctypes.data_as(fp), 3, 4, vi.ctypes.data_as(fp), len(vi), J.ctypes.data_as(ip), W.ctypes.data_as(fp),
                              ni.ctypes.data_as(fp), len(ni), None, None, vi.ctypes.data_as(fp), ni.ctypes.data_as(fp)) == 0
    assert vi.tobytes() == want_v.tobytes() and ni.tobytes() == want_n.tobytes()


def test_refusals_and_their_messages():
    L, fp, ip = ag.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    v, n, _ = dc.one_triangle(True)
    J, W = single_slot(3, 2, 0, (0,), 1.0)
    m = np.ascontiguousarray(JOINTS3).reshape(-1).copy()
    vo, no = np.full_like(v, 7), np.full_like(n, 7)

    def call(m=m, n_joints=3, K=2, v=v, nv=3, J=J, W=W, n=n, nn=3, nJ=None, nW=None, vo=vo, no=no):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)   # noqa: E731
        return L.agpt_skin_arrays(p(m, fp), n_joints, K, p(v, fp), nv, p(J, ip), p(W, fp), p(n, fp), nn, p(nJ, ip), p(nW, fp), p(vo, fp), p(no, fp))

    def refused(what, **kw):
        assert call(**kw) == -1
        err = L.agpt_last_error()
        assert b"agpt_skin_arrays" in err and what in err, err
    assert call() == 0
    vo[:], no[:] = 7, 7
    for name in ("m", "v", "J", "W", "vo"):
        refused(b"NULL", **{name: None})
    refused(b"NULL normals or normals_out", n=None)
    refused(b"NULL normals or normals_out", no=None)
    refused(b"negative count", nv=-1)
    refused(b"negative count", nn=-3)
    for K in (0, 9, -1):
        refused(b"outside 1 .. 8", K=K)
    for nj in (0, 65537, -2):
        refused(b"outside 1 .. 65536", n_joints=nj)
    refused(b"only when n_normals == n_vertices", nn=2)
    refused(b"only when n_normals == n_vertices", nJ=J)          # one of the two alone
    for bad in (3, -1):
        Jb = J.copy()
        Jb[2, 1] = bad                                            # (a slot of weight 0 is checked too)
        refused(b"joint index %d out of range (vertex 2, slot 1" % bad, J=Jb)
        refused(b"out of range (normal 2, slot 1", nJ=Jb, nW=W)
    for bad, what in ((-0.25, b"negative weight"), (np.nan, b"non-finite weight"), (np.inf, b"non-finite weight"), (-np.inf, b"non-finite weight")):
        Wb = W.copy()
        Wb[1, 0] = bad
        refused(what + b" (vertex 1, slot 0)", W=Wb)
        refused(what + b" (normal 1, slot 0)", nJ=J, nW=Wb)
    for cell, value in ((12, 1e-30), (14, -1.0), (15, 2.0), (15, np.nan)):
        mb = m.copy()
        mb[16 + cell] = value
        refused(b"the last row of joint 1 is not (0, 0, 0, 1)", m=mb)
    assert np.all(vo == 7) and np.all(no == 7)        # a refused call writes nothing
    assert call(nv=0, nn=0) == 0                       # nothing to do is not an error
    Wz = W.copy()
    Wz[0, 0] = F(-0.0)                                 # a zero of either sign is a weight
    assert call(W=Wz) == 0


def test_a_singular_joint_leaves_its_normals_as_the_identity_would():
    v, n, _ = dc.strip(True)
    singular = np.array([[1, 2, 3, 0], [2, 4, 6, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F)
    mats = np.stack([singular, JOINTS3[0]])
    J, W = single_slot(len(v), 2, 0, (0,), 1.0)
    got_v, got_n = ag.skin_arrays(mats, v, J, W, n)
    want_v, want_n = ag.transform_arrays(singular, v, n)
    assert got_v.tobytes() == want_v.tobytes() and got_n.tobytes() == want_n.tobytes() == n.tobytes()
    mv, mn = skin_model.skin_arrays(mats, v, J, W, n)
    same_bits(got_v, mv)
    same_bits(got_n, mn)
