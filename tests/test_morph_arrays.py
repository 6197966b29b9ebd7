"""agpt_morph_arrays, CPU side: the host-only twin of agpt_scene_morph_mesh against the numpy model of its definition (morph_model.py),
bit for bit, alone and composed with agpt_skin_arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_update_cases as dc
import morph_model
from helpers import assert_exported, bits
from morph_cases import ACTIVE_SETS, SINGLE_ITEM, single_target, targets, weights, zero_target
from skin_cases import JOINTS3, binding, flat_shaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "agpt.h")).read()
F = np.float32
MESHES = {"triangle": dc.one_triangle, "strip": dc.strip, "grid": dc.bumpy_grid}


def same_bits(got, want):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))


def test_symbols_declared_and_exported():
    names = ("agpt_morph_arrays", "agpt_scene_set_mesh_morph_targets", "agpt_scene_morph_mesh")
    assert_exported(names)
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, HEADER), name
        assert name in ag.binding.EXPORTS
    for name in ("morph_arrays",):
        assert hasattr(ag, name)
    for name in ("set_mesh_morph_targets", "morph_mesh"):
        assert hasattr(ag.Scene, name)


@pytest.mark.parametrize("active", sorted(ACTIVE_SETS))
@pytest.mark.parametrize("T", [1, 3, 17])
@pytest.mark.parametrize("normals", ["none", "rest", "deltas"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_twin_equals_the_model(mesh, normals, T, active):
    """normals: the mesh has none / has normals but the targets no normal deltas / both"""
    v, n, _ = MESHES[mesh](normals != "none")
    dP = targets(len(v), T, seed=100 * T + len(v))
    dN = targets(len(n), T, seed=7 * T + len(v), extent=5.0) if normals == "deltas" else None
    w = weights(T, seed=T, active=ACTIVE_SETS[active](T))
    got_v, got_n = ag.morph_arrays(w, v, dP, n, dN)
    want_v, want_n = morph_model.morph_arrays(w, v, dP, n, dN)
    same_bits(got_v, want_v)
    if active == "none":
        assert got_v.tobytes() == v.tobytes()
    else:                                                      # (first and last are never the all-zero target)
        assert not np.array_equal(bits(got_v), bits(v))
    if normals == "none":
        assert got_n is None
    else:
        same_bits(got_n, want_n)
        if normals == "rest" or active == "none":
            assert got_n.tobytes() == n.tobytes()


def test_the_single_item_target_moves_one_item_and_the_zero_target_none():
    v, n, _ = dc.bumpy_grid(True)
    T = 3
    dP, dN = targets(len(v), T, 1), targets(len(n), T, 2)
    got_v, got_n = ag.morph_arrays(weights(T, 0, [single_target(T)]), v, dP, n, dN)
    moved = (bits(got_v) != bits(v)).any(1)
    assert moved[SINGLE_ITEM] and moved.sum() == 1 and (bits(got_n) != bits(n)).any(1).sum() == 1
    got_v, got_n = ag.morph_arrays(weights(T, 0, [zero_target(T)]), v, dP, n, dN)
    assert got_v.tobytes() == v.tobytes() and got_n.tobytes() == n.tobytes()        # (no coordinate of the grid is -0.0)


def test_normals_of_their_own_count():
    v, _, ix = dc.bumpy_grid(False)
    n = flat_shaded(v, ix[:, 0])
    assert len(n) == 288 != len(v)
    T = 3
    dP, dN = targets(len(v), T, 5), targets(len(n), T, 6)
    w = weights(T, 4, [0, 2])
    got_v, got_n = ag.morph_arrays(w, v, dP, n, dN)
    want_v, want_n = morph_model.morph_arrays(w, v, dP, n, dN)
    same_bits(got_v, want_v)
    same_bits(got_n, want_n)
    assert not np.array_equal(bits(got_n), bits(n))
    got_v, got_n = ag.morph_arrays(w, v, dP, n, None)
    same_bits(got_v, want_v)
    assert got_n.tobytes() == n.tobytes()


def test_all_weights_zero_returns_the_input_bytes():
    v, n, _ = dc.strip(True)
    v[3, 1], n[5, 0] = F(-0.0), F(-0.0)
    dP, dN = targets(len(v), 17, 1), targets(len(n), 17, 2)
    w = np.zeros(17, F)
    w[::2] = F(-0.0)
    got_v, got_n = ag.morph_arrays(w, v, dP, n, dN)
    assert got_v.tobytes() == v.tobytes() and got_n.tobytes() == n.tobytes()


def test_the_skip_is_by_weight_not_by_delta():
    """a rest coordinate of -0.0 under a target of weight 1 whose delta is all zero: -0.0 + 1 * 0.0 = +0.0"""
    v, n, _ = dc.one_triangle(True)
    v[1, 2], n[2, 0] = F(-0.0), F(-0.0)
    dP, dN = np.zeros((1, 3, 3), F), np.zeros((1, 3, 3), F)
    for twin in (ag.morph_arrays, morph_model.morph_arrays):
        got_v, got_n = twin(np.ones(1, F), v, dP, n, dN)
        assert got_v[1, 2] == 0 and not np.signbit(got_v[1, 2]) and got_n[2, 0] == 0 and not np.signbit(got_n[2, 0])
        assert np.array_equal(np.delete(bits(got_v).reshape(-1), 5), np.delete(bits(v).reshape(-1), 5))
        got_v, got_n = twin(np.zeros(1, F), v, dP, n, dN)
        assert np.signbit(got_v[1, 2]) and np.signbit(got_n[2, 0])


def test_in_place():
    v, n, _ = dc.strip(True)
    T = 3
    dP, dN = targets(len(v), T, 3), targets(len(n), T, 4)
    w = weights(T, 1, [0, 1, 2])
    L, fp = ag.lib(), C.POINTER(C.c_float)
    for deltas in (dN, None):
        want_v, want_n = ag.morph_arrays(w, v, dP, n, deltas)
        vi, ni = v.copy(), n.copy()
        assert L.agpt_morph_arrays(w.ctypes.data_as(fp), T, vi.ctypes.data_as(fp), len(vi), dP.ctypes.data_as(fp), ni.ctypes.data_as(fp), len(ni),
                                   None if deltas is None else deltas.ctypes.data_as(fp), vi.ctypes.data_as(fp), ni.ctypes.data_as(fp)) == 0
        assert vi.tobytes() == want_v.tobytes() and ni.tobytes() == want_n.tobytes()


@pytest.mark.parametrize("own_normals", [False, True])
def test_twin_composed_with_the_skin_twin_equals_the_composed_model(own_normals):
    v, n, ix = dc.bumpy_grid(True)
    if own_normals:
        n = flat_shaded(v, ix[:, 0])
    T = 3
    dP, dN = targets(len(v), T, 8), targets(len(n), T, 9)
    w = weights(T, 2, [0, 2])
    J, W = binding(len(v), 4, seed=11)
    nJ, nW = binding(len(n), 4, seed=12) if own_normals else (None, None)
    mv, mn = ag.morph_arrays(w, v, dP, n, dN)
    got_v, got_n = ag.skin_arrays(JOINTS3, mv, J, W, mn, nJ, nW)
    want_v, want_n = morph_model.morph_then_skin(w, JOINTS3, v, dP, J, W, n, dN, nJ, nW)
    same_bits(got_v, want_v)
    same_bits(got_n, want_n)
    plain_v, plain_n = ag.skin_arrays(JOINTS3, v, J, W, n, nJ, nW)
    assert not np.array_equal(bits(got_v), bits(plain_v)) and not np.array_equal(bits(got_n), bits(plain_n))


def test_refusals_and_their_messages():
    L, fp = ag.lib(), C.POINTER(C.c_float)
    v, n, _ = dc.one_triangle(True)
    T = 3
    dP, dN = targets(3, T, 1), targets(3, T, 2)
    w = weights(T, 0, [0, 2])
    vo, no = np.full_like(v, 7), np.full_like(n, 7)

    def call(w=w, T=T, v=v, nv=3, dP=dP, n=n, nn=3, dN=dN, vo=vo, no=no):
        p = lambda a: None if a is None else a.ctypes.data_as(fp)   # noqa: E731
        return L.agpt_morph_arrays(p(w), T, p(v), nv, p(dP), p(n), nn, p(dN), p(vo), p(no))

    def refused(what, **kw):
        assert call(**kw) == -1
        err = L.agpt_last_error()
        assert b"agpt_morph_arrays" in err and what in err, err
    assert call() == 0
    vo[:], no[:] = 7, 7
    for name in ("w", "v", "dP", "vo"):
        refused(b"NULL", **{name: None})
    refused(b"NULL normals or normals_out", n=None)
    refused(b"NULL normals or normals_out", no=None)
    refused(b"negative count", nv=-1)
    refused(b"negative count", nn=-3)
    for bad in (0, -1, 4097):
        refused(b"n_targets is %d, outside 1 .. 4096" % bad, T=bad)
    for bad in (np.nan, np.inf, -np.inf):
        wb = w.copy()
        wb[1] = bad                                           # (the idle target: every weight is checked)
        refused(b"non-finite weight (target 1)", w=wb)
        db = dP.copy()
        db[2, 1, 0] = bad
        refused(b"non-finite position delta (target 2, vertex 1)", dP=db)
        db = dN.copy()
        db[1, 2, 2] = bad                                     # (in the target that is not in use)
        refused(b"non-finite normal delta (target 1, normal 2)", dN=db)
    wb, db = w.copy(), dP.copy()
    wb[2], db[0, 0, 0] = np.nan, np.nan
    refused(b"non-finite weight (target 2)", w=wb, dP=db)     # the weights before the deltas
    assert np.all(vo == 7) and np.all(no == 7)                # a refused call writes nothing
    assert call(nv=0, nn=0) == 0                              # nothing to do is not an error
    assert call(nn=0, n=None, no=None, dN=None) == 0
    assert call(T=4096, w=np.zeros(4096, F), nv=0, nn=0) == 0
