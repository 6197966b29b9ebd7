"""agpt_vertex_normals_arrays, CPU side: the host-only twin of the AGPT_NORMALS_SMOOTH mode against the numpy model of its definition
(normals_model.py), on uint32 views with no tolerance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_update_cases as dc
import normals_cases as nc
import normals_model
from helpers import assert_exported, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "agpt.h")).read()
F = np.float32


def same_bits(got, want):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))


def twin_equals_model(case):
    got = ag.vertex_normals_arrays(*case)
    same_bits(got, normals_model.vertex_normals_arrays(*case))
    return got


def test_symbols_declared_and_exported():
    names = ("agpt_vertex_normals_arrays", "agpt_scene_set_mesh_normals_mode")
    assert_exported(names)
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, HEADER), name
        assert name in ag.binding.EXPORTS
    assert re.search(r"AGPT_NORMALS_GIVEN = 0, AGPT_NORMALS_SMOOTH = 1", HEADER)
    assert (ag.NORMALS_GIVEN, ag.NORMALS_SMOOTH) == (0, 1)
    assert hasattr(ag, "vertex_normals_arrays") and hasattr(ag.Scene, "set_mesh_normals_mode")


@pytest.mark.parametrize("pose", [0, 1])
@pytest.mark.parametrize("prim", nc.ZOO_WITH_NORMALS)
def test_twin_equals_the_model_on_the_zoo(prim, pose):
    got = twin_equals_model(nc.zoo_case(prim, pose))
    length = np.linalg.norm(got.astype(np.float64), axis=1)
    named = np.zeros(len(got), bool)
    named[nc.zoo_case(prim)[1][:, 1]] = True
    assert np.allclose(length[named], 1, atol=1e-6) and (got[~named] == 0).all() and not np.signbit(got[~named]).any()


def test_one_normal_per_triangle():
    case = nc.flat_grid()
    assert len(case[0]) == 170 and case[2] == 288
    got = twin_equals_model(case)
    # an item named by the three corners of one triangle: g + g + g, normalised -- the triangle's own direction
    g = np.array(normals_model.face_vectors(case[0], case[1]), np.float64)
    assert np.allclose(got, g / np.linalg.norm(g, axis=1, keepdims=True), atol=1e-6)


def test_a_grid_of_33_by_33():
    case = nc.grid(33)
    assert case[2] == 1089
    twin_equals_model(case)


@pytest.mark.parametrize("flip", [False, True])
def test_an_exact_plane_gives_exact_unit_normals(flip):
    case = nc.plane_grid(flip=flip)
    got = twin_equals_model(case)
    assert (got == np.array([0, -1 if flip else 1, 0], F)).all()


@pytest.mark.parametrize("name", sorted(nc.specials()))
def test_defined_zeros_and_nothing_else_touched(name):
    case, zeros = nc.specials()[name]
    got = twin_equals_model(case)
    base = ag.vertex_normals_arrays(*nc._extended([], [], 0))
    assert len(base) == 170
    for j in zeros:
        assert got[j].tobytes() == np.zeros(3, F).tobytes(), j         # +0, not -0
    others = [j for j in range(169) if j not in zeros]
    assert len(others) >= 150
    same_bits(got[others], base[others])
    assert (np.abs(np.linalg.norm(base[others].astype(np.float64), axis=1) - 1) < 1e-6).all()
    if name == "unreferenced":
        assert np.abs(np.linalg.norm(got[170].astype(np.float64)) - 1) < 1e-6   # the item between the two unreferenced ones


def test_one_normal_shared_by_every_corner():
    case = nc.shared_normal()
    assert len(case[1]) == 864 and case[2] == 1
    got = twin_equals_model(case)
    assert abs(np.linalg.norm(got[0].astype(np.float64)) - 1) < 1e-6


def test_a_fan_of_200_triangles():
    case = nc.fan(200)
    assert int((case[1][:, 1] == 0).sum()) == 200
    got = twin_equals_model(case)
    assert got[0, 1] > 0.9


def test_the_order_of_the_sum_is_observable():
    """the precondition of every comparison here: summing an item's corners backwards changes bits, so a wrong order cannot pass"""
    v, _, ix = dc.bumpy_grid(True)
    proper = normals_model.vertex_normals_arrays(v, ix, len(v))
    backwards = normals_model.vertex_normals_arrays(v, ix, len(v), reverse=True)
    differ = (bits(proper) != bits(backwards)).any(axis=1)
    assert differ.any()
    assert np.allclose(proper, backwards, atol=1e-6)
    same_bits(ag.vertex_normals_arrays(v, ix, len(v)), proper)


def test_a_refused_call_writes_nothing():
    L = ag.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    v, ix, nn = nc.zoo_case(nc.ZOO_WITH_NORMALS[1])
    ix = np.ascontiguousarray(ix, np.int32)
    poison = np.full((nn, 3), 7.25, F)
    out = poison.copy()
    pv, pi, po = v.ctypes.data_as(fp), ix.ctypes.data_as(ip), out.ctypes.data_as(fp)

    def refused(what, *args):
        assert L.agpt_vertex_normals_arrays(*args) == -1
        assert b"agpt_vertex_normals_arrays" in L.agpt_last_error() and what in L.agpt_last_error(), L.agpt_last_error()
        assert out.tobytes() == poison.tobytes()
    refused(b"NULL", None, len(v), pi, len(ix), nn, po)
    refused(b"NULL", pv, len(v), None, len(ix), nn, po)
    assert L.agpt_vertex_normals_arrays(pv, len(v), pi, len(ix), nn, None) == -1
    refused(b"positive", pv, 0, pi, len(ix), nn, po)
    refused(b"positive", pv, -1, pi, len(ix), nn, po)
    refused(b"positive", pv, len(v), pi, len(ix), 0, po)
    refused(b"positive", pv, len(v), pi, len(ix), -3, po)
    for k in (0, 2, 4, -3):
        refused(b"multiple of 3", pv, len(v), pi, k, nn, po)
    for row, col, value, what in ((5, 0, len(v), b"vertex index"), (len(ix) - 1, 0, -1, b"vertex index"), (7, 1, nn, b"normal index"),
                                  (len(ix) - 1, 1, -1, b"normal index")):
        bad = ix.copy()
        bad[row, col] = value
        refused(what, pv, len(v), bad.ctypes.data_as(ip), len(ix), nn, po)
    refused(b"vertex index", pv, len(v) - 1, pi, len(ix), nn, po)      # the last vertex is now out of range
    refused(b"normal index", pv, len(v), pi, len(ix), nn - 1, po)
    assert L.agpt_vertex_normals_arrays(pv, len(v), pi, len(ix), nn, po) == 0
    same_bits(out, normals_model.vertex_normals_arrays(v, ix, nn))
    with pytest.raises(ag.AgptError):
        ag.vertex_normals_arrays(v, ix, 0)
