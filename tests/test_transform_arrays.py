"""agpt_transform_arrays, CPU side: the host-only twin of agpt_scene_transform_mesh against the OBJ loader, whose `transform16`
arithmetic tests/golden/obj_cases.npz pins to the reference's mat4 -- the rest arrays are the parse with a NULL transform, and the
twin's outputs must be the bytes of the parse with transform16 = M."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import assert_exported
from transform_cases import MATRICES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "agpt.h")).read()
F = np.float32


def obj_text(with_normals, seed=4, n=37):
    """a fan of triangles over n vertices with awkward decimals (and n normals that are not unit length)"""
    rng = np.random.RandomState(seed)
    lines = ["v %.7g %.7g %.7g" % tuple(p) for p in rng.uniform(-3, 3, (n, 3))]
    lines += ["v 0 0 0", "v -0.0 1e-20 3.5e8"]
    n += 2
    if with_normals:
        lines += ["vn %.7g %.7g %.7g" % tuple(p) for p in rng.normal(size=(n, 3))]
    for k in range(1, n - 1):
        a, b, c = 1, k + 1, k + 2
        lines.append(("f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c)) if with_normals else "f %d %d %d" % (a, b, c))
    return "\n".join(lines) + "\n"


def test_symbols_declared_and_exported():
    names = ("agpt_transform_arrays", "agpt_scene_transform_mesh", "agpt_scene_update_mesh_device")
    assert_exported(names)
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, HEADER), name


@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_twin_equals_the_obj_loader(name, with_normals):
    M = MATRICES[name]
    text = obj_text(with_normals)
    rest_v, rest_n, _, idx = ag.load_obj(text=text)
    want_v, want_n, _, want_idx = ag.load_obj(text=text, transform=M)
    assert (rest_n is not None) == with_normals and np.array_equal(idx, want_idx)
    got_v, got_n = ag.transform_arrays(M, rest_v, rest_n)
    assert got_v.tobytes() == want_v.tobytes()
    if with_normals:
        assert got_n.tobytes() == want_n.tobytes()
    else:
        assert got_n is None
    if name == "identity":
        assert got_v.tobytes() == rest_v.tobytes()
    else:
        assert got_v.tobytes() != rest_v.tobytes()
    if name == "projective":   # the branch is taken: some w differs from 1
        w = rest_v.astype(np.float64) @ M[3, :3].astype(np.float64) + M[3, 3]
        assert np.all(np.abs(w - 1) > 1e-3)


def test_in_place_and_null_normals():
    M = MATRICES["scale+shear"]
    v, n, _, _ = ag.load_obj(text=obj_text(True))
    want_v, want_n = ag.transform_arrays(M, v, n)
    L, fp = ag.lib(), C.POINTER(C.c_float)
    m = np.ascontiguousarray(M).reshape(16)
    vi, ni = v.copy(), n.copy()
    assert L.agpt_transform_arrays(m.ctypes.data_as(fp), vi.ctypes.data_as(fp), len(vi), ni.ctypes.data_as(fp), len(ni),
                                   vi.ctypes.data_as(fp), ni.ctypes.data_as(fp)) == 0
    assert vi.tobytes() == want_v.tobytes() and ni.tobytes() == want_n.tobytes()
    out = np.zeros_like(v)
    assert L.agpt_transform_arrays(m.ctypes.data_as(fp), v.ctypes.data_as(fp), len(v), None, 0, out.ctypes.data_as(fp), None) == 0
    assert out.tobytes() == want_v.tobytes()


def test_null_and_count_validation():
    L, fp = ag.lib(), C.POINTER(C.c_float)
    m = np.eye(4, dtype=F).reshape(16)
    v = np.arange(9, dtype=F).reshape(3, 3)
    n = np.ones((2, 3), F)
    vo, no = np.full_like(v, 7), np.full_like(n, 7)
    pm, pv, pn, pvo, pno = (a.ctypes.data_as(fp) for a in (m, v, n, vo, no))
    for args in ((None, pv, 3, pn, 2, pvo, pno), (pm, None, 3, pn, 2, pvo, pno), (pm, pv, 3, pn, 2, None, pno),
                 (pm, pv, -1, pn, 2, pvo, pno), (pm, pv, 3, pn, -2, pvo, pno), (pm, pv, 3, None, 2, pvo, pno),
                 (pm, pv, 3, pn, 2, pvo, None)):
        assert L.agpt_transform_arrays(*args) == -1
        assert b"agpt_transform_arrays" in L.agpt_last_error()
    assert np.all(vo == 7) and np.all(no == 7)   # a refused call writes nothing
    assert L.agpt_transform_arrays(pm, pv, 0, None, 0, pvo, None) == 0   # nothing to do is not an error


def test_a_singular_matrix_keeps_the_loaders_rule():
    """det == 0 (exactly): the reference's Inverted() returns the identity, so the normals pass through unchanged; agpt_obj_parse and
    the twin agree.  (agpt_scene_transform_mesh refuses such a matrix instead.)"""
    M = np.array([[1, 2, 3, 0], [2, 4, 6, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F)
    text = obj_text(True)
    rest_v, rest_n, _, _ = ag.load_obj(text=text)
    want_v, want_n, _, _ = ag.load_obj(text=text, transform=M)
    got_v, got_n = ag.transform_arrays(M, rest_v, rest_n)
    assert got_v.tobytes() == want_v.tobytes() and got_n.tobytes() == want_n.tobytes() == rest_n.tobytes()
