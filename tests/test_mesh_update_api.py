"""agpt_scene_update_mesh / agpt_bvh_refit, CPU side: the symbols, the errors reachable without a device, the host refit against the
builder, against the numpy model (tests/bvh_refit_model.py) and against containment, and the premise the GPU tests rest on -- a tree
refitted to vertices scaled by 2 IS the tree built from them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import bvh_refit_model as model
import mesh_update_cases as cases
from helpers import assert_exported, bits, build_cpp_example, signed_zero_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "agpt.h")).read()
F = np.float32
MESHES = [(pose, mpn) for pose in (0, 1) for mpn in (1, 4)]


def test_symbols_declared_and_exported():
    names = ("agpt_scene_update_mesh", "agpt_bvh_refit")
    assert_exported(names)
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, HEADER), name
    assert re.search(r"AGPT_UPDATE_REFIT\s*=\s*0\b", HEADER) and ag.UPDATE_REFIT == 0
    assert re.search(r"AGPT_UPDATE_REBUILD\s*=\s*1\b", HEADER) and ag.UPDATE_REBUILD == 1
    assert "slower to" in HEADER and "REBUILD" in HEADER   # the documented consequence of refitting far from the build pose


def test_null_scene_is_invalid_before_anything_else():
    L = ag.lib()
    v = np.zeros((3, 3), F)
    pv = v.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((None, 0, pv, 3, None, 0, 0), (None, -5, None, 0, None, 0, 7)):
        assert L.agpt_scene_update_mesh(*args) == -1
        assert b"agpt_scene_update_mesh" in L.agpt_last_error() and b"NULL" in L.agpt_last_error()


def test_refit_refuses_bad_arguments_and_leaves_the_tree_alone():
    v, _, _, idx = cases.blob(0)
    nodes, order, _ = ag.bvh_build(v, idx, 1)
    L = ag.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    ix = np.ascontiguousarray(idx, np.int32)
    assert L.agpt_bvh_refit(None, len(v), ix.ctypes.data_as(ip), len(ix), order.ctypes.data_as(ip), nodes.ctypes.data_as(C.c_void_p),
                            len(nodes) - 1) == -1
    assert b"agpt_bvh_refit" in L.agpt_last_error()
    assert L.agpt_bvh_refit(v.ctypes.data_as(fp), len(v), ix.ctypes.data_as(ip), len(ix), None, nodes.ctypes.data_as(C.c_void_p),
                            len(nodes) - 1) == -1
    broken = nodes.copy()
    broken["first"][0] = 0   # a child pair that is not behind its parent
    before = broken.tobytes()
    with pytest.raises(ag.AgptError, match="agpt_bvh_refit"):
        ag.bvh_refit(v, idx, order, broken)
    assert broken.tobytes() == before
    bad_order = order.copy()
    bad_order[5] = 3 * len(order)
    with pytest.raises(ag.AgptError, match="prim_index"):
        ag.bvh_refit(v, idx, bad_order, nodes)


@pytest.mark.parametrize("pose,mpn", MESHES)
def test_refit_with_the_build_vertices_returns_the_build(pose, mpn):
    v, _, _, idx = cases.blob(pose)
    nodes, order, _ = ag.bvh_build(v, idx, mpn)
    scrubbed = nodes.copy()
    used = np.arange(len(nodes)) != 1   # (slot 1 is the unused one: nobody writes it)
    scrubbed["bmin"][used], scrubbed["bmax"][used] = 7.0, -7.0
    assert ag.bvh_refit(v, idx, order, scrubbed).tobytes() == nodes.tobytes()


@pytest.mark.parametrize("mpn", [1, 4])
def test_refit_of_the_signed_zero_grid_returns_the_build_bit_for_bit(mpn):
    """The tie rule of the shared box: tminf / tmaxf keep the later of equal operands, so whether a bound is +0 or -0 depends on the
    order "box per primitive, then union over the leaf's slots" -- the refit must reproduce the builder's signs."""
    v, idx = signed_zero_grid(12)   # 288 triangles
    nodes, order, _ = ag.bvh_build(v, idx, mpn)
    used = np.arange(len(nodes)) != 1
    assert (nodes["count"][used] > 1).any()   # multi-slot leaves
    for f in ("bmin", "bmax"):   # zeros of both signs among the bounds
        zero = nodes[f][used] == 0
        assert (zero & np.signbit(nodes[f][used])).any() and (zero & ~np.signbit(nodes[f][used])).any()
    scrubbed = nodes.copy()
    scrubbed["bmin"][used], scrubbed["bmax"][used] = 7.0, -7.0
    got = ag.bvh_refit(v, idx, order, scrubbed)
    assert np.array_equal(bits(got["bmin"]), bits(nodes["bmin"])) and np.array_equal(bits(got["bmax"]), bits(nodes["bmax"]))
    assert np.array_equal(got["first"], nodes["first"]) and np.array_equal(got["count"], nodes["count"])


@pytest.mark.parametrize("pose,mpn", MESHES)
def test_refit_with_deformed_vertices_equals_the_model_and_contains_its_subtrees(pose, mpn):
    v, _, _, idx = cases.blob(pose)
    w = cases.blob(1 - pose)[0]
    w = w.copy()
    w[7] = [-0.0, 0.0, -0.0]   # signed zeros: the comparisons' order shows
    w[9] = [0.0, -0.0, 0.0]
    nodes, order, _ = ag.bvh_build(v, idx, mpn)
    got = ag.bvh_refit(w, idx, order, nodes)
    assert got.tobytes() == model.refit(nodes, order, w, idx).tobytes()
    assert np.array_equal(got["first"], nodes["first"]) and np.array_equal(got["count"], nodes["count"])
    for i in [0] + list(range(2, len(got))):
        p = w[model.subtree_vertices(got, order, idx, i)]
        assert np.all(p >= got["bmin"][i]) and np.all(p <= got["bmax"][i]), i
        assert np.array_equal(p.min(0), got["bmin"][i]) and np.array_equal(p.max(0), got["bmax"][i])   # and is tight


@pytest.mark.parametrize("pose,mpn", MESHES)
def test_scaling_by_two_commutes_with_the_build(pose, mpn):
    """Every quantity the builder compares scales by an exact power of two, so build(2 v) == refit(build(v), 2 v), byte for byte: the
    premise of test_gpu_mesh_update.py's oracle-backed REFIT test, for its meshes (offsets and scale as cases.scene applies them)."""
    v = cases.blob(pose)[0]
    idx = cases.blob(pose)[3]
    for offset in ([0, 0, 0], [2.4, 0, 0.5]):
        base = v + np.array(offset, F)
        nodes, order, depth = ag.bvh_build(base, idx, mpn)
        nodes2, order2, depth2 = ag.bvh_build(base * F(2), idx, mpn)
        assert np.array_equal(order, order2) and depth == depth2
        assert ag.bvh_refit(base * F(2), idx, order, nodes).tobytes() == nodes2.tobytes()


def test_cpp_animated_example_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "animated_scene")
