"""Normal maps, CPU side and argument checks (agpt_scene_set_material_normal_texture, agpt_kat_normal_map): the C entry points, every
documented error, the commit checks, the scene descriptions, and the numpy model (tests/normal_map_model.py) on hand-computed cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import normal_map_model as nm
from helpers import assert_exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ERR_INVALID = -1   # AGPT_ERR_INVALID (include/agpt.h)
FLAT = np.broadcast_to(np.array([.5, .5, 1], F), (4, 4, 3))
KINDS = [ag.MAT_DISNEY, ag.MAT_MIRROR, ag.MAT_DIFFUSE_ONLY]


def test_symbols_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "agpt.h")).read()
    assert re.search(r"int agpt_scene_set_material_normal_texture\(agpt_scene\*, int material, int texture, float scale\);", h)
    assert re.search(r"int agpt_kat_normal_map\(agpt_ctx\*, int n, const float\* ns3, const float\* ss3, const float\* rgb3, float scale, "
                     r"float\* ns_out3\);", h)
    assert_exported(("agpt_scene_set_material_normal_texture", "agpt_kat_normal_map"))
    assert ag.lib().agpt_scene_set_material_normal_texture.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_float]


def test_null_arguments_are_invalid_with_a_message():
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    assert L.agpt_scene_set_material_normal_texture(None, 0, 0, 1.0) == ERR_INVALID
    assert b"agpt_scene_set_material_normal_texture" in L.agpt_last_error()
    assert L.agpt_kat_normal_map(None, 1, None, None, None, 1.0, None) == ERR_INVALID
    assert b"agpt_kat_normal_map" in L.agpt_last_error()


def test_scene_descriptions_replay_the_slot_in_op_order():
    d = ag.SceneDesc("n")
    m = d.add_material(ag.MAT_MIRROR, [.5, .5, .5])
    t = d.add_texture(FLAT)
    d.set_material_normal_texture(m, t, 0.25)
    d.set_material_texture(m, t)
    d.set_material_normal_texture(m, -1)
    assert [op for op in d.ops if op[0] == "material_normal_texture"] == [("material_normal_texture", m, t, 0.25),
                                                                          ("material_normal_texture", m, -1, 1.0)]
    calls = []

    class Recorder:
        def __getattr__(self, name):
            return lambda *a: calls.append((name,) + (a if name.startswith("set_material") else ()))
    d.instantiate(Recorder())
    assert [c for c in calls if c[0].startswith("set_material")] == [
        ("set_material_normal_texture", m, t, 0.25), ("set_material_texture", m, t), ("set_material_normal_texture", m, -1, 1.0)]
    names = [c[0] for c in calls]
    assert names.index("add_texture") < names.index("set_material_normal_texture")


def test_model_on_hand_computed_cases():
    z, x = np.array([0, 0, 1], F), np.array([1, 0, 0], F)
    # the flat texel, whatever the scale: untouched, bit for bit (-0 included)
    ns = np.array([-0.0, 0.6, 0.8], F)
    for scale in (1, 3, 0):
        assert nm.perturb(ns, x, [.5, .5, 1], scale).tobytes() == ns.tobytes()
    # ts = cross(ns, ss) = cross(z, x) = +y: red tilts towards +x, green towards +y
    assert np.array_equal(nm.perturb(z, x, [1, .5, .5], 1), [1, 0, 0])
    assert np.array_equal(nm.perturb(z, x, [.5, 1, .5], 1), [0, 1, 0])
    assert np.array_equal(nm.perturb(z, x, [.5, 0, .5], 1), [0, -1, 0])
    got = nm.perturb(z, x, [1, .5, 1], 1)        # m = (1, 0, 1)
    inv = F(1) / np.sqrt(F(2))
    assert np.array_equal(got, np.array([inv, 0, inv], F))
    assert np.array_equal(nm.perturb(z, x, [1, .5, 1], 0), z)                   # scale 0: tx = ty = 0, tz > 0
    assert np.array_equal(nm.perturb(z, x, [.5, .5, 0], 1), [0, 0, -1])         # tz < 0 is not the no-op case
    assert np.array_equal(nm.perturb(z, x, [.5, .5, .5], 1), z)                 # m = 0
    assert np.array_equal(nm.perturb(z, x, [np.inf, .5, 1], 1), z) and np.array_equal(nm.perturb(z, x, [np.nan, .5, 1], 1), z)
    # a frame that is not orthogonal is used as it is
    ss = np.array([.8, 0, .6], F)
    m = ss * F(.5) + nm.cross(z, ss) * F(0) + z * F(1)
    assert np.array_equal(nm.perturb(z, ss, [.75, .5, 1], 1), nm.normalize(m.astype(F)))


def test_triangle_ss_is_the_normalized_dpdu():
    v, n, uv, idx = ag.scenes.grid_mesh(lambda U, V: np.stack([3 * U, 0 * U, 2 * V], -1), 2, 2)
    for tri in range(0, len(idx), 3):
        assert np.allclose(nm.triangle_ss((v, n, uv, idx), tri), [1, 0, 0], atol=1e-6)       # u runs along +x
    swapped = uv[:, ::-1].copy()
    assert np.allclose(nm.triangle_ss((v, n, swapped, idx), 0), [0, 0, 1], atol=1e-6)
    with pytest.raises(ValueError):
        nm.triangle_ss((v, n, np.zeros_like(uv), idx), 0)


def mesh_scene(kind=ag.MAT_DISNEY):
    from helpers import gpu_context
    s = ag.Scene(gpu_context())
    m = s.add_material(kind, [.5, .5, .5], .5, 0.)
    v, n, t, idx = ag.scenes.heightfield(2)
    s.add_mesh(v, n, t, idx, m, 1)
    s.set_camera([0, 3, 3], [0, 0, 0], [0, 1, 0], 1.0)
    return s, m


@pytest.mark.gpu
def test_documented_errors_on_a_scene():
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    f = L.agpt_scene_set_material_normal_texture
    s, m = mesh_scene()
    try:
        tex = s.add_texture(FLAT)
        for mat in (-1, m + 1, 9):
            assert f(s.h, mat, tex, 1.0) == ERR_INVALID and b"material id" in L.agpt_last_error()
        for t in (-2, tex + 1, 7):
            assert f(s.h, m, t, 1.0) == ERR_INVALID and b"texture id" in L.agpt_last_error()
        for scale in (float("inf"), float("-inf"), float("nan")):
            assert f(s.h, m, tex, scale) == ERR_INVALID and b"scale" in L.agpt_last_error()
        s.set_material_normal_texture(m, -1, float("nan"))          # (texture = -1: the scale is ignored)
        for scale in (1.0, 0.0, -2.5):
            s.set_material_normal_texture(m, tex, scale)
        s.commit()
        assert f(s.h, m, tex, 1.0) == ERR_INVALID and b"committed" in L.agpt_last_error()
        assert f(s.h, m, -1, 1.0) == ERR_INVALID and b"committed" in L.agpt_last_error()
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_any_material_type_takes_a_normal_map(kind):
    s, m = mesh_scene(kind)
    try:
        s.set_material_normal_texture(m, s.add_texture(FLAT), 2.0)
        s.commit()
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("analytic", ["sphere", "plane"])
def test_spheres_and_planes_refuse_the_material_at_commit_and_minus_one_restores_it(analytic):
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    s, m = mesh_scene()
    try:
        own = s.add_material(ag.MAT_DIFFUSE_ONLY, [.3, .3, .3])
        if analytic == "sphere":
            s.add_sphere([0, 2, 0], 0.5, own)
        else:
            s.add_plane([0, -2, 0], [4, 4], own)
        tex = s.add_texture(FLAT)
        s.set_material_normal_texture(m, tex)          # on the mesh's material: fine
        s.commit()
        s2, m2 = mesh_scene()
        try:
            own2 = s2.add_material(ag.MAT_DIFFUSE_ONLY, [.3, .3, .3])
            (s2.add_sphere([0, 2, 0], 0.5, own2) if analytic == "sphere" else s2.add_plane([0, -2, 0], [4, 4], own2))
            tex2 = s2.add_texture(FLAT)
            s2.set_material_normal_texture(own2, tex2, 0.5)
            assert L.agpt_scene_commit(s2.h) == ERR_INVALID and b"normal map" in L.agpt_last_error()
            s2.set_material_normal_texture(own2, -1)   # the plain material again
            s2.commit()
        finally:
            s2.close()
    finally:
        s.close()


@pytest.mark.gpu
def test_the_slot_is_independent_of_the_other_three():
    """each of the four slots alone makes a sphere's material unacceptable at commit, and clearing one slot clears that slot only"""
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    R, M = ag.PARAM_ROUGHNESS, ag.PARAM_METALLIC
    setters = {"colour": lambda s, m, t: s.set_material_texture(m, t), "roughness": lambda s, m, t: s.set_material_param_texture(m, R, t, 1),
               "metallic": lambda s, m, t: s.set_material_param_texture(m, M, t, 2), "normal": lambda s, m, t: s.set_material_normal_texture(m, t, 2.0)}
    s, _ = mesh_scene()
    try:
        m = s.add_material(ag.MAT_DISNEY, [.5, .5, .5], .5, 0.)
        s.add_sphere([0, 2, 0], 0.5, m)
        tex = s.add_texture(FLAT)
        for name, put in setters.items():
            put(s, m, tex)
            assert L.agpt_scene_commit(s.h) == ERR_INVALID, name
            put(s, m, -1)
            s.commit()
            s.add_material(ag.MAT_MIRROR, [1, 1, 1])     # (any add_* reopens the scene for the next round)
        # all four set; the other three cleared one by one: the normal slot alone still refuses, and only its own -1 clears it
        for put in setters.values():
            put(s, m, tex)
        for name in ("colour", "roughness", "metallic"):
            setters[name](s, m, -1)
            assert L.agpt_scene_commit(s.h) == ERR_INVALID
        assert b"normal map" in L.agpt_last_error()
        setters["normal"](s, m, -1)
        s.commit()
    finally:
        s.close()
