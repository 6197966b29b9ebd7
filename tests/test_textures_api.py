"""Image textures, CPU side: the two C entry points and their argument checks that need no context, and the numpy model of the
lookup (tests/texture_model.py) against hand-computed cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import texture_model as tm
from helpers import assert_exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ERR_INVALID = -1   # AGPT_ERR_INVALID (include/agpt.h)


def header():
    return open(os.path.join(ROOT, "include", "agpt.h")).read()


def test_symbols_are_declared_and_exported():
    h = header()
    assert re.search(r"int agpt_scene_add_texture\(agpt_scene\*, const float\* rgb, int width, int height\);", h)
    assert re.search(r"int agpt_scene_set_material_texture\(agpt_scene\*, int material, int texture\);", h)
    assert_exported(("agpt_scene_add_texture", "agpt_scene_set_material_texture"))
    L = ag.lib()
    assert L.agpt_scene_add_texture.argtypes == [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int]
    assert L.agpt_scene_set_material_texture.argtypes == [C.c_void_p, C.c_int, C.c_int]


def test_null_arguments_are_invalid_with_a_message():
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    rgb = (C.c_float * 3)(1, 1, 1)
    assert L.agpt_scene_add_texture(None, rgb, 1, 1) == ERR_INVALID
    assert b"agpt_scene_add_texture" in L.agpt_last_error()
    assert L.agpt_scene_set_material_texture(None, 0, 0) == ERR_INVALID
    assert b"agpt_scene_set_material_texture" in L.agpt_last_error()


@pytest.mark.gpu
def test_documented_errors_on_a_scene():
    from helpers import gpu_context
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    s = ag.Scene(gpu_context())
    try:
        rgb = np.ones((2, 2, 3), F)
        p = rgb.ctypes.data_as(C.POINTER(C.c_float))
        for w, h in ((0, 2), (2, 0), (-1, 2), (2, -3)):
            assert L.agpt_scene_add_texture(s.h, p, w, h) == ERR_INVALID and L.agpt_last_error()
        assert L.agpt_scene_add_texture(s.h, None, 2, 2) == ERR_INVALID
        tex = s.add_texture(rgb)
        assert tex == 0 and s.add_texture(rgb[:1]) == 1
        mat = s.add_material(ag.MAT_DISNEY, [.5, .5, .5], .5, 0.)
        for m, t in ((-1, 0), (1, 0), (0, 2), (0, -2)):
            assert L.agpt_scene_set_material_texture(s.h, m, t) == ERR_INVALID and L.agpt_last_error()
        s.set_material_texture(mat, tex)
        s.set_material_texture(mat, -1)
        s.set_material_texture(mat, tex)
        # a textured material on a sphere or a plane: commit refuses, and says why
        sphere_scene = ag.Scene(gpu_context())
        try:
            m2 = sphere_scene.add_material(ag.MAT_DISNEY, [.5, .5, .5], .5, 0.)
            sphere_scene.set_material_texture(m2, sphere_scene.add_texture(rgb))
            sphere_scene.add_sphere([0, 0, 0], 1.0, m2)
            assert L.agpt_scene_commit(sphere_scene.h) == ERR_INVALID
            assert b"sphere or a plane" in L.agpt_last_error()
            sphere_scene.set_material_texture(m2, -1)
            sphere_scene.commit()
        finally:
            sphere_scene.close()
        plane_scene = ag.Scene(gpu_context())
        try:
            m3 = plane_scene.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
            plane_scene.set_material_texture(m3, plane_scene.add_texture(rgb))
            plane_scene.add_plane([0, 0, 0], [2, 2], m3)
            assert L.agpt_scene_commit(plane_scene.h) == ERR_INVALID
        finally:
            plane_scene.close()
        # after commit both calls are refused
        v, n, t, idx = ag.scenes.heightfield(2)
        s.add_mesh(v, n, t, idx, mat, 1)
        s.set_camera([0, 3, 3], [0, 0, 0], [0, 1, 0], 1.0)
        s.commit()
        assert L.agpt_scene_add_texture(s.h, p, 2, 2) == ERR_INVALID and b"committed" in L.agpt_last_error()
        assert L.agpt_scene_set_material_texture(s.h, mat, -1) == ERR_INVALID and b"committed" in L.agpt_last_error()
    finally:
        s.close()


def test_scene_descriptions_carry_textures():
    d = ag.scenes.scene_textured()
    kinds = [op[0] for op in d.ops]
    assert kinds.count("texture") == 2 and kinds.count("material_texture") == 2 and d.n_textures == 2
    plain = ag.scenes.scene_c1()
    assert [op[0] for op in plain.ops] == kinds[:len(plain.ops)] and "texture" not in [op[0] for op in plain.ops]

    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append(name) or 0

    r = d.instantiate(Recorder())
    assert r.calls.count("add_texture") == 2 and r.calls.count("set_material_texture") == 2
    tex = ag.scenes.checker_texture(16, 8, 4)
    assert tex.shape == (8, 16, 3) and tex.dtype == F and len(np.unique(tex.reshape(-1, 3), axis=0)) > 8


# ---- the model against hand-computed cases ---------------------------------------------------------------------------
def test_uv_interpolation_by_hand():
    # the default coordinates (0,0) (1,0) (1,1): b0 = 1 - .25 - .5 = .25, u = 0 * .25 + 1 * .25 + 1 * .5, v = 0 + 0 + 1 * .5
    u, v = tm.interpolate_uv([0, 0], [1, 0], [1, 1], F(.25), F(.5))
    assert (u, v) == (F(.75), F(.5))
    # fp32 rounding of every step: b0 = fl(fl(1 - .1f) - .2f), products rounded before the sums, left to right
    b1, b2 = F(.1), F(.2)
    b0 = F(F(1) - b1) - b2
    uv0, uv1, uv2 = np.array([.3, .7], F), np.array([-1.5, 2.25], F), np.array([4.1, .05], F)
    u, v = tm.interpolate_uv(uv0, uv1, uv2, b1, b2)
    assert u == F(F(F(uv0[0] * b0) + F(uv1[0] * b1)) + F(uv2[0] * b2))
    assert v == F(F(F(uv0[1] * b0) + F(uv1[1] * b1)) + F(uv2[1] * b2))
    # a batch
    U, V = tm.interpolate_uv(np.stack([uv0, uv0]), np.stack([uv1, uv1]), np.stack([uv2, uv2]), np.array([b1, b1]), np.array([b2, b2]))
    assert U.tolist() == [u, u] and V.tolist() == [v, v]


@pytest.mark.parametrize("shape,u,v,xy", [
    ((2, 4), .3, .6, (0, 0)),      # floor(1.2 - .5) = 0, floor(1.2 - .5) = 0
    ((2, 4), 1.0, 1.0, (3, 1)),    # u = 1 exactly: floor(3.5) = 3 -- the last texel, no wrap; floor(1.5) = 1
    ((2, 4), -.1, .5, (3, 0)),     # negative: floor(-.9) = -1 -> Mod -> 3; floor(.5) = 0
    ((2, 4), .05, .1, (3, 1)),     # the half-texel shift wraps the first half texel: floor(-.3) = -1 -> 3, floor(-.3) -> 1
    ((2, 4), 1.3, 1.8, (0, 1)),    # > 1: floor(4.7) = 4 -> 0; floor(3.1) = 3 -> 1
    ((2, 4), 2.7, -1.2, (2, 1)),   # floor(10.3) = 10 -> 2; floor(-2.9) = -3 -> -3 - (-1) * 2 = -1 -> 1
    ((1, 1), .37, -5.2, (0, 0)),   # 1x1: always its one texel
    ((1, 1), 123.4, 1.0, (0, 0)),
    ((5, 3), .5, .5, (1, 2)),      # non-square (width 3, height 5): floor(1.0) = 1, floor(2.0) = 2
    ((5, 3), .49, .49, (0, 1)),    # floor(.97) = 0, floor(1.95) = 1
    ((5, 3), float("nan"), .5, (0, 0)), ((5, 3), .5, float("inf"), (0, 0)),   # non-finite: texel (0, 0)
])
def test_lookup_by_hand(shape, u, v, xy):
    x, y = tm.texel_index(shape, F(u), F(v))
    assert (int(x), int(y)) == xy
    tex = np.arange(shape[0] * shape[1] * 3, dtype=F).reshape(shape[0], shape[1], 3)
    assert tm.value(tex, F(u), F(v)).tolist() == tex[xy[1], xy[0]].tolist()


def test_mod_is_the_reference_mod():
    for b in (1, 3, 4, 7):
        for a in range(-3 * b - 1, 3 * b + 2):
            r = a - int(a / b) * b   # C: truncating division
            assert int(tm.mod(a, b)) == (r + b if r < 0 else r) == a % b


def test_boundary_distance():
    # width 4: u = .375 -> position 1.0, on a boundary; u = .4 -> 1.1, a tenth of a texel away
    assert tm.boundary_distance((4, 4), F(.375), F(.5625)) == 0
    assert abs(tm.boundary_distance((4, 4), F(.4), F(.5)) - .1) < 1e-6
