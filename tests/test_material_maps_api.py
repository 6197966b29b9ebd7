"""Roughness / metallic maps (agpt_scene_set_material_param_texture), the interface: the declaration, the export, the binding, the
argument checks that need no context (CPU) and the documented errors on a live scene (GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ag_pathtracer_amd as ag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ERR_INVALID = -1   # AGPT_ERR_INVALID (include/agpt.h)
NAME = "agpt_scene_set_material_param_texture"


def test_symbol_is_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "agpt.h")).read()
    assert re.search(r"int agpt_scene_set_material_param_texture\(agpt_scene\*, int material, int param, int texture, int channel\);", h)
    assert re.search(r"enum \{ AGPT_PARAM_ROUGHNESS = 0, AGPT_PARAM_METALLIC = 1 \};", h)
    L = ag.lib()
    assert NAME in ag.EXPORTS and hasattr(L, NAME)
    assert getattr(L, NAME).argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    assert (ag.PARAM_ROUGHNESS, ag.PARAM_METALLIC) == (0, 1)


def test_null_scene_is_invalid_with_a_message():
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    assert L.agpt_scene_set_material_param_texture(None, 0, ag.PARAM_ROUGHNESS, 0, 0) == ERR_INVALID
    assert NAME.encode() in L.agpt_last_error()


def test_scene_descriptions_carry_the_maps():
    d = ag.scenes.scene_mapped()
    base = ag.scenes.scene_textured()
    assert [op[0] for op in d.ops[:len(base.ops)]] == [op[0] for op in base.ops]     # scene_textured()'s geometry, then the maps
    extra = d.ops[len(base.ops):]
    assert [op[0] for op in extra] == ["texture"] + ["material_param_texture"] * 4
    image = extra[0][1]
    assert set(np.unique(image[..., 2])) == {0.0, 1.0} and len(np.unique(image[..., 1])) > 8
    assert {(op[1], op[2]) for op in extra[1:]} == {(0, ag.PARAM_ROUGHNESS), (0, ag.PARAM_METALLIC), (2, ag.PARAM_ROUGHNESS), (2, ag.PARAM_METALLIC)}
    assert all(op[3] == d.n_textures - 1 for op in extra[1:])            # one image for both parameters

    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append((name, a)) or 0

    r = d.instantiate(Recorder())
    got = [a for name, a in r.calls if name == "set_material_param_texture"]
    assert got == [op[1:] for op in extra[1:]]


@pytest.mark.gpu
def test_documented_errors_on_a_scene():
    from helpers import gpu_context
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    call = L.agpt_scene_set_material_param_texture
    R, M = ag.PARAM_ROUGHNESS, ag.PARAM_METALLIC
    rgb = np.full((2, 2, 3), .5, F)
    s = ag.Scene(gpu_context())
    try:
        tex = s.add_texture(rgb)
        mat = s.add_material(ag.MAT_DISNEY, [.5, .5, .5], .5, 0.)
        mirror = s.add_material(ag.MAT_MIRROR, [.5, .5, .5], 0., 0.)
        diffuse = s.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
        # unknown material, param, texture, channel
        for args in ((-1, R, tex, 0), (3, R, tex, 0), (mat, -1, tex, 0), (mat, 2, tex, 0), (mat, R, 1, 0), (mat, R, -2, 0),
                     (mat, M, tex, -1), (mat, M, tex, 3)):
            assert call(s.h, *args) == ERR_INVALID and NAME.encode() in L.agpt_last_error(), args
        # mirror and diffuse-only materials have neither parameter
        for m in (mirror, diffuse):
            assert call(s.h, m, R, tex, 0) == ERR_INVALID and b"AGPT_MAT_DISNEY" in L.agpt_last_error()
        # set -> clear -> set; the channel of a cleared slot is ignored
        s.set_material_param_texture(mat, R, tex, 1)
        s.set_material_param_texture(mat, R, -1, 77)
        s.set_material_param_texture(mat, R, tex, 2)
        s.set_material_param_texture(mat, M, tex, 0)
        # a mapped material on a sphere or a plane: commit refuses, and says why; without the map it commits
        for add in (lambda sc, m: sc.add_sphere([0, 0, 0], 1.0, m), lambda sc, m: sc.add_plane([0, 0, 0], [2, 2], m)):
            for param in (R, M):
                other = ag.Scene(gpu_context())
                try:
                    m2 = other.add_material(ag.MAT_DISNEY, [.5, .5, .5], .5, 0.)
                    other.set_material_param_texture(m2, param, other.add_texture(rgb), 0)
                    add(other, m2)
                    other.set_camera([0, 3, 3], [0, 0, 0], [0, 1, 0], 1.0)
                    assert L.agpt_scene_commit(other.h) == ERR_INVALID
                    msg = L.agpt_last_error()
                    assert b"sphere or a plane" in msg and b"roughness / metallic map" in msg
                    other.set_material_param_texture(m2, param, -1)
                    other.commit()
                finally:
                    other.close()
        # after commit the call is refused
        v, n, t, idx = ag.scenes.heightfield(2)
        s.add_mesh(v, n, t, idx, mat, 1)
        s.set_camera([0, 3, 3], [0, 0, 0], [0, 1, 0], 1.0)
        s.commit()
        assert call(s.h, mat, R, -1, 0) == ERR_INVALID and b"committed" in L.agpt_last_error()
        assert call(s.h, mat, M, tex, 0) == ERR_INVALID and b"committed" in L.agpt_last_error()
    finally:
        s.close()
