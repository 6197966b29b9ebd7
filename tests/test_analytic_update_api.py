"""agpt_scene_update_sphere / _plane / _spheres_device and the two radiance calls, CPU side: the symbols, the refusals reachable
without a device, the upper layers' names."""
import ctypes as C
import os
import re

import numpy as np

import ag_pathtracer_amd as ag
from helpers import assert_exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "agpt.h")).read()
F = np.float32
NAMES = ("agpt_scene_update_sphere", "agpt_scene_update_plane", "agpt_scene_set_area_light_radiance", "agpt_scene_set_infinite_light_radiance",
         "agpt_scene_update_spheres_device")


def test_symbols_declared_and_exported():
    assert_exported(NAMES)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, HEADER), name


def test_null_arguments_are_invalid_before_anything_else():
    L = ag.lib()
    fp = C.POINTER(C.c_float)
    v = np.ones(4, F)
    pv = v.ctypes.data_as(fp)
    ids = np.zeros(1, np.int32)
    pi = ids.ctypes.data_as(C.POINTER(C.c_int32))
    calls = {
        "agpt_scene_update_sphere": [(None, 0, pv, 1.0), (None, -3, None, float("nan"))],
        "agpt_scene_update_plane": [(None, 0, pv, pv), (None, 0, None, None)],
        "agpt_scene_set_area_light_radiance": [(None, 0, pv), (None, 9, None)],
        "agpt_scene_set_infinite_light_radiance": [(None, 0, pv), (None, -1, None)],
        "agpt_scene_update_spheres_device": [(None, pi, 1, C.c_void_p(16)), (None, None, -1, None), (None, pi, 0, None)],
    }
    for name, argsets in calls.items():
        for args in argsets:
            assert getattr(L, name)(*args) == -1, (name, args)
            assert name.encode() in L.agpt_last_error() and b"NULL" in L.agpt_last_error()


def test_upper_layers_name_the_calls():
    for m in ("update_sphere", "update_plane", "set_area_light_radiance", "set_infinite_light_radiance", "update_spheres"):
        assert callable(getattr(ag.Scene, m)), m
    hpp = open(os.path.join(ROOT, "include", "agpt_host.hpp")).read()
    for m, fn in zip(("updateSphere", "updatePlane", "setAreaLightRadiance", "setInfiniteLightRadiance", "updateSpheresDevice"), NAMES):
        assert re.search(r"\b%s\s*\(" % m, hpp) and fn in hpp, m
