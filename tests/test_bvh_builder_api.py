"""CPU checks of the device BVH builder's interface: the symbols are declared and exported, the tier constants agree
between include/agpt.h and the binding, and NULL handles fail loudly with the function's name."""
import ctypes as C
import os
import re

import numpy as np

import ag_pathtracer_amd as ag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "agpt.h")).read()


def test_new_symbols_declared_and_exported():
    L = ag.lib()
    for name in ("agpt_scene_set_bvh_builder", "agpt_bvh_build_device"):
        assert re.search(r"\b%s\s*\(" % name, HEADER), name
        assert name in ag.EXPORTS
        assert hasattr(L, name)


def test_builder_and_tier_constants_match_header():
    def enum_value(name):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, HEADER)
        assert m, name
        return int(m.group(1))
    assert enum_value("AGPT_BVH_BUILDER_HOST") == ag.binding.BVH_BUILDER_HOST == 0
    assert enum_value("AGPT_BVH_BUILDER_DEVICE") == ag.binding.BVH_BUILDER_DEVICE == 1
    assert enum_value("AGPT_BVH_DEVICE_LANE_MAX") == ag.BVH_DEVICE_LANE_MAX
    assert enum_value("AGPT_BVH_DEVICE_CHUNK") == ag.BVH_DEVICE_CHUNK
    assert 2 <= ag.BVH_DEVICE_LANE_MAX < ag.BVH_DEVICE_CHUNK


def test_null_scene_and_context_are_invalid():
    L = ag.lib()
    assert L.agpt_scene_set_bvh_builder(None, 1) == -1
    assert b"agpt_scene_set_bvh_builder" in L.agpt_last_error()
    v = np.zeros((3, 3), np.float32)
    ix = np.zeros((3, 3), np.int32)
    ix[:, 0] = [0, 1, 2]
    nodes = np.zeros(4, ag.NODE_DTYPE)
    order = np.zeros(1, np.int32)
    total, depth, on_dev = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = L.agpt_bvh_build_device(None, v.ctypes.data_as(C.POINTER(C.c_float)), 3, ix.ctypes.data_as(C.POINTER(C.c_int32)), 3, 1,
                                 nodes.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.POINTER(C.c_int32)),
                                 C.byref(total), C.byref(depth), C.byref(on_dev))
    assert rc == -1
    assert b"agpt_bvh_build_device" in L.agpt_last_error()
