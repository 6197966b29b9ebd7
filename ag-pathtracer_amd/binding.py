"""ctypes binding of libagpt_hip.so (include/agpt.h) and the host-side mirror of the reference's
Scene / Intersectable / Integrator surface for the path-tracing hot path.

The HIP library is the only compute path: if it cannot be loaded, or no GPU is present, every hot-path call
raises -- there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_LIB = None

MAT_DISNEY, MAT_MIRROR, MAT_DIFFUSE_ONLY = 0, 1, 2

RAY_DTYPE = np.dtype([("o", np.float32, 3), ("d", np.float32, 3), ("tmax", np.float32)])
HIT_DTYPE = np.dtype([("hit", np.int32), ("prim", np.int32), ("tri", np.int32),
                      ("t", np.float32), ("b1", np.float32), ("b2", np.float32)])
# agpt_scene_set_bvh_builder; work tiers of agpt_bvh_build_device (include/agpt.h)
BVH_BUILDER_HOST, BVH_BUILDER_DEVICE = 0, 1
# agpt_scene_update_mesh (include/agpt.h)
UPDATE_REFIT, UPDATE_REBUILD = 0, 1
NORMALS_GIVEN, NORMALS_SMOOTH = 0, 1
# agpt_scene_set_shading_arith (include/agpt.h)
SHADING_EXACT, SHADING_FAST = 0, 1
# agpt_scene_set_material_param_texture (include/agpt.h)
PARAM_ROUGHNESS, PARAM_METALLIC = 0, 1
# agpt_scene_set_texture_sampler (include/agpt.h)
FILTER_NEAREST, FILTER_BILINEAR = 0, 1
WRAP_REPEAT, WRAP_CLAMP, WRAP_MIRROR = 0, 1, 2
BVH_DEVICE_LANE_MAX, BVH_DEVICE_CHUNK = 64, 2048
NODE_DTYPE = np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("first", np.int32), ("count", np.int32)])

# every symbol include/agpt.h declares (tests check the library exports all of them)
EXPORTS = [
    "agpt_last_error", "agpt_version", "agpt_init", "agpt_set_stream", "agpt_destroy", "agpt_scene_create",
    "agpt_scene_destroy", "agpt_scene_add_material", "agpt_scene_add_mesh", "agpt_scene_add_sphere",
    "agpt_scene_add_plane", "agpt_scene_add_area_light", "agpt_scene_add_uniform_infinite_light", "agpt_scene_add_infinite_area_light",
    "agpt_scene_add_texture", "agpt_scene_set_material_texture", "agpt_scene_set_material_param_texture", "agpt_scene_set_material_normal_texture", "agpt_scene_set_texture_sampler", "agpt_scene_set_camera",
    "agpt_scene_commit", "agpt_mesh_num_nodes", "agpt_mesh_num_prims", "agpt_mesh_get_bvh", "agpt_bvh_build", "agpt_bvh_refit", "agpt_scene_update_mesh", "agpt_scene_update_mesh_device", "agpt_scene_transform_mesh", "agpt_transform_arrays", "agpt_skin_arrays", "agpt_scene_set_mesh_skin", "agpt_scene_pose_mesh", "agpt_morph_arrays", "agpt_scene_set_mesh_morph_targets", "agpt_scene_morph_mesh", "agpt_vertex_normals_arrays", "agpt_scene_set_mesh_normals_mode", "agpt_scene_set_bvh_builder", "agpt_scene_set_shading_arith", "agpt_scene_shade_variant", "agpt_bvh_build_device", "agpt_toplevel_build", "agpt_toplevel_pack16", "agpt_create_backdrop",
    "agpt_intersect_batch", "agpt_intersect_device", "agpt_render", "agpt_render_adaptive", "agpt_render_features", "agpt_denoise", "agpt_camera_vectors", "agpt_temporal_accumulate",
    "agpt_scene_snapshot_positions", "agpt_render_features_motion", "agpt_temporal_accumulate_motion", "agpt_temporal_accumulate_clamped", "agpt_li_batch", "agpt_resolve",
    "agpt_scene_snapshot_surfaces", "agpt_render_features_surface_motion", "agpt_temporal_accumulate_surface_motion", "agpt_kat_surface",
    "agpt_scene_update_sphere", "agpt_scene_update_plane", "agpt_scene_set_area_light_radiance", "agpt_scene_set_infinite_light_radiance",
    "agpt_scene_update_spheres_device",
    "agpt_scene_pose_mesh_device", "agpt_scene_morph_mesh_device", "agpt_skin_palette", "agpt_morph_active", "agpt_kat_skin_palette", "agpt_kat_morph_active",
    "agpt_resolve_counts", "agpt_device_alloc", "agpt_device_free",
    "agpt_device_memset", "agpt_device_download", "agpt_device_upload", "agpt_kat_bsdf_eval",
    "agpt_kat_bsdf_sample", "agpt_kat_env_light", "agpt_kat_normal_map", "agpt_kat_rng", "agpt_kat_distribution1d", "agpt_dbg_li_batch", "agpt_obj_load", "agpt_obj_parse", "agpt_obj_counts", "agpt_obj_get",
    "agpt_obj_free", "agpt_obj_last_error", "agpt_write_png", "agpt_write_pfm", "agpt_hdr_load", "agpt_hdr_parse", "agpt_hdr_free",
    "agpt_comm_unique_id", "agpt_comm_init", "agpt_comm_destroy", "agpt_gather_tiles", "agpt_deinterleave_tiles",
]


class AgptError(RuntimeError):
    pass


class CameraDesc(C.Structure):
    """CameraDesc (camera.h:17-25)."""
    _fields_ = [("lookfrom", C.c_float * 3), ("lookat", C.c_float * 3), ("vup", C.c_float * 3),
                ("aspect_ratio", C.c_float), ("vfov", C.c_float), ("aperture", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("closest_rays", C.c_uint64), ("anyhit_rays", C.c_uint64), ("interior_visits", C.c_uint64),
                ("tri_tests", C.c_uint64), ("shaded_vertices", C.c_uint64), ("samples", C.c_uint64),
                ("outliers", C.c_uint64), ("iterations", C.c_uint64), ("trace_ms", C.c_double),
                ("total_ms", C.c_double), ("trace_launches", C.c_uint64), ("root_tests", C.c_uint64),
                ("ext_ms", C.c_double), ("mis_ms", C.c_double), ("shadow_ms", C.c_double), ("answered_rays", C.c_uint64)]

    @property
    def rays(self):
        return int(self.closest_rays + self.anyhit_rays)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("w", C.c_int32), ("h", C.c_int32), ("spp_begin", C.c_int32), ("spp_count", C.c_int32),
                ("seed_base", C.c_uint32), ("max_depth", C.c_int32), ("accum_pitch", C.c_int32),
                ("accum_row0", C.c_int32), ("samples_per_batch", C.c_int32), ("enable_counters", C.c_int32),
                ("enable_timing", C.c_int32), ("interleave_block", C.c_int32), ("interleave_world", C.c_int32),
                ("interleave_rank", C.c_int32), ("trace_all_rays", C.c_int32)]


class AdaptiveParams(C.Structure):
    """agpt_adaptive_params (include/agpt.h)."""
    _fields_ = [("min_spp", C.c_int32), ("max_spp", C.c_int32), ("step_spp", C.c_int32), ("rel_error", C.c_float),
                ("abs_floor", C.c_float)]


class AdaptiveStats(C.Structure):
    """agpt_adaptive_stats (include/agpt.h)."""
    _fields_ = [("rounds", C.c_int32), ("active_last", C.c_int32), ("samples", C.c_uint64), ("pixels_stopped", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DenoiseParams(C.Structure):
    """agpt_denoise_params (include/agpt.h); the sigma defaults are AGPT_DENOISE_SIGMA_*."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("demodulate", C.c_int32),
                ("sigma_z", C.c_float), ("sigma_n", C.c_float), ("sigma_l", C.c_float)]


DENOISE_SIGMA_Z, DENOISE_SIGMA_N, DENOISE_SIGMA_L = 1.0, 0.25, 4.0


class TemporalParams(C.Structure):
    """agpt_temporal_params (include/agpt.h); the depth_tol / normal_cos defaults are AGPT_TEMPORAL_*."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("cam_cur", CameraDesc), ("cam_prev", CameraDesc),
                ("max_history", C.c_float), ("depth_tol", C.c_float), ("normal_cos", C.c_float)]


TEMPORAL_DEPTH_TOL, TEMPORAL_NORMAL_COS, TEMPORAL_MIN_WEIGHT = 0.05, 0.9, 1e-2


class TemporalClampParams(C.Structure):
    """agpt_temporal_clamp_params (include/agpt.h): the window's half-width (1..3), whether the statistics and the clamp work on
    radiance / albedo, the box half-width in standard deviations, and the history count a clamped pixel keeps at most."""
    _fields_ = [("radius", C.c_int32), ("demodulate", C.c_int32), ("gamma", C.c_float), ("clamped_max_history", C.c_float)]


def camera_desc(lookfrom, lookat, vup, aspect_ratio, vfov=45.0, aperture=0.0):
    """A CameraDesc from the arguments of Scene.set_camera, rounded to fp32 the same way."""
    d = CameraDesc()
    d.lookfrom[:] = [float(x) for x in np.float32(lookfrom)]
    d.lookat[:] = [float(x) for x in np.float32(lookat)]
    d.vup[:] = [float(x) for x in np.float32(vup)]
    d.aspect_ratio = float(np.float32(aspect_ratio))
    d.vfov = float(vfov)
    d.aperture = float(aperture)
    return d


def camera_vectors(desc):
    """agpt_camera_vectors: Camera(desc) as the library derives it -- float32[22] = origin, u, v, w, lower_left_corner, horizontal,
    vertical (3 each), lens_radius.  Host only, no GPU needed.  desc: a CameraDesc or the argument tuple of Scene.set_camera."""
    if not isinstance(desc, CameraDesc):
        desc = camera_desc(*desc)
    out = np.zeros(22, np.float32)
    _check(lib().agpt_camera_vectors(C.byref(desc), out.ctypes.data_as(C.POINTER(C.c_float))), "agpt_camera_vectors")
    return out


def library_path():
    return _build.LIB


def lib():
    """Load libagpt_hip.so (building it with hipcc if missing or stale)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB
    variant = os.environ.get("AGPT_LIB_VARIANT")   # developer A/B builds (tools/build_variant.py), never set in production
    if variant:
        path = os.path.join(os.path.dirname(path), "libagpt_hip_%s.so" % variant)
        if not os.path.exists(path):
            raise AgptError("AGPT_LIB_VARIANT=%s: %s does not exist" % (variant, path))
    elif not os.path.exists(path) or (os.path.exists(_build.CSRC) and _build.needs_build()):
        try:
            _build.build()
        except Exception as e:  # noqa: BLE001
            if not os.path.exists(path):
                raise AgptError("libagpt_hip.so is missing and could not be built with hipcc: %s" % e)
    L = C.CDLL(path)
    fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
    L.agpt_last_error.restype = C.c_char_p
    L.agpt_init.argtypes = [C.c_int, C.POINTER(vp)]
    L.agpt_set_stream.argtypes = [vp, vp]
    L.agpt_destroy.argtypes = [vp]
    L.agpt_destroy.restype = None
    L.agpt_scene_create.argtypes = [vp, C.POINTER(vp)]
    L.agpt_scene_destroy.argtypes = [vp]
    L.agpt_scene_destroy.restype = None
    L.agpt_scene_add_material.argtypes = [vp, C.c_int, fp, C.c_float, C.c_float]
    L.agpt_scene_add_mesh.argtypes = [vp, fp, C.c_int, fp, C.c_int, fp, C.c_int, ip, C.c_int, C.c_int, C.c_int]
    L.agpt_scene_add_sphere.argtypes = [vp, fp, C.c_float, C.c_int]
    L.agpt_scene_add_plane.argtypes = [vp, fp, fp, C.c_int]
    L.agpt_scene_add_area_light.argtypes = [vp, fp, C.c_float, fp]
    L.agpt_scene_add_uniform_infinite_light.argtypes = [vp, fp]
    L.agpt_scene_add_infinite_area_light.argtypes = [vp, fp, C.c_int, C.c_int]
    L.agpt_scene_add_texture.argtypes = [vp, fp, C.c_int, C.c_int]
    L.agpt_scene_set_material_texture.argtypes = [vp, C.c_int, C.c_int]
    L.agpt_scene_set_material_param_texture.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.agpt_scene_set_texture_sampler.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.agpt_scene_set_material_normal_texture.argtypes = [vp, C.c_int, C.c_int, C.c_float]
    L.agpt_scene_set_camera.argtypes = [vp, C.POINTER(CameraDesc)]
    L.agpt_scene_commit.argtypes = [vp]
    L.agpt_mesh_num_nodes.argtypes = [vp, C.c_int]
    L.agpt_mesh_num_prims.argtypes = [vp, C.c_int]
    L.agpt_mesh_get_bvh.argtypes = [vp, C.c_int, vp, ip]
    L.agpt_bvh_build.argtypes = [fp, C.c_int, ip, C.c_int, C.c_int, vp, ip, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.agpt_bvh_refit.argtypes = [fp, C.c_int, ip, C.c_int, ip, vp, C.c_int]
    L.agpt_scene_update_mesh.argtypes = [vp, C.c_int, fp, C.c_int, fp, C.c_int, C.c_int]
    for name, args in (("agpt_scene_update_mesh_device", [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int]),
                       ("agpt_scene_transform_mesh", [vp, C.c_int, fp, C.c_int]), ("agpt_transform_arrays", [fp, fp, C.c_int, fp, C.c_int, fp, fp]),
                       ("agpt_skin_arrays", [fp, C.c_int, C.c_int, fp, C.c_int, ip, fp, fp, C.c_int, ip, fp, fp, fp]),
                       ("agpt_scene_set_mesh_skin", [vp, C.c_int, C.c_int, C.c_int, ip, fp, ip, fp]), ("agpt_scene_pose_mesh", [vp, C.c_int, fp, C.c_int, C.c_int]),
                       ("agpt_morph_arrays", [fp, C.c_int, fp, C.c_int, fp, fp, C.c_int, fp, fp, fp]),
                       ("agpt_scene_set_mesh_morph_targets", [vp, C.c_int, C.c_int, fp, fp]),
                       ("agpt_scene_morph_mesh", [vp, C.c_int, fp, C.c_int, fp, C.c_int, C.c_int]),
                       ("agpt_vertex_normals_arrays", [fp, C.c_int, ip, C.c_int, C.c_int, fp]),
                       ("agpt_scene_set_mesh_normals_mode", [vp, C.c_int, C.c_int])):
        if not variant or hasattr(L, name):   # (an A/B variant built from an older commit lacks them: tools/mesh_update_time.py --parent-lib)
            getattr(L, name).argtypes = args
    L.agpt_scene_set_bvh_builder.argtypes = [vp, C.c_int]
    L.agpt_scene_set_shading_arith.argtypes = [vp, C.c_int]
    if not variant or hasattr(L, "agpt_scene_shade_variant"):
        L.agpt_scene_shade_variant.argtypes = [vp, C.POINTER(C.c_int32)]
    L.agpt_bvh_build_device.argtypes = [vp, fp, C.c_int, ip, C.c_int, C.c_int, vp, ip, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]
    L.agpt_toplevel_build.argtypes = [fp, C.c_int, fp]
    L.agpt_toplevel_pack16.argtypes = [fp, C.c_int, C.POINTER(C.c_uint32)]
    L.agpt_create_backdrop.argtypes = [fp, fp, C.c_float, C.c_int, fp, fp, fp, ip, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.agpt_intersect_batch.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.POINTER(Stats)]
    L.agpt_intersect_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.POINTER(Stats)]
    L.agpt_render.argtypes = [vp, C.POINTER(RenderParams), vp, C.POINTER(Stats)]
    L.agpt_render_adaptive.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), vp, vp, C.POINTER(Stats),
                                       C.POINTER(AdaptiveStats)]
    L.agpt_resolve_counts.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_uint32)]
    L.agpt_render_features.argtypes = [vp, C.POINTER(RenderParams), vp, vp]
    L.agpt_denoise.argtypes = [vp, C.POINTER(DenoiseParams), vp, vp, vp, vp, vp]
    L.agpt_camera_vectors.argtypes = [C.POINTER(CameraDesc), fp]
    L.agpt_temporal_accumulate.argtypes = [vp, C.POINTER(TemporalParams)] + [vp] * 10
    if not variant or hasattr(L, "agpt_scene_snapshot_positions"):   # (an A/B variant built from an older commit lacks them)
        L.agpt_scene_snapshot_positions.argtypes = [vp]
        L.agpt_render_features_motion.argtypes = [vp, C.POINTER(RenderParams), vp, vp, vp]
        L.agpt_temporal_accumulate_motion.argtypes = [vp, C.POINTER(TemporalParams)] + [vp] * 11
    if not variant or hasattr(L, "agpt_temporal_accumulate_clamped"):
        L.agpt_temporal_accumulate_clamped.argtypes = [vp, C.POINTER(TemporalParams), C.POINTER(TemporalClampParams)] + [vp] * 11
    if not variant or hasattr(L, "agpt_scene_snapshot_surfaces"):
        L.agpt_scene_snapshot_surfaces.argtypes = [vp]
        L.agpt_render_features_surface_motion.argtypes = [vp, C.POINTER(RenderParams), vp, vp, vp, vp]
        L.agpt_temporal_accumulate_surface_motion.argtypes = [vp, C.POINTER(TemporalParams), C.POINTER(TemporalClampParams)] + [vp] * 12
        L.agpt_kat_surface.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_uint32), fp, fp, fp, fp]
    if not variant or hasattr(L, "agpt_scene_update_spheres_device"):
        L.agpt_scene_update_sphere.argtypes = [vp, C.c_int, fp, C.c_float]
        L.agpt_scene_update_plane.argtypes = [vp, C.c_int, fp, fp]
        L.agpt_scene_set_area_light_radiance.argtypes = [vp, C.c_int, fp]
        L.agpt_scene_set_infinite_light_radiance.argtypes = [vp, C.c_int, fp]
        L.agpt_scene_update_spheres_device.argtypes = [vp, ip, C.c_int, vp]
    if not variant or hasattr(L, "agpt_scene_pose_mesh_device"):
        L.agpt_scene_pose_mesh_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int]
        L.agpt_scene_morph_mesh_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int]
        L.agpt_skin_palette.argtypes = [fp, C.c_int, C.c_int, fp, C.POINTER(C.c_int)]
        L.agpt_morph_active.argtypes = [fp, C.c_int, ip, fp, C.POINTER(C.c_int)]
        L.agpt_kat_skin_palette.argtypes = [vp, fp, C.c_int, C.c_int, fp, C.POINTER(C.c_uint32)]
        L.agpt_kat_morph_active.argtypes = [vp, fp, C.c_int, ip, fp, C.POINTER(C.c_uint32)]
    L.agpt_li_batch.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.c_int, C.c_int, fp, C.POINTER(C.c_uint32), C.POINTER(Stats)]
    L.agpt_resolve.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
    L.agpt_device_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.agpt_device_free.argtypes = [vp, vp]
    L.agpt_device_memset.argtypes = [vp, vp, C.c_int, C.c_size_t]
    L.agpt_device_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.agpt_device_upload.argtypes = [vp, vp, vp, C.c_size_t]
    L.agpt_kat_bsdf_eval.argtypes = [vp, C.c_int, C.c_int, fp, fp, fp, fp]
    L.agpt_kat_bsdf_sample.argtypes = [vp, C.c_int, C.c_int, fp, fp, fp, fp, fp, ip]
    L.agpt_kat_env_light.argtypes = [vp, C.c_int, C.c_int, fp, fp, fp, C.c_int, fp, fp, fp, fp, ip]
    L.agpt_kat_rng.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, fp, C.POINTER(C.c_uint32)]
    L.agpt_kat_normal_map.argtypes = [vp, C.c_int, fp, fp, fp, C.c_float, fp]
    L.agpt_dbg_li_batch.argtypes = [vp, vp, C.c_int, fp]
    L.agpt_kat_distribution1d.argtypes = [vp, fp, C.c_int, fp, C.c_int, fp, fp, fp, fp]
    L.agpt_obj_load.argtypes = [C.c_char_p, fp, C.c_int, C.POINTER(vp)]
    L.agpt_obj_parse.argtypes = [C.c_char_p, C.c_size_t, fp, C.c_int, C.POINTER(vp)]
    L.agpt_obj_counts.argtypes = [vp] + [C.POINTER(C.c_int)] * 4
    L.agpt_obj_get.argtypes = [vp, fp, fp, fp, ip]
    L.agpt_obj_free.argtypes = [vp]
    L.agpt_obj_free.restype = None
    L.agpt_comm_unique_id.argtypes = [vp]
    L.agpt_comm_init.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.agpt_comm_destroy.argtypes = [vp]
    L.agpt_comm_destroy.restype = None
    L.agpt_gather_tiles.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.agpt_deinterleave_tiles.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.agpt_obj_last_error.restype = C.c_char_p
    L.agpt_hdr_load.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(fp)]
    L.agpt_hdr_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(fp)]
    L.agpt_hdr_free.argtypes = [fp]
    L.agpt_hdr_free.restype = None
    _LIB = L
    return L


def _check(rc, what=""):
    if rc < 0:
        raise AgptError("%s failed (%d): %s" % (what, rc, lib().agpt_last_error().decode()))
    return rc


def _f(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def create_backdrop(origin, size, radius, steps):
    """TriangleMesh::CreateBackdrop (trianglemesh.cpp:232-318) -> verts[n,3], normals[n,3], uvs[n,2], indices[m,3]."""
    nv = 2 * (steps + 5)
    verts = np.zeros((nv, 3), np.float32)
    normals = np.zeros((nv, 3), np.float32)
    uvs = np.zeros((nv, 2), np.float32)
    idx = np.zeros((6 * (steps + 4), 3), np.int32)
    _, po = _f(origin)
    _, ps = _f(size)
    n_v, n_i = C.c_int(0), C.c_int(0)
    fp = C.POINTER(C.c_float)
    _check(lib().agpt_create_backdrop(po, ps, float(radius), int(steps), verts.ctypes.data_as(fp),
                                      normals.ctypes.data_as(fp), uvs.ctypes.data_as(fp),
                                      idx.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_v), C.byref(n_i)),
           "agpt_create_backdrop")
    return verts, normals, uvs, idx


def toplevel_build(boxes):
    """agpt_toplevel_build: boxes[n, 6] (bmin, bmax) -> (lo[m, 3], hi[m, 3], skip[m], leaf[m]) with m = 2n - 1 nodes in depth-first
    order; leaf[i] = index of the box at a leaf, -1 at an interior node; skip[i] = the node after i's subtree."""
    boxes, pb = _f(np.asarray(boxes).reshape(-1, 6))
    n = boxes.shape[0]
    out = np.zeros((max(2 * n - 1, 1), 8), np.float32)
    m = _check(lib().agpt_toplevel_build(pb, n, out.ctypes.data_as(C.POINTER(C.c_float))), "agpt_toplevel_build")
    assert m == 2 * n - 1
    words = out.view(np.uint32)
    return out[:, 0:3].copy(), out[:, 4:7].copy(), words[:, 3].astype(np.int64), words[:, 7].astype(np.int32)


def toplevel_pack16(lo, hi, skip, leaf):
    """agpt_toplevel_pack16: the 16-byte node form of a tree from toplevel_build -> (lo16[m, 3], hi16[m, 3] as float16, skip[m], leaf[m])."""
    m = len(skip)
    nodes = np.zeros((m, 8), np.float32)
    nodes[:, 0:3], nodes[:, 4:7] = lo, hi
    w = nodes.view(np.uint32)
    w[:, 3] = np.asarray(skip, np.uint32)
    w[:, 7] = np.asarray(leaf, np.int64).astype(np.uint32)   # -1 -> 0xFFFFFFFF
    packed = np.zeros((m, 4), np.uint32)
    _check(lib().agpt_toplevel_pack16(nodes.ctypes.data_as(C.POINTER(C.c_float)), m, packed.ctypes.data_as(C.POINTER(C.c_uint32))),
           "agpt_toplevel_pack16")
    halves = np.stack([packed[:, 0] & 0xFFFF, packed[:, 0] >> 16, packed[:, 1] & 0xFFFF, packed[:, 1] >> 16, packed[:, 2] & 0xFFFF,
                       packed[:, 2] >> 16], axis=1).astype(np.uint16).view(np.float16)
    leaf16 = (packed[:, 3] >> 16).astype(np.int32)
    leaf16[leaf16 == 0xFFFF] = -1
    return halves[:, 0:3].copy(), halves[:, 3:6].copy(), (packed[:, 3] & 0xFFFF).astype(np.int64), leaf16


def bvh_build(verts, indices, max_prims_in_node=1):
    """BVHTriMesh's constructor on the host (no GPU needed) -> (nodes[total+1], prim_index[n_tris], max_depth)."""
    v, pv = _f(np.asarray(verts).reshape(-1, 3))
    ix, pi = _i(np.asarray(indices).reshape(-1, 3))
    n_tris = ix.shape[0] // 3
    nodes = np.zeros(2 * n_tris + 2, NODE_DTYPE)
    order = np.zeros(n_tris, np.int32)
    total, depth = C.c_int(0), C.c_int(0)
    _check(lib().agpt_bvh_build(pv, v.shape[0], pi, ix.shape[0], int(max_prims_in_node), nodes.ctypes.data_as(C.c_void_p),
                                order.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(total), C.byref(depth)),
           "agpt_bvh_build")
    return nodes[:total.value + 1].copy(), order, depth.value


def bvh_refit(verts, indices, prim_index, nodes):
    """agpt_bvh_refit on the host (no GPU needed): the tree `nodes` (bvh_build's, with its prim_index) with the bounds recomputed
    for `verts`, topology kept -> a new nodes array."""
    v, pv = _f(np.asarray(verts).reshape(-1, 3))
    ix, pi = _i(np.asarray(indices).reshape(-1, 3))
    order, po = _i(np.asarray(prim_index).reshape(-1))
    out = np.array(nodes, NODE_DTYPE, copy=True)
    _check(lib().agpt_bvh_refit(pv, v.shape[0], pi, ix.shape[0], po, out.ctypes.data_as(C.c_void_p), out.shape[0] - 1), "agpt_bvh_refit")
    return out


def bvh_build_device(ctx, verts, indices, max_prims_in_node=1):
    """agpt_bvh_build_device: bvh_build on the context's GPU, the same bytes -> (nodes[total+1], prim_index[n_tris], max_depth,
    on_device); on_device is 0 when non-finite input made the library run the host builder."""
    v, pv = _f(np.asarray(verts).reshape(-1, 3))
    ix, pi = _i(np.asarray(indices).reshape(-1, 3))
    n_tris = ix.shape[0] // 3
    nodes = np.zeros(2 * n_tris + 2, NODE_DTYPE)
    order = np.zeros(n_tris, np.int32)
    total, depth, on_device = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(ctx.L.agpt_bvh_build_device(ctx.h, pv, v.shape[0], pi, ix.shape[0], int(max_prims_in_node), nodes.ctypes.data_as(C.c_void_p),
                                       order.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(total), C.byref(depth), C.byref(on_device)),
           "agpt_bvh_build_device")
    return nodes[:total.value + 1].copy(), order, depth.value, on_device.value


def load_obj(path=None, text=None, transform=None, ignore_normals=False):
    """TriangleMesh::LoadObj (trianglemesh.cpp:157-230): returns (verts[n,3], normals[m,3] or None, uvs[k,2] or None,
    indices[3*tris,3]) ready for Scene.add_mesh.  `transform` is a row-major 4x4 (mat4)."""
    L = lib()
    h = C.c_void_p()
    tp = None
    if transform is not None:
        t = np.ascontiguousarray(transform, np.float32).reshape(16)
        tp = t.ctypes.data_as(C.POINTER(C.c_float))
    if text is not None:
        data = text.encode() if isinstance(text, str) else bytes(text)
        rc = L.agpt_obj_parse(data, len(data), tp, int(bool(ignore_normals)), C.byref(h))
    else:
        rc = L.agpt_obj_load(os.fsencode(path), tp, int(bool(ignore_normals)), C.byref(h))
    if rc < 0:
        raise AgptError("load_obj failed (%d): %s" % (rc, L.agpt_obj_last_error().decode()))
    try:
        nv, nn, nt, ni = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        L.agpt_obj_counts(h, C.byref(nv), C.byref(nn), C.byref(nt), C.byref(ni))
        v = np.zeros((nv.value, 3), np.float32)
        n = np.zeros((nn.value, 3), np.float32)
        t = np.zeros((nt.value, 2), np.float32)
        ix = np.zeros((ni.value, 3), np.int32)
        fp = C.POINTER(C.c_float)
        L.agpt_obj_get(h, v.ctypes.data_as(fp), n.ctypes.data_as(fp), t.ctypes.data_as(fp), ix.ctypes.data_as(C.POINTER(C.c_int32)))
    finally:
        L.agpt_obj_free(h)
    return v, (n if nn.value else None), (t if nt.value else None), ix


def transform_arrays(matrix4x4, verts, normals=None):
    """agpt_transform_arrays on the host (no GPU needed): positions through the row-major 4x4 as the reference's TransformPoint,
    normals through TransformVector of its inverse transpose -> (verts[n, 3], normals[m, 3] or None), the arithmetic of load_obj's
    `transform` and of Scene.transform_mesh."""
    m = np.ascontiguousarray(matrix4x4, np.float32).reshape(16)
    v, pv = _f(np.asarray(verts).reshape(-1, 3))
    n, pn = (None, None) if normals is None else _f(np.asarray(normals).reshape(-1, 3))
    vo = np.empty_like(v)
    no = None if n is None else np.empty_like(n)
    fp = C.POINTER(C.c_float)
    _check(lib().agpt_transform_arrays(m.ctypes.data_as(fp), pv, v.shape[0], pn, 0 if n is None else n.shape[0], vo.ctypes.data_as(fp),
                                       None if no is None else no.ctypes.data_as(fp)), "agpt_transform_arrays")
    return vo, no


def _joint_matrices(matrices):
    m = np.ascontiguousarray(matrices, np.float32)
    if m.ndim < 2 or m.size % 16 or m.shape[1:] not in ((4, 4), (16,)):
        raise ValueError("joint matrices have shape %s, not (n_joints, 4, 4) or (n_joints, 16)" % (m.shape,))
    return m.reshape(-1, 16)


def _on_device(a):
    """a torch tensor that is not on the CPU (update_mesh's test)"""
    return type(a).__module__.split(".")[0] == "torch" and a.device.type != "cpu"


def _influences(joints, weights, what):
    j, w = np.asarray(joints), np.asarray(weights)
    if j.ndim != 2 or j.shape != w.shape:
        raise ValueError("%s joints %s and weights %s must both have shape (n, influences)" % (what, j.shape, w.shape))
    return _i(j) + _f(w)


def skin_arrays(matrices, verts, joints, weights, normals=None, normal_joints=None, normal_weights=None):
    """agpt_skin_arrays on the host (no GPU needed): linear-blend skinning of verts[n, 3] (and normals[m, 3]) by matrices[n_joints, 4, 4]
    (row-major, last row (0, 0, 0, 1)) with joints / weights of shape (n, K), K = 1 .. 8; normals take normal_joints / normal_weights
    (m, K), or the vertices' when m == n and none are given -> (verts[n, 3], normals[m, 3] or None), the arithmetic of
    Scene.pose_mesh."""
    m = _joint_matrices(matrices)
    v, pv = _f(np.asarray(verts).reshape(-1, 3))
    j, pj, w, pw = _influences(joints, weights, "vertex")
    n, pn = (None, None) if normals is None else _f(np.asarray(normals).reshape(-1, 3))
    nj, pnj, nw, pnw = (None,) * 4 if normal_joints is None else _influences(normal_joints, normal_weights, "normal")
    if j.shape[0] != v.shape[0] or (nj is not None and (n is None or nj.shape != (n.shape[0], j.shape[1]))):
        raise ValueError("skin_arrays: one row of K influences per vertex (and per normal)")
    vo = np.empty_like(v)
    no = None if n is None else np.empty_like(n)
    fp = C.POINTER(C.c_float)
    _check(lib().agpt_skin_arrays(m.ctypes.data_as(fp), m.shape[0], j.shape[1], pv, v.shape[0], pj, pw, pn, 0 if n is None else n.shape[0], pnj, pnw,
                                  vo.ctypes.data_as(fp), None if no is None else no.ctypes.data_as(fp)), "agpt_skin_arrays")
    return vo, no


def skin_palette(matrices, with_normals=True):
    """agpt_skin_palette on the host (no GPU needed): the palette Scene.pose_mesh forms from matrices[n_joints, 4, 4] -- per joint rows
    0 .. 2 of M and, with_normals, the 3x3 of its inverse transpose -> (palette[n_joints, 21 or 13], the first joint whose determinant
    is exactly 0 or -1).  What the GPU writes itself when the matrices are a device tensor."""
    m = _joint_matrices(matrices)
    out = np.zeros((m.shape[0], 21 if with_normals else 13), np.float32)
    singular = C.c_int(-1)
    fp = C.POINTER(C.c_float)
    _check(lib().agpt_skin_palette(m.ctypes.data_as(fp), m.shape[0], 1 if with_normals else 0, out.ctypes.data_as(fp), C.byref(singular)), "agpt_skin_palette")
    return out, singular.value


def morph_active(weights):
    """agpt_morph_active on the host (no GPU needed): the (target, weight) pairs Scene.morph_mesh forms from weights[T] -- the weights
    that are not 0, in target order -> (targets[A] int32, weights[A] float32)."""
    w, pw = _f(np.asarray(weights).reshape(-1))
    t, pt = _i(np.zeros(max(w.shape[0], 1), np.int32))
    a, pa = _f(np.zeros(max(w.shape[0], 1), np.float32))
    n = C.c_int(0)
    _check(lib().agpt_morph_active(pw, w.shape[0], pt, pa, C.byref(n)), "agpt_morph_active")
    return t[:n.value].copy(), a[:n.value].copy()


def _deltas(deltas, n, what):
    d = np.ascontiguousarray(deltas, np.float32)
    if d.ndim != 3 or d.shape[1:] != (n, 3) or d.shape[0] < 1:
        raise ValueError("%s deltas have shape %s, not (n_targets, %d, 3)" % (what, d.shape, n))
    return d, d.ctypes.data_as(C.POINTER(C.c_float))


def morph_arrays(weights, verts, position_deltas, normals=None, normal_deltas=None):
    """agpt_morph_arrays on the host (no GPU needed): verts[n, 3] plus the weighted position_deltas[T, n, 3], the targets in order, a
    target of weight 0 skipped, and normals[m, 3] plus normal_deltas[T, m, 3] likewise (None: the normals are returned as they are)
    -> (verts[n, 3], normals[m, 3] or None), the arithmetic of Scene.morph_mesh."""
    v, pv = _f(np.asarray(verts).reshape(-1, 3))
    w, pw = _f(np.asarray(weights).reshape(-1))
    d, pd = _deltas(position_deltas, v.shape[0], "position")
    n, pn = (None, None) if normals is None else _f(np.asarray(normals).reshape(-1, 3))
    nd, pnd = (None, None) if normal_deltas is None or n is None else _deltas(normal_deltas, n.shape[0], "normal")
    if w.shape[0] != d.shape[0] or (nd is not None and nd.shape[0] != d.shape[0]):
        raise ValueError("morph_arrays: one weight and one row of deltas per target")
    vo = np.empty_like(v)
    no = None if n is None else np.empty_like(n)
    fp = C.POINTER(C.c_float)
    _check(lib().agpt_morph_arrays(pw, d.shape[0], pv, v.shape[0], pd, pn, 0 if n is None else n.shape[0], pnd,
                                   vo.ctypes.data_as(fp), None if no is None else no.ctypes.data_as(fp)), "agpt_morph_arrays")
    return vo, no


def vertex_normals_arrays(vertices, indices, n_normals):
    """agpt_vertex_normals_arrays on the host (no GPU needed): smooth vertex normals of verts[n, 3] under indices[k, 3] -- one (vertex,
    normal, texcoord) triplet per corner, as for Scene.add_mesh -- -> normals[n_normals, 3]: per normal item the area-weighted face
    vectors of the corners that name it, summed in corner order and normalised; (0, 0, 0) where that sum has no direction (shading then
    uses the geometric normal).  The arithmetic of a mesh in "smooth" normals mode (Scene.set_mesh_normals_mode)."""
    v, pv = _f(np.asarray(vertices).reshape(-1, 3))
    ix, pi = _i(np.asarray(indices).reshape(-1, 3))
    out = np.empty((max(int(n_normals), 0), 3), np.float32)
    _check(lib().agpt_vertex_normals_arrays(pv, v.shape[0], pi, ix.shape[0], int(n_normals), out.ctypes.data_as(C.POINTER(C.c_float))),
           "agpt_vertex_normals_arrays")
    return out


class Context:
    """One GPU. `stream` may be a raw hipStream_t handle (e.g. torch.cuda.Stream().cuda_stream; torch's default stream is handle 0, the
    null stream).  A non-null handle must come from the HIP runtime instance libagpt_hip.so is bound to: with torch imported first
    that is the wheel's copy, and exactly one libamdhip64 is then listed in /proc/self/maps.  set_stream
    waits for the stream it leaves (include/agpt.h)."""

    def __init__(self, device=0, stream=None):
        self.L = lib()
        h = C.c_void_p()
        _check(self.L.agpt_init(int(device), C.byref(h)), "agpt_init")
        self.h = h
        self.device = device
        self.stream = 0
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        self.stream = int(stream) if stream else 0
        _check(self.L.agpt_set_stream(self.h, C.c_void_p(int(stream) if stream else 0)), "agpt_set_stream")

    def close(self):
        if self.h:
            self.L.agpt_destroy(self.h)
            self.h = None

    def alloc(self, nbytes):
        p = C.c_void_p()
        _check(self.L.agpt_device_alloc(self.h, nbytes, C.byref(p)), "agpt_device_alloc")
        return p.value

    def free(self, ptr):
        _check(self.L.agpt_device_free(self.h, C.c_void_p(ptr)), "agpt_device_free")

    def memset(self, ptr, value, nbytes):
        _check(self.L.agpt_device_memset(self.h, C.c_void_p(ptr), value, nbytes), "agpt_device_memset")

    def download(self, ptr, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        _check(self.L.agpt_device_download(self.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes),
               "agpt_device_download")
        return out

    def upload(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        _check(self.L.agpt_device_upload(self.h, C.c_void_p(ptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes),
               "agpt_device_upload")

    def rng_floats(self, pixel, wh, sample, seed_base, n):
        out = np.zeros(n, np.float32)
        seed = C.c_uint32(0)
        _check(self.L.agpt_kat_rng(self.h, pixel, wh, sample, seed_base, n, out.ctypes.data_as(C.POINTER(C.c_float)),
                                   C.byref(seed)), "agpt_kat_rng")
        return out, seed.value

    def kat_normal_map(self, ns, ss, rgb, scale=1.0):
        """agpt_kat_normal_map: the normal-map perturbation alone (agpt_scene_set_material_normal_texture's definition) on n items --
        shading normals ns[n, 3], tangents ss[n, 3], texels rgb[n, 3] -> the perturbed normals [n, 3]."""
        ns, pns = _f(np.asarray(ns).reshape(-1, 3))
        ss, pss = _f(np.asarray(ss).reshape(-1, 3))
        rgb, prgb = _f(np.asarray(rgb).reshape(-1, 3))
        if not ns.shape == ss.shape == rgb.shape:
            raise ValueError("kat_normal_map: ns, ss and rgb must have the same number of items")
        out = np.zeros_like(ns)
        _check(self.L.agpt_kat_normal_map(self.h, ns.shape[0], pns, pss, prgb, float(scale), out.ctypes.data_as(C.POINTER(C.c_float))),
               "agpt_kat_normal_map")
        return out

    def kat_skin_palette(self, matrices, with_normals=True):
        """agpt_kat_skin_palette: k_pack_palette, the kernel of Scene.pose_mesh with a device tensor, on matrices[n_joints, 4, 4] ->
        (palette[n_joints, 21 or 13], status[3] uint32: the lowest joint with a non-finite entry, a bad last row, a determinant of
        exactly 0; 0xFFFFFFFF = none)."""
        m = _joint_matrices(matrices)
        out = np.zeros((m.shape[0], 21 if with_normals else 13), np.float32)
        status = np.zeros(3, np.uint32)
        fp = C.POINTER(C.c_float)
        _check(self.L.agpt_kat_skin_palette(self.h, m.ctypes.data_as(fp), m.shape[0], 1 if with_normals else 0, out.ctypes.data_as(fp),
                                            status.ctypes.data_as(C.POINTER(C.c_uint32))), "agpt_kat_skin_palette")
        return out, status

    def kat_morph_active(self, weights):
        """agpt_kat_morph_active: k_morph_active, the kernel of Scene.morph_mesh with a device tensor, on weights[T] -> (targets[A],
        weights[A], status[2] uint32: A, the lowest target with a non-finite weight or 0xFFFFFFFF)."""
        w, pw = _f(np.asarray(weights).reshape(-1))
        t, pt = _i(np.zeros(max(w.shape[0], 1), np.int32))
        a, pa = _f(np.zeros(max(w.shape[0], 1), np.float32))
        status = np.zeros(2, np.uint32)
        _check(self.L.agpt_kat_morph_active(self.h, pw, w.shape[0], pt, pa, status.ctypes.data_as(C.POINTER(C.c_uint32))), "agpt_kat_morph_active")
        return t[:int(status[0])].copy(), a[:int(status[0])].copy(), status

    def distribution1d(self, func, u):
        """Distribution1D(func) and SampleContinuous(u[i]) (sampling.h:19-52): (cdf[n + 1], funcInt, x[k], pdf[k])."""
        func = np.ascontiguousarray(func, np.float32)
        u = np.ascontiguousarray(u, np.float32)
        cdf = np.zeros(func.size + 1, np.float32)
        x = np.zeros(max(u.size, 1), np.float32)
        pdf = np.zeros(max(u.size, 1), np.float32)
        fi = C.c_float(0)
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        _check(self.L.agpt_kat_distribution1d(self.h, P(func), func.size, P(u), u.size, P(cdf), C.byref(fi), P(x), P(pdf)),
               "agpt_kat_distribution1d")
        return cdf, np.float32(fi.value), x[:u.size], pdf[:u.size]

    def deinterleave_tiles(self, compact_ptr, W, H, block_rows, world, rank, full_ptr):
        _check(self.L.agpt_deinterleave_tiles(self.h, C.c_void_p(int(compact_ptr)), W, H, block_rows, world, rank, C.c_void_p(int(full_ptr))),
               "agpt_deinterleave_tiles")

    def resolve(self, accum_ptr, n_pixels, samples):
        out = np.zeros(n_pixels, np.uint32)
        _check(self.L.agpt_resolve(self.h, C.c_void_p(accum_ptr), n_pixels, samples,
                                   out.ctypes.data_as(C.POINTER(C.c_uint32))), "agpt_resolve")
        return out

    def resolve_counts(self, accum_ptr, n_pixels):
        """agpt_resolve_counts: CopyToSurface with each pixel's own count in accum.w (0 for a pixel without samples)."""
        out = np.zeros(n_pixels, np.uint32)
        _check(self.L.agpt_resolve_counts(self.h, C.c_void_p(int(accum_ptr)), n_pixels, out.ctypes.data_as(C.POINTER(C.c_uint32))),
               "agpt_resolve_counts")
        return out


    def denoise(self, params, accum_ptr, moment2_ptr, albedo_ptr, normal_depth_ptr, out_ptr):
        """agpt_denoise: the a-trous filter over an adaptive render's buffers (accum with the count in w, moment2) guided by
        render_features' buffers; out_ptr receives float4 (mean radiance, 1).  All DEVICE pointers, full film."""
        _check(self.L.agpt_denoise(self.h, C.byref(params), *[C.c_void_p(int(p)) if p else None for p in
                                                             (accum_ptr, moment2_ptr, albedo_ptr, normal_depth_ptr, out_ptr)]),
               "agpt_denoise")

    def denoise_to_host(self, accum, moment2, albedo, normal_depth, iterations=5, demodulate=True, sigma_z=DENOISE_SIGMA_Z,
                        sigma_n=DENOISE_SIGMA_N, sigma_l=DENOISE_SIGMA_L):
        """Convenience for tests and tools: uploads the four host buffers ([H,W,4], [H,W], [H,W,4], [H,W,4]), runs denoise,
        returns out[H,W,4]."""
        H, W = np.shape(moment2)
        host = [np.ascontiguousarray(a, np.float32) for a in (accum, moment2, albedo, normal_depth)]
        ptrs = []
        try:
            for a in host:
                ptrs.append(self.alloc(a.nbytes))
                self.upload(ptrs[-1], a)
            ptrs.append(self.alloc(W * H * 16))
            self.denoise(DenoiseParams(W, H, int(iterations), int(bool(demodulate)), sigma_z, sigma_n, sigma_l), *ptrs)
            return self.download(ptrs[-1], (H, W, 4))
        finally:
            for p in ptrs:
                self.free(p)

    _NO_CLAMP = object()

    def _temporal(self, name, params, ptrs, clamp=_NO_CLAMP):
        """One agpt_temporal_accumulate* call by name.  ptrs: its DEVICE pointers in the C order (None / 0 -> NULL); clamp, for an entry
        point that takes clamp parameters: a TemporalClampParams, or None -> NULL."""
        head = [C.byref(params)] + ([] if clamp is Context._NO_CLAMP else [C.byref(clamp) if clamp is not None else None])
        _check(getattr(self.L, name)(self.h, *head, *[C.c_void_p(int(p)) if p else None for p in ptrs]), name)

    def temporal_accumulate(self, params, accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev,
                            albedo_prev, normal_depth_prev, hist_accum_out, hist_moment2_out):
        """agpt_temporal_accumulate: this frame's adaptive-render and feature buffers plus the previous frame's history (this
        call's outputs then) and feature buffers -- all four None / 0 on the first frame -- into the history buffers, which have the
        form denoise reads.  All DEVICE pointers, full film."""
        self._temporal("agpt_temporal_accumulate", params,
                       (accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev, normal_depth_prev,
                        hist_accum_out, hist_moment2_out))

    def temporal_accumulate_motion(self, params, accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev,
                                   albedo_prev, normal_depth_prev, hist_accum_out, hist_moment2_out, prev_point_cur):
        """agpt_temporal_accumulate_motion: temporal_accumulate, reprojecting for every pixel whose prev_point_cur.w is 1 the point
        PathTracer.render_features_motion wrote there (where the surface was) instead of the point it sees now.  All DEVICE pointers,
        full film."""
        self._temporal("agpt_temporal_accumulate_motion", params,
                       (accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev, normal_depth_prev,
                        hist_accum_out, hist_moment2_out, prev_point_cur))

    def temporal_accumulate_clamped(self, params, clamp, accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev,
                                    hist_moment2_prev, albedo_prev, normal_depth_prev, hist_accum_out, hist_moment2_out, prev_point_cur=None):
        """agpt_temporal_accumulate_clamped: temporal_accumulate -- or, with prev_point_cur, temporal_accumulate_motion -- whose
        reprojected history is clamped to mean +- clamp.gamma standard deviations of the current frame's neighbourhood
        (clamp: a TemporalClampParams).  All DEVICE pointers, full film."""
        self._temporal("agpt_temporal_accumulate_clamped", params,
                       (accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev, normal_depth_prev,
                        hist_accum_out, hist_moment2_out, prev_point_cur), clamp)

    def temporal_accumulate_surface_motion(self, params, clamp, accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev,
                                           hist_moment2_prev, albedo_prev, normal_depth_prev, hist_accum_out, hist_moment2_out, prev_point_cur,
                                           prev_normal_cur):
        """agpt_temporal_accumulate_surface_motion: temporal_accumulate_motion (clamp None) or temporal_accumulate_clamped with
        prev_point_cur (clamp: a TemporalClampParams) whose normal test uses, for every pixel whose prev_point_cur.w is 1, the normal
        PathTracer.render_features_surface_motion wrote into prev_normal_cur -- the one the surface point had a frame ago.  All DEVICE
        pointers, full film."""
        self._temporal("agpt_temporal_accumulate_surface_motion", params,
                       (accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev, normal_depth_prev,
                        hist_accum_out, hist_moment2_out, prev_point_cur, prev_normal_cur), clamp)

    def temporal_to_host(self, cam_cur, cam_prev, accum, moment2, albedo, normal_depth, prev=None, max_history=32.0,
                         depth_tol=TEMPORAL_DEPTH_TOL, normal_cos=TEMPORAL_NORMAL_COS, prev_point=None, clamp=None, prev_normal=None):
        """Convenience for tests and tools: uploads this frame's host buffers ([H,W,4], [H,W], [H,W,4], [H,W,4]) and, unless prev is
        None (first frame), prev = (hist_accum, hist_moment2, albedo, normal_depth) of the previous frame; runs temporal_accumulate;
        returns (hist_accum[H,W,4], hist_moment2[H,W]).  cam_cur / cam_prev: CameraDesc or the argument tuple of Scene.set_camera.
        prev_point ([H,W,4], render_features_motion's third buffer): temporal_accumulate_motion runs instead.
        clamp (a TemporalClampParams): temporal_accumulate_clamped runs instead of either, with prev_point if that is given.
        prev_normal ([H,W,4], render_features_surface_motion's fourth buffer; needs prev_point): temporal_accumulate_surface_motion
        runs, with or without clamp."""
        if prev_normal is not None and prev_point is None:
            raise ValueError("temporal_to_host: prev_normal needs prev_point")
        H, W = np.shape(moment2)
        cams = [c if isinstance(c, CameraDesc) else camera_desc(*c) for c in (cam_cur, cam_prev)]
        host = [np.ascontiguousarray(a, np.float32) for a in (accum, moment2, albedo, normal_depth) + (tuple(prev) if prev is not None else ())]
        ptrs = []
        try:
            for a in host:
                ptrs.append(self.alloc(a.nbytes))
                self.upload(ptrs[-1], a)
            if prev is None:
                ptrs += [0, 0, 0, 0]
            ptrs.append(self.alloc(W * H * 16))
            ptrs.append(self.alloc(W * H * 4))
            params = TemporalParams(W, H, cams[0], cams[1], max_history, depth_tol, normal_cos)
            if prev_point is not None:
                m = np.ascontiguousarray(prev_point, np.float32)
                ptrs.append(self.alloc(m.nbytes))
                self.upload(ptrs[-1], m)
            if prev_normal is not None:
                m = np.ascontiguousarray(prev_normal, np.float32)
                ptrs.append(self.alloc(m.nbytes))
                self.upload(ptrs[-1], m)
                self.temporal_accumulate_surface_motion(params, clamp, *ptrs)
            elif clamp is not None:
                self.temporal_accumulate_clamped(params, clamp, *ptrs)      # (ten buffers, or eleven with prev_point)
            elif prev_point is not None:
                self.temporal_accumulate_motion(params, *ptrs)
            else:
                self.temporal_accumulate(params, *ptrs)
            return self.download(ptrs[8], (H, W, 4)), self.download(ptrs[9], (H, W))
        finally:
            for p in ptrs:
                if p:
                    self.free(p)


def comm_unique_id():
    """agpt_comm_unique_id: 128 bytes (ncclUniqueId) that rank 0 hands to the other ranks."""
    buf = C.create_string_buffer(128)
    _check(lib().agpt_comm_unique_id(C.cast(buf, C.c_void_p)), "agpt_comm_unique_id")
    return buf.raw


class Comm:
    """agpt_comm: the RCCL communicator of a multi-GPU render (one rank per process / GPU)."""

    def __init__(self, ctx, world=1, rank=0, unique_id=None):
        self.ctx = ctx
        self.L = ctx.L
        h = C.c_void_p()
        idp = C.c_char_p(unique_id) if unique_id is not None else None
        _check(self.L.agpt_comm_init(ctx.h, C.cast(idp, C.c_void_p) if idp else None, int(world), int(rank), C.byref(h)), "agpt_comm_init")
        self.h = h

    def gather_tiles(self, local_ptr, W, H, block_rows, full_ptr):
        _check(self.L.agpt_gather_tiles(self.h, C.c_void_p(int(local_ptr)), W, H, block_rows, C.c_void_p(int(full_ptr) if full_ptr else 0)),
               "agpt_gather_tiles")

    def close(self):
        if self.h:
            self.L.agpt_comm_destroy(self.h)
            self.h = None


def write_png(path, rgb_words, width, height):
    """agpt_write_png: 0x00RRGGBB words (Context.resolve output), top row first."""
    a = np.ascontiguousarray(rgb_words, dtype=np.uint32)
    assert a.size == width * height
    _check(lib().agpt_write_png(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_uint32)), width, height), "agpt_write_png")


def load_hdr(path=None, data=None):
    """HDRTexture's pixels (texture.h:41-52: stbi_loadf of a Radiance .hdr) as float32 [H, W, 3], top row first -- from a file
    or from the file's bytes.  Feed it to Scene.add_infinite_area_light."""
    L = lib()
    w, h = C.c_int(0), C.c_int(0)
    rgb = C.POINTER(C.c_float)()
    if data is not None:
        buf = bytes(data)
        _check(L.agpt_hdr_parse(buf, len(buf), C.byref(w), C.byref(h), C.byref(rgb)), "agpt_hdr_parse")
    else:
        _check(L.agpt_hdr_load(os.fsencode(path), C.byref(w), C.byref(h), C.byref(rgb)), "agpt_hdr_load")
    try:
        return np.ctypeslib.as_array(rgb, (h.value, w.value, 3)).copy()
    finally:
        L.agpt_hdr_free(rgb)


def write_pfm(path, accum_host, samples):
    """agpt_write_pfm: linear float image sum/samples from a host copy of the float4 accumulator [H, W, 4]."""
    a = np.ascontiguousarray(accum_host, dtype=np.float32)
    h, w, _ = a.shape
    _check(lib().agpt_write_pfm(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_float)), w, h, samples), "agpt_write_pfm")


class Scene:
    """GPU-resident Scene (scene.h:3-30): primitives in insertion order, lights, camera."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.L = ctx.L
        h = C.c_void_p()
        _check(self.L.agpt_scene_create(ctx.h, C.byref(h)), "agpt_scene_create")
        self.h = h
        self.n_lights = 0
        self._mesh_normals = {}   # prim -> its number of normals (update_mesh passes it with normals=None in "smooth" mode)
        self._smooth = set()      # the prims in "smooth" normals mode

    def close(self):
        if self.h:
            self.L.agpt_scene_destroy(self.h)
            self.h = None

    def add_material(self, mtype, color, roughness=0.5, metallic=0.0):
        _, p = _f(color)
        return _check(self.L.agpt_scene_add_material(self.h, int(mtype), p, float(roughness), float(metallic)),
                      "agpt_scene_add_material")

    def add_mesh(self, verts, normals, uvs, indices, material, max_prims_in_node=1):
        v, pv = _f(np.asarray(verts).reshape(-1, 3))
        n = np.zeros((0, 3), np.float32) if normals is None else np.asarray(normals).reshape(-1, 3)
        n, pn = _f(n)
        t = np.zeros((0, 2), np.float32) if uvs is None else np.asarray(uvs).reshape(-1, 2)
        t, pt = _f(t)
        ix, pi = _i(np.asarray(indices).reshape(-1, 3))
        prim = _check(self.L.agpt_scene_add_mesh(self.h, pv, v.shape[0], pn, n.shape[0], pt, t.shape[0], pi,
                                                 ix.shape[0], int(material), int(max_prims_in_node)),
                      "agpt_scene_add_mesh")
        self._mesh_normals[prim] = n.shape[0]
        return prim

    @staticmethod
    def _update_mode(mode, what):
        if isinstance(mode, str):
            if mode not in ("refit", "rebuild"):
                raise ValueError("%s: unknown mode %r (refit, rebuild)" % (what, mode))
            mode = UPDATE_REFIT if mode == "refit" else UPDATE_REBUILD
        return int(mode)

    def _device_tensor(self, t, what):
        """data_ptr of a torch tensor handed to update_mesh: contiguous float32 (n, 3) on the context's GPU"""
        import torch
        if t.device.type != "cuda" or (t.device.index if t.device.index is not None else torch.cuda.current_device()) != self.ctx.device:
            raise ValueError("update_mesh: %s is on %s, the context is on GPU %d (a CPU tensor goes through .numpy())" % (what, t.device, self.ctx.device))
        if t.dtype != torch.float32:
            raise ValueError("update_mesh: %s is %s, not float32" % (what, t.dtype))
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("update_mesh: %s has shape %s, not (n, 3)" % (what, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("update_mesh: %s is not contiguous" % what)
        return t.data_ptr()

    def update_mesh(self, prim, verts, normals=None, mode=UPDATE_REFIT):
        """agpt_scene_update_mesh: new positions (and vertex normals, if the mesh has any) for mesh primitive `prim` of the committed
        scene.  mode: UPDATE_REFIT / "refit" (the tree keeps its topology, the mesh's records are rewritten on the GPU) or
        UPDATE_REBUILD / "rebuild" (a new BVH and the full upload).
        torch tensors on the context's GPU (contiguous float32, shape (n, 3)) are handed over as device pointers
        (agpt_scene_update_mesh_device) after torch's current stream has been synchronised -- unless the context runs on that very
        stream; anything else (ndarray, list, CPU tensor) goes through the host call.
        For a mesh in "smooth" normals mode (set_mesh_normals_mode) normals may be None -- NULL goes through with the mesh's own count --
        and is never read."""
        mode = self._update_mode(mode, "update_mesh")
        n_smooth = self._mesh_normals.get(int(prim), 0) if int(prim) in self._smooth else 0   # (the count that goes with a NULL)
        tensors = [type(a).__module__.split(".")[0] == "torch" and a.device.type != "cpu" for a in (verts, normals)]
        if tensors[0] or tensors[1]:
            import torch
            if not tensors[0] or (normals is not None and not tensors[1]):
                raise ValueError("update_mesh: positions and normals must both be device tensors, or neither")
            pv = self._device_tensor(verts, "verts")
            pn = None if normals is None else self._device_tensor(normals, "normals")
            stream = torch.cuda.current_stream(verts.device)
            if not self.ctx.stream or int(stream.cuda_stream) != self.ctx.stream:   # (a context on the null stream always waits)
                stream.synchronize()
            _check(self.L.agpt_scene_update_mesh_device(self.h, int(prim), C.c_void_p(pv), verts.shape[0], C.c_void_p(pn),
                                                        n_smooth if normals is None else normals.shape[0], mode), "agpt_scene_update_mesh_device")
            return
        v, pv = _f(np.asarray(verts).reshape(-1, 3))
        n, pn = (None, None) if normals is None else _f(np.asarray(normals).reshape(-1, 3))
        _check(self.L.agpt_scene_update_mesh(self.h, int(prim), pv, v.shape[0], pn, n_smooth if n is None else n.shape[0], mode),
               "agpt_scene_update_mesh")

    def update_mesh_device(self, prim, verts_ptr, n_vertices, normals_ptr=None, n_normals=0, mode=UPDATE_REFIT):
        """agpt_scene_update_mesh_device with raw device pointers (Context.alloc / upload, or a tensor's data_ptr()): the arrays must
        be complete, or produced on the context's stream."""
        _check(self.L.agpt_scene_update_mesh_device(self.h, int(prim), C.c_void_p(verts_ptr), int(n_vertices), C.c_void_p(normals_ptr or None),
                                                    int(n_normals), self._update_mode(mode, "update_mesh_device")), "agpt_scene_update_mesh_device")

    def transform_mesh(self, prim, matrix4x4, mode=UPDATE_REFIT):
        """agpt_scene_transform_mesh: mesh primitive `prim` placed by a row-major 4x4 applied on the GPU to its rest pose (the arrays
        it last received from add_mesh / update_mesh); absolute, not cumulative.  The scene is what update_mesh(prim,
        *transform_arrays(matrix4x4, rest_verts, rest_normals), mode) leaves."""
        m = np.ascontiguousarray(matrix4x4, np.float32).reshape(16)
        _check(self.L.agpt_scene_transform_mesh(self.h, int(prim), m.ctypes.data_as(C.POINTER(C.c_float)), self._update_mode(mode, "transform_mesh")),
               "agpt_scene_transform_mesh")

    def set_mesh_skin(self, prim, joints, weights, normal_joints=None, normal_weights=None, n_joints=None):
        """agpt_scene_set_mesh_skin: the binding of mesh primitive `prim` for pose_mesh -- joints / weights of shape (n_vertices, K),
        K = 1 .. 8, and normal_joints / normal_weights (n_normals, K) unless the mesh has as many normals as vertices and they share
        the influences.  n_joints: the number of matrices every pose brings (default: the highest index used + 1).  joints=None
        removes the skin."""
        if joints is None:
            _check(self.L.agpt_scene_set_mesh_skin(self.h, int(prim), 0, 0, None, None, None, None), "agpt_scene_set_mesh_skin")
            return
        j, pj, w, pw = _influences(joints, weights, "vertex")
        nj, pnj, nw, pnw = (None,) * 4 if normal_joints is None else _influences(normal_joints, normal_weights, "normal")
        if nj is not None and nj.shape[1] != j.shape[1]:
            raise ValueError("set_mesh_skin: vertices and normals have the same number of influences")
        if n_joints is None:
            n_joints = 1 + max(int(j.max(initial=0)), 0 if nj is None else int(nj.max(initial=0)))
        _check(self.L.agpt_scene_set_mesh_skin(self.h, int(prim), j.shape[1], int(n_joints), pj, pw, pnj, pnw), "agpt_scene_set_mesh_skin")

    def pose_mesh(self, prim, matrices, mode=UPDATE_REFIT):
        """agpt_scene_pose_mesh: mesh primitive `prim` posed on the GPU by matrices[n_joints, 4, 4] (or [n_joints, 16]; row-major, last
        row (0, 0, 0, 1)) through the binding of set_mesh_skin, from its rest pose (the arrays it last received from add_mesh /
        update_mesh); absolute, not cumulative.  The scene is what update_mesh(prim, *skin_arrays(matrices, rest_verts, joints,
        weights, rest_normals, ...), mode) leaves.
        A torch tensor on the context's GPU (contiguous float32, (n_joints, 4, 4) or (n_joints, 16)) is handed over as a device pointer
        (agpt_scene_pose_mesh_device: the GPU forms the palette and checks the matrices itself) after torch's current stream has been
        synchronised -- unless the context runs on that very stream, as update_mesh does; anything else (ndarray, list, CPU tensor)
        goes through the host call."""
        if _on_device(matrices):
            ptr, n = self._input_tensor(matrices, "pose_mesh", "matrices", matrix=True)
            self._wait_for_torch(matrices)
            self.pose_mesh_device(prim, ptr, n, mode)
            return
        m = _joint_matrices(matrices)
        _check(self.L.agpt_scene_pose_mesh(self.h, int(prim), m.ctypes.data_as(C.POINTER(C.c_float)), m.shape[0], self._update_mode(mode, "pose_mesh")),
               "agpt_scene_pose_mesh")

    def pose_mesh_device(self, prim, matrices_ptr, n_joints, mode=UPDATE_REFIT):
        """agpt_scene_pose_mesh_device with a raw device pointer (Context.alloc / upload, or a tensor's data_ptr(); 16-byte aligned): the
        matrices must be complete, or produced on the context's stream."""
        _check(self.L.agpt_scene_pose_mesh_device(self.h, int(prim), C.c_void_p(matrices_ptr), int(n_joints), self._update_mode(mode, "pose_mesh_device")),
               "agpt_scene_pose_mesh_device")

    def _input_tensor(self, t, fn, what, matrix):
        """(data_ptr, count) of a torch tensor handed to pose_mesh / morph_mesh: contiguous float32 on the context's GPU, (n, 4, 4) or
        (n, 16) for matrices, (T,) for weights"""
        import torch
        if t.device.type != "cuda" or (t.device.index if t.device.index is not None else torch.cuda.current_device()) != self.ctx.device:
            raise ValueError("%s: %s is on %s, the context is on GPU %d" % (fn, what, t.device, self.ctx.device))
        if t.dtype != torch.float32:
            raise ValueError("%s: %s is %s, not float32" % (fn, what, t.dtype))
        shape = tuple(t.shape)
        if (len(shape) < 2 or shape[1:] not in ((4, 4), (16,))) if matrix else len(shape) != 1:
            raise ValueError("%s: %s has shape %s, not %s" % (fn, what, shape, "(n_joints, 4, 4) or (n_joints, 16)" if matrix else "(n_targets,)"))
        if not t.is_contiguous():
            raise ValueError("%s: %s is not contiguous" % (fn, what))
        return t.data_ptr(), shape[0]

    def _wait_for_torch(self, t):
        """the same-stream rule of update_mesh: torch's current stream is synchronised unless the context runs on it"""
        import torch
        stream = torch.cuda.current_stream(t.device)
        if not self.ctx.stream or int(stream.cuda_stream) != self.ctx.stream:   # (a context on the null stream always waits)
            stream.synchronize()

    def set_mesh_morph_targets(self, prim, position_deltas, normal_deltas=None):
        """agpt_scene_set_mesh_morph_targets: the targets of mesh primitive `prim` for morph_mesh -- position_deltas of shape
        (T, n_vertices, 3) and, optionally, normal_deltas (T, n_normals, 3), with the mesh's own counts (the library reads that many).
        position_deltas=None removes them."""
        if position_deltas is None:
            _check(self.L.agpt_scene_set_mesh_morph_targets(self.h, int(prim), 0, None, None), "agpt_scene_set_mesh_morph_targets")
            return
        d = np.ascontiguousarray(position_deltas, np.float32)
        nd = None if normal_deltas is None else np.ascontiguousarray(normal_deltas, np.float32)
        if d.ndim != 3 or d.shape[2] != 3 or (nd is not None and (nd.ndim != 3 or nd.shape[2] != 3 or nd.shape[0] != d.shape[0])):
            raise ValueError("set_mesh_morph_targets: deltas of shape (n_targets, n, 3), as many targets for normals as for positions")
        fp = C.POINTER(C.c_float)
        _check(self.L.agpt_scene_set_mesh_morph_targets(self.h, int(prim), d.shape[0], d.ctypes.data_as(fp), None if nd is None else nd.ctypes.data_as(fp)),
               "agpt_scene_set_mesh_morph_targets")

    def morph_mesh(self, prim, weights, matrices=None, mode=UPDATE_REFIT):
        """agpt_scene_morph_mesh: mesh primitive `prim` morphed on the GPU by weights[T] through the targets of set_mesh_morph_targets
        and then, with matrices[n_joints, 4, 4] (or [n_joints, 16]), posed through the binding of set_mesh_skin, from its rest pose;
        absolute, not cumulative.  The scene is what update_mesh(prim, *morph_arrays(weights, rest_verts, ...), mode) leaves -- with
        matrices, those arrays through skin_arrays.
        Torch tensors on the context's GPU (contiguous float32: weights (T,), matrices (n_joints, 4, 4) or (n_joints, 16)) are handed
        over as device pointers (agpt_scene_morph_mesh_device: the GPU compacts the weights and forms the palette itself) after torch's
        current stream has been synchronised -- unless the context runs on that very stream, as update_mesh does.  If only one of the two
        is such a tensor, the other is uploaded by this call.  Host data on both sides goes through the host call."""
        if _on_device(weights) or _on_device(matrices):
            held = []   # this call's uploads of the host one of the two

            def device(a, what, matrix):
                if _on_device(a):
                    ptr_count = self._input_tensor(a, "morph_mesh", what, matrix)
                    self._wait_for_torch(a)
                    return ptr_count
                h = _joint_matrices(a) if matrix else np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))
                held.append(self.ctx.alloc(max(h.nbytes, 16)))
                self.ctx.upload(held[-1], h)
                return held[-1], h.shape[0]
            try:
                pw, T = device(weights, "weights", False)
                pm, J = (None, 0) if matrices is None else device(matrices, "matrices", True)
                self.morph_mesh_device(prim, pw, T, pm, J, mode)
            finally:
                for p in held:
                    self.ctx.free(p)
            return
        w, pw = _f(np.asarray(weights).reshape(-1))
        m = None if matrices is None else _joint_matrices(matrices)
        _check(self.L.agpt_scene_morph_mesh(self.h, int(prim), pw, w.shape[0], None if m is None else m.ctypes.data_as(C.POINTER(C.c_float)),
                                            0 if m is None else m.shape[0], self._update_mode(mode, "morph_mesh")), "agpt_scene_morph_mesh")

    def morph_mesh_device(self, prim, weights_ptr, n_targets, matrices_ptr=None, n_joints=0, mode=UPDATE_REFIT):
        """agpt_scene_morph_mesh_device with raw device pointers (Context.alloc / upload, or a tensor's data_ptr(); the matrices 16-byte
        aligned): the arrays must be complete, or produced on the context's stream."""
        _check(self.L.agpt_scene_morph_mesh_device(self.h, int(prim), C.c_void_p(weights_ptr), int(n_targets), C.c_void_p(matrices_ptr or None),
                                                   int(n_joints), self._update_mode(mode, "morph_mesh_device")), "agpt_scene_morph_mesh_device")

    def set_mesh_normals_mode(self, prim, mode):
        """agpt_scene_set_mesh_normals_mode: "given" (default; NORMALS_GIVEN) -- the normals of mesh primitive `prim` come from the caller or
        from the rest normals -- or "smooth" (NORMALS_SMOOTH) -- every update call of the mesh (update_mesh, transform_mesh, pose_mesh,
        morph_mesh) recomputes them on the GPU from the new positions: the scene is what update_mesh(prim, V, vertex_normals_arrays(V,
        indices, n_normals), mode) leaves in "given" mode.  Changes nothing by itself."""
        if isinstance(mode, str):
            if mode not in ("given", "smooth"):
                raise ValueError("set_mesh_normals_mode: unknown mode %r (given, smooth)" % (mode,))
            mode = NORMALS_GIVEN if mode == "given" else NORMALS_SMOOTH
        _check(self.L.agpt_scene_set_mesh_normals_mode(self.h, int(prim), int(mode)), "agpt_scene_set_mesh_normals_mode")
        (self._smooth.add if int(mode) == NORMALS_SMOOTH else self._smooth.discard)(int(prim))

    def update_sphere(self, prim, center, radius):
        """agpt_scene_update_sphere: a new centre and radius for sphere primitive `prim` of the committed scene -- a sphere, or the
        sphere of an area light (what add_area_light returned).  Absolute, not cumulative; the scene is what building it with the new
        values gives.  Non-finite values and radius <= 0 are refused."""
        c = np.ascontiguousarray(center, np.float32).reshape(3)
        _check(self.L.agpt_scene_update_sphere(self.h, int(prim), c.ctypes.data_as(C.POINTER(C.c_float)), float(radius)), "agpt_scene_update_sphere")

    def update_plane(self, prim, o, size):
        """agpt_scene_update_plane: a new origin o[3] and size[2] for plane primitive `prim` of the committed scene."""
        po = np.ascontiguousarray(o, np.float32).reshape(3)
        ps = np.ascontiguousarray(size, np.float32).reshape(2)
        _check(self.L.agpt_scene_update_plane(self.h, int(prim), po.ctypes.data_as(C.POINTER(C.c_float)), ps.ctypes.data_as(C.POINTER(C.c_float))),
               "agpt_scene_update_plane")

    def set_area_light_radiance(self, prim, L):
        """agpt_scene_set_area_light_radiance: the radiance of the area light whose sphere is primitive `prim`."""
        l = np.ascontiguousarray(L, np.float32).reshape(3)
        _check(self.L.agpt_scene_set_area_light_radiance(self.h, int(prim), l.ctypes.data_as(C.POINTER(C.c_float))), "agpt_scene_set_area_light_radiance")

    def set_infinite_light_radiance(self, light, L):
        """agpt_scene_set_infinite_light_radiance: the radiance of uniform infinite light `light` (what add_uniform_infinite_light returned)."""
        l = np.ascontiguousarray(L, np.float32).reshape(3)
        _check(self.L.agpt_scene_set_infinite_light_radiance(self.h, int(light), l.ctypes.data_as(C.POINTER(C.c_float))),
               "agpt_scene_set_infinite_light_radiance")

    def update_spheres(self, prims, records):
        """agpt_scene_update_spheres_device: records[n, 4] = (cx, cy, cz, radius) for the n distinct sphere primitives `prims`.  A torch
        tensor on the context's GPU (contiguous float32) is handed over as a device pointer after torch's current stream has been
        synchronised -- unless the context runs on that very stream, as update_mesh does; anything else (ndarray, list, CPU tensor)
        is uploaded by this call.  A record with a non-finite value or a radius <= 0 refuses the whole batch with nothing written."""
        ids, pi = _i(np.asarray(prims).reshape(-1))
        n = ids.shape[0]
        if type(records).__module__.split(".")[0] == "torch" and records.device.type != "cpu":
            import torch
            t = records
            if (t.device.index if t.device.index is not None else torch.cuda.current_device()) != self.ctx.device:
                raise ValueError("update_spheres: records is on %s, the context is on GPU %d" % (t.device, self.ctx.device))
            if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (n, 4) or not t.is_contiguous():
                raise ValueError("update_spheres: records must be a contiguous float32 tensor of shape (%d, 4), got %s %s" % (n, t.dtype, tuple(t.shape)))
            stream = torch.cuda.current_stream(t.device)
            if not self.ctx.stream or int(stream.cuda_stream) != self.ctx.stream:   # (a context on the null stream always waits)
                stream.synchronize()
            _check(self.L.agpt_scene_update_spheres_device(self.h, pi, n, C.c_void_p(t.data_ptr())), "agpt_scene_update_spheres_device")
            return
        r = np.ascontiguousarray(np.asarray(records, np.float32).reshape(-1, 4))
        if r.shape[0] != n:
            raise ValueError("update_spheres: %d ids but %d records" % (n, r.shape[0]))
        ptr = self.ctx.alloc(max(r.nbytes, 16))
        try:
            self.ctx.upload(ptr, r)
            _check(self.L.agpt_scene_update_spheres_device(self.h, pi, n, C.c_void_p(ptr)), "agpt_scene_update_spheres_device")
        finally:
            self.ctx.free(ptr)

    def update_spheres_device(self, prims, records_ptr):
        """agpt_scene_update_spheres_device with a raw device pointer (Context.alloc / upload, or a tensor's data_ptr())."""
        ids, pi = _i(np.asarray(prims).reshape(-1))
        _check(self.L.agpt_scene_update_spheres_device(self.h, pi, ids.shape[0], C.c_void_p(records_ptr)), "agpt_scene_update_spheres_device")

    def snapshot_positions(self):
        """agpt_scene_snapshot_positions: once per frame, after the frame's updates (meshes, spheres, planes) and before
        render_features_motion -- the scene's newer generation of triangle positions and analytic records becomes the older one and the
        newer one is filled from the device."""
        _check(self.L.agpt_scene_snapshot_positions(self.h), "agpt_scene_snapshot_positions")

    def snapshot_surfaces(self):
        """agpt_scene_snapshot_surfaces: snapshot_positions plus two generations of the per-triangle shading records; once per frame
        in its place, before render_features_surface_motion."""
        _check(self.L.agpt_scene_snapshot_surfaces(self.h), "agpt_scene_snapshot_surfaces")

    def kat_surface(self, tri_ids, b1, b2, generation=-1):
        """agpt_kat_surface: the surface reconstruction of a mesh hit alone for n global triangle ids and barycentrics, from the live
        shading records (generation -1) or the newer (0) / older (1) generation of snapshot_surfaces -> (ns[n, 3], ss[n, 3])."""
        ids = np.ascontiguousarray(np.asarray(tri_ids).reshape(-1), np.uint32)
        b1, p1 = _f(np.asarray(b1).reshape(-1))
        b2, p2 = _f(np.asarray(b2).reshape(-1))
        if not ids.shape == b1.shape == b2.shape:
            raise ValueError("kat_surface: tri_ids, b1 and b2 must have the same number of items")
        ns = np.zeros((ids.shape[0], 3), np.float32)
        ss = np.zeros((ids.shape[0], 3), np.float32)
        fp = C.POINTER(C.c_float)
        _check(self.L.agpt_kat_surface(self.h, int(generation), ids.shape[0], ids.ctypes.data_as(C.POINTER(C.c_uint32)), p1, p2,
                                       ns.ctypes.data_as(fp), ss.ctypes.data_as(fp)), "agpt_kat_surface")
        return ns, ss

    def set_bvh_builder(self, builder):
        """agpt_scene_set_bvh_builder: "host" (default) or "device" for the meshes added after this call; same bytes either way."""
        code = {"host": BVH_BUILDER_HOST, "device": BVH_BUILDER_DEVICE}[builder]
        _check(self.L.agpt_scene_set_bvh_builder(self.h, code), "agpt_scene_set_bvh_builder")

    def set_shading_arith(self, mode):
        """agpt_scene_set_shading_arith: "exact" (default; bit-identical to the oracle) or "fast" (the path weights through the
        hardware reciprocal / square root; the same rays, include/agpt.h) for the renders, Li and BSDF known-answer calls that
        follow.  An integer is passed through as the C mode value."""
        if isinstance(mode, str):
            if mode not in ("exact", "fast"):
                raise ValueError("set_shading_arith: unknown mode %r (exact, fast)" % mode)
            mode = SHADING_EXACT if mode == "exact" else SHADING_FAST
        _check(self.L.agpt_scene_set_shading_arith(self.h, int(mode)), "agpt_scene_set_shading_arith")

    def shade_variant(self):
        """agpt_scene_shade_variant: (level, fast, lds_tables, env) of the shading kernels the next render or Li call on this committed
        scene launches -- texturing level 0 .. 4, arithmetic, scene tables in LDS or in global memory (the counts, or
        AGPT_SHADE_GLOBAL_TABLES in the environment), an InfiniteAreaLight present.  Host-only."""
        out = (C.c_int32 * 4)()
        _check(self.L.agpt_scene_shade_variant(self.h, out), "agpt_scene_shade_variant")
        return tuple(int(x) for x in out)

    def add_sphere(self, center, radius, material):
        _, p = _f(center)
        return _check(self.L.agpt_scene_add_sphere(self.h, p, float(radius), int(material)), "agpt_scene_add_sphere")

    def add_plane(self, o, size, material):
        """scene->primitives.push_back(make_shared<Plane>(o, size, material)) (intersectable.h:119-157)."""
        _, po = _f(o)
        _, ps = _f(size)
        return _check(self.L.agpt_scene_add_plane(self.h, po, ps, int(material)), "agpt_scene_add_plane")

    def addAreaLight(self, center, radius, L):
        """Scene::addAreaLight(make_shared<Sphere>(center, radius, nullptr), L)."""
        _, p = _f(center)
        _, pl = _f(L)
        self.n_lights += 1
        return _check(self.L.agpt_scene_add_area_light(self.h, p, float(radius), pl), "agpt_scene_add_area_light")

    add_area_light = addAreaLight

    def add_uniform_infinite_light(self, L):
        _, pl = _f(L)
        self.n_lights += 1
        return _check(self.L.agpt_scene_add_uniform_infinite_light(self.h, pl), "agpt_scene_add_uniform_infinite_light")

    def add_infinite_area_light(self, rgb):
        """InfiniteAreaLight from an in-memory HDR image rgb[H, W, 3] (lights.cpp:31-48)."""
        img = np.ascontiguousarray(rgb, np.float32)
        self.n_lights += 1
        return _check(self.L.agpt_scene_add_infinite_area_light(self.h, img.ctypes.data_as(C.POINTER(C.c_float)),
                                                                img.shape[1], img.shape[0]),
                      "agpt_scene_add_infinite_area_light")

    def add_texture(self, rgb):
        """agpt_scene_add_texture: an image texture from rgb[H, W, 3] float32, row 0 = top, LINEAR values; returns its id."""
        img = np.ascontiguousarray(rgb, np.float32)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("add_texture: expected an array of shape [H, W, 3], got %r" % (img.shape,))
        return _check(self.L.agpt_scene_add_texture(self.h, img.ctypes.data_as(C.POINTER(C.c_float)), img.shape[1], img.shape[0]),
                      "agpt_scene_add_texture")

    def set_material_texture(self, material, texture):
        """agpt_scene_set_material_texture: the material's colour at a mesh hit becomes the texture's nearest texel at the hit's uv
        (texture = -1: the constant colour again)."""
        _check(self.L.agpt_scene_set_material_texture(self.h, int(material), int(texture)), "agpt_scene_set_material_texture")

    def set_material_param_texture(self, material, param, texture, channel=0):
        """agpt_scene_set_material_param_texture: a Disney material's roughness (PARAM_ROUGHNESS) or metallic weight (PARAM_METALLIC) at a
        mesh hit becomes channel `channel` (0 = r, 1 = g, 2 = b) of the texture's nearest texel at the hit's uv, and the material is
        rebuilt from it as add_material would have built it (texture = -1: the constant again)."""
        _check(self.L.agpt_scene_set_material_param_texture(self.h, int(material), int(param), int(texture), int(channel)),
               "agpt_scene_set_material_param_texture")

    def set_material_normal_texture(self, material, texture, scale=1.0):
        """agpt_scene_set_material_normal_texture: the material's shading normal at a mesh hit is perturbed by the texture read as a
        tangent-space normal map -- (2r - 1) * scale along the tangent, (2g - 1) * scale along cross(ns, tangent), 2b - 1 along the
        normal (texture = -1: no normal map)."""
        _check(self.L.agpt_scene_set_material_normal_texture(self.h, int(material), int(texture), float(scale)),
               "agpt_scene_set_material_normal_texture")

    def set_texture_sampler(self, texture, filter=FILTER_NEAREST, wrap_u=WRAP_REPEAT, wrap_v=WRAP_REPEAT):
        """agpt_scene_set_texture_sampler: how the texture is read in every slot that names it -- filter FILTER_NEAREST (one texel) or
        FILTER_BILINEAR (the fp32 lerp of the four texels around the position), each axis wrapped WRAP_REPEAT, WRAP_CLAMP or WRAP_MIRROR.
        The default is nearest / repeat / repeat."""
        _check(self.L.agpt_scene_set_texture_sampler(self.h, int(texture), int(filter), int(wrap_u), int(wrap_v)),
               "agpt_scene_set_texture_sampler")

    def set_camera(self, lookfrom, lookat, vup, aspect_ratio, vfov=45.0, aperture=0.0):
        d = camera_desc(lookfrom, lookat, vup, aspect_ratio, vfov, aperture)
        _check(self.L.agpt_scene_set_camera(self.h, C.byref(d)), "agpt_scene_set_camera")

    def commit(self):
        _check(self.L.agpt_scene_commit(self.h), "agpt_scene_commit")

    def bvh(self, prim):
        nn = _check(self.L.agpt_mesh_num_nodes(self.h, prim), "agpt_mesh_num_nodes")
        npr = _check(self.L.agpt_mesh_num_prims(self.h, prim), "agpt_mesh_num_prims")
        nodes = np.zeros(nn + 1, NODE_DTYPE)
        order = np.zeros(npr, np.int32)
        _check(self.L.agpt_mesh_get_bvh(self.h, prim, nodes.ctypes.data_as(C.c_void_p),
                                        order.ctypes.data_as(C.POINTER(C.c_int32))), "agpt_mesh_get_bvh")
        return nodes, order

    def _intersect(self, rays, any_hit, counters):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        out = np.zeros(rays.shape[0], HIT_DTYPE)
        st = Stats()
        _check(self.L.agpt_intersect_batch(self.h, rays.ctypes.data_as(C.c_void_p), rays.shape[0],
                                           out.ctypes.data_as(C.c_void_p), int(any_hit),
                                           C.byref(st) if counters else None),
               "agpt_intersect_batch")
        return out, st

    def intersect_device(self, rays_ptr, n, out_ptr, any_hit=False, counters=False):
        """agpt_intersect_device: rays / hits stay in HBM (pointers from Context.alloc or the host's own allocations)."""
        st = Stats()
        _check(self.L.agpt_intersect_device(self.h, C.c_void_p(rays_ptr), int(n), C.c_void_p(out_ptr), int(any_hit),
                                            C.byref(st) if counters else None), "agpt_intersect_device")
        return st

    def Intersect(self, rays, counters=False):
        """Scene::Intersect for a batch of rays (scene.h:5-13).  counters=True runs the instrumented kernel
        (work counters in the returned stats); the default runs the production kernel."""
        return self._intersect(rays, 0, counters)

    def IntersectP(self, rays, counters=False):
        """Scene::IntersectP for a batch of rays (scene.h:15-19)."""
        return self._intersect(rays, 1, counters)

    def bsdf_eval(self, material, wo, wi):
        wo, pwo = _f(np.asarray(wo).reshape(-1, 3))
        wi, pwi = _f(np.asarray(wi).reshape(-1, 3))
        n = wo.shape[0]
        f = np.zeros((n, 3), np.float32)
        pdf = np.zeros(n, np.float32)
        fp = C.POINTER(C.c_float)
        _check(self.L.agpt_kat_bsdf_eval(self.h, material, n, pwo, pwi, f.ctypes.data_as(fp), pdf.ctypes.data_as(fp)),
               "agpt_kat_bsdf_eval")
        return f, pdf

    def bsdf_sample(self, material, wo, u):
        wo, pwo = _f(np.asarray(wo).reshape(-1, 3))
        u, pu = _f(np.asarray(u).reshape(-1, 2))
        n = wo.shape[0]
        wi = np.zeros((n, 3), np.float32)
        f = np.zeros((n, 3), np.float32)
        pdf = np.zeros(n, np.float32)
        spec = np.zeros(n, np.int32)
        fp = C.POINTER(C.c_float)
        _check(self.L.agpt_kat_bsdf_sample(self.h, material, n, pwo, pu, wi.ctypes.data_as(fp), f.ctypes.data_as(fp),
                                           pdf.ctypes.data_as(fp), spec.ctypes.data_as(C.POINTER(C.c_int32))),
               "agpt_kat_bsdf_sample")
        return wi, f, pdf, spec

    def env_light(self, light, d=None, u=None):
        """agpt_kat_env_light: the device's InfiniteAreaLight functions on the map of light `light` of this scene's light list, in the
        scene's shading arithmetic.  d[n, 3] directions, taken as given -> Le[n, 3], Pdf_Li[n]; u[k] draws -> Sample_Li's wi[k, 3],
        pdf[k], radiance[k, 3], ok[k] (0 and zeros where it samples nothing).  Returns the six arrays in that order."""
        d, pd = _f(np.zeros((0, 3), np.float32) if d is None else np.asarray(d).reshape(-1, 3))
        u, pu = _f(np.zeros(0, np.float32) if u is None else np.asarray(u).reshape(-1))
        n, k = d.shape[0], u.shape[0]
        le, pli = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        wi, pdf, sle, ok = np.zeros((k, 3), np.float32), np.zeros(k, np.float32), np.zeros((k, 3), np.float32), np.zeros(k, np.int32)
        fp = C.POINTER(C.c_float)
        P = lambda a: a.ctypes.data_as(fp) if a.size else None
        _check(self.L.agpt_kat_env_light(self.h, int(light), n, P(d), P(le), P(pli), k, P(u), P(wi), P(pdf), P(sle),
                                         ok.ctypes.data_as(C.POINTER(C.c_int32)) if k else None), "agpt_kat_env_light")
        return le, pli, wi, pdf, sle, ok


class PathTracer:
    """PathTracer (integrator.h:120-196) driving the per-pixel loop of MyApp::Tick (myapp.cpp:163-175) on the GPU."""

    def __init__(self, maxDepth=5):
        self.MaxDepth = int(maxDepth)

    def render(self, scene, W, H, spp, accum_ptr, tile=None, spp_begin=0, seed_base=0, accum_pitch=None, accum_row0=0,
               samples_per_batch=0, counters=False, timing=False, want_stats=True, interleave=None, trace_all_rays=False):
        """Adds `spp` samples per pixel of `tile` (x0, y0, w, h) into the DEVICE float4 buffer at accum_ptr.
        interleave=(block_rows, world, rank) renders this rank's row blocks of the whole film into its compact buffer
        (see tiles.py) in one call.  counters: False/0 = off, True/1 = the reference-order instrumented kernel (the
        reference recursion's visit counts), 2 = the production trace kernel counting the records it fetches itself."""
        x0, y0, w, h = tile if tile is not None else (0, 0, W, H)
        il = interleave if interleave is not None else (0, 0, 0)
        rp = RenderParams(W, H, x0, y0, w, h, spp_begin, spp, seed_base & 0xFFFFFFFF, self.MaxDepth,
                          accum_pitch if accum_pitch is not None else W, accum_row0, samples_per_batch,
                          int(counters), 1 if timing else 0, il[0], il[1], il[2], 1 if trace_all_rays else 0)
        st = Stats()
        _check(scene.L.agpt_render(scene.h, C.byref(rp), C.c_void_p(int(accum_ptr)), C.byref(st) if want_stats else None),
               "agpt_render")
        return st

    def render_adaptive(self, scene, W, H, accum_ptr, moment2_ptr, min_spp, max_spp, step_spp, rel_error, abs_floor=0.0, tile=None,
                        seed_base=0, accum_pitch=None, accum_row0=0, samples_per_batch=0, counters=False, timing=False, want_stats=True,
                        interleave=None, trace_all_rays=False, spp_begin=0, spp_count=0):
        """agpt_render_adaptive: rounds of step_spp samples for the pixels of `tile` whose stop test fails, until none is active
        (include/agpt.h).  accum_ptr / moment2_ptr: DEVICE float4 / float buffers, the count in accum.w; zeroed for a fresh frame,
        kept between calls to continue one.  Other arguments as in render (spp_begin / spp_count must stay 0).
        Returns (stats, adaptive stats)."""
        x0, y0, w, h = tile if tile is not None else (0, 0, W, H)
        il = interleave if interleave is not None else (0, 0, 0)
        rp = RenderParams(W, H, x0, y0, w, h, spp_begin, spp_count, seed_base & 0xFFFFFFFF, self.MaxDepth,
                          accum_pitch if accum_pitch is not None else W, accum_row0, samples_per_batch,
                          int(counters), 1 if timing else 0, il[0], il[1], il[2], 1 if trace_all_rays else 0)
        ap = AdaptiveParams(int(min_spp), int(max_spp), int(step_spp), float(rel_error), float(abs_floor))
        st, ast = Stats(), AdaptiveStats()
        _check(scene.L.agpt_render_adaptive(scene.h, C.byref(rp), C.byref(ap), C.c_void_p(int(accum_ptr)),
                                            C.c_void_p(int(moment2_ptr)) if moment2_ptr else None, C.byref(st) if want_stats else None,
                                            C.byref(ast)), "agpt_render_adaptive")
        return st, ast

    def render_adaptive_to_host(self, scene, W, H, min_spp, max_spp, step_spp, rel_error, accum=None, moment2=None, **kw):
        """Convenience for tests and tools: uploads accum[H,W,4] / moment2[H,W] (zeros when None: a fresh frame), runs
        render_adaptive, returns (accum[H,W,4], moment2[H,W], stats, adaptive stats)."""
        ctx = scene.ctx
        acc = np.zeros((H, W, 4), np.float32) if accum is None else np.ascontiguousarray(accum, np.float32)
        m2 = np.zeros((H, W), np.float32) if moment2 is None else np.ascontiguousarray(moment2, np.float32)
        pa = ctx.alloc(acc.nbytes)
        try:
            pm = ctx.alloc(m2.nbytes)
            try:
                ctx.upload(pa, acc)
                ctx.upload(pm, m2)
                st, ast = self.render_adaptive(scene, W, H, pa, pm, min_spp, max_spp, step_spp, rel_error, **kw)
                acc = ctx.download(pa, (H, W, 4))
                m2 = ctx.download(pm, (H, W))
            finally:
                ctx.free(pm)
        finally:
            ctx.free(pa)
        return acc, m2, st, ast

    def _features(self, name, scene, W, H, ptrs, tile=None, accum_pitch=None, accum_row0=0, seed_base=0, spp_begin=0, spp_count=0,
                  interleave=None):
        """One agpt_render_features* call by name: ptrs are its DEVICE output buffers in the C order"""
        x0, y0, w, h = tile if tile is not None else (0, 0, W, H)
        il = interleave if interleave is not None else (0, 0, 0)
        rp = RenderParams(W, H, x0, y0, w, h, spp_begin, spp_count, seed_base & 0xFFFFFFFF, self.MaxDepth,
                          accum_pitch if accum_pitch is not None else W, accum_row0, 0, 0, 0, il[0], il[1], il[2], 0)
        _check(getattr(scene.L, name)(scene.h, C.byref(rp), *[C.c_void_p(int(p)) if p else None for p in ptrs]), name)

    def _features_to_host(self, call, n, scene, W, H, **kw):
        """call (one of the render_features* methods) into its n zeroed full-film buffers -> the n arrays [H,W,4]"""
        ctx = scene.ctx
        ptrs = []
        try:
            for _ in range(n):
                ptrs.append(ctx.alloc(W * H * 16))
                ctx.memset(ptrs[-1], 0, W * H * 16)
            call(scene, W, H, *ptrs, **kw)
            return tuple(ctx.download(p, (H, W, 4)) for p in ptrs)
        finally:
            for p in ptrs:
                ctx.free(p)

    def render_features(self, scene, W, H, albedo_ptr, normal_depth_ptr, tile=None, accum_pitch=None, accum_row0=0, seed_base=0,
                        spp_begin=0, spp_count=0, interleave=None):
        """agpt_render_features: one unjittered closest-hit query per pixel of `tile`; albedo_ptr / normal_depth_ptr are DEVICE
        float4 buffers indexed like render's accum: (material colour, flag 0 miss / 1 surface / 2 emitter) and (shading normal, t).
        seed_base is ignored; spp_begin, spp_count and interleave must stay at their defaults."""
        self._features("agpt_render_features", scene, W, H, (albedo_ptr, normal_depth_ptr), tile, accum_pitch, accum_row0, seed_base,
                       spp_begin, spp_count, interleave)

    def render_features_to_host(self, scene, W, H, **kw):
        """Convenience for tests and tools: render_features into zeroed full-film buffers, returns (albedo[H,W,4],
        normal_depth[H,W,4])."""
        return self._features_to_host(self.render_features, 2, scene, W, H, **kw)

    def render_features_motion(self, scene, W, H, albedo_ptr, normal_depth_ptr, prev_point_ptr, tile=None, accum_pitch=None, accum_row0=0):
        """agpt_render_features_motion: render_features plus, from the same hits, prev_point_ptr (DEVICE float4, indexed like the other
        two) = (where the hit surface point was at the scene's older position snapshot, w): w 0 a miss, 2 not moved, 1 moved.  Needs
        scene.snapshot_positions() first."""
        self._features("agpt_render_features_motion", scene, W, H, (albedo_ptr, normal_depth_ptr, prev_point_ptr), tile, accum_pitch, accum_row0)

    def render_features_motion_to_host(self, scene, W, H, **kw):
        """Convenience for tests and tools: render_features_motion into zeroed full-film buffers, returns (albedo[H,W,4],
        normal_depth[H,W,4], prev_point[H,W,4])."""
        return self._features_to_host(self.render_features_motion, 3, scene, W, H, **kw)

    def render_features_surface_motion(self, scene, W, H, albedo_ptr, normal_depth_ptr, prev_point_ptr, prev_normal_ptr, tile=None,
                                       accum_pitch=None, accum_row0=0):
        """agpt_render_features_surface_motion: render_features_motion plus prev_normal_ptr (DEVICE float4, indexed like the other
        three) = (the shading normal the hit surface point had at the scene's older snapshot, prev_point's w).  Needs
        scene.snapshot_surfaces() first."""
        self._features("agpt_render_features_surface_motion", scene, W, H, (albedo_ptr, normal_depth_ptr, prev_point_ptr, prev_normal_ptr), tile,
                       accum_pitch, accum_row0)

    def render_features_surface_motion_to_host(self, scene, W, H, **kw):
        """Convenience for tests and tools: render_features_surface_motion into zeroed full-film buffers, returns (albedo[H,W,4],
        normal_depth[H,W,4], prev_point[H,W,4], prev_normal[H,W,4])."""
        return self._features_to_host(self.render_features_surface_motion, 4, scene, W, H, **kw)

    def Li(self, scene, rays, rng_states):
        """Integrator::Li (integrator.h:28-31, 120-191) for a batch of rays (RAY_DTYPE) with one xorshift32 state each:
        returns (radiance [n, 3] float32 -- unfiltered --, the states after the paths, stats)."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        states = np.ascontiguousarray(rng_states, np.uint32)
        n = len(rays)
        assert states.shape == (n,)
        out = np.zeros((n, 3), np.float32)
        after = np.zeros(n, np.uint32)
        st = Stats()
        u32 = C.POINTER(C.c_uint32)
        _check(scene.L.agpt_li_batch(scene.h, rays.ctypes.data_as(C.c_void_p), states.ctypes.data_as(u32), n, self.MaxDepth,
                                     out.ctypes.data_as(C.POINTER(C.c_float)), after.ctypes.data_as(u32), C.byref(st)), "agpt_li_batch")
        return out, after, st

    @staticmethod
    def DbgLi(scene, rays):
        """DbgIntegrator::Li (integrator.h:107-118) for a batch of rays: (u, v, 0) / 5 of the hit's texture coordinates, red where
        u or v is 0, black on a miss; float32 [n, 3]."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        out = np.zeros((len(rays), 3), np.float32)
        _check(scene.L.agpt_dbg_li_batch(scene.h, rays.ctypes.data_as(C.c_void_p), len(rays), out.ctypes.data_as(C.POINTER(C.c_float))),
               "agpt_dbg_li_batch")
        return out

    def render_to_host(self, scene, W, H, spp, **kw):
        """Convenience for tests: allocates a zeroed accumulator, renders, returns (accum[H,W,4], stats)."""
        ctx = scene.ctx
        nbytes = W * H * 16
        ptr = ctx.alloc(nbytes)
        try:
            ctx.memset(ptr, 0, nbytes)
            st = self.render(scene, W, H, spp, ptr, **kw)
            acc = ctx.download(ptr, (H, W, 4))
        finally:
            ctx.free(ptr)
        return acc, st
