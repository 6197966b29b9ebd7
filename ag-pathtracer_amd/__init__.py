"""ag-pathtracer_amd: the MI355X-native path-tracing hot path of voxel-tracer/ag-pathtracer.

Hand-written gfx950 HIP kernels (BVH traversal, triangle/sphere tests, Disney/microfacet shading, NEE + MIS) behind
the C ABI of include/agpt.h, plus this thin host mirror of the reference's Scene / Integrator surface.
"""
from . import build as _build  # noqa: F401
from .binding import (MAT_DIFFUSE_ONLY, MAT_DISNEY, MAT_MIRROR, AgptError, CameraDesc, Context, PathTracer,  # noqa: F401
                      RenderParams, AdaptiveParams, AdaptiveStats, DenoiseParams, DENOISE_SIGMA_Z, DENOISE_SIGMA_N, DENOISE_SIGMA_L, TemporalParams, TemporalClampParams, TEMPORAL_DEPTH_TOL, TEMPORAL_NORMAL_COS, TEMPORAL_MIN_WEIGHT, camera_desc, camera_vectors, Scene, Stats, Comm, comm_unique_id, create_backdrop, bvh_build, bvh_refit, bvh_build_device, transform_arrays, skin_arrays, skin_palette, morph_arrays, morph_active, vertex_normals_arrays, toplevel_build, toplevel_pack16, load_obj, load_hdr, lib, library_path, HIT_DTYPE, NODE_DTYPE, RAY_DTYPE, BVH_DEVICE_CHUNK, BVH_DEVICE_LANE_MAX,
                      UPDATE_REFIT, UPDATE_REBUILD, NORMALS_GIVEN, NORMALS_SMOOTH, SHADING_EXACT, SHADING_FAST, PARAM_ROUGHNESS, PARAM_METALLIC,
                      FILTER_NEAREST, FILTER_BILINEAR, WRAP_REPEAT, WRAP_CLAMP, WRAP_MIRROR,
                      EXPORTS)
from . import scenes  # noqa: F401
from .scenes import SceneDesc  # noqa: F401


def build(force=False, verbose=False):
    """Compile libagpt_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    return _build.build(force=force, verbose=verbose)
