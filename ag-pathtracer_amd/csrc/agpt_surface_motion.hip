// agpt_surface_motion.hip -- agpt_temporal_accumulate_surface_motion (include/agpt.h) and its two kernels: k_temporal_motion
// (agpt_motion.hip) and k_temporal_clamp (agpt_temporal_clamp.hip) whose step 4 compares, for a moved pixel, the normal the surface point
// had a frame ago -- prev_normal_cur of agpt_render_features_surface_motion -- with the previous tap's.  The bodies are the shared ones
// (temporal_pixel, agpt_temporal.h; temporal_clamp_block, agpt_temporal_clamp.h) with their SURFACE flag: 16 B more for a moved pixel,
// nothing else; one thread per pixel, no atomics.  The other two calls of the feature live beside what they extend:
// agpt_scene_snapshot_surfaces in agpt_motion.hip, the PREV feature kernels in agpt_denoise.hip, agpt_kat_surface in agpt_kat.hip.
// Compiled with the library's common flags (-ffp-contract=off, IEEE divide / sqrt).
#include <hip/hip_runtime.h>

#include <string>

#include "agpt_internal.h"
#include "agpt_temporal_clamp.h"

using agpt::fail;

__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal_surface(TemporalConsts tc, const float4* __restrict__ accum_cur, const float* __restrict__ moment2_cur,
                   const float4* __restrict__ albedo_cur, const float4* __restrict__ normal_depth_cur, const float4* __restrict__ hist_accum_prev,
                   const float* __restrict__ hist_moment2_prev, const float4* __restrict__ albedo_prev,
                   const float4* __restrict__ normal_depth_prev, const float4* __restrict__ prev_point_cur,
                   const float4* __restrict__ prev_normal_cur, float4* __restrict__ hist_accum_out, float* __restrict__ hist_moment2_out) {
    temporal_pixel<true, true>(tc, accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev,
                               normal_depth_prev, prev_point_cur, hist_accum_out, hist_moment2_out, prev_normal_cur);
}
__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal_clamp_surface(TemporalConsts tc, TemporalClampConsts cc, const float4* __restrict__ accum_cur, const float* __restrict__ moment2_cur,
                         const float4* __restrict__ albedo_cur, const float4* __restrict__ normal_depth_cur,
                         const float4* __restrict__ hist_accum_prev, const float* __restrict__ hist_moment2_prev,
                         const float4* __restrict__ albedo_prev, const float4* __restrict__ normal_depth_prev,
                         const float4* __restrict__ prev_point_cur, const float4* __restrict__ prev_normal_cur,
                         float4* __restrict__ hist_accum_out, float* __restrict__ hist_moment2_out) {
    __shared__ float4 tile[AGPT_TC_TILE_W * AGPT_TC_TILE_H];
    temporal_clamp_block<true>(tc, cc, tile, accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev,
                               albedo_prev, normal_depth_prev, prev_point_cur, hist_accum_out, hist_moment2_out, prev_normal_cur);
}

extern "C" {

// One launch: k_temporal_surface, or -- cp given -- k_temporal_clamp_surface
int agpt_temporal_accumulate_surface_motion(agpt_ctx* c, const agpt_temporal_params* p, const agpt_temporal_clamp_params* cp,
                                            const float* accum_cur_dev, const float* moment2_cur_dev, const float* albedo_cur_dev,
                                            const float* normal_depth_cur_dev, const float* hist_accum_prev_dev,
                                            const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
                                            float* hist_accum_out_dev, float* hist_moment2_out_dev, const float* prev_point_cur_dev,
                                            const float* prev_normal_cur_dev) {
    const char* fn = "agpt_temporal_accumulate_surface_motion";
    const std::string f(fn);
    const float* in[8] = {accum_cur_dev, moment2_cur_dev, albedo_cur_dev, normal_depth_cur_dev,
                          hist_accum_prev_dev, hist_moment2_prev_dev, albedo_prev_dev, normal_depth_prev_dev};
    TemporalConsts tc;
    dim3 tiles;
    if (const int rc = agpt::temporal_prepare(fn, c, p, in, hist_accum_out_dev, hist_moment2_out_dev, tc, tiles)) return rc;
    if (cp)
        if (const int rc = agpt::check_clamp(fn, cp)) return rc;
    if (!prev_point_cur_dev) return fail(AGPT_ERR_INVALID, f + ": NULL prev_point_cur_dev");
    if (prev_point_cur_dev == hist_accum_out_dev || prev_point_cur_dev == hist_moment2_out_dev)
        return fail(AGPT_ERR_INVALID, f + ": an output aliases prev_point_cur_dev");
    if (!prev_normal_cur_dev) return fail(AGPT_ERR_INVALID, f + ": NULL prev_normal_cur_dev");
    if (prev_normal_cur_dev == hist_accum_out_dev || prev_normal_cur_dev == hist_moment2_out_dev)
        return fail(AGPT_ERR_INVALID, f + ": an output aliases prev_normal_cur_dev");
    HIP_TRY(hipSetDevice(c->device));
    if (cp) {
        const TemporalClampConsts cc = agpt::clamp_consts(cp, true);
        hipLaunchKernelGGL(k_temporal_clamp_surface, tiles, dim3(AGPT_BLOCK), 0, c->stream, tc, cc, (const float4*)accum_cur_dev, moment2_cur_dev,
                           (const float4*)albedo_cur_dev, (const float4*)normal_depth_cur_dev, (const float4*)hist_accum_prev_dev,
                           hist_moment2_prev_dev, (const float4*)albedo_prev_dev, (const float4*)normal_depth_prev_dev,
                           (const float4*)prev_point_cur_dev, (const float4*)prev_normal_cur_dev, (float4*)hist_accum_out_dev,
                           hist_moment2_out_dev);
    } else {
        hipLaunchKernelGGL(k_temporal_surface, tiles, dim3(AGPT_BLOCK), 0, c->stream, tc, (const float4*)accum_cur_dev, moment2_cur_dev,
                           (const float4*)albedo_cur_dev, (const float4*)normal_depth_cur_dev, (const float4*)hist_accum_prev_dev,
                           hist_moment2_prev_dev, (const float4*)albedo_prev_dev, (const float4*)normal_depth_prev_dev,
                           (const float4*)prev_point_cur_dev, (const float4*)prev_normal_cur_dev, (float4*)hist_accum_out_dev,
                           hist_moment2_out_dev);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

}  // extern "C"
