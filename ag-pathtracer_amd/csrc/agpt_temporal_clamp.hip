// agpt_temporal_clamp.hip -- the kernel of agpt_temporal_accumulate_clamped (include/agpt.h): agpt_temporal_accumulate or, with a
// prev_point buffer, agpt_temporal_accumulate_motion, whose reprojected history mean is clamped to the box mu +- gamma * sigma of the
// CURRENT frame's (2r+1)^2 neighbourhood before it is blended -- history that geometry accepts but whose lighting went stale (the
// shadow a moved mesh left behind) is pulled to what the frame's own samples say, and its count is cut so that it fades.
//
// One launch.  A block of k_denoise_pass' tiling (64 x 4 pixels, one thread each) first stages, cooperatively, its tile plus a halo of
// r pixels in LDS: one float4 per pixel = (the demodulated mean x.rgb, the flag), w = NaN for a pixel that no window may use (outside
// the film, or without samples: a NaN compares unequal to every flag).  The tile is sized for r = 3: 70 x 10 x 16 B = 11200 B a block.
// One barrier, reached by every thread of the block, then each thread runs steps 3 and 4 (temporal_gather, agpt_temporal.h: the
// definition k_temporal and k_temporal_motion use) and, only if its pixel has history, walks its window from LDS in the contract's
// order -- dy = -r .. r outermost in FILM rows, which are the buffer's rows backwards -- and runs step 5'.  No atomics, no cross-lane
// sums: tests/temporal_clamp_model.py reproduces it operation by operation.  Compiled with the library's common flags
// (-ffp-contract=off, IEEE divide / sqrt).
// Traffic: k_temporal_motion's, plus the halo's re-read of accum_cur and albedo_cur (32 B a staged pixel: 700 staged for 256 produced
// at r = 3, mostly L2 hits on the neighbouring blocks' lines), plus up to 49 ds_read_b128 a pixel -- consecutive lanes read consecutive
// 16 B, no bank conflicts.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "agpt_internal.h"
#include "agpt_temporal_clamp.h"

using agpt::fail;

__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal_clamp(TemporalConsts tc, TemporalClampConsts cc, const float4* __restrict__ accum_cur, const float* __restrict__ moment2_cur,
                 const float4* __restrict__ albedo_cur, const float4* __restrict__ normal_depth_cur, const float4* __restrict__ hist_accum_prev,
                 const float* __restrict__ hist_moment2_prev, const float4* __restrict__ albedo_prev,
                 const float4* __restrict__ normal_depth_prev, const float4* __restrict__ prev_point_cur, float4* __restrict__ hist_accum_out,
                 float* __restrict__ hist_moment2_out) {
    __shared__ float4 tile[AGPT_TC_TILE_W * AGPT_TC_TILE_H];
    temporal_clamp_block<false>(tc, cc, tile, accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev,
                                albedo_prev, normal_depth_prev, prev_point_cur, hist_accum_out, hist_moment2_out, nullptr);
}

// agpt_temporal_accumulate_clamped's checks of its clamp parameters, in the header's order, under the name `fn`
namespace agpt {

int check_clamp(const char* fn, const agpt_temporal_clamp_params* cp) {
    const std::string f(fn);
    if (!cp) return fail(AGPT_ERR_INVALID, f + ": NULL clamp params");
    if (cp->radius < 1 || cp->radius > AGPT_TC_RADIUS_MAX) return fail(AGPT_ERR_INVALID, f + ": radius must be 1..3");
    if (cp->demodulate != 0 && cp->demodulate != 1) return fail(AGPT_ERR_INVALID, f + ": demodulate must be 0 or 1");
    if (!(cp->gamma >= 0.f)) return fail(AGPT_ERR_INVALID, f + ": gamma must be non-negative");
    if (!(cp->clamped_max_history > 0.f) || std::isinf(cp->clamped_max_history))
        return fail(AGPT_ERR_INVALID, f + ": clamped_max_history must be positive and finite");
    return AGPT_OK;
}
TemporalClampConsts clamp_consts(const agpt_temporal_clamp_params* cp, bool motion) {
    TemporalClampConsts cc;
    cc.radius = cp->radius;
    cc.demodulate = cp->demodulate;
    cc.motion = motion;
    cc.gamma = cp->gamma;
    cc.clamped_max_history = cp->clamped_max_history;
    return cc;
}

}  // namespace agpt

extern "C" {

// One k_temporal_clamp launch
int agpt_temporal_accumulate_clamped(agpt_ctx* c, const agpt_temporal_params* p, const agpt_temporal_clamp_params* cp,
                                     const float* accum_cur_dev, const float* moment2_cur_dev, const float* albedo_cur_dev,
                                     const float* normal_depth_cur_dev, const float* hist_accum_prev_dev, const float* hist_moment2_prev_dev,
                                     const float* albedo_prev_dev, const float* normal_depth_prev_dev, float* hist_accum_out_dev,
                                     float* hist_moment2_out_dev, const float* prev_point_cur_dev) {
    const float* in[8] = {accum_cur_dev, moment2_cur_dev, albedo_cur_dev, normal_depth_cur_dev,
                          hist_accum_prev_dev, hist_moment2_prev_dev, albedo_prev_dev, normal_depth_prev_dev};
    TemporalConsts tc;
    dim3 tiles;
    if (const int rc = agpt::temporal_prepare("agpt_temporal_accumulate_clamped", c, p, in, hist_accum_out_dev, hist_moment2_out_dev, tc, tiles))
        return rc;
    if (const int rc = agpt::check_clamp("agpt_temporal_accumulate_clamped", cp)) return rc;
    if (prev_point_cur_dev && (prev_point_cur_dev == hist_accum_out_dev || prev_point_cur_dev == hist_moment2_out_dev))
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate_clamped: an output aliases prev_point_cur_dev");
    const TemporalClampConsts cc = agpt::clamp_consts(cp, prev_point_cur_dev != nullptr);
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_temporal_clamp, tiles, dim3(AGPT_BLOCK), 0, c->stream, tc, cc, (const float4*)accum_cur_dev, moment2_cur_dev,
                       (const float4*)albedo_cur_dev, (const float4*)normal_depth_cur_dev, (const float4*)hist_accum_prev_dev,
                       hist_moment2_prev_dev, (const float4*)albedo_prev_dev, (const float4*)normal_depth_prev_dev,
                       (const float4*)prev_point_cur_dev, (float4*)hist_accum_out_dev, hist_moment2_out_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

}  // extern "C"
