// agpt_temporal.h -- host-side launcher of the temporal reprojection unit (agpt_temporal.hip), used by agpt_temporal_accumulate in
// agpt_api.hip.
#pragma once

#include "agpt_denoise.h"

struct TemporalConsts {
    int32_t W, H;
    int32_t identity;      // 1: the two camera descriptions are the same bytes -- every pixel reads its own history, no arithmetic
    float max_history, depth_tol, normal_cos;
    DevCamera cur, prev;   // make_camera of the two descriptions
};

namespace agpt {
// one thread per film pixel in k_denoise_pass' tiling; the four prev pointers are all NULL (first frame) or all set
void launch_temporal(hipStream_t stream, const TemporalConsts& tc, const float4* accum_cur, const float* moment2_cur, const float4* albedo_cur,
                     const float4* normal_depth_cur, const float4* hist_accum_prev, const float* hist_moment2_prev, const float4* albedo_prev,
                     const float4* normal_depth_prev, float4* hist_accum_out, float* hist_moment2_out);
}  // namespace agpt
