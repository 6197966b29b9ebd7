// agpt_temporal.hip -- the kernel of agpt_temporal_accumulate (include/agpt.h): per pixel, find where the surface seen now was on
// the previous film, blend the history found there from the (up to) four pixels around that position, and add it to this frame's
// sums in the form agpt_denoise reads (sums, the count in w, the luminance second moment).
//
// Every pixel is computed by one thread in a fixed tap order: no atomics, no cross-lane sums, no LDS, so tests/temporal_model.py
// reproduces it operation by operation.  Compiled with the library's common flags (-ffp-contract=off, IEEE divide / sqrt).
// A bandwidth kernel: per pixel 52 B of this frame read and 20 B written, contiguous per wave (a wave is 64 consecutive pixels of a
// row), plus per tap 4 B of flag, 16 B of history and -- for accepted geometry -- 16 B of normal_depth and 4 B of moment, gathered
// around the reprojected position (neighbouring pixels land on neighbouring taps: the lines are shared through L1 / L2).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "agpt_internal.h"
#include "agpt_temporal.h"

using agpt::fail;

__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal(TemporalConsts tc, const float4* __restrict__ accum_cur, const float* __restrict__ moment2_cur,
           const float4* __restrict__ albedo_cur, const float4* __restrict__ normal_depth_cur, const float4* __restrict__ hist_accum_prev,
           const float* __restrict__ hist_moment2_prev, const float4* __restrict__ albedo_prev, const float4* __restrict__ normal_depth_prev,
           float4* __restrict__ hist_accum_out, float* __restrict__ hist_moment2_out) {
    temporal_pixel<false>(tc, accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev,
                          normal_depth_prev, nullptr, hist_accum_out, hist_moment2_out);
}

namespace agpt {

// The argument checks of agpt_temporal_accumulate in the header's order (`fn` names the entry point that was called), then the
// kernel's constants and grid: shared with agpt_temporal_accumulate_motion (agpt_motion.hip), which adds its own checks behind them.
int temporal_prepare(const char* fn, agpt_ctx* c, const agpt_temporal_params* p, const float* const in[8], const float* hist_accum_out_dev,
                     const float* hist_moment2_out_dev, TemporalConsts& tc, dim3& tiles) {
    const std::string f(fn);
    if (!p) return fail(AGPT_ERR_INVALID, f + ": NULL argument");
    if (p->width <= 0 || p->height <= 0 || (uint64_t)p->width * (uint64_t)p->height > 0x7FFFFFFFull)
        return fail(AGPT_ERR_INVALID, f + ": bad film size");
    if (!(p->max_history > 0.f) || std::isinf(p->max_history))
        return fail(AGPT_ERR_INVALID, f + ": max_history must be positive and finite");
    if (!(p->depth_tol >= 0.f) || std::isinf(p->depth_tol))
        return fail(AGPT_ERR_INVALID, f + ": depth_tol must be non-negative and finite");
    if (!(p->normal_cos >= -1.f && p->normal_cos <= 1.f))
        return fail(AGPT_ERR_INVALID, f + ": normal_cos must be in [-1, 1]");
    if (!c || !in[0] || !in[1] || !in[2] || !in[3] || !hist_accum_out_dev || !hist_moment2_out_dev)
        return fail(AGPT_ERR_INVALID, f + ": NULL argument");
    const int n_prev = (in[4] != nullptr) + (in[5] != nullptr) + (in[6] != nullptr) + (in[7] != nullptr);
    if (n_prev != 0 && n_prev != 4)
        return fail(AGPT_ERR_INVALID, f + ": the four prev buffers must be all NULL (first frame) or all given");
    for (int k = 0; k < 8; k++)
        if (in[k] && (in[k] == hist_accum_out_dev || in[k] == hist_moment2_out_dev))
            return fail(AGPT_ERR_INVALID, f + ": an output aliases an input");
    if (hist_accum_out_dev == hist_moment2_out_dev) return fail(AGPT_ERR_INVALID, f + ": the two outputs are one buffer");
    tc = TemporalConsts{};
    tc.W = p->width; tc.H = p->height;
    tc.identity = std::memcmp(&p->cam_prev, &p->cam_cur, sizeof(agpt_camera_desc)) == 0;
    tc.max_history = p->max_history; tc.depth_tol = p->depth_tol; tc.normal_cos = p->normal_cos;
    tc.cur = agpt::make_camera(p->cam_cur);
    tc.prev = agpt::make_camera(p->cam_prev);
    // one thread per film pixel in k_denoise_pass' tiling
    static_assert(AGPT_DN_TX * AGPT_DN_TY == AGPT_BLOCK, "one thread per tile pixel");
    tiles = dim3((unsigned)((tc.W + AGPT_DN_TX - 1) / AGPT_DN_TX), (unsigned)((tc.H + AGPT_DN_TY - 1) / AGPT_DN_TY));
    return AGPT_OK;
}

}  // namespace agpt

extern "C" {

// One k_temporal launch: this frame's buffers plus the previous frame's history, reprojected, into the history buffers the next
// agpt_denoise and the next frame's call read.
int agpt_temporal_accumulate(agpt_ctx* c, const agpt_temporal_params* p, const float* accum_cur_dev, const float* moment2_cur_dev,
                             const float* albedo_cur_dev, const float* normal_depth_cur_dev, const float* hist_accum_prev_dev,
                             const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
                             float* hist_accum_out_dev, float* hist_moment2_out_dev) {
    const float* in[8] = {accum_cur_dev, moment2_cur_dev, albedo_cur_dev, normal_depth_cur_dev,
                          hist_accum_prev_dev, hist_moment2_prev_dev, albedo_prev_dev, normal_depth_prev_dev};
    TemporalConsts tc;
    dim3 tiles;
    if (const int rc = agpt::temporal_prepare("agpt_temporal_accumulate", c, p, in, hist_accum_out_dev, hist_moment2_out_dev, tc, tiles)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_temporal, tiles, dim3(AGPT_BLOCK), 0, c->stream, tc, (const float4*)accum_cur_dev, moment2_cur_dev,
                       (const float4*)albedo_cur_dev, (const float4*)normal_depth_cur_dev, (const float4*)hist_accum_prev_dev,
                       hist_moment2_prev_dev, (const float4*)albedo_prev_dev, (const float4*)normal_depth_prev_dev,
                       (float4*)hist_accum_out_dev, hist_moment2_out_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

}  // extern "C"
