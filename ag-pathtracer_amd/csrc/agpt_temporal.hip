// agpt_temporal.hip -- the temporal reprojection of render history (include/agpt.h): the four agpt_temporal_accumulate* entry points and
// their five kernels over one body (agpt_temporal.h).  Per pixel, find where the surface seen now was on the previous film, blend the
// history found there from the (up to) four pixels around that position, and add it to this frame's sums in the form agpt_denoise reads
// (sums, the count in w, the luminance second moment).
//   k_temporal                agpt_temporal_accumulate
//   k_temporal_motion         agpt_temporal_accumulate_motion: step 3 decided per pixel by prev_point_cur
//   k_temporal_surface        agpt_temporal_accumulate_surface_motion: step 4 compares, for a moved pixel, prev_normal_cur
//   k_temporal_clamp          agpt_temporal_accumulate_clamped, with or without prev_point_cur (cc.motion): the reprojected history mean
//                             is clamped to the box mu +- gamma * sigma of the CURRENT frame's (2r+1)^2 neighbourhood before it is
//                             blended -- history that geometry accepts but whose lighting went stale (the shadow a moved mesh left
//                             behind) is pulled to what the frame's own samples say, and its count is cut so that it fades
//   k_temporal_clamp_surface  agpt_temporal_accumulate_surface_motion with clamp parameters
// The other calls of the motion features live beside what they extend: the snapshots and k_motion in agpt_motion.hip, the feature
// kernels in agpt_denoise.hip, agpt_kat_surface in agpt_kat.hip.
//
// One launch a call.  Every pixel is computed by one thread in a fixed tap order: no atomics, no cross-lane sums, and LDS only for the
// clamp kernels' tile of the current frame (sized for r = 3: 70 x 10 x 16 B = 11200 B a block), so tests/temporal_model.py,
// tests/motion_model.py and tests/temporal_clamp_model.py reproduce them operation by operation.  Compiled with the library's common
// flags (-ffp-contract=off, IEEE divide / sqrt).
// Bandwidth kernels: per pixel 52 B of this frame read and 20 B written, contiguous per wave (a wave is 64 consecutive pixels of a
// row), plus per tap 4 B of flag, 16 B of history and -- for accepted geometry -- 16 B of normal_depth and 4 B of moment, gathered
// around the reprojected position (neighbouring pixels land on neighbouring taps: the lines are shared through L1 / L2).  MOTION adds
// 16 B a pixel, SURFACE 16 B for a moved pixel.  The clamp kernels add the halo's re-read of accum_cur and albedo_cur (32 B a staged
// pixel: 700 staged for 256 produced at r = 3, mostly L2 hits on the neighbouring blocks' lines) and up to 49 ds_read_b128 a pixel --
// consecutive lanes read consecutive 16 B, no bank conflicts.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "agpt_internal.h"
#include "agpt_temporal.h"

using agpt::fail;

// The kernels' parameter lists -- each buffer a __restrict__ parameter of its own -- and the TemporalIO a kernel builds from them
// (point, normal: its prev_point_cur and prev_normal_cur parameters, or nullptr)
#define AGPT_TP_INPUTS                                                                                                                \
    const float4* __restrict__ accum_cur, const float* __restrict__ moment2_cur, const float4* __restrict__ albedo_cur,               \
        const float4* __restrict__ normal_depth_cur, const float4* __restrict__ hist_accum_prev, const float* __restrict__ hist_moment2_prev, \
        const float4* __restrict__ albedo_prev, const float4* __restrict__ normal_depth_prev
#define AGPT_TP_POINT const float4* __restrict__ prev_point_cur
#define AGPT_TP_NORMAL const float4* __restrict__ prev_normal_cur
#define AGPT_TP_OUTPUTS float4* __restrict__ hist_accum_out, float* __restrict__ hist_moment2_out
#define AGPT_TP_IO(point, normal)                                                                                                     \
    TemporalIO {                                                                                                                      \
        accum_cur, moment2_cur, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev, normal_depth_prev, point, \
            normal, hist_accum_out, hist_moment2_out                                                                                  \
    }

__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal(TemporalConsts tc, AGPT_TP_INPUTS, AGPT_TP_OUTPUTS) {
    temporal_block<false, false>(tc, AGPT_TP_IO(nullptr, nullptr), false);
}
__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal_motion(TemporalConsts tc, AGPT_TP_INPUTS, AGPT_TP_POINT, AGPT_TP_OUTPUTS) {
    temporal_block<false, false>(tc, AGPT_TP_IO(prev_point_cur, nullptr), true);
}
__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal_surface(TemporalConsts tc, AGPT_TP_INPUTS, AGPT_TP_POINT, AGPT_TP_NORMAL, AGPT_TP_OUTPUTS) {
    temporal_block<true, false>(tc, AGPT_TP_IO(prev_point_cur, prev_normal_cur), true);
}
__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal_clamp(TemporalConsts tc, TemporalClampConsts cc, AGPT_TP_INPUTS, AGPT_TP_POINT, AGPT_TP_OUTPUTS) {
    __shared__ float4 tile[AGPT_TC_TILE_W * AGPT_TC_TILE_H];
    temporal_block<false, true>(tc, AGPT_TP_IO(prev_point_cur, nullptr), cc.motion, &cc, tile);
}
__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal_clamp_surface(TemporalConsts tc, TemporalClampConsts cc, AGPT_TP_INPUTS, AGPT_TP_POINT, AGPT_TP_NORMAL, AGPT_TP_OUTPUTS) {
    __shared__ float4 tile[AGPT_TC_TILE_W * AGPT_TC_TILE_H];
    temporal_block<true, true>(tc, AGPT_TP_IO(prev_point_cur, prev_normal_cur), cc.motion, &cc, tile);
}

#undef AGPT_TP_INPUTS
#undef AGPT_TP_POINT
#undef AGPT_TP_NORMAL
#undef AGPT_TP_OUTPUTS
#undef AGPT_TP_IO

// The argument checks of agpt_temporal_accumulate in the header's order (`fn` names the entry point that was called), then the
// kernels' constants and grid; in = the four current and the four prev buffers
static int temporal_prepare(const char* fn, agpt_ctx* c, const agpt_temporal_params* p, const float* const in[8], const float* hist_accum_out_dev,
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

// agpt_temporal_accumulate_clamped's checks of its clamp parameters, in the header's order, under the name `fn`
static int check_clamp(const char* fn, const agpt_temporal_clamp_params* cp) {
    const std::string f(fn);
    if (!cp) return fail(AGPT_ERR_INVALID, f + ": NULL clamp params");
    if (cp->radius < 1 || cp->radius > AGPT_TC_RADIUS_MAX) return fail(AGPT_ERR_INVALID, f + ": radius must be 1..3");
    if (cp->demodulate != 0 && cp->demodulate != 1) return fail(AGPT_ERR_INVALID, f + ": demodulate must be 0 or 1");
    if (!(cp->gamma >= 0.f)) return fail(AGPT_ERR_INVALID, f + ": gamma must be non-negative");
    if (!(cp->clamped_max_history > 0.f) || std::isinf(cp->clamped_max_history))
        return fail(AGPT_ERR_INVALID, f + ": clamped_max_history must be positive and finite");
    return AGPT_OK;
}
static TemporalClampConsts clamp_consts(const agpt_temporal_clamp_params* cp, bool motion) {
    TemporalClampConsts cc;
    cc.radius = cp->radius;
    cc.demodulate = cp->demodulate;
    cc.motion = motion;
    cc.gamma = cp->gamma;
    cc.clamped_max_history = cp->clamped_max_history;
    return cc;
}

// What an entry point requires of its optional arguments: NULL is an error (otherwise the kernel is the one that does without it)
enum { NEED_CLAMP = 1, NEED_POINT = 2, NEED_NORMAL = 4 };

// Every agpt_temporal_accumulate* call under its name `fn`: the checks in the header's order, then one launch and the wait for it.
// in: the four current and the four prev buffers; cp, point (prev_point_cur_dev), normal (prev_normal_cur_dev): NULL from an entry point
// that has no such argument.
static int temporal_accumulate(const char* fn, int need, agpt_ctx* c, const agpt_temporal_params* p, const agpt_temporal_clamp_params* cp,
                               const float* const (&in)[8], const float* point, const float* normal, float* hist_accum_out_dev,
                               float* hist_moment2_out_dev) {
    const std::string f(fn);
    TemporalConsts tc;
    dim3 tiles;
    if (const int rc = temporal_prepare(fn, c, p, in, hist_accum_out_dev, hist_moment2_out_dev, tc, tiles)) return rc;
    if ((need & NEED_CLAMP) || cp)
        if (const int rc = check_clamp(fn, cp)) return rc;
    if ((need & NEED_POINT) && !point) return fail(AGPT_ERR_INVALID, f + ": NULL prev_point_cur_dev");
    if (point && (point == hist_accum_out_dev || point == hist_moment2_out_dev))
        return fail(AGPT_ERR_INVALID, f + ": an output aliases prev_point_cur_dev");
    if ((need & NEED_NORMAL) && !normal) return fail(AGPT_ERR_INVALID, f + ": NULL prev_normal_cur_dev");
    if (normal && (normal == hist_accum_out_dev || normal == hist_moment2_out_dev))
        return fail(AGPT_ERR_INVALID, f + ": an output aliases prev_normal_cur_dev");
    const float4 *pp = (const float4*)point, *pn = (const float4*)normal;
    HIP_TRY(hipSetDevice(c->device));
    // (a kernel's arguments: tc, the clamp kernels' cc, the eight inputs, the kernel's own of pp and pn, the two outputs)
#define LAUNCH(kernel, ...)                                                                                                           \
    hipLaunchKernelGGL(kernel, tiles, dim3(AGPT_BLOCK), 0, c->stream, tc, __VA_ARGS__, (float4*)hist_accum_out_dev, hist_moment2_out_dev)
#define INPUTS                                                                                                                        \
    (const float4*)in[0], in[1], (const float4*)in[2], (const float4*)in[3], (const float4*)in[4], in[5], (const float4*)in[6], (const float4*)in[7]
    if (cp) {
        const TemporalClampConsts cc = clamp_consts(cp, pp != nullptr);
        if (pn) LAUNCH(k_temporal_clamp_surface, cc, INPUTS, pp, pn);
        else LAUNCH(k_temporal_clamp, cc, INPUTS, pp);
    } else if (pn) {
        LAUNCH(k_temporal_surface, INPUTS, pp, pn);
    } else if (pp) {
        LAUNCH(k_temporal_motion, INPUTS, pp);
    } else {
        LAUNCH(k_temporal, INPUTS);
    }
#undef INPUTS
#undef LAUNCH
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

extern "C" {

int agpt_temporal_accumulate(agpt_ctx* c, const agpt_temporal_params* p, const float* accum_cur_dev, const float* moment2_cur_dev,
                             const float* albedo_cur_dev, const float* normal_depth_cur_dev, const float* hist_accum_prev_dev,
                             const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
                             float* hist_accum_out_dev, float* hist_moment2_out_dev) {
    return temporal_accumulate("agpt_temporal_accumulate", 0, c, p, nullptr,
                               {accum_cur_dev, moment2_cur_dev, albedo_cur_dev, normal_depth_cur_dev, hist_accum_prev_dev, hist_moment2_prev_dev,
                                albedo_prev_dev, normal_depth_prev_dev},
                               nullptr, nullptr, hist_accum_out_dev, hist_moment2_out_dev);
}

int agpt_temporal_accumulate_motion(agpt_ctx* c, const agpt_temporal_params* p, const float* accum_cur_dev, const float* moment2_cur_dev,
                                    const float* albedo_cur_dev, const float* normal_depth_cur_dev, const float* hist_accum_prev_dev,
                                    const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
                                    float* hist_accum_out_dev, float* hist_moment2_out_dev, const float* prev_point_cur_dev) {
    return temporal_accumulate("agpt_temporal_accumulate_motion", NEED_POINT, c, p, nullptr,
                               {accum_cur_dev, moment2_cur_dev, albedo_cur_dev, normal_depth_cur_dev, hist_accum_prev_dev, hist_moment2_prev_dev,
                                albedo_prev_dev, normal_depth_prev_dev},
                               prev_point_cur_dev, nullptr, hist_accum_out_dev, hist_moment2_out_dev);
}

int agpt_temporal_accumulate_clamped(agpt_ctx* c, const agpt_temporal_params* p, const agpt_temporal_clamp_params* cp,
                                     const float* accum_cur_dev, const float* moment2_cur_dev, const float* albedo_cur_dev,
                                     const float* normal_depth_cur_dev, const float* hist_accum_prev_dev, const float* hist_moment2_prev_dev,
                                     const float* albedo_prev_dev, const float* normal_depth_prev_dev, float* hist_accum_out_dev,
                                     float* hist_moment2_out_dev, const float* prev_point_cur_dev) {
    return temporal_accumulate("agpt_temporal_accumulate_clamped", NEED_CLAMP, c, p, cp,
                               {accum_cur_dev, moment2_cur_dev, albedo_cur_dev, normal_depth_cur_dev, hist_accum_prev_dev, hist_moment2_prev_dev,
                                albedo_prev_dev, normal_depth_prev_dev},
                               prev_point_cur_dev, nullptr, hist_accum_out_dev, hist_moment2_out_dev);
}

int agpt_temporal_accumulate_surface_motion(agpt_ctx* c, const agpt_temporal_params* p, const agpt_temporal_clamp_params* cp,
                                            const float* accum_cur_dev, const float* moment2_cur_dev, const float* albedo_cur_dev,
                                            const float* normal_depth_cur_dev, const float* hist_accum_prev_dev,
                                            const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
                                            float* hist_accum_out_dev, float* hist_moment2_out_dev, const float* prev_point_cur_dev,
                                            const float* prev_normal_cur_dev) {
    return temporal_accumulate("agpt_temporal_accumulate_surface_motion", NEED_POINT | NEED_NORMAL, c, p, cp,
                               {accum_cur_dev, moment2_cur_dev, albedo_cur_dev, normal_depth_cur_dev, hist_accum_prev_dev, hist_moment2_prev_dev,
                                albedo_prev_dev, normal_depth_prev_dev},
                               prev_point_cur_dev, prev_normal_cur_dev, hist_accum_out_dev, hist_moment2_out_dev);
}

}  // extern "C"
