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

#define AGPT_TP_DEPTH_FLOOR 1e-3f

__global__ void __launch_bounds__(AGPT_BLOCK)
k_temporal(TemporalConsts tc, const float4* __restrict__ accum_cur, const float* __restrict__ moment2_cur,
           const float4* __restrict__ albedo_cur, const float4* __restrict__ normal_depth_cur, const float4* __restrict__ hist_accum_prev,
           const float* __restrict__ hist_moment2_prev, const float4* __restrict__ albedo_prev, const float4* __restrict__ normal_depth_prev,
           float4* __restrict__ hist_accum_out, float* __restrict__ hist_moment2_out) {
    const int x = (int)(blockIdx.x * AGPT_DN_TX + (threadIdx.x & (AGPT_DN_TX - 1)));
    const int row = (int)(blockIdx.y * AGPT_DN_TY + threadIdx.x / AGPT_DN_TX);   // buffer row: film row H - 1 - row
    if (x >= tc.W || row >= tc.H) return;
    const int y = tc.H - 1 - row;
    const size_t i = (size_t)row * (size_t)tc.W + (size_t)x;
    float4 out = accum_cur[i];
    float m_out = moment2_cur[i];
    if (hist_accum_prev) {
        const float flag = albedo_cur[i].w;
        const float4 g = normal_depth_cur[i];
        const bool geometry = flag != 0.f;
        // the position on the previous film
        bool found = true;
        int x0 = x, y0 = y;
        float fx = 0.f, fy = 0.f, te = g.w;
        if (!tc.identity) {
            v3 O, D;
            feature_ray(tc.cur, x, y, tc.W, tc.H, O, D);
            const DevCamera& P = tc.prev;
            const v3 Q = geometry ? (tc.cur.origin + g.w * D) - P.origin : D;   // a miss: the point at infinity along D
            te = length(Q);
            const v3 L = P.lower_left_corner - P.origin;
            const float dw = dot(Q, P.w);
            found = dw < 0.f;                                                     // in front of the previous camera
            const float k = dot(L, P.w) / dw;
            const v3 R = Q * k - L;
            const float s = dot(R, P.horizontal) / dot(P.horizontal, P.horizontal);
            const float t = dot(R, P.vertical) / dot(P.vertical, P.vertical);
            const float sx = s * tc.W - .5f, sy = t * tc.H - .5f;
            found = found && sx > -1.f && sx < tc.W && sy > -1.f && sy < tc.H;    // (false for NaN)
            const float flx = floorf(sx), fly = floorf(sy);
            x0 = found ? (int)flx : 0;
            y0 = found ? (int)fly : 0;
            fx = sx - flx;
            fy = sy - fly;
        }
        if (found) {
            const float b4[4] = {(1.f - fx) * (1.f - fy), fx * (1.f - fy), (1.f - fx) * fy, fx * fy};
            const float zmax = tc.depth_tol * fmaxf(te, AGPT_TP_DEPTH_FLOOR);
            float sb = 0.f, sn = 0.f, sr = 0.f, sg = 0.f, sbl = 0.f, sm = 0.f;
#pragma unroll
            for (int tap = 0; tap < 4; ++tap) {
                const int qx = x0 + (tap & 1), qy = y0 + (tap >> 1);
                const float b = b4[tap];
                if (qx < 0 || qx >= tc.W || qy < 0 || qy >= tc.H || !(b > 0.f)) continue;
                const size_t q = (size_t)(tc.H - 1 - qy) * (size_t)tc.W + (size_t)qx;
                // a rejected tap costs its flag and its history record (the count) only
                const float flag_q = albedo_prev[q].w;
                const float4 hq = hist_accum_prev[q];
                const float n_q = hq.w;
                if (!(n_q > 0.f) || flag_q != flag) continue;
                if (geometry) {
                    const float4 gq = normal_depth_prev[q];
                    // (one test on the whole record: the compiler would split a short-circuit into a 4-byte and a 12-byte load)
                    const bool near = fabsf(te - gq.w) <= zmax;
                    const bool facing = dot(V3(g.x, g.y, g.z), V3(gq.x, gq.y, gq.z)) >= tc.normal_cos;
                    if (!(near & facing)) continue;
                }
                sb += b;
                sn += b * n_q;
                sr += b * (hq.x / n_q);
                sg += b * (hq.y / n_q);
                sbl += b * (hq.z / n_q);
                sm += b * (hist_moment2_prev[q] / n_q);
            }
            if (sb >= AGPT_TEMPORAL_MIN_WEIGHT) {
                const float n_h = fminf(sn / sb, tc.max_history);
                out.x = out.x + (sr / sb) * n_h;
                out.y = out.y + (sg / sb) * n_h;
                out.z = out.z + (sbl / sb) * n_h;
                out.w = out.w + n_h;
                m_out = m_out + (sm / sb) * n_h;
            }
        }
    }
    hist_accum_out[i] = out;
    hist_moment2_out[i] = m_out;
}

extern "C" {

// One k_temporal launch: this frame's buffers plus the previous frame's history, reprojected, into the history buffers the next
// agpt_denoise and the next frame's call read.
int agpt_temporal_accumulate(agpt_ctx* c, const agpt_temporal_params* p, const float* accum_cur_dev, const float* moment2_cur_dev,
                             const float* albedo_cur_dev, const float* normal_depth_cur_dev, const float* hist_accum_prev_dev,
                             const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
                             float* hist_accum_out_dev, float* hist_moment2_out_dev) {
    if (!p) return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: NULL argument");
    if (p->width <= 0 || p->height <= 0 || (uint64_t)p->width * (uint64_t)p->height > 0x7FFFFFFFull)
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: bad film size");
    if (!(p->max_history > 0.f) || std::isinf(p->max_history))
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: max_history must be positive and finite");
    if (!(p->depth_tol >= 0.f) || std::isinf(p->depth_tol))
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: depth_tol must be non-negative and finite");
    if (!(p->normal_cos >= -1.f && p->normal_cos <= 1.f))
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: normal_cos must be in [-1, 1]");
    if (!c || !accum_cur_dev || !moment2_cur_dev || !albedo_cur_dev || !normal_depth_cur_dev || !hist_accum_out_dev || !hist_moment2_out_dev)
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: NULL argument");
    const float* prev[4] = {hist_accum_prev_dev, hist_moment2_prev_dev, albedo_prev_dev, normal_depth_prev_dev};
    const int n_prev = (prev[0] != nullptr) + (prev[1] != nullptr) + (prev[2] != nullptr) + (prev[3] != nullptr);
    if (n_prev != 0 && n_prev != 4)
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: the four prev buffers must be all NULL (first frame) or all given");
    const float* in[8] = {accum_cur_dev, moment2_cur_dev, albedo_cur_dev, normal_depth_cur_dev, prev[0], prev[1], prev[2], prev[3]};
    for (const float* q : in)
        if (q && (q == hist_accum_out_dev || q == hist_moment2_out_dev))
            return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: an output aliases an input");
    if (hist_accum_out_dev == hist_moment2_out_dev) return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: the two outputs are one buffer");
    HIP_TRY(hipSetDevice(c->device));
    TemporalConsts tc{};
    tc.W = p->width; tc.H = p->height;
    tc.identity = std::memcmp(&p->cam_prev, &p->cam_cur, sizeof(agpt_camera_desc)) == 0;
    tc.max_history = p->max_history; tc.depth_tol = p->depth_tol; tc.normal_cos = p->normal_cos;
    tc.cur = agpt::make_camera(p->cam_cur);
    tc.prev = agpt::make_camera(p->cam_prev);
    // one thread per film pixel in k_denoise_pass' tiling
    static_assert(AGPT_DN_TX * AGPT_DN_TY == AGPT_BLOCK, "one thread per tile pixel");
    const dim3 tiles((unsigned)((tc.W + AGPT_DN_TX - 1) / AGPT_DN_TX), (unsigned)((tc.H + AGPT_DN_TY - 1) / AGPT_DN_TY));
    hipLaunchKernelGGL(k_temporal, tiles, dim3(AGPT_BLOCK), 0, c->stream, tc, (const float4*)accum_cur_dev, moment2_cur_dev,
                       (const float4*)albedo_cur_dev, (const float4*)normal_depth_cur_dev, (const float4*)hist_accum_prev_dev,
                       hist_moment2_prev_dev, (const float4*)albedo_prev_dev, (const float4*)normal_depth_prev_dev,
                       (float4*)hist_accum_out_dev, hist_moment2_out_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

}  // extern "C"
