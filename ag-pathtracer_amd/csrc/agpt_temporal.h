// agpt_temporal.h -- the constants and the per-pixel body of k_temporal (agpt_temporal.hip, which also defines agpt_temporal_accumulate)
// and of k_temporal_motion (agpt_motion.hip, agpt_temporal_accumulate_motion): one body, so the two agree wherever nothing moved.
// Its first half, temporal_gather (steps 3 and 4), is also k_temporal_clamp's (agpt_temporal_clamp.hip), whose step 5 differs.
#pragma once

#include "../../include/agpt.h"
#include "agpt_denoise.h"

struct TemporalConsts {
    int32_t W, H;
    int32_t identity;      // 1: the two camera descriptions are the same bytes -- every pixel reads its own history, no arithmetic
    float max_history, depth_tol, normal_cos;
    DevCamera cur, prev;   // make_camera of the two descriptions
};

#define AGPT_TP_DEPTH_FLOOR 1e-3f

// What steps 3 and 4 of agpt_temporal_accumulate's contract leave for a pixel that has history: the sums over the accepted taps
struct TemporalSums {
    float sb, sn, sr, sg, sbl, sm;
};

// Steps 3 and 4 for film pixel (x, y), buffer index i, by the calling thread alone -> whether the pixel has history (step 5's
// sb >= AGPT_TEMPORAL_MIN_WEIGHT), and then its sums.  moved: reproject the point m (agpt_temporal_accumulate_motion's w == 1:
// Q = m - P.origin, with the arithmetic even when the cameras are the same bytes) instead of the point the pixel sees now.
// SURFACE (agpt_temporal_accumulate_surface_motion): for a moved pixel the normal that step 4 compares with each tap's is
// prev_normal_cur[i].xyz -- the one that surface point had a frame ago (agpt_render_features_surface_motion) -- read for moved pixels only;
// every other pixel, and every caller without SURFACE, compares the current one.
template <bool SURFACE = false>
__device__ __forceinline__ bool temporal_gather(const TemporalConsts& tc, int x, int y, size_t i, bool moved, v3 m,
                                                const float4* __restrict__ albedo_cur, const float4* __restrict__ normal_depth_cur,
                                                const float4* __restrict__ hist_accum_prev, const float* __restrict__ hist_moment2_prev,
                                                const float4* __restrict__ albedo_prev, const float4* __restrict__ normal_depth_prev,
                                                TemporalSums& ts, const float4* __restrict__ prev_normal_cur = nullptr) {
    const float flag = albedo_cur[i].w;
    const float4 g = normal_depth_cur[i];
    const bool geometry = flag != 0.f;
    v3 nref = V3(g.x, g.y, g.z);
    if constexpr (SURFACE) {
        if (moved) {
            const float4 pn = prev_normal_cur[i];
            nref = V3(pn.x, pn.y, pn.z);
        }
    }
    // the position on the previous film
    bool found = true;
    int x0 = x, y0 = y;
    float fx = 0.f, fy = 0.f, te = g.w;
    if (!tc.identity || moved) {
        const DevCamera& P = tc.prev;
        v3 Q;
        if (moved) {
            Q = m - P.origin;                                                     // where this surface point was
        } else {
            v3 O, D;
            feature_ray(tc.cur, x, y, tc.W, tc.H, O, D);
            Q = geometry ? (tc.cur.origin + g.w * D) - P.origin : D;          // a miss: the point at infinity along D
        }
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
    if (!found) return false;
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
            const bool facing = dot(nref, V3(gq.x, gq.y, gq.z)) >= tc.normal_cos;
            if (!(near & facing)) continue;
        }
        sb += b;
        sn += b * n_q;
        sr += b * (hq.x / n_q);
        sg += b * (hq.y / n_q);
        sbl += b * (hq.z / n_q);
        sm += b * (hist_moment2_prev[q] / n_q);
    }
    ts.sb = sb; ts.sn = sn; ts.sr = sr; ts.sg = sg; ts.sbl = sbl; ts.sm = sm;
    return sb >= AGPT_TEMPORAL_MIN_WEIGHT;
}

// One film pixel of agpt_temporal_accumulate's contract (include/agpt.h), steps 1-6, by the calling thread alone.
// MOTION (agpt_temporal_accumulate_motion): prev_point_cur[i] = (p.xyz, w) of agpt_render_features_motion; w == 1 makes p the point
// that is reprojected, any other w leaves step 3 as it is without MOTION.  Read only when there is history to fetch.
// SURFACE: temporal_gather's, with prev_normal_cur.
template <bool MOTION, bool SURFACE = false>
__device__ __forceinline__ void temporal_pixel(const TemporalConsts& tc, const float4* __restrict__ accum_cur, const float* __restrict__ moment2_cur,
                                               const float4* __restrict__ albedo_cur, const float4* __restrict__ normal_depth_cur,
                                               const float4* __restrict__ hist_accum_prev, const float* __restrict__ hist_moment2_prev,
                                               const float4* __restrict__ albedo_prev, const float4* __restrict__ normal_depth_prev,
                                               const float4* __restrict__ prev_point_cur, float4* __restrict__ hist_accum_out,
                                               float* __restrict__ hist_moment2_out, const float4* __restrict__ prev_normal_cur = nullptr) {
    const int x = (int)(blockIdx.x * AGPT_DN_TX + (threadIdx.x & (AGPT_DN_TX - 1)));
    const int row = (int)(blockIdx.y * AGPT_DN_TY + threadIdx.x / AGPT_DN_TX);   // buffer row: film row H - 1 - row
    if (x >= tc.W || row >= tc.H) return;
    const int y = tc.H - 1 - row;
    const size_t i = (size_t)row * (size_t)tc.W + (size_t)x;
    float4 out = accum_cur[i];
    float m_out = moment2_cur[i];
    if (hist_accum_prev) {
        bool moved = false;                                                       // (stays false without MOTION)
        v3 m = V3s(0.f);
        if constexpr (MOTION) {
            const float4 m4 = prev_point_cur[i];
            moved = m4.w == 1.f;
            m = V3(m4.x, m4.y, m4.z);
        }
        TemporalSums ts;
        if (temporal_gather<SURFACE>(tc, x, y, i, moved, m, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev,
                                     normal_depth_prev, ts, prev_normal_cur)) {
            const float n_h = fminf(ts.sn / ts.sb, tc.max_history);
            out.x = out.x + (ts.sr / ts.sb) * n_h;
            out.y = out.y + (ts.sg / ts.sb) * n_h;
            out.z = out.z + (ts.sbl / ts.sb) * n_h;
            out.w = out.w + n_h;
            m_out = m_out + (ts.sm / ts.sb) * n_h;
        }
    }
    hist_accum_out[i] = out;
    hist_moment2_out[i] = m_out;
}
