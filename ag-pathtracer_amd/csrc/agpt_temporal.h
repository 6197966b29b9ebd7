// agpt_temporal.h -- the constants, the argument record and the body of the five temporal kernels (agpt_temporal.hip, the only unit that
// includes this file).  temporal_block is every kernel's: one film pixel of agpt_temporal_accumulate's contract (include/agpt.h) a thread,
// with temporal_gather for steps 3 and 4 and, at compile time, either step 5 (temporal_blend) or the clamp kernels' LDS tile of the
// current frame and step 5' -- so the variants agree wherever their extra inputs decide nothing.
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

#define AGPT_TC_RADIUS_MAX 3
#define AGPT_TC_ALBEDO_FLOOR 1e-3f   // agpt_denoise's demodulation floor
// a block's tile of k_denoise_pass' tiling plus a halo of the largest radius, one float4 per pixel: 70 x 10 x 16 B = 11200 B
#define AGPT_TC_TILE_W (AGPT_DN_TX + 2 * AGPT_TC_RADIUS_MAX)
#define AGPT_TC_TILE_H (AGPT_DN_TY + 2 * AGPT_TC_RADIUS_MAX)
#define AGPT_TC_LDS_BYTES (AGPT_TC_TILE_W * AGPT_TC_TILE_H * 16)

// the clamp's parameters as k_temporal_clamp and k_temporal_clamp_surface take them
struct TemporalClampConsts {
    int32_t radius;
    int32_t demodulate;
    int32_t motion;        // 1: prev_point_cur is given (agpt_temporal_accumulate_motion's step 3), 0: it is NULL
    float gamma, clamped_max_history;
};

// The twelve buffers of a temporal call.  Each kernel builds one from its own __restrict__ parameters (which is where the compiler
// learns that they do not alias) with nullptr for what it does not take; the host builds one from the entry point's arguments.
struct TemporalIO {
    const float4* accum_cur;
    const float* moment2_cur;
    const float4* albedo_cur;
    const float4* normal_depth_cur;
    const float4* hist_accum_prev;     // the four prev buffers: all NULL on the first frame
    const float* hist_moment2_prev;
    const float4* albedo_prev;
    const float4* normal_depth_prev;
    const float4* prev_point_cur;      // (p.xyz, w) of agpt_render_features_motion, or NULL
    const float4* prev_normal_cur;     // agpt_render_features_surface_motion's, or NULL
    float4* hist_accum_out;
    float* hist_moment2_out;
};

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
template <bool SURFACE>
__device__ __forceinline__ bool temporal_gather(const TemporalConsts& tc, const TemporalIO& io, int x, int y, size_t i, bool moved, v3 m,
                                                TemporalSums& ts) {
    const float flag = io.albedo_cur[i].w;
    const float4 g = io.normal_depth_cur[i];
    const bool geometry = flag != 0.f;
    v3 nref = V3(g.x, g.y, g.z);
    if constexpr (SURFACE) {
        if (moved) {
            const float4 pn = io.prev_normal_cur[i];
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
        const float flag_q = io.albedo_prev[q].w;
        const float4 hq = io.hist_accum_prev[q];
        const float n_q = hq.w;
        if (!(n_q > 0.f) || flag_q != flag) continue;
        if (geometry) {
            const float4 gq = io.normal_depth_prev[q];
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
        sm += b * (io.hist_moment2_prev[q] / n_q);
    }
    ts.sb = sb; ts.sn = sn; ts.sr = sr; ts.sg = sg; ts.sbl = sbl; ts.sm = sm;
    return sb >= AGPT_TEMPORAL_MIN_WEIGHT;
}

// Step 5 for a pixel that has history: its sums ts added to out / m_out
__device__ __forceinline__ void temporal_blend(const TemporalConsts& tc, const TemporalSums& ts, float4& out, float& m_out) {
    const float n_h = fminf(ts.sn / ts.sb, tc.max_history);
    out.x = out.x + (ts.sr / ts.sb) * n_h;
    out.y = out.y + (ts.sg / ts.sb) * n_h;
    out.z = out.z + (ts.sbl / ts.sb) * n_h;
    out.w = out.w + n_h;
    m_out = m_out + (ts.sm / ts.sb) * n_h;
}

// The body of all five kernels: a block of k_denoise_pass' tiling (64 x 4 pixels), one film pixel of the contract -- steps 1 to 6 -- by
// each thread alone.
// motion: prev_point_cur[i] = (p.xyz, w) of agpt_render_features_motion is given; w == 1 makes p the point that is reprojected, any
// other w leaves step 3 as it is without it.  Read only when there is history to fetch.  A constant in k_temporal (false),
// k_temporal_motion and k_temporal_surface (true); the clamp kernels' run-time cc.motion, so that one kernel serves
// agpt_temporal_accumulate_clamped with and without the buffer.
// SURFACE: temporal_gather's, with prev_normal_cur.
// CLAMP: step 5' in place of step 5, with cc and tile, the block's AGPT_TC_TILE_W * AGPT_TC_TILE_H float4 of LDS (both unused
// without it).  The block first stages, cooperatively, its tile plus a halo of r pixels: one float4 per pixel = (the demodulated mean
// x.rgb, the flag), w = NaN for a pixel that no window may use (outside the film, or without samples: a NaN compares unequal to every
// flag).  One barrier, reached by every thread of the block; then a pixel that has history walks its window from LDS in the contract's
// order -- dy = -r .. r outermost in FILM rows, which are the buffer's rows backwards.
// (The two CLAMP sections are written out here, not in functions of their own, and r is one constant read first: either change makes
// the compiler allocate the clamp kernels' registers differently, and their instruction streams are pinned.)
template <bool SURFACE, bool CLAMP>
__device__ __forceinline__ void temporal_block(const TemporalConsts& tc, const TemporalIO& io, bool motion,
                                               const TemporalClampConsts* cc = nullptr, float4* tile = nullptr) {
    const int r = CLAMP ? cc->radius : 0;                                         // 1 .. AGPT_TC_RADIUS_MAX (checked by the entry point)
    const int tx = (int)(threadIdx.x & (AGPT_DN_TX - 1)), ty = (int)(threadIdx.x / AGPT_DN_TX);
    if constexpr (CLAMP) {
        if (io.hist_accum_prev) {                                                 // (the first frame reads the current pixel only)
            const int tw = AGPT_DN_TX + 2 * r, th = AGPT_DN_TY + 2 * r;          // <= AGPT_TC_TILE_W, AGPT_TC_TILE_H
            const int bx = (int)(blockIdx.x * AGPT_DN_TX) - r, brow = (int)(blockIdx.y * AGPT_DN_TY) - r;
            for (int t = (int)threadIdx.x; t < tw * th; t += AGPT_BLOCK) {
                const int ly = t / tw, lx = t - ly * tw;
                const int qx = bx + lx, qrow = brow + ly;
                float4 v;
                v.x = 0.f; v.y = 0.f; v.z = 0.f; v.w = __uint_as_float(0x7FC00000u);
                if (qx >= 0 && qx < tc.W && qrow >= 0 && qrow < tc.H) {
                    const size_t q = (size_t)qrow * (size_t)tc.W + (size_t)qx;
                    const float4 a = io.accum_cur[q];
                    if (a.w > 0.f) {
                        const float4 al = io.albedo_cur[q];
                        v.x = a.x / a.w; v.y = a.y / a.w; v.z = a.z / a.w;
                        if (cc->demodulate) {
                            v.x = v.x / fmaxf(al.x, AGPT_TC_ALBEDO_FLOOR);
                            v.y = v.y / fmaxf(al.y, AGPT_TC_ALBEDO_FLOOR);
                            v.z = v.z / fmaxf(al.z, AGPT_TC_ALBEDO_FLOOR);
                        }
                        v.w = al.w;
                    }
                }
                tile[ly * AGPT_TC_TILE_W + lx] = v;
            }
        }
        __syncthreads();
    }
    const int x = (int)(blockIdx.x * AGPT_DN_TX) + tx;
    const int row = (int)(blockIdx.y * AGPT_DN_TY) + ty;                          // buffer row: film row H - 1 - row
    if (x >= tc.W || row >= tc.H) return;
    const int y = tc.H - 1 - row;
    const size_t i = (size_t)row * (size_t)tc.W + (size_t)x;
    float4 out = io.accum_cur[i];
    float m_out = io.moment2_cur[i];
    if (io.hist_accum_prev) {
        bool moved = false;                                                       // (stays false without motion)
        v3 m = V3s(0.f);
        if (motion) {
            const float4 m4 = io.prev_point_cur[i];
            moved = m4.w == 1.f;
            m = V3(m4.x, m4.y, m4.z);
        }
        TemporalSums ts;
        if (temporal_gather<SURFACE>(tc, io, x, y, i, moved, m, ts)) {
            if constexpr (CLAMP) {
                const float4 al = io.albedo_cur[i];
                // the statistics of the current frame around the pixel
                float k = 0.f;
                v3 s1 = V3s(0.f), s2 = V3s(0.f);
                for (int dy = -r; dy <= r; ++dy) {
                    const float4* line = tile + ((ty + r) - dy) * AGPT_TC_TILE_W + tx;   // film row y + dy is buffer row `row - dy`
                    for (int dx = 0; dx <= 2 * r; ++dx) {
                        const float4 q = line[dx];
                        if (q.w == al.w) {
                            k += 1.f;
                            s1.x += q.x; s1.y += q.y; s1.z += q.z;
                            s2.x += q.x * q.x; s2.y += q.y * q.y; s2.z += q.z * q.z;
                        }
                    }
                }
                // step 5'
                const float n_raw = fminf(ts.sn / ts.sb, tc.max_history);
                float c_h[3] = {ts.sr / ts.sb, ts.sg / ts.sb, ts.sbl / ts.sb};
                float m_h = ts.sm / ts.sb;
                float n_h = n_raw;
                if (k > 0.f) {
                    const float s1v[3] = {s1.x, s1.y, s1.z}, s2v[3] = {s2.x, s2.y, s2.z};
                    const float av[3] = {fmaxf(al.x, AGPT_TC_ALBEDO_FLOOR), fmaxf(al.y, AGPT_TC_ALBEDO_FLOOR), fmaxf(al.z, AGPT_TC_ALBEDO_FLOOR)};
                    const float y_old = luminance(V3(c_h[0], c_h[1], c_h[2]));
                    bool clamped = false;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float mu = s1v[j] / k;
                        const float sd = sqrtf(fmaxf(s2v[j] / k - mu * mu, 0.f));
                        const float lo = mu - cc->gamma * sd, hi = mu + cc->gamma * sd;
                        const float d = cc->demodulate ? c_h[j] / av[j] : c_h[j];
                        const float e = fminf(fmaxf(d, lo), hi);
                        if (!(e == d)) {                                          // (an unclamped channel keeps its bits)
                            clamped = true;
                            c_h[j] = cc->demodulate ? e * av[j] : e;
                        }
                    }
                    if (clamped) {
                        const float y_new = luminance(V3(c_h[0], c_h[1], c_h[2]));
                        m_h = fmaxf(m_h - y_old * y_old, 0.f) + y_new * y_new;    // the history's variance, around the new mean
                        n_h = fminf(n_raw, cc->clamped_max_history);
                    }
                }
                out.x = out.x + c_h[0] * n_h;
                out.y = out.y + c_h[1] * n_h;
                out.z = out.z + c_h[2] * n_h;
                out.w = out.w + n_h;
                m_out = m_out + m_h * n_h;
            } else {
                temporal_blend(tc, ts, out, m_out);
            }
        }
    }
    io.hist_accum_out[i] = out;
    io.hist_moment2_out[i] = m_out;
}
