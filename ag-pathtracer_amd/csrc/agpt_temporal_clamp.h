// agpt_temporal_clamp.h -- the constants of k_temporal_clamp (agpt_temporal_clamp.hip, which also defines
// agpt_temporal_accumulate_clamped): the clamp's parameters as the kernel takes them and the LDS tile its blocks stage; and the kernel's
// body, which k_temporal_clamp_surface (agpt_surface_motion.hip) instantiates a second time.
#pragma once

#include "agpt_temporal.h"

#define AGPT_TC_RADIUS_MAX 3
#define AGPT_TC_ALBEDO_FLOOR 1e-3f   // agpt_denoise's demodulation floor
// a block's tile of k_denoise_pass' tiling plus a halo of the largest radius, one float4 per pixel: 70 x 10 x 16 B = 11200 B
#define AGPT_TC_TILE_W (AGPT_DN_TX + 2 * AGPT_TC_RADIUS_MAX)
#define AGPT_TC_TILE_H (AGPT_DN_TY + 2 * AGPT_TC_RADIUS_MAX)
#define AGPT_TC_LDS_BYTES (AGPT_TC_TILE_W * AGPT_TC_TILE_H * 16)

struct TemporalClampConsts {
    int32_t radius;
    int32_t demodulate;
    int32_t motion;        // 1: prev_point_cur is given (agpt_temporal_accumulate_motion's step 3), 0: it is NULL
    float gamma, clamped_max_history;
};

// The body of k_temporal_clamp (agpt_temporal_clamp.hip) and -- SURFACE: temporal_gather's flag (agpt_temporal.h), with prev_normal_cur -- of
// k_temporal_clamp_surface (agpt_surface_motion.hip); tile: the block's AGPT_TC_TILE_W * AGPT_TC_TILE_H float4 of LDS.
template <bool SURFACE>
__device__ __forceinline__ void temporal_clamp_block(const TemporalConsts& tc, const TemporalClampConsts& cc, float4* tile,
                                                     const float4* __restrict__ accum_cur, const float* __restrict__ moment2_cur,
                                                     const float4* __restrict__ albedo_cur, const float4* __restrict__ normal_depth_cur,
                                                     const float4* __restrict__ hist_accum_prev, const float* __restrict__ hist_moment2_prev,
                                                     const float4* __restrict__ albedo_prev, const float4* __restrict__ normal_depth_prev,
                                                     const float4* __restrict__ prev_point_cur, float4* __restrict__ hist_accum_out,
                                                     float* __restrict__ hist_moment2_out, const float4* __restrict__ prev_normal_cur) {
    const int r = cc.radius;                                                      // 1 .. AGPT_TC_RADIUS_MAX (checked by the entry point)
    const int tx = (int)(threadIdx.x & (AGPT_DN_TX - 1)), ty = (int)(threadIdx.x / AGPT_DN_TX);
    if (hist_accum_prev) {                                                        // (the first frame reads the current pixel only)
        const int tw = AGPT_DN_TX + 2 * r, th = AGPT_DN_TY + 2 * r;              // <= AGPT_TC_TILE_W, AGPT_TC_TILE_H
        const int bx = (int)(blockIdx.x * AGPT_DN_TX) - r, brow = (int)(blockIdx.y * AGPT_DN_TY) - r;
        for (int t = (int)threadIdx.x; t < tw * th; t += AGPT_BLOCK) {
            const int ly = t / tw, lx = t - ly * tw;
            const int qx = bx + lx, qrow = brow + ly;
            float4 v;
            v.x = 0.f; v.y = 0.f; v.z = 0.f; v.w = __uint_as_float(0x7FC00000u);
            if (qx >= 0 && qx < tc.W && qrow >= 0 && qrow < tc.H) {
                const size_t q = (size_t)qrow * (size_t)tc.W + (size_t)qx;
                const float4 a = accum_cur[q];
                if (a.w > 0.f) {
                    const float4 al = albedo_cur[q];
                    v.x = a.x / a.w; v.y = a.y / a.w; v.z = a.z / a.w;
                    if (cc.demodulate) {
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

    const int x = (int)(blockIdx.x * AGPT_DN_TX) + tx;
    const int row = (int)(blockIdx.y * AGPT_DN_TY) + ty;                          // buffer row: film row H - 1 - row
    if (x >= tc.W || row >= tc.H) return;
    const int y = tc.H - 1 - row;
    const size_t i = (size_t)row * (size_t)tc.W + (size_t)x;
    float4 out = accum_cur[i];
    float m_out = moment2_cur[i];
    if (hist_accum_prev) {
        bool moved = false;
        v3 m = V3s(0.f);
        if (cc.motion) {
            const float4 m4 = prev_point_cur[i];
            moved = m4.w == 1.f;
            m = V3(m4.x, m4.y, m4.z);
        }
        TemporalSums ts;
        if (temporal_gather<SURFACE>(tc, x, y, i, moved, m, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev,
                                     normal_depth_prev, ts, prev_normal_cur)) {
            // the statistics of the current frame around the pixel
            const float4 al = albedo_cur[i];
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
                    const float lo = mu - cc.gamma * sd, hi = mu + cc.gamma * sd;
                    const float d = cc.demodulate ? c_h[j] / av[j] : c_h[j];
                    const float e = fminf(fmaxf(d, lo), hi);
                    if (!(e == d)) {                                              // (an unclamped channel keeps its bits)
                        clamped = true;
                        c_h[j] = cc.demodulate ? e * av[j] : e;
                    }
                }
                if (clamped) {
                    const float y_new = luminance(V3(c_h[0], c_h[1], c_h[2]));
                    m_h = fmaxf(m_h - y_old * y_old, 0.f) + y_new * y_new;        // the history's variance, around the new mean
                    n_h = fminf(n_raw, cc.clamped_max_history);
                }
            }
            out.x = out.x + c_h[0] * n_h;
            out.y = out.y + c_h[1] * n_h;
            out.z = out.z + c_h[2] * n_h;
            out.w = out.w + n_h;
            m_out = m_out + m_h * n_h;
        }
    }
    hist_accum_out[i] = out;
    hist_moment2_out[i] = m_out;
}


struct agpt_ctx;
namespace agpt {
// (agpt_temporal_clamp.hip) agpt_temporal_accumulate_clamped's checks of its clamp parameters in the header's order under the name `fn`, and
// the kernel's constants from them
int check_clamp(const char* fn, const agpt_temporal_clamp_params* cp);
TemporalClampConsts clamp_consts(const agpt_temporal_clamp_params* cp, bool motion);
}  // namespace agpt
