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
        if (temporal_gather(tc, x, y, i, moved, m, albedo_cur, normal_depth_cur, hist_accum_prev, hist_moment2_prev, albedo_prev,
                            normal_depth_prev, ts)) {
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
    if (!cp) return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate_clamped: NULL clamp params");
    if (cp->radius < 1 || cp->radius > AGPT_TC_RADIUS_MAX) return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate_clamped: radius must be 1..3");
    if (cp->demodulate != 0 && cp->demodulate != 1) return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate_clamped: demodulate must be 0 or 1");
    if (!(cp->gamma >= 0.f)) return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate_clamped: gamma must be non-negative");
    if (!(cp->clamped_max_history > 0.f) || std::isinf(cp->clamped_max_history))
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate_clamped: clamped_max_history must be positive and finite");
    if (prev_point_cur_dev && (prev_point_cur_dev == hist_accum_out_dev || prev_point_cur_dev == hist_moment2_out_dev))
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate_clamped: an output aliases prev_point_cur_dev");
    TemporalClampConsts cc;
    cc.radius = cp->radius;
    cc.demodulate = cp->demodulate;
    cc.motion = prev_point_cur_dev != nullptr;
    cc.gamma = cp->gamma;
    cc.clamped_max_history = cp->clamped_max_history;
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
