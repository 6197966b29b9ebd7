// agpt_denoise.hip -- the kernels of agpt_render_features and agpt_denoise (include/agpt.h).
//
// Features: k_feature_rays writes one camera ray per tile pixel through the pixel centre (Camera::GetRay with a zero lens offset, no
// RNG), the library's closest-hit trace launch follows (agpt_api.hip, the path of agpt_intersect_device), and k_features turns each
// hit record into (material colour, flag) and (shading normal, t) with the surface reconstruction k_shade uses (agpt_shade.h;
// spheres: (p - c) / r, see k_features).  agpt_render_features_surface_motion runs the PREV siblings of the four feature kernels, which
// also write the shading normal a moved triangle's hit had a frame ago (features_pixel's PREV flag).
//
// Denoiser: k_denoise_prepare turns the adaptive buffers into the per-pixel state (mean radiance -- demodulated by the albedo on
// request --, variance of the mean luminance), k_denoise_pass is one a-trous pass of 25 taps at a given spacing.  Every pixel is
// computed by one thread from the previous pass' buffer in a fixed tap order: no atomics, no cross-lane sums, so tests/denoise_model.py
// reproduces it operation by operation.  Compiled with the library's common flags (-ffp-contract=off, IEEE divide / sqrt).
#include <hip/hip_runtime.h>

#include <cmath>

#include "agpt_denoise.h"
#include "agpt_internal.h"
#include "agpt_shade.h"

using agpt::fail;

#define AGPT_DN_ALBEDO_FLOOR 1e-3f
#define AGPT_DN_DEPTH_FLOOR 1e-3f
#define AGPT_DN_LUM_EPS 1e-6f

namespace {

// exp of an fp32 argument as the correctly rounded fp32 value, through fp64 (the convention of cr_acosf / cr_atan2f, agpt_math.h)
__device__ __forceinline__ float cr_expf(float x) { return (float)exp((double)x); }

__device__ __forceinline__ v3 albedo_floor(float4 a) {
    return V3(fmaxf(a.x, AGPT_DN_ALBEDO_FLOOR), fmaxf(a.y, AGPT_DN_ALBEDO_FLOOR), fmaxf(a.z, AGPT_DN_ALBEDO_FLOOR));
}

}  // namespace

// one feature_ray (agpt_denoise.h) per tile pixel
__global__ void __launch_bounds__(AGPT_BLOCK)
k_feature_rays(DevCamera c, RenderConsts rc, float4* __restrict__ ray_o, float4* __restrict__ ray_d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rc.NP) return;
    int x, y;
    size_t unused_index;
    pixel_of(rc, i, x, y, unused_index);
    v3 O, D;
    feature_ray(c, x, y, rc.W, rc.H, O, D);
    float4 o4, d4;
    o4.x = O.x; o4.y = O.y; o4.z = O.z; o4.w = AGPT_FLT_MAX;
    d4.x = D.x; d4.y = D.y; d4.z = D.z; d4.w = 0.f;
    ray_o[i] = o4;
    ray_d[i] = d4;
}

// albedo = (colour, flag): flag 1 a primitive with a material, 2 an emitter (null material), 0 a miss (colour 1 for both);
// normal_depth = (Surface::ns -- spheres: (p - c) / r --, t), zero on a miss
// TEXTURED (scenes with a textured material): on a mesh hit the colour of a textured material is the texel k_shade_textured shades
// that hit with (triangle_uv + texture_value, agpt_shade.h); SAMPLED (scenes in which a material names a texture with a non-default
// sampler): the filtered colour k_shade_sampled shades it with (texture_address / texture_load / texture_blend); NORMAL (scenes in which
// a material has a normal map): SAMPLED, and normal_depth.xyz is the shading normal k_shade_normal perturbs at that hit
// (surface_apply_normal_map, agpt_shade.h) -- the albedo stays the colour
// PREV (agpt_render_features_surface_motion): prev_normal = (n.xyz, prev_point.w), prev_point being what k_motion wrote for this launch's
// hits.  n = normal_depth.xyz, except on a moved triangle (w == 1): there the same reconstruction runs a second time on the triangle's
// record in tri_shade_old -- the older generation of agpt_scene_snapshot_surfaces -- at this hit's barycentrics, and at NORMAL the same
// texel and scale perturb it: the shading normal this surface point had a frame ago.  Zero on a miss.
template <bool TEXTURED, bool SAMPLED = false, bool NORMAL = false, bool PREV = false>
__device__ __forceinline__ void features_pixel(const DevScene& sc, const RenderConsts& rc, const float4* __restrict__ colors,
                                               const DevHit* __restrict__ hits, const float4* __restrict__ ray_o,
                                               const float4* __restrict__ ray_d, float4* __restrict__ albedo,
                                               float4* __restrict__ normal_depth, const float4* __restrict__ tri_shade_old = nullptr,
                                               const float4* __restrict__ prev_point = nullptr, float4* __restrict__ prev_normal = nullptr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rc.NP) return;
    int x, y;
    size_t ai;
    pixel_of(rc, i, x, y, ai);
    const DevHit h = hits[i];
    float4 a, nd;
    a.x = 1.f; a.y = 1.f; a.z = 1.f; a.w = 0.f;
    nd.x = 0.f; nd.y = 0.f; nd.z = 0.f; nd.w = 0.f;
    [[maybe_unused]] float4 pn;
    [[maybe_unused]] Surface s_old;
    [[maybe_unused]] bool followed = false;   // a moved triangle: s_old is its hit as the older record has it
    if constexpr (PREV) {
        pn.x = 0.f; pn.y = 0.f; pn.z = 0.f; pn.w = 0.f;
    }
    if (h.id != AGPT_HIT_MISS) {
        const float4 o4 = ray_o[i], d4 = ray_d[i];
        const v3 O = V3(o4.x, o4.y, o4.z), D = V3(d4.x, d4.y, d4.z);
        Surface s;
        if constexpr (PREV) pn.w = prev_point[ai].w;
        if (h.id & AGPT_HIT_SPHERE) {
            const int prim = (int)(h.id & 0x7FFFFFFFu);
            const DevPrim& P = sc.prims[prim];
            if (P.type == AGPT_PRIM_SPHERE) {
                // (p - c) / r, the value Sphere::Intersect's normalize(cross(dpdv, dpdu)) (surface_from_sphere) has for a p exactly
                // on the sphere.  That expression takes x and y from r sin(acos(z / r)) and z from sqrt(x^2 + y^2): near the poles
                // of the sphere's z axis it amplifies the distance of the fp32 hit point from the sphere by r^2 / (r^2 - z^2)
                // (measured: up to 1.8e-4 off (p - c) / r), which a path's shading tolerates and a guide buffer need not carry.
                s.prim = prim;
                s.ns = (O + h.t * D - V3(P.cx, P.cy, P.cz)) / P.r;
            } else {
                surface_from_sphere(sc, prim, O, D, h.t, s);   // (a plane: ns = +y)
            }
        } else {
            surface_from_triangle(sc, h.id, h.b1, h.b2, O, D, h.t, s);
            if constexpr (PREV) {
                if (pn.w == 1.f) {   // (k_motion sets it for ids below the snapshots' triangle count only)
                    DevScene was = sc;
                    was.tri_shade = tri_shade_old;
                    surface_from_triangle(was, h.id, h.b1, h.b2, O, D, h.t, s_old);
                    followed = true;
                }
            }
        }
        const int mat = sc.prims[s.prim].material;
        a.w = 2.f;
        if (mat >= 0) {
            a = colors[mat];
            if constexpr (TEXTURED) {
                const int tex = sc.material_texture[mat];
                if (tex >= 0 && !(h.id & AGPT_HIT_SPHERE)) {
                    float tu, tv;
                    triangle_uv(sc.tri_uv[2 * (size_t)h.id], sc.tri_uv[2 * (size_t)h.id + 1], h.b1, h.b2, &tu, &tv);
                    v3 c;
                    if constexpr (NORMAL) {   // (a material with a normal map always has a colour texture, agpt_scene_commit)
                        // both records, both addresses, all the taps, then the blends -- one round trip, as in k_shade_normal; a normal map
                        // that is the colour image reuses its blend
                        const DevNormalSlot slot = normal_slot(sc.material_texture, sc.n_materials, mat);
                        const DevTexture ct = sc.textures[tex];
                        const bool n_own = slot.texture >= 0 && slot.texture != tex;
                        TextureAddress ta, na;
                        TextureTaps k, nk;
                        texture_address(ct, tu, tv, ta);
                        texture_address(n_own ? slot.tex : ct, tu, tv, na);
                        texture_load(ta, k);
                        if (n_own) texture_load(na, nk);
                        c = texture_blend(ta, k);
                        if (slot.texture >= 0) {
                            const v3 texel = n_own ? texture_blend(na, nk) : c;
                            surface_apply_normal_map(s, texel, slot.scale);
                            if constexpr (PREV) {
                                if (followed) surface_apply_normal_map(s_old, texel, slot.scale);
                            }
                        }
                    } else if constexpr (SAMPLED) {
                        TextureAddress ta;
                        TextureTaps k;
                        texture_address(sc.textures[tex], tu, tv, ta);
                        texture_load(ta, k);
                        c = texture_blend(ta, k);
                    } else {
                        c = texture_value(sc.textures[tex], tu, tv);
                    }
                    a.x = c.x; a.y = c.y; a.z = c.z;
                }
            }
            a.w = 1.f;
        }
        nd.x = s.ns.x; nd.y = s.ns.y; nd.z = s.ns.z; nd.w = h.t;
        if constexpr (PREV) {
            const v3 n = followed ? s_old.ns : s.ns;
            pn.x = n.x; pn.y = n.y; pn.z = n.z;
        }
    }
    albedo[ai] = a;
    normal_depth[ai] = nd;
    if constexpr (PREV) prev_normal[ai] = pn;
}
__global__ void __launch_bounds__(AGPT_BLOCK)
k_features(DevScene sc, RenderConsts rc, const float4* __restrict__ colors, const DevHit* __restrict__ hits, const float4* __restrict__ ray_o,
           const float4* __restrict__ ray_d, float4* __restrict__ albedo, float4* __restrict__ normal_depth) {
    features_pixel<false>(sc, rc, colors, hits, ray_o, ray_d, albedo, normal_depth);
}
__global__ void __launch_bounds__(AGPT_BLOCK)
k_features_textured(DevScene sc, RenderConsts rc, const float4* __restrict__ colors, const DevHit* __restrict__ hits,
                    const float4* __restrict__ ray_o, const float4* __restrict__ ray_d, float4* __restrict__ albedo,
                    float4* __restrict__ normal_depth) {
    features_pixel<true>(sc, rc, colors, hits, ray_o, ray_d, albedo, normal_depth);
}
__global__ void __launch_bounds__(AGPT_BLOCK)
k_features_sampled(DevScene sc, RenderConsts rc, const float4* __restrict__ colors, const DevHit* __restrict__ hits,
                   const float4* __restrict__ ray_o, const float4* __restrict__ ray_d, float4* __restrict__ albedo,
                   float4* __restrict__ normal_depth) {
    features_pixel<true, true>(sc, rc, colors, hits, ray_o, ray_d, albedo, normal_depth);
}

__global__ void __launch_bounds__(AGPT_BLOCK)
k_features_normal(DevScene sc, RenderConsts rc, const float4* __restrict__ colors, const DevHit* __restrict__ hits,
                  const float4* __restrict__ ray_o, const float4* __restrict__ ray_d, float4* __restrict__ albedo,
                  float4* __restrict__ normal_depth) {
    features_pixel<true, true, true>(sc, rc, colors, hits, ray_o, ray_d, albedo, normal_depth);
}

// the four siblings of agpt_render_features_surface_motion: the same bodies with PREV
#define AGPT_FEATURES_PREV_KERNEL(name, ...)                                                                                            \
    __global__ void __launch_bounds__(AGPT_BLOCK)                                                                                       \
    name(DevScene sc, RenderConsts rc, const float4* __restrict__ colors, const DevHit* __restrict__ hits, const float4* __restrict__ ray_o,   \
         const float4* __restrict__ ray_d, float4* __restrict__ albedo, float4* __restrict__ normal_depth,                              \
         const float4* __restrict__ tri_shade_old, const float4* __restrict__ prev_point, float4* __restrict__ prev_normal) {            \
        features_pixel<__VA_ARGS__, true>(sc, rc, colors, hits, ray_o, ray_d, albedo, normal_depth, tri_shade_old, prev_point, prev_normal); \
    }
AGPT_FEATURES_PREV_KERNEL(k_features_prev, false, false, false)
AGPT_FEATURES_PREV_KERNEL(k_features_textured_prev, true, false, false)
AGPT_FEATURES_PREV_KERNEL(k_features_sampled_prev, true, true, false)
AGPT_FEATURES_PREV_KERNEL(k_features_normal_prev, true, true, true)
#undef AGPT_FEATURES_PREV_KERNEL

// state = (c.rgb, v): c = accum.rgb / n, v = the variance of the mean luminance from agpt_render_adaptive's estimate
// (max(0, moment2 / n - mu * mu) * n / (n - 1) / n; 0 for n < 2); with demodulate both in units of the floored albedo.
// v = -1 marks a pixel without samples.
__global__ void __launch_bounds__(AGPT_BLOCK)
k_denoise_prepare(DenoiseConsts dc, const float4* __restrict__ accum, const float* __restrict__ moment2, const float4* __restrict__ albedo,
                  float4* __restrict__ state) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)dc.W * (uint32_t)dc.H) return;
    const float4 a = accum[i];
    const float n = a.w;
    float4 st;
    st.x = 0.f; st.y = 0.f; st.z = 0.f; st.w = -1.f;
    if (n > 0.f) {
        v3 c = V3(a.x / n, a.y / n, a.z / n);
        float v = 0.f;
        if (n >= 2.f) {
            const float mu = luminance(V3(a.x, a.y, a.z)) / n;
            const float var = fmaxf(0.f, moment2[i] / n - mu * mu) * n / (n - 1.f);
            v = var / n;
        }
        if (dc.demodulate) {
            const v3 al = albedo_floor(albedo[i]);
            c = V3(c.x / al.x, c.y / al.y, c.z / al.z);
            const float la = luminance(al);
            v = v / (la * la);
        }
        st.x = c.x; st.y = c.y; st.z = c.z; st.w = v;
    }
    state[i] = st;
}

// One a-trous pass: the 25 taps q = p + step * (dx, dy), dx, dy in -2..2, inside the film, dy outermost.  A tap with another flag or
// without samples is skipped; the others weigh h * exp(-(ez + en + el)) (include/agpt.h) and the sums run in tap order.
// A wave is 64 consecutive pixels of one row: every tap is one contiguous 1 KiB (state, normal_depth) or 256 B (flag) read, at every
// spacing, and a pass re-reads each line 25 times from L1 / L2.
__global__ void __launch_bounds__(AGPT_BLOCK)
k_denoise_pass(DenoiseConsts dc, const float4* __restrict__ state_in, const float4* __restrict__ albedo, const float4* __restrict__ normal_depth,
               float4* __restrict__ state_out) {
    const int x = (int)(blockIdx.x * AGPT_DN_TX + (threadIdx.x & (AGPT_DN_TX - 1)));
    const int y = (int)(blockIdx.y * AGPT_DN_TY + threadIdx.x / AGPT_DN_TX);
    if (x >= dc.W || y >= dc.H) return;
    const size_t p = (size_t)y * (size_t)dc.W + (size_t)x;
    const float4 sp = state_in[p];
    float4 out;
    out.x = 0.f; out.y = 0.f; out.z = 0.f; out.w = dc.last ? 1.f : -1.f;
    if (sp.w < 0.f) {
        state_out[p] = out;
        return;
    }
    const float4 ap = albedo[p];
    const float4 gp = normal_depth[p];
    const float flag_p = ap.w;
    const float Yp = luminance(V3(sp.x, sp.y, sp.z));
    const float lden = dc.sigma_l * sqrtf(sp.w) + AGPT_DN_LUM_EPS;
    const float zden = dc.sigma_z * (float)dc.step * fmaxf(gp.w, AGPT_DN_DEPTH_FLOOR);
    const float nden = dc.sigma_n * dc.sigma_n;
    const bool geometry = flag_p != 0.f;
    const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * dc.step;
        if (qy < 0 || qy >= dc.H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * dc.step;
            if (qx < 0 || qx >= dc.W) continue;
            const size_t q = (size_t)qy * (size_t)dc.W + (size_t)qx;
            const float flag_q = albedo[q].w;
            const float4 sq = state_in[q];
            if (flag_q != flag_p || sq.w < 0.f) continue;
            float ez = 0.f, en = 0.f;
            if (geometry) {
                const float4 gq = normal_depth[q];
                ez = fabsf(gp.w - gq.w) / zden;
                const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
                en = (nx * nx + ny * ny + nz * nz) / nden;
            }
            const float Yq = luminance(V3(sq.x, sq.y, sq.z));
            const float el = fabsf(Yp - Yq) / lden;
            const float w = (k[dx + 2] * k[dy + 2]) * cr_expf(-((ez + en) + el));
            sw += w;
            sr += w * sq.x;
            sg += w * sq.y;
            sb += w * sq.z;
            sv += (w * w) * sq.w;
        }
    }
    v3 c = V3(sr / sw, sg / sw, sb / sw);
    if (dc.last) {
        if (dc.demodulate) c = c * albedo_floor(ap);
        out.w = 1.f;
    } else {
        out.w = sv / (sw * sw);
    }
    out.x = c.x; out.y = c.y; out.z = c.z;
    state_out[p] = out;
}

namespace agpt {

void launch_feature_rays(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, float4* ray_o, float4* ray_d) {
    hipLaunchKernelGGL(k_feature_rays, agpt_blocks(rc.NP), dim3(AGPT_BLOCK), 0, stream, sc.cam, rc, ray_o, ray_d);
}
void launch_features(hipStream_t stream, const DevScene& sc, ShadeLevel level, const RenderConsts& rc, const float4* colors,
                     const DevHit* hits, const float4* ray_o, const float4* ray_d, float4* albedo, float4* normal_depth) {
    auto* kernel = k_features;   // SHADE_PLAIN
    switch (level) {
    case SHADE_TEXTURED:
    case SHADE_MAPPED: kernel = k_features_textured; break;   // (the albedo is the colour slot's nearest texel at both levels)
    case SHADE_SAMPLED: kernel = k_features_sampled; break;
    case SHADE_NORMAL: kernel = k_features_normal; break;
    default: break;
    }
    hipLaunchKernelGGL(kernel, agpt_blocks(rc.NP), dim3(AGPT_BLOCK), 0, stream, sc, rc, colors, hits, ray_o, ray_d, albedo, normal_depth);
}
void launch_features_prev(hipStream_t stream, const DevScene& sc, ShadeLevel level, const RenderConsts& rc, const float4* colors,
                          const DevHit* hits, const float4* ray_o, const float4* ray_d, float4* albedo, float4* normal_depth,
                          const float4* tri_shade_old, const float4* prev_point, float4* prev_normal) {
    auto* kernel = k_features_prev;   // SHADE_PLAIN
    switch (level) {
    case SHADE_TEXTURED:
    case SHADE_MAPPED: kernel = k_features_textured_prev; break;
    case SHADE_SAMPLED: kernel = k_features_sampled_prev; break;
    case SHADE_NORMAL: kernel = k_features_normal_prev; break;
    default: break;
    }
    hipLaunchKernelGGL(kernel, agpt_blocks(rc.NP), dim3(AGPT_BLOCK), 0, stream, sc, rc, colors, hits, ray_o, ray_d, albedo, normal_depth,
                       tri_shade_old, prev_point, prev_normal);
}

}  // namespace agpt

extern "C" {

// k_denoise_prepare, then `iterations` passes that ping-pong between out_dev and the context's scratch buffer so that the last one,
// which also re-modulates and sets w = 1, lands in out_dev.
int agpt_denoise(agpt_ctx* c, const agpt_denoise_params* p, const float* accum_dev, const float* moment2_dev, const float* albedo_dev,
                 const float* normal_depth_dev, float* out_dev) {
    if (!p) return fail(AGPT_ERR_INVALID, "agpt_denoise: NULL argument");
    if (p->width <= 0 || p->height <= 0 || (uint64_t)p->width * (uint64_t)p->height > 0x7FFFFFFFull)
        return fail(AGPT_ERR_INVALID, "agpt_denoise: bad film size");
    if (p->iterations < 1 || p->iterations > 8) return fail(AGPT_ERR_INVALID, "agpt_denoise: iterations must be in 1..8");
    if (p->demodulate != 0 && p->demodulate != 1) return fail(AGPT_ERR_INVALID, "agpt_denoise: demodulate must be 0 or 1");
    if (!(p->sigma_z > 0.f) || !(p->sigma_n > 0.f) || !(p->sigma_l > 0.f) || std::isinf(p->sigma_z) || std::isinf(p->sigma_n) ||
        std::isinf(p->sigma_l))
        return fail(AGPT_ERR_INVALID, "agpt_denoise: sigma_z, sigma_n and sigma_l must be positive and finite");
    if (!c || !accum_dev || !moment2_dev || !albedo_dev || !normal_depth_dev || !out_dev)
        return fail(AGPT_ERR_INVALID, "agpt_denoise: NULL argument");
    if (out_dev == accum_dev || out_dev == moment2_dev || out_dev == albedo_dev || out_dev == normal_depth_dev)
        return fail(AGPT_ERR_INVALID, "agpt_denoise: out_dev aliases an input");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)p->width * (size_t)p->height;
    const int rc = c->denoise_state.ensure(n);
    if (rc) return rc;
    DenoiseConsts dc{};
    dc.W = p->width; dc.H = p->height; dc.demodulate = p->demodulate;
    dc.sigma_z = p->sigma_z; dc.sigma_n = p->sigma_n; dc.sigma_l = p->sigma_l;
    float4* buf[2] = {(float4*)out_dev, c->denoise_state.p};
    int cur = p->iterations & 1;   // pass i reads buf[cur] and writes the other: an even number of passes starts in out_dev
    // state = (c.rgb, v); v = -1 marks a pixel without samples
    hipLaunchKernelGGL(k_denoise_prepare, agpt_blocks(n), dim3(AGPT_BLOCK), 0, c->stream, dc, (const float4*)accum_dev, moment2_dev,
                       (const float4*)albedo_dev, buf[cur]);
    static_assert(AGPT_DN_TX * AGPT_DN_TY == AGPT_BLOCK, "one thread per tile pixel");
    const dim3 tiles((unsigned)((dc.W + AGPT_DN_TX - 1) / AGPT_DN_TX), (unsigned)((dc.H + AGPT_DN_TY - 1) / AGPT_DN_TY));
    for (int i = 0; i < p->iterations; ++i, cur ^= 1) {
        dc.step = 1 << i;
        dc.last = i == p->iterations - 1;
        hipLaunchKernelGGL(k_denoise_pass, tiles, dim3(AGPT_BLOCK), 0, c->stream, dc, (const float4*)buf[cur], (const float4*)albedo_dev,
                           (const float4*)normal_depth_dev, buf[cur ^ 1]);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

}  // extern "C"
