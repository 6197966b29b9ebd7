// agpt_kernels.h -- the gfx950 kernels of the wavefront path tracer: how an iteration is put together, and the small kernels that
// agpt_api.hip launches itself (ray preparation and export, path generation, resolve).
//
// One agpt_render batch = S samples x NP tile pixels paths (path order: sample_group / pixel_of, agpt_wavefront.h).  Per iteration:
//     k_trace_fast<0>(ext queue)     continuation rays, closest hit                     -> hit[]
//     k_trace_fast<2>(mis queue)     BSDF-sampled MIS rays as exact early-exit queries  -> mis_ok[]
//     k_trace_fast<1>(shadow queue)  NEE shadow rays, any hit                           -> occluded[]
//     k_shade(ext queue)             resolves the previous vertex' NEE, then PathTracer::Li's loop body for the
//                                    new hit; appends to the next iteration's queues with one atomic per queue per
//                                    wave-private 256-path tile (ballot counts, order-preserving offsets)
// A path that ends with its last vertex' light sample pending joins no queue: the sample is added where the batch is consumed
// (finished_radiance: in k_accumulate and k_export_li themselves; for agpt_render_adaptive by one k_resolve_pending pass over the
// finished batch).  (k_shade, k_accumulate, k_export_li and k_resolve_pending live in agpt_shade_kernels.h, translation units of their own with
// their own code-generation options; the instrumented / fallback k_trace traces MIS rays as closest hits into mis_hit[]).  Scenes with more than 64
// primitives run k_candidates (top-level tree over Scene::primitives) in front of each trace launch.  The trace kernels are
// persistent: a fixed grid of waves pulls 64-ray chunks off the queue; queue lengths stay on the device (no host round
// trip per iteration).  Path state is SoA float4 in HBM (coalesced 16 B/lane); the per-lane traversal stack lives in LDS
// (23 entries x 4 B x 256 lanes = 23 KiB/block, deeper entries in an HBM spill column).  A continuation ray that retires on a
// primitive without a material is re-cast by the closest-hit kernel itself (CUR_RECAST), so a render has max_depth + 3 iterations.
//
// The trace kernels (k_trace, k_trace_fast, k_candidates) live in agpt_trace_kernels.h, compiled by agpt_trace_kernels.hip alone and
// reached through agpt::launch_trace (agpt_internal.h).  Rules that kernels must agree on bit for bit live in one place each: path
// start, film write-back and launch grid (camera_sample_ray, start_path, film_sample, resolve_word, agpt_blocks) in agpt_wavefront.h;
// the conservative slab test (conservative_slab) and the hit record (store_hit) in agpt_trace.h.  What the trace kernels still write
// out more than once is listed at the top of agpt_trace_kernels.h.
#pragma once

#include "agpt_wavefront.h"

// agpt_intersect_batch: Ray ctor (camera.h:6) normalises D
__global__ void k_prepare_rays(const agpt_ray* __restrict__ in, int n, float4* __restrict__ ray_o, float4* __restrict__ ray_d) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    agpt_ray r = in[i];
    v3 d = normalize(V3(r.d[0], r.d[1], r.d[2]));
    float4 o4, d4;
    o4.x = r.o[0]; o4.y = r.o[1]; o4.z = r.o[2]; o4.w = r.tmax;
    d4.x = d.x; d4.y = d.y; d4.z = d.z; d4.w = 0.f;
    ray_o[i] = o4;
    ray_d[i] = d4;
}
__global__ void k_export_hits(const DevScene sc, const DevHit* __restrict__ hits, const uint32_t* __restrict__ occluded,
                              int n, int any_hit, agpt_hit* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    agpt_hit o;
    o.hit = 0; o.prim = -1; o.tri = -1; o.t = 0; o.b1 = 0; o.b2 = 0;
    if (any_hit) {
        o.hit = occluded[i] ? 1 : 0;
    } else {
        DevHit h = hits[i];
        if (h.id != AGPT_HIT_MISS) {
            o.hit = 1;
            o.t = h.t;
            if (h.id & AGPT_HIT_SPHERE) {
                o.prim = (int)(h.id & 0x7FFFFFFFu);
            } else {
                int prim = (int)__float_as_uint(sc.tri_shade[4 * (size_t)h.id + 3].w);
                o.prim = prim;
                o.tri = 3 * ((int)h.id - sc.prims[prim].tri_base);
                o.b1 = h.b1;
                o.b2 = h.b2;
            }
        }
    }
    out[i] = o;
}

// ---------------------------------------------------------------------------------------------------------
// myapp.cpp:165-167: jittered film position -> camera_sample_ray -> start_path (agpt_wavefront.h)
__global__ void __launch_bounds__(AGPT_BLOCK)
k_generate(DevScene sc, RenderConsts rc, PathBuffers pb, Queues q) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t total = rc.NP * (uint32_t)rc.S;
    if (i >= total) return;
    const uint32_t G = sample_group(rc.S);
    const uint32_t sj = i % G, tt = i / G;
    const uint32_t sg = tt / rc.NP, p = tt - sg * rc.NP;
    const uint32_t sl = sg * G + sj;
    int x, y;
    size_t unused_index;
    pixel_of(rc, p, x, y, unused_index);
    uint32_t rng = sample_seed((uint32_t)(y * rc.W + x), (uint32_t)(rc.W * rc.H), (uint32_t)(rc.s0 + (int)sl), rc.seed_base);
    float px = x + rng_float(rng);
    float py = y + rng_float(rng);
    float s = px / rc.W, t = py / rc.H;
    v3 O, D;
    camera_sample_ray(sc.cam, s, t, rng, O, D);
    start_path(pb, q, i, total, O, D, AGPT_FLT_MAX, rng, rc.max_depth);
}

// agpt_li_batch: Integrator::Li(ray, scene) (integrator.h:28-31) for n caller-supplied rays, each with its own RandomFloat() stream
// (an xorshift32 state, template/template.cpp:667-675).  The Ray ctor normalises D (camera.h:6); ray.t is the caller's tmax.
__global__ void __launch_bounds__(AGPT_BLOCK)
k_generate_li(const agpt_ray* __restrict__ rays, const uint32_t* __restrict__ rng_states, uint32_t n, PathBuffers pb, Queues q, int max_depth) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const agpt_ray r = rays[i];
    const v3 d = normalize(V3(r.d[0], r.d[1], r.d[2]));
    start_path(pb, q, i, n, V3(r.o[0], r.o[1], r.o[2]), d, r.tmax, rng_states[i], max_depth);
}
// (k_export_li, which hands out Li's return value and the stream's end state, finishes the paths: agpt_shade_kernels.h)

// ---------------------------------------------------------------------------------------------------------
// Accumulator::CopyToSurface over the accumulator of a uniform render (resolve_word, agpt_wavefront.h)
__global__ void k_resolve(const float4* __restrict__ accum, int n, int samples, uint32_t* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = resolve_word(accum[i], (float)samples);
}
