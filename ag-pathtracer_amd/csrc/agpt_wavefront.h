// agpt_wavefront.h -- what the kernels of the wavefront path tracer share: the per-path state in HBM (PathBuffers), the path-id
// queues between the kernels, the per-batch constants, the path / pixel order and the counters.  Included by agpt_trace_kernels.h
// (trace), agpt_kernels.h (generate, ...) and by agpt_shade_kernels.h (k_shade and the kernels that finish a batch: k_accumulate, k_export_li,
// k_resolve_pending), which are separate translation units because they are compiled with different code-generation options (build.py).
#pragma once

#include "agpt_math.h"
#include "agpt_scene.h"

#define AGPT_BLOCK 256
#define AGPT_CHUNK 64

// path flags (beta4.w)
#define PF_BOUNCE_MASK 0xFFu
#define PF_SPECULAR 0x100u   // specularBounce
#define PF_DEAD 0x200u       // path ended; only the pending NEE of its last vertex is left to add (finished_radiance, agpt_shade_kernels.h)
#define PF_PEND_C1 0x400u    // light-sampling leg contribution waits for its shadow ray
#define PF_PEND_C2 0x800u    // BSDF-sampling leg contribution waits for its MIS ray
#define PF_PENDING 0x1000u   // a vertex' UniformSampleOneLight result is still to be added to L

struct PathBuffers {
    float4 *ext_o, *ext_d;        // continuation ray (o.w = tmax)
    float4 *sh_o, *sh_d;          // shadow ray
    float4 *mis_o, *mis_d;        // MIS ray
    DevHit *hit, *mis_hit;
    uint32_t* occluded;
    uint32_t* mis_ok;             // MIS-query result of the production kernel (mis_mode 1)
    float4* beta4;                // beta.xyz, flags
    float4* L4;                   // L.xyz, rng state
    float4* fac4;                 // f*|wi.ns|/pdf of the sampled continuation, chosen light index
    float4 *c1, *c2;              // pending NEE contributions (light leg / BSDF leg)
};

#define AGPT_QSTRIDE 32  // queue counters live on separate 128-B lines: same-line atomics serialise (~11 ns each)
#ifndef AGPT_FRONTIERS
#define AGPT_FRONTIERS 8u
#endif // work-queue frontiers per trace launch (one per XCD), AGPT_QSTRIDE words apart
// ext: the live paths, each with a continuation ray -- what k_trace_fast<0> traces is what k_shade then shades.  A path that has
// ended is in no queue: its last shadow ray / MIS query, if any, is in those two, and its radiance is complete once they are traced.
struct Queues {
    uint32_t *ext, *mis, *shadow;   // path ids
    uint32_t* counts;               // [q * AGPT_QSTRIDE]: q = 0 ext, 1 mis, 2 shadow
};
#define AGPT_NQUEUES 3
#define QCOUNT(q, i) ((q).counts[(i) * AGPT_QSTRIDE])

struct RenderConsts {
    int32_t W, H, x0, y0, w, h;
    int32_t s0, S;            // first sample index of the batch, samples in the batch
    uint32_t seed_base;
    int32_t max_depth;
    int32_t accum_pitch, accum_row0;
    uint32_t NP;              // pixels of the tile this call renders (w * rows)
    int32_t il_block, il_world, il_rank;  // row-block interleave (il_block == 0: off)
    int32_t mis_mode;                     // 0: MIS rays traced as closest-hit (mis_hit), 1: as MIS queries (mis_ok)
    int32_t answer_rays;                  // 1: ray queries that cannot reach the image are counted, not traced
};

// Path order inside a batch of S samples x NP pixels: the samples of a pixel are adjacent in runs of G = the largest power
// of two <= 64 that divides S (path id = ((s / G) * NP + p) * G + s % G), so that with 64 spp a wave starts on the 64 samples
// of ONE pixel: the primary rays of a wave are one bundle and the first hits share a few triangles (-3.5 ms per C3 step over
// one-sample-per-pixel waves).  Like the pixel order below, invisible outside.
__host__ __device__ __forceinline__ uint32_t sample_group(int32_t S) {   // (host: k_accumulate's grid)
    const uint32_t low = (uint32_t)S & (0u - (uint32_t)S);
    return low < 64u ? low : 64u;
}

// local pixel index -> film pixel (x, y) and the accumulator element it adds into
__device__ __forceinline__ void pixel_of(const RenderConsts& rc, uint32_t p, int& x, int& y, size_t& accum_index) {
    // Local pixel order: 8x8-pixel blocks, row-major inside a block and over the blocks, when the region's width and its number
    // of rows are multiples of 8 (1080p is; so is every rank's share of 8-row blocks) -- a wave then starts on a compact 8x8
    // patch of the film instead of a 64x1 strip, and the queues keep that order.  Plain row-major otherwise.  (The order is
    // invisible outside: RNG streams and accumulator elements are addressed by the film pixel.)
    const uint32_t w = (uint32_t)rc.w, n_rows = rc.NP / w;
    uint32_t row, col;
    if (((w | n_rows) & 7u) == 0u) {
        const uint32_t blk = p >> 6, inner = p & 63u, per_row = w >> 3;
        const uint32_t brow = blk / per_row;
        row = brow * 8u + (inner >> 3);
        col = (blk - brow * per_row) * 8u + (inner & 7u);
    } else {
        row = p / w;
        col = p - row * w;
    }
    x = rc.x0 + (int)col;
    if (rc.il_block == 0) {
        y = rc.y0 + (int)row;
        accum_index = (size_t)((rc.H - 1 - y) - rc.accum_row0) * (size_t)rc.accum_pitch + (size_t)x;
    } else {
        const int j = (int)row / rc.il_block, within = (int)row % rc.il_block;
        const int yb = (j * rc.il_world + rc.il_rank) * rc.il_block;
        const int hb = min(rc.il_block, rc.H - yb);
        y = yb + within;
        accum_index = (size_t)(j * rc.il_block + (hb - 1 - within)) * (size_t)rc.accum_pitch + (size_t)x;
    }
}

// the grid of a one-thread-per-item launch with AGPT_BLOCK threads per block (64-bit: n may be a product of two 32-bit counts)
static inline dim3 agpt_blocks(uint64_t n) { return dim3((unsigned)((n + AGPT_BLOCK - 1) / AGPT_BLOCK)); }

// ---------------------------------------------------------------------------------------------------------
// The two ends of a path, each written once: how it starts (k_generate, k_generate_li, k_generate_list; the pixel-centre rays of
// agpt_denoise.h) and how its radiance reaches the film (k_accumulate, k_accumulate_list; k_resolve, k_resolve_counts).
// Camera::GetRay (camera.h:58-64) for the film position (s, t) and the lens offset rd: the ray is (O, D), D normalised once
__device__ __forceinline__ void camera_ray(const DevCamera& c, float s, float t, float rdx, float rdy, v3& O, v3& D) {
    v3 offset = c.u * rdx + c.v * rdy;
    v3 pixel = c.lower_left_corner + s * c.horizontal + t * c.vertical;
    O = c.origin + offset;
    D = normalize(pixel - c.origin - offset);
}
// ... with rd drawn on the lens disk by rejection (common.h:65-71) from the path's stream; no draw for a pinhole
__device__ __forceinline__ void camera_sample_ray(const DevCamera& c, float s, float t, uint32_t& rng, v3& O, v3& D) {
    v3 rd = V3s(0.f);
    if (c.lens_radius > 0.f) {
        for (;;) {
            float a = -1.f + (1.f - -1.f) * rng_float(rng);
            float b = -1.f + (1.f - -1.f) * rng_float(rng);
            v3 pd = V3(a, b, 0);
            if (sqrlen(pd) >= 1) continue;
            rd = c.lens_radius * pd;
            break;
        }
    }
    camera_ray(c, s, t, rd.x, rd.y, O, D);
}
// The initial state of path i of a batch of `total`: its continuation ray, beta = 1, L = 0 with the stream's state, its place in
// the ext queue; path 0 sets the three queue lengths.
__device__ __forceinline__ void start_path(const PathBuffers& pb, const Queues& q, uint32_t i, uint32_t total, v3 O, v3 D, float tmax,
                                           uint32_t rng, int32_t max_depth) {
    float4 o4, d4, b4, l4;
    o4.x = O.x; o4.y = O.y; o4.z = O.z; o4.w = tmax;
    d4.x = D.x; d4.y = D.y; d4.z = D.z;
    d4.w = max_depth > 0 ? 2.f : 0.f;   // 2: a camera ray that may be re-cast through emitters by the trace kernel (see k_trace_fast)
    b4.x = 1.f; b4.y = 1.f; b4.z = 1.f; b4.w = __uint_as_float(0u);
    l4.x = 0.f; l4.y = 0.f; l4.z = 0.f; l4.w = __uint_as_float(rng);
    pb.ext_o[i] = o4;
    pb.ext_d[i] = d4;
    pb.beta4[i] = b4;
    pb.L4[i] = l4;
    q.ext[i] = i;
    if (i == 0) {
        QCOUNT(q, 0) = total;
        QCOUNT(q, 1) = 0;
        QCOUNT(q, 2) = 0;
    }
}
// myapp.cpp:169-173: a sample with a NaN component or an infinite luminance is added as black and counted in `bad`.  (Values in,
// values out: with clr or bad passed by reference the kernels compile to other code than with the test written out in them.)
struct FilmSample { v3 clr; uint32_t bad; };
__device__ __forceinline__ FilmSample film_sample(v3 clr, uint32_t bad) {
    if (isnan(clr.x) || isnan(clr.y) || isnan(clr.z) || isinf(luminance(clr))) {
        clr = V3s(0.f);
        bad++;
    }
    return FilmSample{clr, bad};
}
// Accumulator::CopyToSurface (myapp.h:34-41) with lin2rgb / rgb2uint (template/common.h:41-51): the display word of a pixel that holds
// the sum a.xyz of n samples
__device__ __forceinline__ uint32_t resolve_word(const float4& a, float n) {
    float e = 1 / 2.2f;
    float r = powf(a.x / n, e), g = powf(a.y / n, e), b = powf(a.z / n, e);
    int ri = (int)(256 * tclampf(r, 0.0f, 0.999f));
    int gi = (int)(256 * tclampf(g, 0.0f, 0.999f));
    int bi = (int)(256 * tclampf(b, 0.0f, 0.999f));
    return (uint32_t)((ri << 16) + (gi << 8) + bi);
}

struct DevCounters {
    unsigned long long closest_rays, anyhit_rays, interior, tris, shaded, outliers, samples, roots, answered;
#if defined(AGPT_TRACE_STATS) || defined(AGPT_SHADE_CLOCK)
    unsigned long long dbg[96];  // developer builds only (tools/build_variant.py): wave-step statistics of k_trace_fast, phase clocks
#define AGPT_DBG_COH 64          // first of the 20 slots of the coherent closest-hit launch (the 16 of a mode + its scalar-path counts)
#define AGPT_DBG_ROOT_PASS 84    // four slots (modes 0..2, coherent): root-pair steps whose root box passes (the steps: slot 15 of the mode)
#endif
};
#ifdef AGPT_TRACE_STATS
#define TS(...) __VA_ARGS__
#else
#define TS(...)
#endif
// developer build only (-DAGPT_TRACE_STATS -DAGPT_TRACE_CLOCK): s_memtime stamps around the phases of k_trace_fast
#ifdef AGPT_TRACE_CLOCK
#define TCK(...) __VA_ARGS__
#define TCK_NOW() __builtin_amdgcn_s_memtime()
#else
#define TCK(...)
#endif

// Wave-uniform bookkeeping values that the compiler cannot prove uniform (loop-carried through regions with per-lane
// branches) are pinned to scalar registers with readfirstlane: they then cost SALU instead of VALU + exec-mask juggling.
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ bool uni(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }
// A value the compiler already holds in a scalar register, made opaque as a 32-bit word: what is computed from it afterwards is not
// rewritten in terms of the wider value it was narrowed from (a popcount of a ballot: readfirstlane of it folds away, and a compare of
// two of them goes back to 64 bits, for which the scalar unit has no ordered compare).
__device__ __forceinline__ uint32_t uni_word(uint32_t v) {
    asm("" : "+s"(v));
    return v;
}

// ---------------------------------------------------------------------------------------------------------
// wave-aggregated queue append: one atomic per wave, order inside the wave preserved
__device__ __forceinline__ void queue_push(uint32_t* q, uint32_t* count, bool pred, uint32_t value) {
    unsigned long long mask = __ballot(pred);
    if (mask == 0) return;
    int lane = __lane_id();
    int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    if (pred) {
        uint32_t off = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        q[base + off] = value;
    }
}


// ---------------------------------------------------------------------------------------------------------
// host side of the shading translation units (agpt_shade_kernels*.hip)
namespace agpt {
// the scene's Scene::primitives records, materials and lights fit the LDS copies k_shade<LDS_TABLES> works from
bool shade_tables_fit_lds(int n_prims, int n_materials, int n_lights);
// The texturing level of a scene: each level is the one below plus what its row in agpt_shade_kernels.h's table adds.
// agpt_scene_commit derives it, and it picks the shading unit (launch_shading) and the feature kernel (launch_features).
enum ShadeLevel { SHADE_PLAIN = 0, SHADE_TEXTURED = 1, SHADE_MAPPED = 2, SHADE_SAMPLED = 3, SHADE_NORMAL = 4, SHADE_LEVELS = 5 };
// Which shading kernels an iteration runs: the unit (level; fast: agpt_scene_set_shading_arith(AGPT_SHADING_FAST)) and k_shade's
// <LDS_TABLES, ENV> instantiation in it.
struct ShadeVariant {
    ShadeLevel level;
    bool fast, lds_tables, env;
};
// the shading of one wavefront iteration: k_shade over qin's live paths
void launch_shading(hipStream_t stream, const ShadeVariant& v, int shade_grid, const DevScene& sc, const RenderConsts& rc,
                    const PathBuffers& pb, const Queues& qin, const Queues& qout, DevCounters* counters, uint32_t* tile_heads);
// What consumes a finished batch.  A path that ended with its last light sample pending still has it in c1 / c2 / occluded / mis_ok:
// it is added by finished_radiance, in the arithmetic of the shading unit `fast` names.
// k_accumulate: the batch of rc into the accumulator, samples in sample order
void launch_accumulate(hipStream_t stream, bool fast, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, float4* accum,
                       DevCounters* counters);
// k_export_li: Li's return value (radiance3[3 n]) and, if asked for, the RNG end state of the paths 0 .. n of agpt_li_batch
void launch_export_li(hipStream_t stream, bool fast, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t n,
                      float* radiance3, uint32_t* rng_out);
// k_resolve_pending: the same for the consumer that lives in another unit (k_accumulate_list, agpt_adaptive.hip) -- one pass over the
// finished batch's paths 0 .. n that leaves every path's radiance complete in L4
void launch_finish_paths(hipStream_t stream, bool fast, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t n);
// the known-answer kernels of the fast-arithmetic unit (k_kat_bsdf_eval_fast, k_kat_bsdf_sample_fast; one lane per case, 64-lane blocks)
void launch_kat_bsdf_eval_fast(hipStream_t stream, const DevScene& sc, int material, int n, const float* wo3, const float* wi3, float* f3o,
                               float* pdfo);
void launch_kat_bsdf_sample_fast(hipStream_t stream, const DevScene& sc, int material, int n, const float* wo3, const float* u2, float* wi3o,
                                 float* f3o, float* pdfo, int32_t* speco);
// k_kat_env_light_fast: one lane per direction (n_dirs) or draw (n_draws)
void launch_kat_env_light_fast(hipStream_t stream, const DevScene& sc, int light, int n_dirs, const float* d3, float* le3o, float* pdf_li_o,
                               int n_draws, const float* u, float* wi3o, float* pdfo, float* sle3o, int32_t* oko);
}  // namespace agpt
