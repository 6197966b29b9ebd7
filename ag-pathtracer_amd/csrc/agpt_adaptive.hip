// agpt_adaptive.hip -- the kernels of agpt_render_adaptive (include/agpt.h): per round, k_adaptive_select decides which tile pixels
// take more samples and k_adaptive_compact lists them in ascending local order; k_generate_list and k_accumulate_list then run a
// wavefront batch over the listed pixels only (the trace and shade kernels in between are agpt_render's, unchanged).
// k_resolve_counts is CopyToSurface with the per-pixel count.
//
// A pixel's samples use the streams of agpt_render (sample_seed(pixel, W*H, sample, seed_base)) and are added in sample order with
// k_accumulate's arithmetic, so a pixel that holds n samples is bit-identical to agpt_render's pixel at spp = n.  The count lives in
// accum.w, the luminance second moment in moment2 (one float per pixel, indexed like accum).  Compiled with the library's common
// flags (-ffp-contract=off, no fast math): k_generate_list computes the camera rays of k_generate bit for bit (one camera_sample_ray,
// agpt_wavefront.h, under the same flags).
#include <hip/hip_runtime.h>

#include "agpt_adaptive.h"
#include "agpt_internal.h"

using agpt::fail;

namespace {

// the decision of one pixel: 0 inactive, 1 active, 2 stopped by the test (min_spp <= n < max_spp), -1 count off the grid
__device__ __forceinline__ int pixel_state(const AdaptiveConsts& ac, float4 a, float m2, uint32_t& n_out) {
    const float wf = a.w;
    if (!(wf >= 0.f && wf <= 16777216.f) || wf != floorf(wf)) return -1;
    const uint32_t n = (uint32_t)wf;
    n_out = n;
    if (n % (uint32_t)ac.step_spp != 0u) return -1;
    if (n >= (uint32_t)ac.max_spp) return 0;
    if (n < (uint32_t)ac.min_spp || !(ac.rel_error > 0.f)) return 1;
    // stop <=> sqrt(var / n) <= rel_error * max(mu, abs_floor), var the unbiased sample variance of the luminance
    const float nf = (float)n;
    const float mu = luminance(V3(a.x, a.y, a.z)) / nf;
    const float var = fmaxf(0.f, m2 / nf - mu * mu) * nf / (nf - 1.f);
    return sqrtf(var / nf) <= ac.rel_error * fmaxf(mu, ac.abs_floor) ? 2 : 1;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor(v, off));
    return v;
}

}  // namespace

// Pass 1: thread t of block b decides the pixels p = b * AGPT_ADAPT_BLOCK_PIXELS + j * AGPT_BLOCK + t (bit j of its mask word), and
// the block writes its active count.  The host's words are integer sums and maxima: the same whatever the order of the atomics.
__global__ void __launch_bounds__(AGPT_BLOCK)
k_adaptive_select(RenderConsts rc, AdaptiveConsts ac, const float4* __restrict__ accum, const float* __restrict__ moment2,
                  uint32_t* __restrict__ masks, uint32_t* __restrict__ block_counts, uint32_t* __restrict__ words) {
    __shared__ uint32_t red[5][AGPT_BLOCK / 64];
    const uint32_t t = threadIdx.x, base = blockIdx.x * AGPT_ADAPT_BLOCK_PIXELS;
    uint32_t bits = 0, invalid = 0, stopped = 0, inv_min = 0, nmax = 0;
    for (uint32_t j = 0; j < AGPT_ADAPT_PER_THREAD; ++j) {
        const uint32_t p = base + j * AGPT_BLOCK + t;
        if (p >= rc.NP) break;
        int x, y;
        size_t ai;
        pixel_of(rc, p, x, y, ai);
        uint32_t n = 0;
        const int st = pixel_state(ac, accum[ai], moment2[ai], n);
        if (st < 0) {
            invalid++;
            continue;
        }
        inv_min = max(inv_min, ~n);
        nmax = max(nmax, n);
        if (st == 1) bits |= 1u << j;
        if (st == 2) stopped++;
    }
    masks[blockIdx.x * AGPT_BLOCK + t] = bits;
    const uint32_t v[5] = {wave_sum((uint32_t)__popc(bits)), wave_sum(invalid), wave_max(inv_min), wave_max(nmax), wave_sum(stopped)};
    const uint32_t lane = t & 63u, wv = t >> 6;
    if (lane == 0)
        for (int k = 0; k < 5; ++k) red[k][wv] = v[k];
    __syncthreads();
    if (t == 0) {
        uint32_t r[5] = {0, 0, 0, 0, 0};
        for (uint32_t w = 0; w < AGPT_BLOCK / 64; ++w) {
            r[0] += red[0][w];
            r[1] += red[1][w];
            r[2] = max(r[2], red[2][w]);
            r[3] = max(r[3], red[3][w]);
            r[4] += red[4][w];
        }
        block_counts[blockIdx.x] = r[0];
        if (r[1]) atomicAdd(&words[AGPT_AW_INVALID], r[1]);
        if (r[2]) atomicMax(&words[AGPT_AW_INV_MIN], r[2]);
        if (r[3]) atomicMax(&words[AGPT_AW_MAX], r[3]);
        if (r[4]) atomicAdd(&words[AGPT_AW_STOPPED], r[4]);
    }
}

// Pass 2: block b starts at the sum of the active counts of blocks 0 .. b-1 and writes its active pixels in ascending order, one
// pass of AGPT_BLOCK pixels at a time (wave ballots + a scan over the block's waves) -- no atomics, the same list on every run.
// The last block writes the list's length.
__global__ void __launch_bounds__(AGPT_BLOCK)
k_adaptive_compact(const uint32_t* __restrict__ masks, const uint32_t* __restrict__ block_counts, uint32_t* __restrict__ list,
                   uint32_t* __restrict__ words) {
    __shared__ uint32_t red[AGPT_BLOCK / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, b = blockIdx.x;
    uint32_t s = 0;
    for (uint32_t k = t; k < b; k += AGPT_BLOCK) s += block_counts[k];
    s = wave_sum(s);
    if (lane == 0) red[wv] = s;
    __syncthreads();
    uint32_t offset = 0;
    for (uint32_t w = 0; w < AGPT_BLOCK / 64; ++w) offset += red[w];
    __syncthreads();
    const uint32_t bits = masks[b * AGPT_BLOCK + t];
    const uint32_t base = b * AGPT_ADAPT_BLOCK_PIXELS;
    for (uint32_t j = 0; j < AGPT_ADAPT_PER_THREAD; ++j) {
        const bool f = (bits >> j) & 1u;
        const unsigned long long bal = __ballot(f);
        if (lane == 0) red[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < AGPT_BLOCK / 64; ++w) {
            before += w < wv ? red[w] : 0u;
            total += red[w];
        }
        if (f) list[offset + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = base + j * AGPT_BLOCK + t;
        offset += total;
        __syncthreads();
    }
    if (b == gridDim.x - 1 && t == 0) words[AGPT_AW_ACTIVE] = offset;
}

// k_generate over the listed pixels: path id ((s / G) * na + a) * G + s % G for sample s of listed pixel a (G = sample_group(S)),
// sample index n + s with n = the pixel's count; from the seed on it is k_generate (agpt_kernels.h), through the same two functions.
__global__ void __launch_bounds__(AGPT_BLOCK)
k_generate_list(DevScene sc, RenderConsts rc, const uint32_t* __restrict__ list, uint32_t a0, uint32_t na, const float4* __restrict__ accum,
                PathBuffers pb, Queues q) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t total = na * (uint32_t)rc.S;
    if (i >= total) return;
    const uint32_t G = sample_group(rc.S);
    const uint32_t sj = i % G, tt = i / G;
    const uint32_t sg = tt / na, ia = tt - sg * na;
    const uint32_t sl = sg * G + sj;
    const uint32_t p = list ? list[a0 + ia] : a0 + ia;
    int x, y;
    size_t ai;
    pixel_of(rc, p, x, y, ai);
    const uint32_t n = (uint32_t)accum[ai].w;
    uint32_t rng = sample_seed((uint32_t)(y * rc.W + x), (uint32_t)(rc.W * rc.H), n + sl, rc.seed_base);
    float px = x + rng_float(rng);
    float py = y + rng_float(rng);
    float s = px / rc.W, t = py / rc.H;
    v3 O, D;
    camera_sample_ray(sc.cam, s, t, rng, O, D);
    start_path(pb, q, i, total, O, D, AGPT_FLT_MAX, rng, rc.max_depth);
}

// k_accumulate over the listed pixels (same rgb additions in sample order, film_sample's NaN / inf reject), plus the luminance second
// moment moment2 += Y * Y and the count accum.w += S.  Reads finished paths: agpt_render_adaptive runs agpt::launch_finish_paths
// (k_resolve_pending, agpt_shade_kernels.h) over the batch first, which adds an ended path's pending light sample to L4
__global__ void __launch_bounds__(AGPT_BLOCK)
k_accumulate_list(RenderConsts rc, const uint32_t* __restrict__ list, uint32_t a0, uint32_t na, PathBuffers pb, float4* __restrict__ accum,
                  float* __restrict__ moment2, DevCounters* __restrict__ counters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= na) return;
    const uint32_t p = list ? list[a0 + i] : a0 + i;
    int x, y;
    size_t ai;
    pixel_of(rc, p, x, y, ai);
    float4 a = accum[ai];
    float m = moment2[ai];
    uint32_t bad = 0;
    const uint32_t G = sample_group(rc.S);
    for (int s = 0; s < rc.S; s++) {
        const float4 l4 = pb.L4[((size_t)((uint32_t)s / G) * na + i) * G + (uint32_t)s % G];
        const FilmSample fs = film_sample(V3(l4.x, l4.y, l4.z), bad);
        const v3 clr = fs.clr;
        bad = fs.bad;
        a.x += clr.x;
        a.y += clr.y;
        a.z += clr.z;
        const float Y = luminance(clr);
        m += Y * Y;
    }
    a.w = (float)((uint32_t)a.w + (uint32_t)rc.S);
    accum[ai] = a;
    moment2[ai] = m;
    if (bad) atomicAdd(&counters->outliers, (unsigned long long)bad);  // outliers are rare
}

// k_resolve (resolve_word) with each pixel's own count accum.w; a pixel without samples resolves to 0
__global__ void k_resolve_counts(const float4* __restrict__ accum, int n, uint32_t* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 a = accum[i];
    if (!(a.w > 0.f)) {
        out[i] = 0u;
        return;
    }
    out[i] = resolve_word(a, a.w);
}

namespace agpt {

void launch_adaptive_select(hipStream_t stream, const RenderConsts& rc, const AdaptiveConsts& ac, const float4* accum, const float* moment2,
                            uint32_t* masks, uint32_t* block_counts, uint32_t* words) {
    const dim3 g((rc.NP + AGPT_ADAPT_BLOCK_PIXELS - 1) / AGPT_ADAPT_BLOCK_PIXELS);
    hipLaunchKernelGGL(k_adaptive_select, g, dim3(AGPT_BLOCK), 0, stream, rc, ac, accum, moment2, masks, block_counts, words);
}
void launch_adaptive_compact(hipStream_t stream, uint32_t np, const uint32_t* masks, const uint32_t* block_counts, uint32_t* list,
                             uint32_t* words) {
    const dim3 g((np + AGPT_ADAPT_BLOCK_PIXELS - 1) / AGPT_ADAPT_BLOCK_PIXELS);
    hipLaunchKernelGGL(k_adaptive_compact, g, dim3(AGPT_BLOCK), 0, stream, masks, block_counts, list, words);
}
void launch_generate_list(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, const uint32_t* list, uint32_t a0, uint32_t na,
                          const float4* accum, const PathBuffers& pb, const Queues& q) {
    hipLaunchKernelGGL(k_generate_list, agpt_blocks((uint64_t)na * (uint64_t)rc.S), dim3(AGPT_BLOCK), 0, stream, sc, rc, list, a0, na, accum,
                       pb, q);
}
void launch_accumulate_list(hipStream_t stream, const RenderConsts& rc, const uint32_t* list, uint32_t a0, uint32_t na, const PathBuffers& pb,
                            float4* accum, float* moment2, DevCounters* counters) {
    hipLaunchKernelGGL(k_accumulate_list, agpt_blocks(na), dim3(AGPT_BLOCK), 0, stream, rc, list, a0, na, pb, accum, moment2, counters);
}

}  // namespace agpt

extern "C" {

int agpt_resolve_counts(agpt_ctx* c, const float* accum_dev, int n_pixels, uint32_t* out_rgb) {
    if (!c || !accum_dev || !out_rgb || n_pixels <= 0) return fail(AGPT_ERR_INVALID, "agpt_resolve_counts: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> d;
    HIP_TRY(d.alloc((size_t)n_pixels));
    hipLaunchKernelGGL(k_resolve_counts, agpt_blocks((uint64_t)n_pixels), dim3(AGPT_BLOCK), 0, c->stream, (const float4*)accum_dev, n_pixels, d.p);
    HIP_TRY(hipGetLastError());
    if (const int rc = d.out(out_rgb, (size_t)n_pixels, &c->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

}  // extern "C"
