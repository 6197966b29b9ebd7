// agpt_api.hip -- the C ABI of include/agpt.h: the context and its path-state pool, the wavefront loop and the entry points that run
// them.  The trace kernels are behind agpt::launch_trace (agpt_trace_kernels.hip); the small kernels of agpt_kernels.h are launched
// from here, the only unit that includes it (they are not templates: a second includer would define them again).  The other
// entry points: agpt_scene_api.hip, agpt_kat.hip, agpt_comm.hip, and agpt_adaptive.hip / agpt_denoise.hip / agpt_temporal.hip beside
// their kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "agpt_adaptive.h"
#include "agpt_denoise.h"
#include "agpt_internal.h"
#include "agpt_kernels.h"
#include "agpt_motion.h"

namespace agpt {

static thread_local std::string g_error;

int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

int interleave_rows(int H, int block, int world, int rank) {
    int rows = 0;
    for (int k = rank, y = k * block; y < H; k += world, y = k * block) rows += std::min(block, H - y);
    return rows;
}

}  // namespace agpt
using agpt::fail;

using agpt::launch_trace;
using agpt::TraceLaunch;
using agpt::use_fast_trace;

static void release_pool(agpt_ctx* c) {
#define X(T, name) c->name.release();
    AGPT_POOL_BUFFERS(X)
#undef X
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < AGPT_NQUEUES; j++) c->q[i][j].release();
    c->cand_mask.release();
    c->cand_chunks.release();
    c->pool_paths = 0;
}
static hipEvent_t next_event(agpt_ctx* c) {
    if (c->tev_used == c->tev.size()) {
        hipEvent_t e = nullptr;
        c->note(hipEventCreate(&e));
        c->tev.push_back(e);
    }
    return c->tev[c->tev_used++];
}

// a trace launch of the wavefront loop: its asynchronous errors are noted, and with `timing` it sits between two events of `kind`
static void launch_trace_timed(agpt_ctx* c, int mode, bool timing, int kind, const DevScene& sc, const TraceLaunch& t) {
    if (timing) {
        c->note(hipEventRecord(next_event(c), t.stream));
        c->tev_kind.push_back(kind);
    }
    launch_trace(c, mode, sc, t);
    c->note(hipGetLastError());
    if (timing) c->note(hipEventRecord(next_event(c), t.stream));
}
extern "C" {

const char* agpt_last_error(void) { return agpt::g_error.c_str(); }
int agpt_version(void) { return 1; }

int agpt_init(int device, agpt_ctx** out) {
    if (!out) return fail(AGPT_ERR_INVALID, "agpt_init: out is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(AGPT_ERR_DEVICE, "agpt_init: no HIP device (the MI355X path has no CPU fallback)");
    if (device < 0 || device >= n) return fail(AGPT_ERR_INVALID, "agpt_init: bad device index");
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<agpt_ctx> c(new agpt_ctx());
    c->device = device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    for (auto& ev : c->ev) HIP_TRY(hipEventCreate(&ev));
    for (auto& st : c->aux_stream) HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (auto& ev : c->aux_ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (const char* ms = getenv("AGPT_MULTI_STREAM")) c->multi_stream = atoi(ms);
    if (const char* sp = getenv("AGPT_SMALL_BATCH_PATHS")) c->small_batch_paths = strtoull(sp, nullptr, 10);
    HIP_TRY(hipHostMalloc((void**)&c->host_pinned, 2 * AGPT_NQUEUES * AGPT_QSTRIDE * sizeof(uint32_t)));
    const char* fg = getenv("AGPT_FORCE_GENERIC");
    c->force_generic = fg && fg[0] == '1';
    if (const char* mc = getenv("AGPT_MIS_CLOSEST")) c->mis_closest = mc[0] == '1';
    if (const char* bp = getenv("AGPT_BLOCKS_PER_CU")) c->fast_blocks_per_cu = std::max(1, atoi(bp));
    if (const char* sb = getenv("AGPT_SHADE_BLOCKS_PER_CU")) c->shade_blocks_per_cu = std::min(64, std::max(1, atoi(sb)));
    if (const char* rf = getenv("AGPT_REFILL")) c->refill = std::min(64, std::max(1, atoi(rf)));
    if (const char* rf = getenv("AGPT_REFILL_ANY")) c->refill_any = std::min(64, std::max(1, atoi(rf)));
    *out = c.release();
    return AGPT_OK;
}

int agpt_set_stream(agpt_ctx* c, void* s) {
    if (!c) return fail(AGPT_ERR_INVALID, "agpt_set_stream: ctx is NULL");
    if ((hipStream_t)s == c->stream) return AGPT_OK;
    // the pool, queues, counters, events and pinned words are one set per context: what the stream being left still has queued
    // (agpt_render's accumulate pass, the tile kernels) finishes before a call on the new stream can touch them
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = (hipStream_t)s;
    return AGPT_OK;
}

void agpt_destroy(agpt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->host_pinned) (void)hipHostFree(c->host_pinned);
    for (auto& ev : c->tev) (void)hipEventDestroy(ev);
    for (auto& ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : c->aux_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& st : c->aux_stream)
        if (st) (void)hipStreamDestroy(st);
    delete c;   // (and with it every device buffer the context holds)
}

// ---- device helpers -----------------------------------------------------------------------------------------
int agpt_device_alloc(agpt_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return fail(AGPT_ERR_INVALID, "agpt_device_alloc: NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(AGPT_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return AGPT_OK;
}
int agpt_device_free(agpt_ctx* c, void* p) {
    if (!c) return fail(AGPT_ERR_INVALID, "agpt_device_free: ctx is NULL");
    if (p) HIP_TRY(hipFree(p));
    return AGPT_OK;
}
int agpt_device_memset(agpt_ctx* c, void* p, int value, size_t bytes) {
    if (!c || !p) return fail(AGPT_ERR_INVALID, "agpt_device_memset: NULL argument");
    HIP_TRY(hipMemsetAsync(p, value, bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}
int agpt_device_download(agpt_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return fail(AGPT_ERR_INVALID, "agpt_device_download: NULL argument");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}
int agpt_device_upload(agpt_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return fail(AGPT_ERR_INVALID, "agpt_device_upload: NULL argument");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

// ---- hot path -----------------------------------------------------------------------------------------------
// bytes of pool state per path: the AGPT_POOL_BUFFERS elements + 2 x AGPT_NQUEUES queue words
#define X(T, name) +sizeof(T)
constexpr size_t AGPT_BYTES_PER_PATH = (0 AGPT_POOL_BUFFERS(X)) + 2 * AGPT_NQUEUES * sizeof(uint32_t);
#undef X
static_assert(AGPT_BYTES_PER_PATH == 240, "11 float4 arrays + 2 hit arrays (16 B) + 2 flag words + 6 queue words");
// extra pool bytes per path for a scene: the candidate words of lists longer than 64 primitives (k_candidates)
static size_t candidate_bytes_per_path(int n_prims) { return n_prims > 64 ? 4 + 8 * (size_t)((n_prims + 63) / 64) : 0; }
static int ensure_pool(agpt_ctx* c, size_t paths, int n_prims) {
    int rc;
    // the pool never shrinks: a small call after a large one keeps the capacity (agpt_render sizes its batches by it, and the
    // candidate words are laid out [chunk][pool_paths])
    paths = std::max(paths, c->pool_paths);
    if (n_prims > 64) {
        if ((rc = c->cand_chunks.ensure(paths))) return rc;
        if ((rc = c->cand_mask.ensure(paths * (size_t)((n_prims + 63) / 64)))) return rc;
    }
#define X(T, name) \
    if ((rc = c->name.ensure(paths))) return rc;
    AGPT_POOL_BUFFERS(X)
#undef X
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < AGPT_NQUEUES; j++)
            if ((rc = c->q[i][j].ensure(paths))) return rc;
    if ((rc = c->qcounts.ensure(2 * AGPT_NQUEUES * AGPT_QSTRIDE))) return rc;
    if ((rc = c->work.ensure(4096))) return rc;
    if ((rc = c->counters.ensure(1))) return rc;
    c->pool_paths = paths;
    return AGPT_OK;
}

// The batch-size policy of the renderers: a pool for unit * count paths, `count` halved until it fits.  The batch is a
// performance choice, not a semantic one (the image is batch-split invariant): when the pool has to grow, keep it within the
// memory that is actually free (other ranks or applications may share the GPU), and halve the batch if an allocation still fails.
static int fit_pool(agpt_ctx* c, const agpt_scene* s, size_t unit, uint64_t& count) {
    if (unit * (size_t)count > c->pool_paths) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t per_path = AGPT_BYTES_PER_PATH + candidate_bytes_per_path(s->dev.n_prims);
            const size_t avail = free_b + c->pool_paths * per_path;
            const size_t fit = (size_t)((double)avail * 0.9) / per_path;
            while (count > 1 && unit * (size_t)count > fit) count = (count + 1) / 2;
        }
    }
    int rc = ensure_pool(c, unit * (size_t)count, s->dev.n_prims);
    while (rc == AGPT_ERR_NOMEM && count > 1) {
        release_pool(c);
        count = (count + 1) / 2;
        rc = ensure_pool(c, unit * (size_t)count, s->dev.n_prims);
    }
    return rc;
}

static bool shade_tables_fit_lds(const DevScene& d) {
    return agpt::shade_tables_fit_lds(d.n_prims, d.n_materials, d.n_lights) && !getenv("AGPT_SHADE_GLOBAL_TABLES");
}

// Which shading kernels the next call on the scene launches (begin_wavefront, agpt_scene_shade_variant)
static agpt::ShadeVariant shade_variant_of(const agpt_scene* s) {
    agpt::ShadeVariant v;
    v.fast = s->shading_arith == AGPT_SHADING_FAST;   // agpt_scene_set_shading_arith
    v.level = s->shade_level;                         // agpt_scene_commit
    v.lds_tables = shade_tables_fit_lds(s->dev);
    v.env = !s->envs.empty();                         // an InfiniteAreaLight is present
    return v;
}

int agpt_scene_shade_variant(const agpt_scene* s, int32_t out4[4]) {
    if (!s || !out4) return fail(AGPT_ERR_INVALID, "agpt_scene_shade_variant: NULL scene or output");
    if (!s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_shade_variant: scene not committed");
    const agpt::ShadeVariant v = shade_variant_of(s);
    out4[0] = (int32_t)v.level; out4[1] = v.fast ? 1 : 0; out4[2] = v.lds_tables ? 1 : 0; out4[3] = v.env ? 1 : 0;
    return AGPT_OK;
}

// What a call that runs the wavefront loop sets up once (begin_wavefront): the pool as the kernels see it, how rays are traced and
// counted, which shading kernels run; and what the loop adds up for the call's statistics (fill_stats).
struct WavefrontRun {
    PathBuffers pb;
    Queues q[2];
    bool mis_mode, timing;
    bool camera_rays = false;   // the batches come from k_generate (agpt_render): a run of sample_group(S) path ids is one pixel's samples
    int count;              // enable_counters, normalised (see use_fast_trace)
    agpt::ShadeVariant shade;
    uint64_t iterations = 0, launches = 0;
};

static int begin_wavefront(agpt_ctx* c, const agpt_scene* s, int enable_counters, bool timing, WavefrontRun& run) {
#define X(T, name) run.pb.name = c->name.p;
    AGPT_POOL_BUFFERS(X)
#undef X
    for (int i = 0; i < 2; i++) {
        Queues& q = run.q[i];
        q.ext = c->q[i][0].p; q.mis = c->q[i][1].p; q.shadow = c->q[i][2].p;
        q.counts = c->qcounts.p + AGPT_NQUEUES * AGPT_QSTRIDE * i;
    }
    run.count = enable_counters == 2 ? 2 : (enable_counters != 0 ? 1 : 0);
    run.mis_mode = use_fast_trace(c, s->dev, run.count) && !c->mis_closest;
    run.timing = timing;
    run.shade = shade_variant_of(s);
    c->tev_used = 0;
    c->tev_kind.clear();
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, sizeof(DevCounters), c->stream));
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    return AGPT_OK;
}

// the part of RenderConsts that the wavefront loop's kernels read
static void set_wavefront_consts(RenderConsts& rc, const WavefrontRun& run, int max_depth, bool trace_all_rays) {
    rc.max_depth = max_depth;
    rc.mis_mode = run.mis_mode ? 1 : 0;
    rc.answer_rays = (run.mis_mode && !trace_all_rays) ? 1 : 0;
}

// The wavefront loop of PathTracer::Li (integrator.h:124-191) over the paths k_generate / k_generate_li have set up in q[0]:
// per iteration the three trace launches and k_shade.  A path needs at most max_depth + 2 iterations unless it crosses emitter
// spheres (pass-through re-casts do not count as bounces, integrator.h:152-161): that many run without a host round trip, then the
// loop keeps going while any of the three queues is non-empty -- an ended path's last shadow ray and MIS query have to be traced
// before the batch is finished (finished_radiance, agpt_shade_kernels.h, reads their answers).
static int run_wavefront(agpt_ctx* c, agpt_scene* s, const RenderConsts& rcn, WavefrontRun& run) {
    const int count = run.count;
    const PathBuffers& pb = run.pb;
    Queues* const q = run.q;
    const int shade_grid = c->num_cus * c->shade_blocks_per_cu;
    const bool small_batch = (unsigned long long)rcn.NP * (unsigned long long)rcn.S < c->small_batch_paths;
    const bool recast = !getenv("AGPT_NO_RECAST");   // (developer knob: emitter pass-throughs through k_shade, an iteration each)
    // iteration 0 of an agpt_render batch at a sample group of 64: every wave of the closest-hit launch traces one pixel's camera rays
    // (k_trace_fast<COH>); AGPT_NO_COHERENT (developer knob) keeps the ordinary instantiation
    const bool coherent = run.camera_rays && sample_group(rcn.S) == 64 && use_fast_trace(c, s->dev, count) && s->dev.n_prims <= 64 &&
                          count == 0 && !getenv("AGPT_NO_COHERENT");
    // side streams: not where the launches share scratch buffers (the HBM stack spill of deep BVHs, the candidate words of long
    // lists), nor with the reference-order kernels
    const bool side = (c->multi_stream == 2 || (c->multi_stream == 1 && small_batch)) && use_fast_trace(c, s->dev, count) &&
                      s->dev.max_depth <= AGPT_FAST_STACK && s->dev.n_prims <= 64;
    // AGPT_MULTI_STREAM: the three trace launches of an iteration are independent -- MIS and shadow rays on streams of their own,
    // beside the closest-hit launch
    const hipStream_t main_stream = c->stream, mis_stream = side ? c->aux_stream[0] : main_stream,
                      shadow_stream = side ? c->aux_stream[1] : main_stream;
    int cur = 0;
    const int planned = rcn.max_depth + 2;
    for (int it = 0;; it++) {
        if (it >= planned) {
            // Termination check, one iteration behind: this iteration's queue counters (ext, mis and shadow) are copied out
            // asynchronously, and what is looked at is the copy made an iteration ago, which has
            // arrived by now -- the stream never waits for the host (a synchronous check left it idle for ~50 us per iteration,
            // and the iterations out here are a few hundred microseconds long).  The price is one iteration of launches over
            // empty queues at the very end (the kernels return at once on those).
            uint32_t* slot = c->host_pinned + (it & 1) * (AGPT_NQUEUES * AGPT_QSTRIDE);
            HIP_TRY(hipMemcpyAsync(slot, q[cur].counts, ((AGPT_NQUEUES - 1) * AGPT_QSTRIDE + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, main_stream));
            HIP_TRY(hipEventRecord(c->ev[2 + (it & 1)], main_stream));
            if (it > planned) {
                const uint32_t* seen = c->host_pinned + ((it - 1) & 1) * (AGPT_NQUEUES * AGPT_QSTRIDE);
                HIP_TRY(hipEventSynchronize(c->ev[2 + ((it - 1) & 1)]));
                if (seen[0] == 0 && seen[AGPT_QSTRIDE] == 0 && seen[2 * AGPT_QSTRIDE] == 0) break;
            }
            if (it > 4096) return fail(AGPT_ERR_LIMIT, "agpt: path did not terminate");
        }
        const int nxt = cur ^ 1;
        HIP_TRY(hipMemsetAsync(q[nxt].counts, 0, AGPT_NQUEUES * AGPT_QSTRIDE * sizeof(uint32_t), main_stream));
        HIP_TRY(hipMemsetAsync(c->work.p, 0, 4 * AGPT_FRONTIERS * AGPT_QSTRIDE * sizeof(uint32_t), main_stream));
        // the launches' work heads and k_shade's tile heads, zeroed above
        uint32_t* const heads[4] = {c->work.p, c->work.p + AGPT_FRONTIERS * AGPT_QSTRIDE, c->work.p + 2 * AGPT_FRONTIERS * AGPT_QSTRIDE,
                                    c->work.p + 3 * AGPT_FRONTIERS * AGPT_QSTRIDE};
        // (the closest-hit launch over the continuation rays may re-cast in place, see k_trace_fast)
        const TraceLaunch ext{main_stream, q[cur].ext, &QCOUNT(q[cur], 0), 0, heads[0], pb.ext_o, pb.ext_d, pb.hit, nullptr,
                              count, small_batch, recast, coherent && it == 0};
        const TraceLaunch mis{mis_stream, q[cur].mis, &QCOUNT(q[cur], 1), 0, heads[1], pb.mis_o, pb.mis_d,
                              run.mis_mode ? nullptr : pb.mis_hit, run.mis_mode ? pb.mis_ok : nullptr, count, small_batch, false, false};
        const TraceLaunch shadow{shadow_stream, q[cur].shadow, &QCOUNT(q[cur], 2), 0, heads[2], pb.sh_o, pb.sh_d, nullptr, pb.occluded,
                                 count, small_batch, false, false};
        auto trace_ext = [&]() { launch_trace_timed(c, 0, run.timing, 0, s->dev, ext); };
        auto trace_mis = [&]() { launch_trace_timed(c, run.mis_mode ? 2 : 0, run.timing, 1, s->dev, mis); };
        auto trace_shadow = [&]() { launch_trace_timed(c, 1, run.timing, 2, s->dev, shadow); };
        if (side) {
            HIP_TRY(hipEventRecord(c->aux_ev[0], main_stream));
            HIP_TRY(hipStreamWaitEvent(mis_stream, c->aux_ev[0], 0));
            HIP_TRY(hipStreamWaitEvent(shadow_stream, c->aux_ev[0], 0));
            trace_mis();
            HIP_TRY(hipEventRecord(c->aux_ev[1], mis_stream));
            trace_shadow();
            HIP_TRY(hipEventRecord(c->aux_ev[2], shadow_stream));
            trace_ext();
            HIP_TRY(hipStreamWaitEvent(main_stream, c->aux_ev[1], 0));
            HIP_TRY(hipStreamWaitEvent(main_stream, c->aux_ev[2], 0));
        } else {
            trace_ext();
            trace_mis();
            trace_shadow();
        }
        agpt::launch_shading(main_stream, run.shade, shade_grid, s->dev, rcn, pb, q[cur], q[nxt], c->counters.p, heads[3]);
        cur = nxt;
        run.iterations++;
        run.launches += 3;
    }
    return AGPT_OK;
}

static void read_counters(const DevCounters& d, agpt_stats* st) {
    st->closest_rays = d.closest_rays;
    st->anyhit_rays = d.anyhit_rays;
    st->interior_visits = d.interior;
    st->root_tests = d.roots;
    st->tri_tests = d.tris;
    st->shaded_vertices = d.shaded;
    st->outliers = d.outliers;
    st->samples = d.samples;
    st->answered_rays = d.answered;
}

// Closes what begin_wavefront opened: the asynchronous errors of the work the call enqueued are reported here.
static int end_wavefront(agpt_ctx* c) {
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(c->take_deferred());
    return AGPT_OK;
}

// DevCounters, the run and the events -> agpt_stats, after end_wavefront (waits for the stream; nothing to do without `stats`)
static int fill_stats(agpt_ctx* c, const WavefrontRun& run, uint64_t samples, agpt_stats* stats) {
    if (!stats) return AGPT_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memset(stats, 0, sizeof(*stats));
    DevCounters dc;
    HIP_TRY(hipMemcpy(&dc, c->counters.p, sizeof(dc), hipMemcpyDeviceToHost));
    read_counters(dc, stats);
#ifdef AGPT_SHADE_CLOCK
    {
        const double tot = (double)dc.dbg[55];
        static const char* names[8] = {"record loads", "resolve pending", "surface", "emission/termination", "BSDF set-up + light sampling",
                                       "evaluations + ray stores", "final stores", "queue appends + barriers"};
        std::fprintf(stderr, "[shade clock] wave-cycles %.4g:", tot);
        for (int k = 0; k < 8; ++k) std::fprintf(stderr, "  %s %.1f%%", names[k], 100. * dc.dbg[56 + k] / tot);
        std::fprintf(stderr, "\n");
    }
#endif
#ifdef AGPT_TRACE_STATS
    for (int mode = 0; mode < 4; ++mode) {   // (3: the coherent closest-hit launch, counted apart from the other mode-0 launches)
        const unsigned long long* d = dc.dbg + (mode < 3 ? 16 * mode : AGPT_DBG_COH);
        const double steps = (double)(d[0] + d[1] + d[2]);
        if (steps == 0) continue;
        if (mode == 3)
            std::fprintf(stderr, "[trace stats mode 3] scalar path: B %.3g of %.3g wave-steps (%.1f%%), %.3g of %.3g lane-steps (%.1f%%);  "
                         "C %.3g of %.3g wave-steps (%.1f%%), %.3g of %.3g lane-steps (%.1f%%)\n",
                         (double)d[16], (double)d[1], d[1] ? 100. * d[16] / d[1] : 0., (double)d[18], (double)d[4], d[4] ? 100. * d[18] / d[4] : 0.,
                         (double)d[17], (double)d[2], d[2] ? 100. * d[17] / d[2] : 0., (double)d[19], (double)d[5], d[5] ? 100. * d[19] / d[5] : 0.);
        std::fprintf(stderr,
                     "[trace stats mode %d] steps A/B/C %.3g/%.3g/%.3g (%.1f%%/%.1f%%/%.1f%%)  lanes per step A %.1f B %.1f C %.1f  "
                     "active lanes per step %.1f  refills %.3g (%.1f lanes each)  prefilter batches %.3g\n", mode,
                     (double)d[0], (double)d[1], (double)d[2], 100 * d[0] / steps, 100 * d[1] / steps, 100 * d[2] / steps,
                     d[0] ? (double)d[3] / d[0] : 0., d[1] ? (double)d[4] / d[1] : 0., d[2] ? (double)d[5] / d[2] : 0.,
                     (double)d[6] / steps, (double)d[7], d[7] ? (double)d[8] / d[7] : 0., (double)d[9]);
#ifndef AGPT_TRACE_CLOCK
        std::fprintf(stderr, "[trace stats mode %d] root-pair lane-steps %.4g (%.2f%% of B lane-steps), root box passes on %.4g of them (%.2f%%)\n", mode,
                     (double)d[15], d[4] ? 100. * d[15] / d[4] : 0., (double)dc.dbg[AGPT_DBG_ROOT_PASS + mode], d[15] ? 100. * dc.dbg[AGPT_DBG_ROOT_PASS + mode] / d[15] : 0.);
        std::fprintf(stderr, "[trace stats mode %d] stack pushes %.3g: to depth > 4 %.2f%%  > 6 %.3f%%  > 8 %.4f%%  > 12 %.5f%%\n", mode, (double)d[10],
                     d[10] ? 100. * d[11] / d[10] : 0., d[10] ? 100. * d[12] / d[10] : 0., d[10] ? 100. * d[13] / d[10] : 0.,
                     d[10] ? 100. * d[14] / d[10] : 0.);
#endif
#ifdef AGPT_TRACE_CLOCK
        const double tot = (double)dc.dbg[48 + mode];
        std::fprintf(stderr,
                     "[trace clock mode %d] wave-cycles %.4g: refill %.1f%%  vote %.1f%%  B %.1f%% (of which load wait %.1f%%)  C %.1f%%  A %.1f%%;"
                     "  cycles per step: B %.0f (wait %.0f)  C %.0f  A %.0f  vote %.0f; per refill %.0f\n", mode, tot,
                     100 * d[10] / tot, 100 * d[11] / tot, 100 * d[13] / tot, 100 * d[12] / tot, 100 * d[14] / tot, 100 * d[15] / tot,
                     d[1] ? (double)d[13] / d[1] : 0., d[1] ? (double)d[12] / d[1] : 0., d[2] ? (double)d[14] / d[2] : 0.,
                     d[0] ? (double)d[15] / d[0] : 0., (double)d[11] / steps, d[7] ? (double)d[10] / d[7] : 0.);
#endif
    }
#endif
    stats->samples = samples;
    stats->iterations = run.iterations;
    stats->trace_launches = run.launches;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    stats->total_ms = ms;
    if (run.timing) {
        for (size_t i = 0; i + 1 < c->tev_used; i += 2) {
            float t = 0;
            HIP_TRY(hipEventElapsedTime(&t, c->tev[i], c->tev[i + 1]));
            const int kind = c->tev_kind[i / 2];
            stats->trace_ms += t;
            if (kind == 0) stats->ext_ms += t;
            else if (kind == 1) stats->mis_ms += t;
            else stats->shadow_ms += t;
        }
    }
    return AGPT_OK;
}

// ---- what the tile-based entry points (agpt_render, agpt_render_adaptive, agpt_render_features) share ----------------------------
// (`fn` is the entry point that was called: its name opens the message)
static int check_depth(const char* fn, int max_depth) {
    if (max_depth < 0 || max_depth > 200) return fail(AGPT_ERR_INVALID, std::string(fn) + ": max_depth must be in 0 .. 200");
    return AGPT_OK;
}
// film and tile of `rp`
static int check_tile(const char* fn, const agpt_render_params* rp) {
    if (rp->width <= 0 || rp->height <= 0 || rp->w <= 0 || rp->h <= 0 || rp->x0 < 0 || rp->y0 < 0 || rp->x0 + rp->w > rp->width ||
        rp->y0 + rp->h > rp->height || rp->accum_pitch < rp->x0 + rp->w)
        return fail(AGPT_ERR_INVALID, std::string(fn) + ": bad tile / film");
    return AGPT_OK;
}

// rows of the tile this call renders: rp->h, or with the row interleave on this rank's share of the film (which may be empty)
static int tile_rows(const char* fn, const agpt_render_params* rp, uint32_t& rows) {
    rows = (uint32_t)rp->h;
    if (rp->interleave_block <= 0) return AGPT_OK;
    if (rp->interleave_world < 1 || rp->interleave_rank < 0 || rp->interleave_rank >= rp->interleave_world || rp->x0 != 0 ||
        rp->y0 != 0 || rp->w != rp->width || rp->h != rp->height)
        return fail(AGPT_ERR_INVALID, std::string(fn) + ": row interleave needs the whole film as tile and 0 <= rank < world");
    rows = (uint32_t)agpt::interleave_rows(rp->height, rp->interleave_block, rp->interleave_world, rp->interleave_rank);
    return AGPT_OK;
}

// the part of RenderConsts that says where the NP pixels of the tile lie on the film and in the accumulator; the rest is zero
static RenderConsts tile_consts(const agpt_render_params* rp, uint32_t NP) {
    RenderConsts rc{};
    rc.W = rp->width; rc.H = rp->height; rc.x0 = rp->x0; rc.y0 = rp->y0; rc.w = rp->w; rc.h = rp->h;
    rc.accum_pitch = rp->accum_pitch; rc.accum_row0 = rp->accum_row0; rc.NP = NP;
    rc.il_block = rp->interleave_block; rc.il_world = rp->interleave_world; rc.il_rank = rp->interleave_rank;
    return rc;
}

// paths of a renderer's default batch: up to 128 Mi (27 GB of path state -- MI355X has 288 GB); fewer, larger wavefront launches
static uint64_t samples_per_batch(const agpt_render_params* rp, uint32_t NP) {
    return rp->samples_per_batch > 0 ? (uint64_t)rp->samples_per_batch : std::max<uint64_t>(1, (128ull << 20) / NP);
}

// n rays in ext_o / ext_d -> hit / occluded, one launch outside the wavefront loop (agpt_intersect_device, agpt_render_features)
static void trace_rays(agpt_ctx* c, int mode, const DevScene& sc, uint32_t n, int count) {
    const TraceLaunch t{c->stream, nullptr, nullptr, n, c->work.p, c->ext_o.p, c->ext_d.p, c->hit.p, c->occluded.p,
                        count, (unsigned long long)n < c->small_batch_paths, false, false};
    launch_trace(c, mode, sc, t);
}

int agpt_intersect_device(agpt_scene* s, const agpt_ray* d_rays, int n, agpt_hit* d_out, int any_hit, agpt_stats* stats) {
    if (!s || !d_rays || !d_out || n < 0) return fail(AGPT_ERR_INVALID, "agpt_intersect_device: bad argument");
    if (!s->committed) return fail(AGPT_ERR_INVALID, "agpt_intersect_device: scene not committed");
    if (n == 0) return AGPT_OK;
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_pool(c, (size_t)n, s->dev.n_prims);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, sizeof(DevCounters), c->stream));
    HIP_TRY(hipMemsetAsync(c->work.p, 0, AGPT_FRONTIERS * AGPT_QSTRIDE * sizeof(uint32_t), c->stream));
    const dim3 blocks = agpt_blocks((uint64_t)n);
    hipLaunchKernelGGL(k_prepare_rays, blocks, dim3(AGPT_BLOCK), 0, c->stream, d_rays, n, c->ext_o.p, c->ext_d.p);
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    // stats requested -> the instrumented reference-order kernel (work counters); AGPT_INTERSECT_TIMING=1 (developer knob)
    // keeps the production kernel so that stats->trace_ms times it
    const int instrumented = (stats != nullptr && !getenv("AGPT_INTERSECT_TIMING")) ? 1 : 0;
    trace_rays(c, any_hit ? 1 : 0, s->dev, (uint32_t)n, instrumented);
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    hipLaunchKernelGGL(k_export_hits, blocks, dim3(AGPT_BLOCK), 0, c->stream, s->dev, c->hit.p, c->occluded.p, n, any_hit,
                       d_out);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(c->take_deferred());
    WavefrontRun one{};   // no loop: one launch between ev[0] and ev[1], and no samples
    one.launches = 1;
    if ((rc = fill_stats(c, one, 0, stats))) return rc;
    if (stats) stats->trace_ms = stats->total_ms;
    return AGPT_OK;
}

int agpt_intersect_batch(agpt_scene* s, const agpt_ray* rays, int n, agpt_hit* out, int any_hit, agpt_stats* stats) {
    if (!s || !rays || !out || n < 0) return fail(AGPT_ERR_INVALID, "agpt_intersect_batch: bad argument");
    if (!s->committed) return fail(AGPT_ERR_INVALID, "agpt_intersect_batch: scene not committed");
    if (n == 0) return AGPT_OK;
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<agpt_ray> d_rays;
    DevBuf<agpt_hit> d_out;
    if (d_rays.alloc((size_t)n) != hipSuccess || d_out.alloc((size_t)n) != hipSuccess)
        return fail(AGPT_ERR_NOMEM, "agpt_intersect_batch: out of device memory");
    HIP_TRY(hipMemcpyAsync(d_rays.p, rays, (size_t)n * sizeof(agpt_ray), hipMemcpyHostToDevice, c->stream));
    int rc = agpt_intersect_device(s, d_rays.p, n, d_out.p, any_hit, stats);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, d_out.p, (size_t)n * sizeof(agpt_hit), hipMemcpyDeviceToHost));
    return AGPT_OK;
}

int agpt_render(agpt_scene* s, const agpt_render_params* rp, float* accum_dev, agpt_stats* stats) {
    if (!s || !rp || !accum_dev) return fail(AGPT_ERR_INVALID, "agpt_render: NULL argument");
    if (!s->committed || !s->has_camera) return fail(AGPT_ERR_INVALID, "agpt_render: scene not committed or camera not set");
    int rc;
    if ((rc = check_tile("agpt_render", rp)) || (rc = check_depth("agpt_render", rp->max_depth))) return rc;
    if (rp->spp_count < 0) return fail(AGPT_ERR_INVALID, "agpt_render: bad sample range");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t rows;
    if ((rc = tile_rows("agpt_render", rp, rows))) return rc;
    if (rows == 0) return AGPT_OK;   // (a rank that owns no rows)
    const uint32_t NP = (uint32_t)rp->w * rows;
    uint64_t batch = std::min<uint64_t>(samples_per_batch(rp, NP), (uint64_t)std::max(1, rp->spp_count));
    if ((uint64_t)NP * batch > 0x7FFFFFFFull) return fail(AGPT_ERR_LIMIT, "agpt_render: batch too large");
    if ((rc = fit_pool(c, s, NP, batch))) return rc;
    const int S = (int)batch;
    s->dev.cam = s->cam;

    WavefrontRun run;
    if ((rc = begin_wavefront(c, s, rp->enable_counters, rp->enable_timing != 0 && stats != nullptr, run))) return rc;
    RenderConsts rcn = tile_consts(rp, NP);
    rcn.seed_base = rp->seed_base;
    set_wavefront_consts(rcn, run, rp->max_depth, rp->trace_all_rays != 0);
    run.camera_rays = true;
    for (int s0 = rp->spp_begin; s0 < rp->spp_begin + rp->spp_count; s0 += S) {
        rcn.s0 = s0;
        rcn.S = std::min(S, rp->spp_begin + rp->spp_count - s0);
        const uint32_t total = NP * (uint32_t)rcn.S;
        hipLaunchKernelGGL(k_generate, agpt_blocks(total), dim3(AGPT_BLOCK), 0, c->stream, s->dev, rcn, run.pb,
                           run.q[0]);
        if ((rc = run_wavefront(c, s, rcn, run))) return rc;
        agpt::launch_accumulate(c->stream, run.shade.fast, s->dev, rcn, run.pb, (float4*)accum_dev, c->counters.p);
    }
    if ((rc = end_wavefront(c))) return rc;
    return fill_stats(c, run, (uint64_t)NP * (uint64_t)rp->spp_count, stats);
}

// Rounds of: the decision (k_adaptive_select + k_adaptive_compact over the tile, one read-back of the active count), then wavefront
// batches over the active list (k_generate_list -> run_wavefront -> k_accumulate_list) in chunks of whole pixels.
int agpt_render_adaptive(agpt_scene* s, const agpt_render_params* rp, const agpt_adaptive_params* ap, float* accum_dev,
                         float* moment2_dev, agpt_stats* stats, agpt_adaptive_stats* astats) {
    if (!s || !rp || !ap || !accum_dev || !moment2_dev) return fail(AGPT_ERR_INVALID, "agpt_render_adaptive: NULL argument");
    if (!s->committed || !s->has_camera) return fail(AGPT_ERR_INVALID, "agpt_render_adaptive: scene not committed or camera not set");
    int rc;
    if ((rc = check_tile("agpt_render_adaptive", rp)) || (rc = check_depth("agpt_render_adaptive", rp->max_depth))) return rc;
    if (rp->spp_begin != 0 || rp->spp_count != 0)
        return fail(AGPT_ERR_INVALID, "agpt_render_adaptive: spp_begin and spp_count must be 0 (the counts are in accum.w)");
    const int step = ap->step_spp, min_spp = ap->min_spp, max_spp = ap->max_spp;
    if (step < 1 || min_spp < 2 || min_spp > max_spp || max_spp > (1 << 24) || min_spp % step != 0 || max_spp % step != 0 ||
        !(ap->abs_floor >= 0.f) || ap->rel_error != ap->rel_error)
        return fail(AGPT_ERR_INVALID, "agpt_render_adaptive: need 1 <= step_spp, 2 <= min_spp <= max_spp <= 2^24, both multiples of "
                                      "step_spp, abs_floor >= 0, rel_error not NaN");
    if (astats) std::memset(astats, 0, sizeof(*astats));
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t rows;
    if ((rc = tile_rows("agpt_render_adaptive", rp, rows))) return rc;
    if (rows == 0) return AGPT_OK;
    const uint32_t NP = (uint32_t)rp->w * rows;
    // paths of one wavefront batch: at most w * rows * samples_per_batch (agpt_render's default), and no more than the largest batch a
    // call can run (the whole tile at max(step_spp, min_spp) samples); then kept within free memory as agpt_render
    uint64_t cap = std::min<uint64_t>((uint64_t)NP * samples_per_batch(rp, NP), (uint64_t)NP * (uint64_t)std::max(step, min_spp));
    if (cap > 0x7FFFFFFFull) return fail(AGPT_ERR_LIMIT, "agpt_render_adaptive: batch too large");
    if ((rc = fit_pool(c, s, 1, cap))) return rc;
    const uint32_t n_blocks = (NP + AGPT_ADAPT_BLOCK_PIXELS - 1) / AGPT_ADAPT_BLOCK_PIXELS;
    if ((rc = c->adapt_masks.ensure((size_t)n_blocks * AGPT_BLOCK)) || (rc = c->adapt_blocks.ensure(n_blocks)) ||
        (rc = c->adapt_list.ensure(NP)) || (rc = c->adapt_words.ensure(AGPT_AW_COUNT)))
        return rc;
    s->dev.cam = s->cam;

    WavefrontRun run;
    if ((rc = begin_wavefront(c, s, rp->enable_counters, rp->enable_timing != 0 && stats != nullptr, run))) return rc;
    RenderConsts base = tile_consts(rp, NP);
    base.seed_base = rp->seed_base;
    set_wavefront_consts(base, run, rp->max_depth, rp->trace_all_rays != 0);
    AdaptiveConsts ac;
    ac.min_spp = min_spp; ac.max_spp = max_spp; ac.step_spp = step; ac.rel_error = ap->rel_error; ac.abs_floor = ap->abs_floor;
    float4* const accum = (float4*)accum_dev;
    uint64_t samples = 0;

    // `spp` more samples for each of the na pixels list[0 .. na) (list NULL: the local pixels 0 .. na): batches of at most cap paths,
    // split into chunks of whole pixels, and a pixel's samples into several batches only if cap < spp.  Each batch reads the
    // pixels' counts afresh (k_generate_list), so the samples stay in order.
    auto add_samples = [&](const uint32_t* list, uint32_t na, uint32_t spp) -> int {
        const uint32_t S = (uint32_t)std::min<uint64_t>(spp, cap);
        const uint32_t per_chunk = (uint32_t)std::min<uint64_t>(na, cap / S);
        for (uint32_t done = 0; done < spp; done += S) {
            RenderConsts rcg = base;
            rcg.S = (int32_t)std::min(S, spp - done);
            for (uint32_t a0 = 0; a0 < na; a0 += per_chunk) {
                const uint32_t nc = std::min(per_chunk, na - a0);
                agpt::launch_generate_list(c->stream, s->dev, rcg, list, a0, nc, accum, run.pb, run.q[0]);
                RenderConsts rcw = rcg;
                rcw.NP = nc;   // (run_wavefront reads NP * S only to pick the small-batch trace kernels: the batch's real path count)
                if (const int rc_run = run_wavefront(c, s, rcw, run)) return rc_run;
                agpt::launch_finish_paths(c->stream, run.shade.fast, s->dev, rcg, run.pb, nc * (uint32_t)rcg.S);
                agpt::launch_accumulate_list(c->stream, rcg, list, a0, nc, run.pb, accum, moment2_dev, c->counters.p);
            }
        }
        samples += (uint64_t)na * spp;
        return AGPT_OK;
    };

    int rounds = 0;
    uint32_t active_last = 0, stopped = 0;
    for (;;) {
        uint32_t* const words = c->adapt_words.p;
        HIP_TRY(hipMemsetAsync(words, 0, AGPT_AW_COUNT * sizeof(uint32_t), c->stream));
        agpt::launch_adaptive_select(c->stream, base, ac, accum, moment2_dev, c->adapt_masks.p, c->adapt_blocks.p, words);
        agpt::launch_adaptive_compact(c->stream, NP, c->adapt_masks.p, c->adapt_blocks.p, c->adapt_list.p, words);
        HIP_TRY(hipGetLastError());
        uint32_t w[AGPT_AW_COUNT];
        HIP_TRY(hipMemcpyAsync(w, words, sizeof(w), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (w[AGPT_AW_INVALID]) {
            (void)c->take_deferred();
            return fail(AGPT_ERR_INVALID, "agpt_render_adaptive: " + std::to_string(w[AGPT_AW_INVALID]) +
                                              " tile pixels hold a count (accum.w) that is not a multiple of step_spp in [0, 2^24]");
        }
        const uint32_t na = w[AGPT_AW_ACTIVE];
        if (na == 0) {
            stopped = w[AGPT_AW_STOPPED];
            break;
        }
        // every round adds step_spp to each active pixel and a pixel at max_spp is never active: max_spp / step_spp rounds at most
        if (++rounds > max_spp / step + 1) return fail(AGPT_ERR_LIMIT, "agpt_render_adaptive: rounds did not end");
        const uint32_t n_min = ~w[AGPT_AW_INV_MIN], n_max = w[AGPT_AW_MAX];
        // every pixel at the same n < min_spp (a fresh frame): no decision falls before min_spp -- one full-tile warm-up batch
        const int rc_add = (n_min == n_max && n_min < (uint32_t)min_spp) ? add_samples(nullptr, NP, (uint32_t)min_spp - n_min)
                                                                          : add_samples(c->adapt_list.p, na, (uint32_t)step);
        if (rc_add) return rc_add;
        active_last = na;
    }
    if ((rc = end_wavefront(c))) return rc;
    if (astats) {
        astats->rounds = rounds;
        astats->active_last = (int32_t)active_last;
        astats->samples = samples;
        astats->pixels_stopped = stopped;
    }
    return fill_stats(c, run, samples, stats);
}

// One closest-hit query per tile pixel through the pixel centre (k_feature_rays -> the trace launch of agpt_intersect_device), then
// k_features: material colour + flag and shading normal + t.  motion (agpt_render_features_motion, `fn` names the entry point that was
// called): k_motion then reads the same hits and rays into prev_point_dev.  surfaces (agpt_render_features_surface_motion): k_motion runs
// first and the feature kernel's PREV sibling reads its prev_point and the older tri_shade generation into prev_normal_dev.
static int render_features(const char* fn, bool motion, bool surfaces, agpt_scene* s, const agpt_render_params* rp, float* albedo_dev,
                           float* normal_depth_dev, float* prev_point_dev, float* prev_normal_dev) {
    const std::string f(fn);
    if (!rp) return fail(AGPT_ERR_INVALID, f + ": NULL argument");
    if (rp->spp_begin != 0 || rp->spp_count != 0)
        return fail(AGPT_ERR_INVALID, f + ": spp_begin and spp_count must be 0 (one unjittered ray per pixel)");
    if (rp->interleave_block != 0 || rp->interleave_world != 0 || rp->interleave_rank != 0)
        return fail(AGPT_ERR_INVALID, f + ": the interleave fields must be 0");
    if (!s || !albedo_dev || !normal_depth_dev) return fail(AGPT_ERR_INVALID, f + ": NULL argument");
    if (!s->committed || !s->has_camera) return fail(AGPT_ERR_INVALID, f + ": scene not committed or camera not set");
    int rc;
    if ((rc = check_tile(fn, rp))) return rc;
    if (albedo_dev == normal_depth_dev) return fail(AGPT_ERR_INVALID, f + ": the two outputs are one buffer");
    if (motion) {
        if (!prev_point_dev) return fail(AGPT_ERR_INVALID, f + ": NULL prev_point_dev");
        if (prev_point_dev == albedo_dev || prev_point_dev == normal_depth_dev)
            return fail(AGPT_ERR_INVALID, f + ": prev_point_dev aliases another output");
        if (!s->snapshots.valid)
            return fail(AGPT_ERR_INVALID, f + ": no position snapshot yet (agpt_scene_snapshot_positions comes first)");
    }
    if (surfaces) {
        if (!prev_normal_dev) return fail(AGPT_ERR_INVALID, f + ": NULL prev_normal_dev");
        if (prev_normal_dev == albedo_dev || prev_normal_dev == normal_depth_dev || prev_normal_dev == prev_point_dev)
            return fail(AGPT_ERR_INVALID, f + ": prev_normal_dev aliases another output");
        if (!s->snapshots.surfaces)
            return fail(AGPT_ERR_INVALID, f + ": no generations of the shading records (agpt_scene_snapshot_surfaces comes first)");
    }
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t np64 = (uint64_t)rp->w * (uint64_t)rp->h;
    if (np64 > 0x7FFFFFFFull) return fail(AGPT_ERR_LIMIT, f + ": tile too large");
    const uint32_t NP = (uint32_t)np64;
    if ((rc = ensure_pool(c, (size_t)NP, s->dev.n_prims))) return rc;
    s->dev.cam = s->cam;
    const RenderConsts rcn = tile_consts(rp, NP);   // (the interleave fields are 0)
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, sizeof(DevCounters), c->stream));
    HIP_TRY(hipMemsetAsync(c->work.p, 0, AGPT_FRONTIERS * AGPT_QSTRIDE * sizeof(uint32_t), c->stream));
    agpt::launch_feature_rays(c->stream, s->dev, rcn, c->ext_o.p, c->ext_d.p);
    trace_rays(c, 0, s->dev, NP, 0);
    const agpt_scene::PositionSnapshots& ps = s->snapshots;
    if (!surfaces)
        agpt::launch_features(c->stream, s->dev, s->shade_level, rcn, s->d_colors.p, c->hit.p, c->ext_o.p, c->ext_d.p, (float4*)albedo_dev,
                              (float4*)normal_depth_dev);
    if (motion)
        agpt::launch_motion(c->stream, rcn, c->hit.p, c->ext_o.p, c->ext_d.p, ps.gen[ps.newest ^ 1].p, ps.gen[ps.newest].p, (uint32_t)ps.n_tris,
                            ps.analytic[ps.newest ^ 1].p, ps.analytic[ps.newest].p, (uint32_t)ps.n_prims, (float4*)prev_point_dev);
    if (surfaces)
        agpt::launch_features_prev(c->stream, s->dev, s->shade_level, rcn, s->d_colors.p, c->hit.p, c->ext_o.p, c->ext_d.p, (float4*)albedo_dev,
                                   (float4*)normal_depth_dev, ps.shade[ps.newest ^ 1].p, (const float4*)prev_point_dev,
                                   (float4*)prev_normal_dev);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(c->take_deferred());
    return AGPT_OK;
}

int agpt_render_features(agpt_scene* s, const agpt_render_params* rp, float* albedo_dev, float* normal_depth_dev) {
    return render_features("agpt_render_features", false, false, s, rp, albedo_dev, normal_depth_dev, nullptr, nullptr);
}

int agpt_render_features_motion(agpt_scene* s, const agpt_render_params* rp, float* albedo_dev, float* normal_depth_dev, float* prev_point_dev) {
    return render_features("agpt_render_features_motion", true, false, s, rp, albedo_dev, normal_depth_dev, prev_point_dev, nullptr);
}

int agpt_render_features_surface_motion(agpt_scene* s, const agpt_render_params* rp, float* albedo_dev, float* normal_depth_dev,
                                        float* prev_point_dev, float* prev_normal_dev) {
    return render_features("agpt_render_features_surface_motion", true, true, s, rp, albedo_dev, normal_depth_dev, prev_point_dev,
                           prev_normal_dev);
}

int agpt_li_batch(agpt_scene* s, const agpt_ray* rays, const uint32_t* rng_states, int n, int max_depth, float* radiance3_out,
                  uint32_t* rng_states_out, agpt_stats* stats) {
    if (!s || !rays || !rng_states || !radiance3_out || n < 0 || max_depth < 0 || max_depth > 200)
        return fail(AGPT_ERR_INVALID, "agpt_li_batch: bad argument");
    if (!s->committed) return fail(AGPT_ERR_INVALID, "agpt_li_batch: scene not committed");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return AGPT_OK;
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<agpt_ray> d_rays;
    DevBuf<uint32_t> d_rng;
    DevBuf<float> d_out;
    if (d_rays.alloc((size_t)n) != hipSuccess || d_rng.alloc((size_t)n) != hipSuccess || d_out.alloc(3 * (size_t)n) != hipSuccess)
        return fail(AGPT_ERR_NOMEM, "agpt_li_batch: out of device memory");
    HIP_TRY(hipMemcpyAsync(d_rays.p, rays, (size_t)n * sizeof(agpt_ray), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_rng.p, rng_states, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    int rc = ensure_pool(c, (size_t)n, s->dev.n_prims);
    if (rc) return rc;
    // counters off, no timing; every answerable ray query is answered (no trace_all_rays here); NP = S = 0 in the constants, so the
    // trace launches are the small-batch ones whatever n is
    WavefrontRun run;
    if ((rc = begin_wavefront(c, s, 0, false, run))) return rc;
    RenderConsts rcn{};
    set_wavefront_consts(rcn, run, max_depth, false);
    const dim3 grid = agpt_blocks((uint64_t)n), block(AGPT_BLOCK);
    hipLaunchKernelGGL(k_generate_li, grid, block, 0, c->stream, (const agpt_ray*)d_rays.p, (const uint32_t*)d_rng.p, (uint32_t)n, run.pb,
                       run.q[0], max_depth);
    if ((rc = run_wavefront(c, s, rcn, run))) return rc;
    agpt::launch_export_li(c->stream, run.shade.fast, s->dev, rcn, run.pb, (uint32_t)n, d_out.p, rng_states_out ? d_rng.p : (uint32_t*)nullptr);
    if ((rc = end_wavefront(c))) return rc;
    HIP_TRY(hipMemcpyAsync(radiance3_out, d_out.p, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (rng_states_out) HIP_TRY(hipMemcpyAsync(rng_states_out, d_rng.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return fill_stats(c, run, (uint64_t)n, stats);
}

int agpt_resolve(agpt_ctx* c, const float* accum_dev, int n_pixels, int samples, uint32_t* out_rgb) {
    if (!c || !accum_dev || !out_rgb || n_pixels <= 0 || samples <= 0) return fail(AGPT_ERR_INVALID, "agpt_resolve: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> d;
    HIP_TRY(d.alloc((size_t)n_pixels));
    hipLaunchKernelGGL(k_resolve, agpt_blocks((uint64_t)n_pixels), dim3(AGPT_BLOCK), 0, c->stream, (const float4*)accum_dev, n_pixels, samples, d.p);
    HIP_TRY(hipGetLastError());
    if (const int rc = d.out(out_rgb, (size_t)n_pixels, &c->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

}  // extern "C"
