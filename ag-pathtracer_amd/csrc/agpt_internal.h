// agpt_internal.h -- what the units that define the C entry points of include/agpt.h share: error reporting, the owning device
// buffer, and the context and the scene behind the two opaque handles.  Those units are agpt_api.hip (context, pool, wavefront loop,
// renderers; its trace launches go through launch_trace below, agpt_trace_kernels.hip), agpt_scene_api.hip (scene building, commit, host BVH, mesh updates), agpt_kat.hip, agpt_comm.hip, and
// the entry points that sit beside their kernels (agpt_adaptive.hip, agpt_denoise.hip, agpt_temporal.hip, agpt_motion.hip,
// agpt_analytic.hip).  Only .hip / .cpp units include this file, no other header does.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/agpt.h"
#include "agpt_host_scene.hpp"
#include "agpt_update.h"
#include "agpt_wavefront.h"

// LDS stack entries of the production trace kernel (23 KiB of stack + 8 KiB = 31 KiB per block -> five blocks per CU) and the
// blocks per CU that go with it; deeper BVHs spill the entries beyond into agpt_ctx::spill (HBM)
#ifndef AGPT_FAST_STACK
#define AGPT_FAST_STACK 23
#endif
#ifndef AGPT_FAST_BLOCKS_PER_CU
#define AGPT_FAST_BLOCKS_PER_CU 5
#endif
// the `refill` argument of k_trace_fast (agpt_trace_kernels.h): the defaults of agpt_ctx::refill / refill_any
#define AGPT_REFILL 20      // idle lanes that trigger a refill, closest-hit launches (tuned on C3: 16-24 equal)
#define AGPT_REFILL_ANY 40  // same, any-hit / MIS-query launches: short traversals, refills are cheaper in bulk

// The helpers that cross a unit boundary (each defined in agpt_api.hip).
namespace agpt {
// records `msg` as the calling thread's agpt_last_error and returns `code`; the library's other units (agpt_image.cpp, agpt_obj.cpp,
// agpt_bvh_device.hip, agpt_update.hip) declare it themselves
int fail(int code, const std::string& msg);
// film rows of the row blocks k with k % world == rank (blocks of `block` rows, the last one of a film may be shorter)
int interleave_rows(int H, int block, int world, int rank);
}  // namespace agpt

// AGPT_ERR_NOMEM when the runtime says it is out of memory, AGPT_ERR_DEVICE for every other failure
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return agpt::fail(e_ == hipErrorOutOfMemory ? AGPT_ERR_NOMEM : AGPT_ERR_DEVICE,             \
                              std::string(#expr) + ": " + hipGetErrorString(e_));                       \
    } while (0)

// A device allocation that belongs to its holder: freed when the holder goes (a context, a scene, a local of an entry point on
// every return path).  Move-only: std::vector<DevBuf<...>> is resized.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) {
        o.p = nullptr;
        o.n = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~DevBuf() { release(); }
    // exactly `count` elements (at least one), whatever was held before
    hipError_t alloc(size_t count) {
        release();
        const hipError_t e = hipMalloc((void**)&p, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        else p = nullptr;
        return e;
    }
    // at least `count` elements: grows, never shrinks
    int ensure(size_t count) {
        if (count <= n) return AGPT_OK;
        const hipError_t e = alloc(count);
        if (e != hipSuccess) return agpt::fail(AGPT_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        return AGPT_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    // Staging for an entry point that takes host arrays.  in: exactly `count` elements, copied from `host` before the call returns.
    int in(const T* host, size_t count) {
        HIP_TRY(alloc(count));
        HIP_TRY(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
        return AGPT_OK;
    }
    // out: the first `count` elements into `host`, before the call returns or -- `st` given -- as a copy enqueued on that stream
    int out(T* host, size_t count, const hipStream_t* st = nullptr) const {
        if (st) HIP_TRY(hipMemcpyAsync(host, p, count * sizeof(T), hipMemcpyDeviceToHost, *st));
        else HIP_TRY(hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost));
        return AGPT_OK;
    }
};

// The per-path pool, listed once: X(element type, name), the names being PathBuffers' members.  The context's buffers, their
// allocation and release, the binding into PathBuffers and the bytes-per-path figure of the batch-size policy all come from here.
#define AGPT_POOL_BUFFERS(X)                                                                                                  \
    X(float4, ext_o) X(float4, ext_d) X(float4, sh_o) X(float4, sh_d) X(float4, mis_o) X(float4, mis_d) X(float4, beta4)      \
    X(float4, L4) X(float4, fac4) X(float4, c1) X(float4, c2) X(DevHit, hit) X(DevHit, mis_hit) X(uint32_t, occluded)          \
    X(uint32_t, mis_ok)

struct agpt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int num_cus = 256;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t aux_stream[2] = {nullptr, nullptr};   // small batches: the MIS and shadow launches of an iteration run beside the closest-hit one
    hipEvent_t aux_ev[3] = {nullptr, nullptr, nullptr};
    int multi_stream = 0;
    // path-state pool (sized for the largest batch seen): AGPT_POOL_BUFFERS and the path-id queues, one element per path each
    size_t pool_paths = 0;
#define X(T, name) DevBuf<T> name;
    AGPT_POOL_BUFFERS(X)
#undef X
    DevBuf<uint32_t> q[2][AGPT_NQUEUES];
    DevBuf<uint32_t> qcounts;   // 2 x AGPT_NQUEUES queue lengths
    DevBuf<uint32_t> work;      // work-queue heads of the persistent trace launches
    DevBuf<DevCounters> counters;
    uint32_t* host_pinned = nullptr;
    int blocks_per_cu = 4;       // generic trace kernel (32-entry LDS stacks)
    int shade_blocks_per_cu = 8;   // AGPT_SHADE_BLOCKS_PER_CU: k_shade's grid (its waves take wave tiles from work heads)
    int fast_blocks_per_cu = AGPT_FAST_BLOCKS_PER_CU;  // AGPT_BLOCKS_PER_CU: production trace kernel (AGPT_FAST_STACK-entry LDS stacks)
    DevBuf<uint32_t> spill;      // traversal-stack entries beyond the LDS part (BVHs deeper than AGPT_FAST_STACK)
    // primitive lists longer than 64 entries: per-path candidate words written by k_candidates, read by k_trace_fast<LIST>
    DevBuf<unsigned long long> cand_mask;   // [chunk][pool_paths]
    DevBuf<uint32_t> cand_chunks;           // [pool_paths]
    // agpt_render_adaptive: per-thread decision masks and per-block active counts of the select pass, the active list, the words
    // the host reads back each round (agpt_adaptive.h)
    DevBuf<uint32_t> adapt_masks, adapt_blocks, adapt_list, adapt_words;
    DevBuf<float4> denoise_state;   // agpt_denoise: the ping-pong partner of the caller's output buffer
    int refill = AGPT_REFILL;    // AGPT_REFILL: idle lanes that trigger an in-flight refill (closest-hit launches)
    int refill_any = AGPT_REFILL_ANY;  // AGPT_REFILL_ANY: same for the any-hit / MIS-query launches
    bool mis_closest = false;    // AGPT_MIS_CLOSEST=1: trace MIS rays as full closest-hit queries (A/B, tests)
    bool force_generic = false;  // AGPT_FORCE_GENERIC=1: always use the generic k_trace (tests)
    // AGPT_SMALL_BATCH_PATHS=<n>: batches below n paths (rays) run the PEEK instantiation of the trace launches (see k_trace_fast);
    // 0 = none (tests)
    unsigned long long small_batch_paths = 48ull << 20;
    // per-launch HIP-event timing of the trace kernels (agpt_render_params::enable_timing)
    std::vector<hipEvent_t> tev;
    size_t tev_used = 0;
    std::vector<int> tev_kind;  // 0 = closest (continuation), 1 = closest (MIS), 2 = any-hit
    // first error of an asynchronous helper (memset / event record / kernel launch inside the launch helpers); checked and
    // cleared by the entry point that enqueued the work
    hipError_t deferred = hipSuccess;
    void note(hipError_t e) {
        if (e != hipSuccess && deferred == hipSuccess) deferred = e;
    }
    hipError_t take_deferred() {
        const hipError_t e = deferred;
        deferred = hipSuccess;
        return e;
    }
};

// The trace launches (agpt_trace_kernels.hip, the only unit that sees the trace kernels of agpt_trace_kernels.h).
namespace agpt {
// One trace launch, said in full: where it is enqueued, what it reads and writes, and what picks its kernel instantiation.
struct TraceLaunch {
    hipStream_t stream;
    const uint32_t* queue;       // path ids and their number on the device, or (nullptr, nullptr, n): the rays 0 .. n
    const uint32_t* count_ptr;
    uint32_t count_imm;
    uint32_t* work_head;         // the launch's work-queue frontiers in agpt_ctx::work, zeroed by the caller
    float4 *ro, *rd;             // (written only by a re-casting launch)
    DevHit* hits;
    uint32_t* occ;
    int count;                   // see use_fast_trace
    bool small_batch;            // the rays of the batch number fewer than agpt_ctx::small_batch_paths: k_trace_fast<PEEK>
    bool recast;                 // the wavefront loop's own closest-hit launch (its rays carry d.w): may re-cast a ray in place, see
                                 // the retire branch of k_trace_fast
    bool coherent;               // the rays are k_generate's camera rays in sample groups of 64, a pixel per wave: k_trace_fast<COH>
                                 // (run_wavefront says when; no other caller sets it)
};
// count: 0 = off, 1 = reference-order counters (the generic kernel: what the reference's recursion does, equal to the
// oracle's counters), 2 = the production kernel counting its own work (bench.py's roofline)
bool use_fast_trace(const agpt_ctx* c, const DevScene& sc, int count);
// mode 0 closest, 1 any-hit, 2 MIS query (production kernel only; the generic kernel traces MIS rays as closest hits).  Enqueues the
// launch on t.stream; what fails on the way is left in c->note
void launch_trace(agpt_ctx* c, int mode, const DevScene& sc, const TraceLaunch& t);
}  // namespace agpt

struct agpt_scene {
    agpt_ctx* ctx = nullptr;
    std::vector<agpt::HostMesh> meshes;
    std::vector<agpt::HostSphere> spheres;
    std::vector<agpt::HostPrim> prims;
    std::vector<agpt::HostLight> lights;
    std::vector<agpt::HostEnv> envs;
    std::vector<DevMaterial> materials;
    std::vector<float4> colors;   // per material: the colour as given (agpt_render_features' albedo)
    // image textures (agpt_scene_add_texture / agpt_scene_set_material_texture): texels as float4, per material the texture id or -1
    struct HostTexture {
        int width = 0, height = 0;
        int filter = AGPT_FILTER_NEAREST, wrap_u = AGPT_WRAP_REPEAT, wrap_v = AGPT_WRAP_REPEAT;   // agpt_scene_set_texture_sampler
        std::vector<float4> texels;
        bool default_sampler() const { return filter == AGPT_FILTER_NEAREST && wrap_u == AGPT_WRAP_REPEAT && wrap_v == AGPT_WRAP_REPEAT; }
    };
    std::vector<HostTexture> textures;
    std::vector<int32_t> material_texture;
    std::vector<uint32_t> material_param_slots;   // agpt_scene_set_material_param_texture: per material, param_slots_pack (0 = no map)
    // set by agpt_scene_commit: the highest texturing level a material needs -> which shading / feature kernels run (agpt_shade_kernels.h)
    agpt::ShadeLevel shade_level = agpt::SHADE_PLAIN;
    // agpt_scene_set_material_normal_texture: per material the texture id (-1 = no normal map) and the scale
    std::vector<int32_t> material_normal_texture;
    std::vector<float> material_normal_scale;
    DevBuf<float4> d_tri_uv;
    DevBuf<DevTexture> d_textures;
    DevBuf<int32_t> d_material_texture;
    std::vector<DevBuf<float4>> d_texels;
    DevCamera cam{};
    bool has_camera = false;
    bool committed = false;
    int max_depth = 0;
    int bvh_builder = AGPT_BVH_BUILDER_HOST;  // agpt_scene_set_bvh_builder
    int shading_arith = AGPT_SHADING_EXACT;   // agpt_scene_set_shading_arith
    DevBuf<float4> d_nodes, d_tri_verts, d_tri_shade, d_prefilter, d_colors;
    DevBuf<uint32_t> d_toplevel;
    DevBuf<unsigned long long> d_chunk_mesh_masks;
    DevBuf<uint32_t> d_bigleaves;
    DevBuf<DevPrim> d_prims;
    DevBuf<DevMaterial> d_materials;
    DevBuf<DevLight> d_lights;
    DevBuf<DevEnv> d_envs;
    std::vector<DevBuf<float4>> d_env_pixels;
    std::vector<DevBuf<float>> d_env_func, d_env_cdf;
    DevScene dev{};
    // agpt_scene_update_mesh and its front ends: one owner of the update state per mesh, host copies and device cache (agpt_update.h)
    std::vector<agpt::MeshUpdate> updates;
    // agpt_scene_snapshot_positions: two generations of world-space triangle positions, float4[3 * n_tris] each, indexed by the GLOBAL
    // triangle id (not by BVH slot).  Allocated by the first snapshot; gen[newest] is the newer one.  agpt_scene_commit drops them; an
    // AGPT_UPDATE_REBUILD, which re-commits with the triangle ids unchanged, keeps them (update_on_host).
    // analytic[]: the same two generations of the sphere and plane records, two float4 per primitive index (agpt_analytic.h), with the
    // same lifetime; filled from d_prims, so every update route is seen.  Empty for a scene without a sphere or a plane.
    // shade[]: agpt_scene_snapshot_surfaces' two generations of the tri_shade records, float4[4 * n_tris] each, copied from d_tri_shade,
    // flipped with the positions (shade[newest] is the newer one).  surfaces: they are present -- the scene's last snapshot was made by
    // agpt_scene_snapshot_surfaces; agpt_scene_snapshot_positions frees them.  Never allocated for a scene that does not call it.
    struct PositionSnapshots {
        DevBuf<float4> gen[2], analytic[2], shade[2];
        int newest = 0;
        size_t n_tris = 0, n_prims = 0;
        bool valid = false, surfaces = false;
        void drop_surfaces() {
            shade[0].release();
            shade[1].release();
            surfaces = false;
        }
        void drop() {
            for (int g = 0; g < 2; g++) {
                gen[g].release();
                analytic[g].release();
            }
            drop_surfaces();
            n_tris = n_prims = 0;
            valid = false;
        }
    };
    PositionSnapshots snapshots;
    // agpt_scene_update_spheres_device (agpt_analytic.hip): the uploaded id list and k_check_spheres' word, allocated by the first such
    // call.  spheres_stale: `spheres` is behind d_prims (brought up to date by sync_mirror before anything reads it).
    DevBuf<int32_t> d_sphere_ids;
    DevBuf<uint32_t> d_sphere_flag;
    bool spheres_stale = false;
};

// `count` elements of `host` into `buf` (grown if it holds fewer, at least one element) as a copy enqueued on `st`
template <class T>
static int upload(DevBuf<T>& buf, const T* host, size_t count, hipStream_t st) {
    int rc = buf.ensure(count ? count : 1);
    if (rc) return rc;
    if (count) HIP_TRY(hipMemcpyAsync(buf.p, host, count * sizeof(T), hipMemcpyHostToDevice, st));
    return AGPT_OK;
}
template <class T>
static int upload(DevBuf<T>& buf, const std::vector<T>& host, hipStream_t st) {
    return upload(buf, host.data(), host.size(), st);
}
