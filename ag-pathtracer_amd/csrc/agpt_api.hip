// agpt_api.hip -- the C ABI of include/agpt.h on top of the kernels in agpt_kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/agpt.h"
#include "agpt_adaptive.h"
#include "agpt_bvh_device.h"
#include "agpt_denoise.h"
#include "agpt_host_scene.hpp"
#include "agpt_kernels.h"
#include "agpt_temporal.h"
#include "agpt_update.h"

// LDS stack entries of the production trace kernel (23 KiB of stack + 8 KiB = 31 KiB per block -> five blocks per CU) and the
// blocks per CU that go with it; deeper BVHs spill the entries beyond into agpt_ctx::spill (HBM)
#ifndef AGPT_FAST_STACK
#define AGPT_FAST_STACK 23
#endif
#ifndef AGPT_FAST_BLOCKS_PER_CU
#define AGPT_FAST_BLOCKS_PER_CU 5
#endif


namespace {

thread_local std::string g_error;

int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

}  // namespace
namespace agpt {
// error reporting for the library's other translation units (agpt_image.cpp)
int report_error(int code, const std::string& msg) { return fail(code, msg); }
}  // namespace agpt
namespace {

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(AGPT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));           \
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
        if (e != hipSuccess) return fail(AGPT_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        return AGPT_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

}  // namespace

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
    // agpt_scene_update_mesh: per mesh the device path's cache (created by the mesh's first REFIT, agpt_update.h) and whether the
    // bounds of HostMesh::nodes are behind the device's (root box excepted; brought up to date by sync_mirror)
    // arrays_stale: HostMesh::vertices / normals are behind the device's as well (a device-pointer or transform REFIT: the new arrays
    // exist only in the updater); rest: the rest pose of agpt_scene_transform_mesh, a host copy taken by the mesh's first transform
    // after its arrays were last given explicitly (DESIGN.md section 5.7 lists who reads the mirror).
    std::vector<agpt::MeshUpdater*> updaters;
    std::vector<char> bounds_stale, arrays_stale;
    struct RestPose {
        bool valid = false;
        std::vector<v3> vertices, normals;
    };
    std::vector<RestPose> rest;
    ~agpt_scene() {
        for (agpt::MeshUpdater* u : updaters) agpt::mesh_updater_destroy(u);
    }
};

template <class T>
static int upload(DevBuf<T>& buf, const std::vector<T>& host, hipStream_t st) {
    int rc = buf.ensure(host.empty() ? 1 : host.size());
    if (rc) return rc;
    if (!host.empty()) HIP_TRY(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return AGPT_OK;
}

static int trace_grid(const agpt_ctx* c) { return c->num_cus * c->blocks_per_cu; }           // generic kernel
static int fast_grid(const agpt_ctx* c) { return c->num_cus * c->fast_blocks_per_cu; }       // production kernel

// count: 0 = off, 1 = reference-order counters (the generic kernel: what the reference's recursion does, equal to the
// oracle's counters), 2 = the production kernel counting its own work (bench.py's roofline)
static bool use_fast_trace(const agpt_ctx* c, const DevScene& sc, int count) {
    return count != 1 && sc.n_prims <= 64 * AGPT_MAX_CHUNKS && !c->force_generic;
}

#define AGPT_SMALL_BATCH (48ull << 20)   // paths: below this the trace launches run the PEEK instantiation (see k_trace_fast)

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
    bool small_batch;            // the rays of the batch number fewer than AGPT_SMALL_BATCH: k_trace_fast<PEEK>
    bool recast;                 // the wavefront loop's own closest-hit launch (its rays carry d.w): may re-cast a ray in place, see
                                 // the retire branch of k_trace_fast
};

template <int MODE, bool COUNT, bool SPILL, bool PEEK>
static void launch_trace_fast(agpt_ctx* c, const DevScene& sc, const TraceLaunch& t) {
    const dim3 block(AGPT_BLOCK), g(fast_grid(c));
    const int refill = MODE == 0 ? c->refill : c->refill_any;
    if (sc.n_prims <= 64) {
        hipLaunchKernelGGL((k_trace_fast<MODE, AGPT_FAST_STACK, false, COUNT, SPILL, PEEK>), g, block, 0, t.stream, sc, t.queue, t.count_ptr,
                           t.count_imm, t.work_head, t.ro, t.rd, t.hits, t.occ, c->counters.p,
                           refill, 0u, c->spill.p, (const unsigned long long*)nullptr, (const uint32_t*)nullptr, MODE == 0 && t.recast,
                           (const float4*)c->beta4.p, c->L4.p);
        return;
    }
    // more than 64 primitives: the top-level tree gives every ray its candidates (one word per chunk of 64 primitives), then
    // ONE traversal launch walks them in list order
    const uint32_t stride = (uint32_t)c->pool_paths;
    if (c->cand_chunks.n < c->pool_paths || c->cand_mask.n < (size_t)((sc.n_prims + 63) / 64) * c->pool_paths) {
        c->note(hipErrorOutOfMemory);   // (ensure_pool sizes both for the scene: not reached)
        return;
    }
    hipLaunchKernelGGL((k_candidates<MODE>), dim3(c->num_cus * 8), block, 0, t.stream, sc, t.queue, t.count_ptr, t.count_imm, t.ro, t.rd,
                       c->cand_mask.p, c->cand_chunks.p, stride);
    hipLaunchKernelGGL((k_trace_fast<MODE, AGPT_FAST_STACK, true, COUNT, SPILL, PEEK>), g, block, 0, t.stream, sc, t.queue, t.count_ptr,
                       t.count_imm, t.work_head, t.ro, t.rd, t.hits, t.occ, c->counters.p, refill, stride, c->spill.p,
                       (const unsigned long long*)c->cand_mask.p, (const uint32_t*)c->cand_chunks.p, false, (const float4*)nullptr,
                       (float4*)nullptr);
}

template <bool ANY, bool COUNT, int DEPTH>
static void launch_trace_generic(agpt_ctx* c, int grid, const DevScene& sc, const TraceLaunch& t) {
    hipLaunchKernelGGL((k_trace<ANY, COUNT, DEPTH>), dim3(grid), dim3(AGPT_BLOCK), 0, t.stream, sc, t.queue, t.count_ptr, t.count_imm,
                       t.work_head, t.ro, t.rd, t.hits, t.occ, c->counters.p);
}

// MODE 0 closest, 1 any-hit, 2 MIS query (production kernel only; the generic kernel traces MIS rays as closest hits)
template <int MODE>
static void launch_trace(agpt_ctx* c, const DevScene& sc, const TraceLaunch& t) {
    constexpr bool ANY = MODE == 1;
    if (use_fast_trace(c, sc, t.count)) {
        const bool spill = sc.max_depth > AGPT_FAST_STACK;
        if (spill) {
            // one column of (max_depth - AGPT_FAST_STACK) entries per thread of the grid
            const size_t need = (size_t)(sc.max_depth - AGPT_FAST_STACK) * (size_t)fast_grid(c) * AGPT_BLOCK;
            if (c->spill.ensure(need) != AGPT_OK) {
                c->note(hipErrorOutOfMemory);
                return;
            }
        }
        // <COUNT, SPILL, PEEK>: a counting launch never peeks, so six of the eight combinations exist
        if (t.count) {
            if (spill) launch_trace_fast<MODE, true, true, false>(c, sc, t);
            else launch_trace_fast<MODE, true, false, false>(c, sc, t);
        } else if (t.small_batch) {   // (see PEEK in k_trace_fast)
            if (spill) launch_trace_fast<MODE, false, true, true>(c, sc, t);
            else launch_trace_fast<MODE, false, false, true>(c, sc, t);
        } else {
            if (spill) launch_trace_fast<MODE, false, true, false>(c, sc, t);
            else launch_trace_fast<MODE, false, false, false>(c, sc, t);
        }
    } else if (sc.max_depth > AGPT_STACK_DEPTH) {
        if (t.count) launch_trace_generic<ANY, true, AGPT_STACK_DEPTH_MAX>(c, c->num_cus * 2, sc, t);
        else launch_trace_generic<ANY, false, AGPT_STACK_DEPTH_MAX>(c, c->num_cus * 2, sc, t);
    } else if (t.count)
        launch_trace_generic<ANY, true, AGPT_STACK_DEPTH>(c, trace_grid(c), sc, t);
    else
        launch_trace_generic<ANY, false, AGPT_STACK_DEPTH>(c, trace_grid(c), sc, t);
}

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
template <int MODE>
static void launch_trace_timed(agpt_ctx* c, bool timing, int kind, const DevScene& sc, const TraceLaunch& t) {
    if (timing) {
        c->note(hipEventRecord(next_event(c), t.stream));
        c->tev_kind.push_back(kind);
    }
    launch_trace<MODE>(c, sc, t);
    c->note(hipGetLastError());
    if (timing) c->note(hipEventRecord(next_event(c), t.stream));
}

extern "C" {

const char* agpt_last_error(void) { return g_error.c_str(); }
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

// ---- scene building -----------------------------------------------------------------------------------------
int agpt_scene_create(agpt_ctx* c, agpt_scene** out) {
    if (!c || !out) return fail(AGPT_ERR_INVALID, "agpt_scene_create: NULL argument");
    agpt_scene* s = new agpt_scene();
    s->ctx = c;
    *out = s;
    return AGPT_OK;
}

void agpt_scene_destroy(agpt_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipDeviceSynchronize();
    delete s;
}

int agpt_scene_add_material(agpt_scene* s, int type, const float color[3], float roughness, float metallic) {
    if (!s || !color) return fail(AGPT_ERR_INVALID, "agpt_scene_add_material: NULL argument");
    if (type < AGPT_MAT_DISNEY || type > AGPT_MAT_DIFFUSE_ONLY) return fail(AGPT_ERR_INVALID, "unknown material type");
    s->materials.push_back(agpt::make_material(type, color, roughness, metallic));
    s->colors.push_back(make_float4(color[0], color[1], color[2], 0.f));
    s->material_texture.push_back(-1);
    s->material_param_slots.push_back(0u);
    s->material_normal_texture.push_back(-1);
    s->material_normal_scale.push_back(0.f);
    s->committed = false;
    return (int)s->materials.size() - 1;
}

// the Scene::primitives record of a mesh / sphere / plane just added; returns its primitive id
static int add_prim(agpt_scene* s, int type, int index, int material) {
    agpt::HostPrim p;
    p.type = type;
    p.index = index;
    p.material = material;
    p.arealight = -1;
    s->prims.push_back(p);
    s->committed = false;
    return (int)s->prims.size() - 1;
}

int agpt_scene_add_mesh(agpt_scene* s, const float* vertices, int n_vertices, const float* normals, int n_normals,
                        const float* texcoords, int n_texcoords, const int32_t* indices, int n_indices, int material,
                        int max_prims_in_node) {
    if (!s || !vertices || !indices) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: NULL argument");
    if (n_indices < 3 || n_indices % 3 != 0 || n_vertices <= 0)
        return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: need at least one triangle (the reference's BVH build does not terminate on an empty mesh)");
    if (material < -1 || material >= (int)s->materials.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: bad material id");
    for (int i = 0; i < n_indices; i++) {
        const int32_t* ix = indices + 3 * i;
        if (ix[0] < 0 || ix[0] >= n_vertices) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: vertex index out of range");
        if (n_normals > 0 && (ix[1] < 0 || ix[1] >= n_normals)) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: normal index out of range");
        if (n_texcoords > 0 && (ix[2] < 0 || ix[2] >= n_texcoords)) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: texcoord index out of range");
    }
    agpt::HostMesh m;
    m.vertices.resize(n_vertices);
    for (int i = 0; i < n_vertices; i++) m.vertices[i] = V3(vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]);
    if (normals && n_normals > 0) {
        m.normals.resize(n_normals);
        for (int i = 0; i < n_normals; i++) m.normals[i] = V3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
    }
    if (texcoords && n_texcoords > 0) {
        m.texcoords.resize(n_texcoords);
        for (int i = 0; i < n_texcoords; i++) {
            m.texcoords[i].x = texcoords[2 * i];
            m.texcoords[i].y = texcoords[2 * i + 1];
        }
    }
    m.indices.assign(indices, indices + (size_t)3 * n_indices);
    m.material = material;
    if (s->bvh_builder == AGPT_BVH_BUILDER_DEVICE) {
        // same bytes as build_bvh (agpt_bvh_device.hip)
        HIP_TRY(hipSetDevice(s->ctx->device));
        const int n_tris = n_indices / 3;
        m.nodes.resize((size_t)2 * n_tris + 2);
        m.prim_index.resize(n_tris);
        int on_device = 0;
        const int rc = agpt::build_bvh_device(s->ctx->stream, vertices, n_vertices, indices, n_tris, max_prims_in_node, m.nodes.data(),
                                              m.prim_index.data(), &m.total_nodes, &m.max_depth, &on_device);
        if (rc != AGPT_OK) return rc;
        m.nodes.resize((size_t)m.total_nodes + 1);
        m.max_prims_in_node = max_prims_in_node;
    } else {
        agpt::build_bvh(m, max_prims_in_node);
    }
    s->meshes.push_back(std::move(m));
    return add_prim(s, AGPT_PRIM_MESH, (int)s->meshes.size() - 1, material);
}

int agpt_scene_add_sphere(agpt_scene* s, const float center[3], float radius, int material) {
    if (!s || !center) return fail(AGPT_ERR_INVALID, "agpt_scene_add_sphere: NULL argument");
    if (material < -1 || material >= (int)s->materials.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_add_sphere: bad material id");
    agpt::HostSphere sp;
    sp.center = V3(center[0], center[1], center[2]);
    sp.r = radius;
    sp.r2 = radius * radius;
    s->spheres.push_back(sp);
    return add_prim(s, AGPT_PRIM_SPHERE, (int)s->spheres.size() - 1, material);
}

int agpt_scene_add_plane(agpt_scene* s, const float o[3], const float size[2], int material) {
    if (!s || !o || !size) return fail(AGPT_ERR_INVALID, "agpt_scene_add_plane: NULL argument");
    if (material < -1 || material >= (int)s->materials.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_add_plane: bad material id");
    agpt::HostSphere sp;  // reused record: center = O, r = HalfSize.x, r2 = HalfSize.y
    sp.center = V3(o[0], o[1], o[2]);
    sp.r = size[0] / 2;
    sp.r2 = size[1] / 2;
    s->spheres.push_back(sp);
    return add_prim(s, AGPT_PRIM_PLANE, (int)s->spheres.size() - 1, material);
}

int agpt_scene_add_area_light(agpt_scene* s, const float center[3], float radius, const float L[3]) {
    if (!s || !center || !L) return fail(AGPT_ERR_INVALID, "agpt_scene_add_area_light: NULL argument");
    int prim = agpt_scene_add_sphere(s, center, radius, -1);
    if (prim < 0) return prim;
    agpt::HostLight l;
    l.type = AGPT_LIGHT_AREA;
    l.shape = prim;
    l.L = V3(L[0], L[1], L[2]);
    s->lights.push_back(l);
    s->prims[prim].arealight = (int)s->lights.size() - 1;
    return prim;
}

int agpt_scene_add_uniform_infinite_light(agpt_scene* s, const float L[3]) {
    if (!s || !L) return fail(AGPT_ERR_INVALID, "agpt_scene_add_uniform_infinite_light: NULL argument");
    agpt::HostLight l;
    l.type = AGPT_LIGHT_UNIFORM_INFINITE;
    l.shape = -1;
    l.L = V3(L[0], L[1], L[2]);
    s->lights.push_back(l);
    s->committed = false;
    return (int)s->lights.size() - 1;
}

int agpt_scene_add_infinite_area_light(agpt_scene* s, const float* rgb, int width, int height) {
    if (!s || !rgb || width <= 0 || height <= 0 || (long long)width * height > (1ll << 28))
        return fail(AGPT_ERR_INVALID, "agpt_scene_add_infinite_area_light: bad argument");
    s->envs.push_back(agpt::make_env(rgb, width, height));
    agpt::HostLight l;
    l.type = AGPT_LIGHT_INFINITE_AREA;
    l.shape = -1;
    l.L = V3s(0.f);
    l.env = (int)s->envs.size() - 1;
    s->lights.push_back(l);
    s->committed = false;
    return (int)s->lights.size() - 1;
}

int agpt_scene_add_texture(agpt_scene* s, const float* rgb, int width, int height) {
    if (!s || !rgb) return fail(AGPT_ERR_INVALID, "agpt_scene_add_texture: NULL argument");
    if (width <= 0 || height <= 0 || (long long)width * height > (1ll << 28))
        return fail(AGPT_ERR_INVALID, "agpt_scene_add_texture: width and height must be positive (at most 2^28 texels)");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_add_texture: the scene is already committed");
    agpt_scene::HostTexture t;
    t.width = width;
    t.height = height;
    t.texels.resize((size_t)width * height);
    for (size_t i = 0; i < t.texels.size(); i++) t.texels[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.f);
    s->textures.push_back(std::move(t));
    return (int)s->textures.size() - 1;
}

int agpt_scene_set_material_texture(agpt_scene* s, int material, int texture) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_texture: scene is NULL");
    if (material < 0 || material >= (int)s->materials.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_texture: bad material id");
    if (texture < -1 || texture >= (int)s->textures.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_texture: bad texture id");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_texture: the scene is already committed");
    s->material_texture[material] = texture;
    return AGPT_OK;
}

static_assert(AGPT_PARAM_ROUGHNESS == 0 && AGPT_PARAM_METALLIC == 1, "param_slots_pack (agpt_scene.h) numbers the parameters like agpt.h");

int agpt_scene_set_material_param_texture(agpt_scene* s, int material, int param, int texture, int channel) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: scene is NULL");
    if (material < 0 || material >= (int)s->materials.size())
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: bad material id");
    if (param != AGPT_PARAM_ROUGHNESS && param != AGPT_PARAM_METALLIC)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: param is neither AGPT_PARAM_ROUGHNESS nor AGPT_PARAM_METALLIC");
    if (texture < -1 || texture >= (int)s->textures.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: bad texture id");
    if (texture >= 0 && (channel < 0 || channel > 2))
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: channel must be 0 (r), 1 (g) or 2 (b)");
    if (s->materials[material].type != AGPT_MAT_DISNEY)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: only AGPT_MAT_DISNEY materials have a roughness and a metallic weight");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: the scene is already committed");
    if (texture > AGPT_PARAM_MAX_TEXTURE)
        return fail(AGPT_ERR_LIMIT, "agpt_scene_set_material_param_texture: a parameter map must be one of the scene's first " +
                                        std::to_string(AGPT_PARAM_MAX_TEXTURE + 1) + " textures");
    const uint32_t old = s->material_param_slots[material];
    int tex[2] = {param_slot_texture(old, 0), param_slot_texture(old, 1)};
    int ch[2] = {param_slot_channel(old, 0), param_slot_channel(old, 1)};
    tex[param] = texture;
    ch[param] = texture >= 0 ? channel : 0;
    s->material_param_slots[material] = param_slots_pack(tex[0], ch[0], tex[1], ch[1]);
    return AGPT_OK;
}

int agpt_scene_set_material_normal_texture(agpt_scene* s, int material, int texture, float scale) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: scene is NULL");
    if (material < 0 || material >= (int)s->materials.size())
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: bad material id");
    if (texture < -1 || texture >= (int)s->textures.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: bad texture id");
    if (texture >= 0 && !std::isfinite(scale)) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: scale is not finite");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: the scene is already committed");
    s->material_normal_texture[material] = texture;
    s->material_normal_scale[material] = texture >= 0 ? scale : 0.f;
    return AGPT_OK;
}

static_assert(AGPT_WRAP_REPEAT == (int)AGPT_TEXTURE_WRAP_REPEAT && AGPT_WRAP_CLAMP == (int)AGPT_TEXTURE_WRAP_CLAMP &&
                  AGPT_WRAP_MIRROR == (int)AGPT_TEXTURE_WRAP_MIRROR && AGPT_FILTER_NEAREST == 0 && AGPT_FILTER_BILINEAR == 1,
              "texture_size_pack (agpt_scene.h) numbers filters and wrap modes like agpt.h");

int agpt_scene_set_texture_sampler(agpt_scene* s, int texture, int filter, int wrap_u, int wrap_v) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: scene is NULL");
    if (texture < 0 || texture >= (int)s->textures.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: bad texture id");
    if (filter != AGPT_FILTER_NEAREST && filter != AGPT_FILTER_BILINEAR)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: filter is neither AGPT_FILTER_NEAREST nor AGPT_FILTER_BILINEAR");
    for (int wrap : {wrap_u, wrap_v})
        if (wrap != AGPT_WRAP_REPEAT && wrap != AGPT_WRAP_CLAMP && wrap != AGPT_WRAP_MIRROR)
            return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: a wrap mode is none of AGPT_WRAP_REPEAT, AGPT_WRAP_CLAMP, AGPT_WRAP_MIRROR");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: the scene is already committed");
    agpt_scene::HostTexture& t = s->textures[texture];
    t.filter = filter;
    t.wrap_u = wrap_u;
    t.wrap_v = wrap_v;
    return AGPT_OK;
}

int agpt_scene_set_camera(agpt_scene* s, const agpt_camera_desc* d) {
    if (!s || !d) return fail(AGPT_ERR_INVALID, "agpt_scene_set_camera: NULL argument");
    s->cam = agpt::make_camera(*d);
    s->has_camera = true;
    s->dev.cam = s->cam;
    return AGPT_OK;
}

// the bounds of the host copies of meshes that were refitted on the device (agpt_scene_update_mesh) and, with `arrays`, the positions
// and normals of those whose new arrays never existed on the host (agpt_scene_update_mesh_device, agpt_scene_transform_mesh)
static int sync_mirror(agpt_scene* s, bool arrays) {
    for (size_t m = 0; m < s->bounds_stale.size(); m++) {
        if (s->bounds_stale[m]) {
            HIP_TRY(hipSetDevice(s->ctx->device));
            if (const int rc = agpt::download_bounds(s->ctx->stream, s->updaters[m], s->meshes[m])) return rc;
            s->bounds_stale[m] = 0;
        }
        if (arrays && s->arrays_stale[m]) {
            HIP_TRY(hipSetDevice(s->ctx->device));
            if (const int rc = agpt::download_arrays(s->ctx->stream, s->updaters[m], s->meshes[m].vertices, s->meshes[m].normals)) return rc;
            s->arrays_stale[m] = 0;
        }
    }
    return AGPT_OK;
}

// DevScene::mdiv_coords_ok from the host's copies of the root boxes (kept current by commit and by refit_done).  A non-finite
// coordinate does not clear it: such a mesh is traced as before (the reference's own answer to a NaN vertex is a hit at t = NaN and,
// behind it, a path that an emitter re-casts for ever).
static int32_t mdiv_coords_ok(const agpt_scene* s) {
    auto outside = [](float x) { return std::isfinite(x) && !(std::fabs(x) < AGPT_MDIV_COORD_LIMIT); };
    for (const agpt::HostMesh& m : s->meshes) {
        if (m.nodes.empty()) continue;
        for (int a = 0; a < 3; a++)
            if (outside(m.nodes[0].bmin[a]) || outside(m.nodes[0].bmax[a])) return 0;
    }
    return 1;
}

int agpt_scene_commit(agpt_scene* s) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_commit: scene is NULL");
    if (const int rc = sync_mirror(s, true)) return rc;   // flatten_scene reads every mesh's arrays and boxes
    // The scene's texturing level: the highest one a material needs.  Every level's kernels are those of the level below plus one
    // thing (same uv records, same texture table), so the conditions below compare against it.
    bool has_texture = false, has_map = false, has_sampler = false, has_normal_map = false;
    for (size_t m = 0; m < s->material_texture.size(); m++) {
        has_texture = has_texture || s->material_texture[m] >= 0;
        has_map = has_map || s->material_param_slots[m] != 0;
        has_normal_map = has_normal_map || s->material_normal_texture[m] >= 0;
        // a texture that the material names -- in its colour slot or in a parameter slot -- has a sampler of its own
        for (int t : {(int)s->material_texture[m], param_slot_texture(s->material_param_slots[m], 0), param_slot_texture(s->material_param_slots[m], 1)})
            has_sampler = has_sampler || (t >= 0 && !s->textures[t].default_sampler());
    }
    const agpt::ShadeLevel level = has_normal_map ? agpt::SHADE_NORMAL : has_sampler ? agpt::SHADE_SAMPLED : has_map ? agpt::SHADE_MAPPED
                                   : has_texture  ? agpt::SHADE_TEXTURED : agpt::SHADE_PLAIN;
    const bool textured = level >= agpt::SHADE_TEXTURED;
    if (textured)
        for (const agpt::HostPrim& hp : s->prims)
            if (hp.type != AGPT_PRIM_MESH && hp.material >= 0 &&
                (s->material_texture[hp.material] >= 0 || s->material_param_slots[hp.material] != 0 || s->material_normal_texture[hp.material] >= 0))
                return fail(AGPT_ERR_INVALID, "agpt_scene_commit: a sphere or a plane has a material with a colour texture, a roughness / metallic map or a normal map "
                                              "(textures apply to triangle meshes only)");
    HIP_TRY(hipSetDevice(s->ctx->device));
    agpt::FlatScene flat;
    flat.want_tri_uv = textured;
    agpt::flatten_scene(s->meshes, s->spheres, s->prims, flat);
    s->max_depth = flat.max_depth;
    if (flat.max_depth > AGPT_STACK_DEPTH_MAX)
        return fail(AGPT_ERR_LIMIT, "agpt_scene_commit: BVH depth " + std::to_string(flat.max_depth) +
                                        " exceeds the deepest traversal stack (" + std::to_string(AGPT_STACK_DEPTH_MAX) + ")");
    std::vector<DevLight> lights(s->lights.size());
    int n_inf = 0;
    for (size_t i = 0; i < lights.size(); i++) {
        lights[i].type = s->lights[i].type;
        lights[i].shape = s->lights[i].shape;
        lights[i].L[0] = s->lights[i].L.x;
        lights[i].L[1] = s->lights[i].L.y;
        lights[i].L[2] = s->lights[i].L.z;
        lights[i].env = s->lights[i].env;
        if (lights[i].type != AGPT_LIGHT_AREA) n_inf++;
    }
    hipStream_t st = s->ctx->stream;
    int rc;
    if ((rc = upload(s->d_nodes, flat.nodes, st))) return rc;
    if (flat.bigleaves.empty()) flat.bigleaves.assign(2, 0u);
    if ((rc = upload(s->d_bigleaves, flat.bigleaves, st))) return rc;
    if ((rc = upload(s->d_tri_verts, flat.tri_verts, st))) return rc;
    if ((rc = upload(s->d_tri_shade, flat.tri_shade, st))) return rc;
    if ((rc = upload(s->d_prefilter, flat.prefilter, st))) return rc;
    if ((rc = upload(s->d_toplevel, flat.toplevel16, st))) return rc;
    {
        std::vector<unsigned long long> mm(flat.mesh_masks, flat.mesh_masks + AGPT_MAX_CHUNKS);
        if ((rc = upload(s->d_chunk_mesh_masks, mm, st))) return rc;
    }
    if ((rc = upload(s->d_prims, flat.prims, st))) return rc;
    if ((rc = upload(s->d_materials, s->materials, st))) return rc;
    if ((rc = upload(s->d_colors, s->colors, st))) return rc;
    if ((rc = upload(s->d_lights, lights, st))) return rc;
    std::vector<DevEnv> envs(s->envs.size());
    s->d_env_pixels.resize(envs.size());
    s->d_env_func.resize(envs.size());
    s->d_env_cdf.resize(envs.size());
    for (size_t i = 0; i < envs.size(); i++) {
        const agpt::HostEnv& he = s->envs[i];
        if ((rc = upload(s->d_env_pixels[i], he.pixels, st))) return rc;
        if ((rc = upload(s->d_env_func[i], he.func, st))) return rc;
        if ((rc = upload(s->d_env_cdf[i], he.cdf, st))) return rc;
        envs[i].pixels = s->d_env_pixels[i].p;
        envs[i].func = s->d_env_func[i].p;
        envs[i].cdf = s->d_env_cdf[i].p;
        envs[i].width = he.width;
        envs[i].height = he.height;
        envs[i].n = he.width * he.height;
        envs[i].funcInt = he.funcInt;
    }
    if ((rc = upload(s->d_envs, envs, st))) return rc;
    // texture coordinates, texels and the tables are uploaded only for a scene that has a textured material
    std::vector<DevTexture> textures(textured ? s->textures.size() : 0);
    std::vector<std::vector<float4>> own_texels;   // (kept until the copies below have completed)
    if (textured) {
        // The device's material_texture table.  A material with a roughness / metallic map or a normal map and no colour texture gets a 1x1 texture of
        // its constant colour here (any uv reads that texel, and the texel has the constant's bits), so the MAPPED kernels have
        // one source for the colour; with maps the table's second half holds the packed slots (agpt_scene.h).
        std::vector<int32_t> table = s->material_texture;
        for (size_t m = 0; m < table.size(); m++)
            if ((s->material_param_slots[m] != 0 || s->material_normal_texture[m] >= 0) && table[m] < 0) {
                table[m] = (int32_t)(s->textures.size() + own_texels.size());
                own_texels.push_back(std::vector<float4>(1, s->colors[m]));
            }
        if (level >= agpt::SHADE_MAPPED)   // (the kernels above MAPPED read the slots too: all 0 in a scene without maps)
            table.insert(table.end(), s->material_param_slots.begin(), s->material_param_slots.end());
        textures.resize(s->textures.size() + own_texels.size());
        s->d_texels.resize(textures.size());
        for (size_t i = 0; i < textures.size(); i++) {
            const bool own = i >= s->textures.size();
            if ((rc = upload(s->d_texels[i], own ? own_texels[i - s->textures.size()] : s->textures[i].texels, st))) return rc;
            textures[i].texels = s->d_texels[i].p;
            textures[i].width = own ? 1 : s->textures[i].width;
            textures[i].height = own ? 1 : s->textures[i].height;
            if (level >= agpt::SHADE_SAMPLED && !own) {   // (only the kernels from SAMPLED up decode the size words, agpt_scene.h: DevTexture)
                textures[i].width = texture_size_pack(s->textures[i].width, s->textures[i].wrap_u, s->textures[i].filter);
                textures[i].height = texture_size_pack(s->textures[i].height, s->textures[i].wrap_v, 0);
            }
        }
        if (level == agpt::SHADE_NORMAL) {   // one DevNormalSlot per material behind the two halves (agpt_scene.h)
            static_assert(sizeof(DevNormalSlot) == 8 * sizeof(int32_t), "a normal slot is two 16-byte loads");
            const size_t off = (size_t)normal_slots_offset((int)s->materials.size());
            table.resize(off + 8 * s->materials.size(), 0);
            for (size_t m = 0; m < s->materials.size(); m++) {
                const int t = s->material_normal_texture[m];
                DevNormalSlot slot{};
                slot.tex = textures[t >= 0 ? t : 0];
                slot.scale = s->material_normal_scale[m];
                slot.texture = t;
                memcpy(&table[off + 8 * m], &slot, sizeof(slot));
            }
        }
        if ((rc = upload(s->d_tri_uv, flat.tri_uv, st))) return rc;
        if ((rc = upload(s->d_textures, textures, st))) return rc;
        if ((rc = upload(s->d_material_texture, table, st))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    s->shade_level = level;
    s->dev.tri_uv = textured ? s->d_tri_uv.p : nullptr;
    s->dev.textures = textured ? s->d_textures.p : nullptr;
    s->dev.material_texture = textured ? s->d_material_texture.p : nullptr;
    s->dev.envs = s->d_envs.p;
    s->dev.nodes = s->d_nodes.p;
    s->dev.bigleaves = s->d_bigleaves.p;
    s->dev.tri_verts = s->d_tri_verts.p;
    s->dev.tri_shade = s->d_tri_shade.p;
    s->dev.prims = s->d_prims.p;
    s->dev.materials = s->d_materials.p;
    s->dev.lights = s->d_lights.p;
    s->dev.n_prims = (int)flat.prims.size();
    s->dev.n_lights = (int)lights.size();
    s->dev.n_materials = (int)s->materials.size();
    s->dev.n_infinite = n_inf;
    s->dev.max_depth = flat.max_depth;
    s->dev.rootpair_base = flat.rootpair_base;
    for (int ch = 0; ch < AGPT_MAX_CHUNKS; ch++) s->dev.mesh_masks[ch] = flat.mesh_masks[ch];
    for (int ch = 0; ch < AGPT_MAX_CHUNKS; ch++) s->dev.analytic_masks[ch] = flat.analytic_masks[ch];
    for (int ch = 0; ch <= AGPT_MAX_CHUNKS; ch++) s->dev.pf_begin[ch] = flat.pf_begin[ch];
    s->dev.prefilter = s->d_prefilter.p;
    s->dev.toplevel = reinterpret_cast<const uint4*>(s->d_toplevel.p);
    s->dev.n_toplevel = flat.n_toplevel;
    s->dev.chunk_mesh_masks = s->d_chunk_mesh_masks.p;
    s->dev.n_meshes = 0;
    for (const DevPrim& dp : flat.prims)
        if (dp.type == AGPT_PRIM_MESH && dp.n_tris > 0) s->dev.n_meshes++;
    s->dev.cam = s->cam;
    s->dev.mdiv_coords_ok = mdiv_coords_ok(s);
    s->committed = true;
    return AGPT_OK;
}

static const agpt::HostMesh* mesh_of(const agpt_scene* s, int prim) {
    if (!s || prim < 0 || prim >= (int)s->prims.size() || s->prims[prim].type != AGPT_PRIM_MESH) return nullptr;
    return &s->meshes[s->prims[prim].index];
}
int agpt_mesh_num_nodes(const agpt_scene* s, int prim) {
    const agpt::HostMesh* m = mesh_of(s, prim);
    return m ? m->total_nodes : fail(AGPT_ERR_INVALID, "agpt_mesh_num_nodes: not a mesh primitive");
}
int agpt_mesh_num_prims(const agpt_scene* s, int prim) {
    const agpt::HostMesh* m = mesh_of(s, prim);
    return m ? (int)m->prim_index.size() : fail(AGPT_ERR_INVALID, "agpt_mesh_num_prims: not a mesh primitive");
}
int agpt_mesh_get_bvh(const agpt_scene* s, int prim, agpt_bvh_node* nodes_out, int32_t* prim_index_out) {
    const agpt::HostMesh* m = mesh_of(s, prim);
    if (!m) return fail(AGPT_ERR_INVALID, "agpt_mesh_get_bvh: not a mesh primitive");
    if (const int rc = sync_mirror(const_cast<agpt_scene*>(s), false)) return rc;   // (the boxes only)
    if (nodes_out) std::memcpy(nodes_out, m->nodes.data(), m->nodes.size() * sizeof(agpt_bvh_node));
    if (prim_index_out) std::memcpy(prim_index_out, m->prim_index.data(), m->prim_index.size() * sizeof(int32_t));
    return AGPT_OK;
}

// the mesh arguments of agpt_bvh_build / agpt_bvh_build_device (n_indices index triplets, as agpt_scene_add_mesh)
static int check_bvh_input(const char* fn, const float* vertices, int n_vertices, const int32_t* indices, int n_indices) {
    if (!vertices || !indices || n_vertices <= 0 || n_indices < 3 || n_indices % 3 != 0)
        return fail(AGPT_ERR_INVALID, std::string(fn) + ": need at least one triangle");
    for (int i = 0; i < n_indices; i++)
        if (indices[3 * i] < 0 || indices[3 * i] >= n_vertices) return fail(AGPT_ERR_INVALID, std::string(fn) + ": vertex index out of range");
    return AGPT_OK;
}

int agpt_bvh_build(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, int max_prims_in_node,
                   agpt_bvh_node* nodes_out, int32_t* prim_index_out, int* total_nodes_out, int* max_depth_out) {
    if (const int rc = check_bvh_input("agpt_bvh_build", vertices, n_vertices, indices, n_indices)) return rc;
    agpt::HostMesh m;
    m.vertices.resize(n_vertices);
    for (int i = 0; i < n_vertices; i++) m.vertices[i] = V3(vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]);
    m.indices.assign(indices, indices + (size_t)3 * n_indices);
    agpt::build_bvh(m, max_prims_in_node);
    if (nodes_out) std::memcpy(nodes_out, m.nodes.data(), m.nodes.size() * sizeof(agpt_bvh_node));
    if (prim_index_out) std::memcpy(prim_index_out, m.prim_index.data(), m.prim_index.size() * sizeof(int32_t));
    if (total_nodes_out) *total_nodes_out = m.total_nodes;
    if (max_depth_out) *max_depth_out = m.max_depth;
    return AGPT_OK;
}

int agpt_bvh_refit(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, const int32_t* prim_index,
                   agpt_bvh_node* nodes_inout, int total_nodes) {
    if (const int rc = check_bvh_input("agpt_bvh_refit", vertices, n_vertices, indices, n_indices)) return rc;
    const int n_tris = n_indices / 3;
    if (!prim_index || !nodes_inout || total_nodes < 1 || total_nodes > 2 * n_tris)
        return fail(AGPT_ERR_INVALID, "agpt_bvh_refit: NULL tree or a node count outside [1, 2 * triangles]");
    for (int t = 0; t < n_tris; t++)
        if (prim_index[t] < 0 || prim_index[t] % 3 != 0 || prim_index[t] / 3 >= n_tris) return fail(AGPT_ERR_INVALID, "agpt_bvh_refit: bad prim_index");
    std::vector<v3> v((size_t)n_vertices);
    for (int i = 0; i < n_vertices; i++) v[i] = V3(vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]);
    const std::vector<int32_t> ix(indices, indices + (size_t)3 * n_indices), order(prim_index, prim_index + n_tris);
    std::vector<agpt_bvh_node> nodes(nodes_inout, nodes_inout + total_nodes + 1);   // (a refused call changes nothing)
    if (!agpt::refit_bvh(v, ix, order, nodes.data(), total_nodes)) return fail(AGPT_ERR_INVALID, "agpt_bvh_refit: not a tree of agpt_bvh_build's");
    std::memcpy(nodes_inout, nodes.data(), nodes.size() * sizeof(agpt_bvh_node));
    return AGPT_OK;
}

// the top-level tree again (lists longer than 64 primitives): its topology depends on the root boxes (flatten_scene)
static int upload_toplevel(agpt_scene* s) {
    std::vector<float> boxes;
    std::vector<uint32_t> index;
    for (size_t pi = 0; pi < std::min<size_t>(s->prims.size(), 64 * (size_t)AGPT_MAX_CHUNKS); pi++)
        if (s->prims[pi].type == AGPT_PRIM_MESH) {
            const agpt_bvh_node& r = s->meshes[s->prims[pi].index].nodes[0];
            boxes.insert(boxes.end(), {r.bmin[0], r.bmin[1], r.bmin[2], r.bmax[0], r.bmax[1], r.bmax[2]});
            index.push_back((uint32_t)pi);
        }
    std::vector<float4> tree;
    std::vector<uint32_t> packed;
    agpt::build_skip_tree(boxes.data(), index.data(), (int)index.size(), tree);
    agpt::pack_skip_tree16(tree, packed);
    if (packed.size() > s->d_toplevel.n || (int32_t)(tree.size() / 2) != s->dev.n_toplevel)
        return fail(AGPT_ERR_DEVICE, "agpt_scene_update_mesh: the top-level tree changed size");
    HIP_TRY(hipMemcpyAsync(s->d_toplevel.p, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return AGPT_OK;
}

// the argument checks the three update calls share, in agpt_scene_update_mesh's order (`fn` names the call in the message)
static int check_update(const char* fn, const agpt_scene* s, int prim, const void* vertices, int n_vertices, const void* normals, int n_normals,
                        int mode) {
    const std::string f(fn);
    if (!s || !vertices) return fail(AGPT_ERR_INVALID, f + ": NULL scene or vertices");
    if (!s->committed) return fail(AGPT_ERR_INVALID, f + ": the scene is not committed");
    if (prim < 0 || prim >= (int)s->prims.size() || s->prims[prim].type != AGPT_PRIM_MESH)
        return fail(AGPT_ERR_INVALID, f + ": primitive " + std::to_string(prim) + " is not a mesh of this scene");
    const agpt::HostMesh& mesh = s->meshes[(size_t)s->prims[prim].index];
    if (n_vertices != (int)mesh.vertices.size() || n_normals != (int)mesh.normals.size() || (!normals && !mesh.normals.empty()))
        return fail(AGPT_ERR_INVALID, f + ": the mesh has " + std::to_string(mesh.vertices.size()) + " vertices and " +
                                          std::to_string(mesh.normals.size()) + " normals; both counts stay (normals may be NULL only without any)");
    if (mode != AGPT_UPDATE_REFIT && mode != AGPT_UPDATE_REBUILD) return fail(AGPT_ERR_INVALID, f + ": unknown mode " + std::to_string(mode));
    return AGPT_OK;
}

static void size_update_state(agpt_scene* s) {
    if (s->updaters.size() < s->meshes.size()) {
        s->updaters.resize(s->meshes.size(), nullptr);
        s->bounds_stale.resize(s->meshes.size(), 0);
        s->arrays_stale.resize(s->meshes.size(), 0);
        s->rest.resize(s->meshes.size());
    }
}

// the mesh's arrays were given explicitly: they are the rest pose of the transforms that follow
static void forget_rest(agpt_scene* s, size_t mi) {
    s->rest[mi] = agpt_scene::RestPose();
    agpt::drop_rest(s->updaters[mi]);
}

// Host orchestration of what exists, from host arrays: a new tree (REBUILD) or the host refit (a non-finite position under REFIT),
// then the full commit.
static int update_on_host(agpt_scene* s, size_t mi, const float* vertices, const float* normals, int mode) {
    agpt::HostMesh& mesh = s->meshes[mi];
    const int n_vertices = (int)mesh.vertices.size(), n_normals = (int)mesh.normals.size();
    auto set_arrays = [&]() {
        for (int i = 0; i < n_vertices; i++) mesh.vertices[i] = V3(vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]);
        for (int i = 0; i < n_normals; i++) mesh.normals[i] = V3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
    };
    if (mode == AGPT_UPDATE_REBUILD && s->bvh_builder == AGPT_BVH_BUILDER_DEVICE) {
        const int n_tris = (int)mesh.prim_index.size();
        std::vector<agpt_bvh_node> nodes((size_t)2 * n_tris + 2);
        std::vector<int32_t> order(n_tris);
        int total = 0, depth = 0, on_device = 0;
        const int rc = agpt::build_bvh_device(s->ctx->stream, vertices, n_vertices, mesh.indices.data(), n_tris, mesh.max_prims_in_node,
                                              nodes.data(), order.data(), &total, &depth, &on_device);
        if (rc != AGPT_OK) return rc;
        nodes.resize((size_t)total + 1);
        set_arrays();
        mesh.nodes.swap(nodes);
        mesh.prim_index.swap(order);
        mesh.total_nodes = total;
        mesh.max_depth = depth;
    } else if (mode == AGPT_UPDATE_REBUILD) {
        set_arrays();
        agpt::build_bvh(mesh, mesh.max_prims_in_node);
    } else {
        set_arrays();
        agpt::refit_bvh(mesh.vertices, mesh.indices, mesh.prim_index, mesh.nodes.data(), mesh.total_nodes);
    }
    s->bounds_stale[mi] = 0;   // every box of this mesh has just been computed on the host,
    s->arrays_stale[mi] = 0;   // from arrays that are now the mirror's
    if (mode == AGPT_UPDATE_REBUILD) {   // the cache holds the old topology
        agpt::mesh_updater_destroy(s->updaters[mi]);
        s->updaters[mi] = nullptr;
    }
    return agpt_scene_commit(s);
}

// REFIT on the device: where flatten_scene put this mesh
static agpt::UpdateTarget update_target(const agpt_scene* s, int prim, size_t mi) {
    size_t node_base = 0, tri_base = 0;
    for (size_t m = 0; m < mi; m++) {
        node_base += (s->meshes[m].nodes.size() + 1) & ~size_t(1);
        tri_base += s->meshes[m].prim_index.size();
    }
    int ordinal = 0;   // its prefilter record: non-empty meshes before it in the list (every mesh has a triangle)
    for (int pi = 0; pi < prim; pi++) ordinal += s->prims[pi].type == AGPT_PRIM_MESH;
    const bool listed = prim < 64 * AGPT_MAX_CHUNKS;   // root pairs and prefilter records exist for these only
    agpt::UpdateTarget tg;
    tg.nodes = s->d_nodes.p;
    tg.tri_verts = s->d_tri_verts.p;
    tg.tri_shade = s->d_tri_shade.p;
    tg.prim = s->d_prims.p + prim;
    tg.rootpair = listed ? s->d_nodes.p + 4 * (((size_t)s->dev.rootpair_base + 2 * (size_t)prim) >> 1) : nullptr;
    tg.prefilter = listed ? s->d_prefilter.p + 2 * (size_t)ordinal : nullptr;
    tg.node_base = (uint32_t)node_base;
    tg.tri_base = (uint32_t)tri_base;
    tg.prim_id = (uint32_t)prim;
    return tg;
}

// the host's share of a device REFIT: the root box (the top-level tree is built from it) and what the mirror now lacks
static int refit_done(agpt_scene* s, size_t mi, const float root[6], bool arrays_on_device_only) {
    agpt::HostMesh& mesh = s->meshes[mi];
    std::memcpy(mesh.nodes[0].bmin, root, 12);
    std::memcpy(mesh.nodes[0].bmax, root + 3, 12);
    s->bounds_stale[mi] = 1;
    s->arrays_stale[mi] = arrays_on_device_only ? 1 : 0;
    s->dev.mdiv_coords_ok = mdiv_coords_ok(s);
    if (s->prims.size() > 64) return upload_toplevel(s);
    return AGPT_OK;
}

int agpt_scene_update_mesh(agpt_scene* s, int prim, const float* vertices, int n_vertices, const float* normals, int n_normals, int mode) {
    if (const int rc = check_update("agpt_scene_update_mesh", s, prim, vertices, n_vertices, normals, n_normals, mode)) return rc;
    const size_t mi = (size_t)s->prims[prim].index;
    agpt::HostMesh& mesh = s->meshes[mi];
    HIP_TRY(hipSetDevice(s->ctx->device));
    size_update_state(s);
    forget_rest(s, mi);
    bool finite = true;
    for (int i = 0; i < 3 * n_vertices && finite; i++) finite = std::isfinite(vertices[i]);
    if (mode == AGPT_UPDATE_REBUILD || !finite) return update_on_host(s, mi, vertices, normals, mode);
    const agpt::UpdateTarget tg = update_target(s, prim, mi);
    float root[6];
    if (const int rc = agpt::update_mesh_device(s->ctx->stream, &s->updaters[mi], mesh, vertices, normals, tg, root)) return rc;
    for (int i = 0; i < n_vertices; i++) mesh.vertices[i] = V3(vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]);
    for (int i = 0; i < n_normals; i++) mesh.normals[i] = V3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
    return refit_done(s, mi, root, false);
}

// the new arrays are in the mesh's updater (copied or transformed there): REFIT from them, or -- REBUILD, a non-finite position --
// bring them to the host and do what agpt_scene_update_mesh does with host arrays
static int update_from_updater(agpt_scene* s, int prim, size_t mi, int mode) {
    agpt::HostMesh& mesh = s->meshes[mi];
    if (mode == AGPT_UPDATE_REFIT) {
        const agpt::UpdateTarget tg = update_target(s, prim, mi);
        float root[6];
        bool finite = true;
        if (const int rc = agpt::refit_device_arrays(s->ctx->stream, s->updaters[mi], mesh, tg, root, &finite)) return rc;
        if (finite) return refit_done(s, mi, root, true);
    }
    std::vector<v3> v(mesh.vertices.size()), n(mesh.normals.size());
    if (const int rc = agpt::download_arrays(s->ctx->stream, s->updaters[mi], v, n)) return rc;
    return update_on_host(s, mi, &v.data()->x, n.empty() ? nullptr : &n.data()->x, mode);
}

int agpt_scene_update_mesh_device(agpt_scene* s, int prim, const float* vertices_dev, int n_vertices, const float* normals_dev, int n_normals,
                                  int mode) {
    if (const int rc = check_update("agpt_scene_update_mesh_device", s, prim, vertices_dev, n_vertices, normals_dev, n_normals, mode)) return rc;
    const size_t mi = (size_t)s->prims[prim].index;
    HIP_TRY(hipSetDevice(s->ctx->device));
    size_update_state(s);
    if (mode == AGPT_UPDATE_REBUILD) {   // the builders take host arrays
        std::vector<float> v((size_t)3 * n_vertices), n((size_t)3 * n_normals);
        HIP_TRY(hipMemcpyAsync(v.data(), vertices_dev, v.size() * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream));
        if (!n.empty()) HIP_TRY(hipMemcpyAsync(n.data(), normals_dev, n.size() * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream));
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        forget_rest(s, mi);
        return update_on_host(s, mi, v.data(), n.empty() ? nullptr : n.data(), mode);
    }
    if (const int rc = agpt::copy_arrays_device(s->ctx->stream, &s->updaters[mi], s->meshes[mi], vertices_dev, normals_dev)) return rc;
    forget_rest(s, mi);
    return update_from_updater(s, prim, mi, mode);
}

int agpt_scene_transform_mesh(agpt_scene* s, int prim, const float* transform16, int mode) {
    {   // the checks of agpt_scene_update_mesh with the mesh's own counts, then the matrix
        const agpt::HostMesh* m = s && s->committed ? mesh_of(s, prim) : nullptr;
        const int dummy = 0;
        if (const int rc = check_update("agpt_scene_transform_mesh", s, prim, &dummy, m ? (int)m->vertices.size() : 0, &dummy,
                                        m ? (int)m->normals.size() : 0, mode))
            return rc;
    }
    if (!transform16) return fail(AGPT_ERR_INVALID, "agpt_scene_transform_mesh: NULL matrix");
    agpt::Mat4 M;
    std::memcpy(M.c, transform16, sizeof(M.c));
    for (float c : M.c)
        if (!std::isfinite(c)) return fail(AGPT_ERR_INVALID, "agpt_scene_transform_mesh: the matrix has a non-finite entry");
    float det = 0;
    const agpt::Mat4 N = agpt::inverse_transpose(M, &det);
    if (det == 0) return fail(AGPT_ERR_INVALID, "agpt_scene_transform_mesh: the matrix is singular (its determinant is exactly 0)");
    const size_t mi = (size_t)s->prims[prim].index;
    HIP_TRY(hipSetDevice(s->ctx->device));
    size_update_state(s);
    agpt_scene::RestPose& rest = s->rest[mi];
    if (!rest.valid) {   // the arrays the mesh last received explicitly: the mirror, brought up to date if they came as device pointers
        if (const int rc = sync_mirror(s, true)) return rc;
        rest.vertices = s->meshes[mi].vertices;
        rest.normals = s->meshes[mi].normals;
        rest.valid = true;
        agpt::drop_rest(s->updaters[mi]);
    }
    if (const int rc = agpt::transform_arrays_device(s->ctx->stream, &s->updaters[mi], s->meshes[mi], rest.vertices, rest.normals, M, N)) return rc;
    return update_from_updater(s, prim, mi, mode);
}

int agpt_scene_set_bvh_builder(agpt_scene* s, int builder) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_bvh_builder: NULL scene");
    if (builder != AGPT_BVH_BUILDER_HOST && builder != AGPT_BVH_BUILDER_DEVICE)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_bvh_builder: unknown builder " + std::to_string(builder));
    s->bvh_builder = builder;
    return AGPT_OK;
}

int agpt_scene_set_shading_arith(agpt_scene* s, int mode) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_shading_arith: NULL scene");
    if (mode != AGPT_SHADING_EXACT && mode != AGPT_SHADING_FAST)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_shading_arith: unknown mode " + std::to_string(mode));
    s->shading_arith = mode;
    return AGPT_OK;
}

int agpt_bvh_build_device(agpt_ctx* c, const float* vertices, int n_vertices, const int32_t* indices, int n_indices,
                          int max_prims_in_node, agpt_bvh_node* nodes_out, int32_t* prim_index_out, int* total_nodes_out,
                          int* max_depth_out, int* on_device_out) {
    if (!c) return fail(AGPT_ERR_INVALID, "agpt_bvh_build_device: NULL context");
    if (const int rc = check_bvh_input("agpt_bvh_build_device", vertices, n_vertices, indices, n_indices)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int total = 0, depth = 0, on_device = 0;
    const int rc = agpt::build_bvh_device(c->stream, vertices, n_vertices, indices, n_indices / 3, max_prims_in_node, nodes_out,
                                          prim_index_out, &total, &depth, &on_device);
    if (rc != AGPT_OK) return rc;
    if (total_nodes_out) *total_nodes_out = total;
    if (max_depth_out) *max_depth_out = depth;
    if (on_device_out) *on_device_out = on_device;
    return AGPT_OK;
}

int agpt_toplevel_build(const float* boxes6, int n, float* nodes8_out) {
    if (!boxes6 || !nodes8_out || n < 1) return fail(AGPT_ERR_INVALID, "agpt_toplevel_build: need at least one box");
    std::vector<uint32_t> payload((size_t)n);
    for (int k = 0; k < n; k++) payload[k] = (uint32_t)k;
    std::vector<float4> nodes;
    agpt::build_skip_tree(boxes6, payload.data(), n, nodes);
    std::memcpy(nodes8_out, nodes.data(), nodes.size() * sizeof(float4));
    return (int)(nodes.size() / 2);
}

int agpt_toplevel_pack16(const float* nodes8, int n_nodes, uint32_t* packed4_out) {
    if (!nodes8 || !packed4_out || n_nodes < 1) return fail(AGPT_ERR_INVALID, "agpt_toplevel_pack16: need at least one node");
    std::vector<float4> nodes((size_t)2 * n_nodes);
    std::memcpy(nodes.data(), nodes8, nodes.size() * sizeof(float4));
    std::vector<uint32_t> packed;
    agpt::pack_skip_tree16(nodes, packed);
    std::memcpy(packed4_out, packed.data(), packed.size() * sizeof(uint32_t));
    return n_nodes;
}

int agpt_create_backdrop(const float origin[3], const float size[3], float radius, int steps, float* vertices, float* normals,
                         float* texcoords, int32_t* indices, int* n_vertices, int* n_indices) {
    if (!origin || !size || !vertices || !normals || !texcoords || !indices || steps < 1)
        return fail(AGPT_ERR_INVALID, "agpt_create_backdrop: bad argument");
    std::vector<v3> v, n;
    std::vector<v2> t;
    std::vector<int32_t> ix;
    agpt::create_backdrop(V3(origin[0], origin[1], origin[2]), V3(size[0], size[1], size[2]), radius, steps, v, n, t, ix);
    for (size_t i = 0; i < v.size(); i++) {
        vertices[3 * i] = v[i].x; vertices[3 * i + 1] = v[i].y; vertices[3 * i + 2] = v[i].z;
        normals[3 * i] = n[i].x; normals[3 * i + 1] = n[i].y; normals[3 * i + 2] = n[i].z;
        texcoords[2 * i] = t[i].x; texcoords[2 * i + 1] = t[i].y;
    }
    std::memcpy(indices, ix.data(), ix.size() * sizeof(int32_t));
    if (n_vertices) *n_vertices = (int)v.size();
    if (n_indices) *n_indices = (int)ix.size() / 3;
    return AGPT_OK;
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

// What a call that runs the wavefront loop sets up once (begin_wavefront): the pool as the kernels see it, how rays are traced and
// counted, which shading kernels run; and what the loop adds up for the call's statistics (fill_stats).
struct WavefrontRun {
    PathBuffers pb;
    Queues q[2];
    bool mis_mode, timing;
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
    run.shade.fast = s->shading_arith == AGPT_SHADING_FAST;   // agpt_scene_set_shading_arith
    run.shade.level = s->shade_level;                         // agpt_scene_commit
    run.shade.lds_tables = shade_tables_fit_lds(s->dev);
    run.shade.env = !s->envs.empty();                         // an InfiniteAreaLight is present
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
    const bool small_batch = (unsigned long long)rcn.NP * (unsigned long long)rcn.S < AGPT_SMALL_BATCH;
    const bool recast = !getenv("AGPT_NO_RECAST");   // (developer knob: emitter pass-throughs through k_shade, an iteration each)
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
                              count, small_batch, recast};
        const TraceLaunch mis{mis_stream, q[cur].mis, &QCOUNT(q[cur], 1), 0, heads[1], pb.mis_o, pb.mis_d,
                              run.mis_mode ? nullptr : pb.mis_hit, run.mis_mode ? pb.mis_ok : nullptr, count, small_batch, false};
        const TraceLaunch shadow{shadow_stream, q[cur].shadow, &QCOUNT(q[cur], 2), 0, heads[2], pb.sh_o, pb.sh_d, nullptr, pb.occluded,
                                 count, small_batch, false};
        auto trace_ext = [&]() { launch_trace_timed<0>(c, run.timing, 0, s->dev, ext); };
        auto trace_mis = [&]() {
            if (run.mis_mode) launch_trace_timed<2>(c, run.timing, 1, s->dev, mis);
            else launch_trace_timed<0>(c, run.timing, 1, s->dev, mis);
        };
        auto trace_shadow = [&]() { launch_trace_timed<1>(c, run.timing, 2, s->dev, shadow); };
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
    for (int mode = 0; mode < 3; ++mode) {
        const unsigned long long* d = dc.dbg + 16 * mode;
        const double steps = (double)(d[0] + d[1] + d[2]);
        if (steps == 0) continue;
        std::fprintf(stderr,
                     "[trace stats mode %d] steps A/B/C %.3g/%.3g/%.3g (%.1f%%/%.1f%%/%.1f%%)  lanes per step A %.1f B %.1f C %.1f  "
                     "active lanes per step %.1f  refills %.3g (%.1f lanes each)  prefilter batches %.3g\n", mode,
                     (double)d[0], (double)d[1], (double)d[2], 100 * d[0] / steps, 100 * d[1] / steps, 100 * d[2] / steps,
                     d[0] ? (double)d[3] / d[0] : 0., d[1] ? (double)d[4] / d[1] : 0., d[2] ? (double)d[5] / d[2] : 0.,
                     (double)d[6] / steps, (double)d[7], d[7] ? (double)d[8] / d[7] : 0., (double)d[9]);
#ifndef AGPT_TRACE_CLOCK
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

// film rows of the row blocks k with k % world == rank (blocks of `block` rows, the last one of a film may be shorter)
static int interleave_rows(int H, int block, int world, int rank) {
    int rows = 0;
    for (int k = rank, y = k * block; y < H; k += world, y = k * block) rows += std::min(block, H - y);
    return rows;
}

// rows of the tile this call renders: rp->h, or with the row interleave on this rank's share of the film (which may be empty)
static int tile_rows(const char* fn, const agpt_render_params* rp, uint32_t& rows) {
    rows = (uint32_t)rp->h;
    if (rp->interleave_block <= 0) return AGPT_OK;
    if (rp->interleave_world < 1 || rp->interleave_rank < 0 || rp->interleave_rank >= rp->interleave_world || rp->x0 != 0 ||
        rp->y0 != 0 || rp->w != rp->width || rp->h != rp->height)
        return fail(AGPT_ERR_INVALID, std::string(fn) + ": row interleave needs the whole film as tile and 0 <= rank < world");
    rows = (uint32_t)interleave_rows(rp->height, rp->interleave_block, rp->interleave_world, rp->interleave_rank);
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
static void trace_rays(agpt_ctx* c, const DevScene& sc, uint32_t n, bool any_hit, int count) {
    const TraceLaunch t{c->stream, nullptr, nullptr, n, c->work.p, c->ext_o.p, c->ext_d.p, c->hit.p, c->occluded.p,
                        count, (unsigned long long)n < AGPT_SMALL_BATCH, false};
    if (any_hit) launch_trace<1>(c, sc, t);
    else launch_trace<0>(c, sc, t);
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
    trace_rays(c, s->dev, (uint32_t)n, any_hit != 0, instrumented);
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    hipLaunchKernelGGL(k_export_hits, blocks, dim3(AGPT_BLOCK), 0, c->stream, s->dev, c->hit.p, c->occluded.p, n, any_hit,
                       d_out);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(c->take_deferred());
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        DevCounters dc;
        HIP_TRY(hipMemcpy(&dc, c->counters.p, sizeof(dc), hipMemcpyDeviceToHost));
        read_counters(dc, stats);
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        stats->trace_ms = ms;
        stats->total_ms = ms;
        stats->trace_launches = 1;
    }
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

// DbgIntegrator::Li (integrator.h:107-118): Scene::Intersect on the GPU, then the hit's uv -- which only this debug view reads, so
// the device keeps no texture coordinates -- from the host copy of the scene in the arithmetic of trianglemesh.cpp:46-57,
// intersectable.h:133 and :187-201.
int agpt_dbg_li_batch(agpt_scene* s, const agpt_ray* rays, int n, float* radiance3_out) {
    if (!s || !rays || !radiance3_out || n < 0) return fail(AGPT_ERR_INVALID, "agpt_dbg_li_batch: bad argument");
    if (n == 0) return AGPT_OK;
    std::vector<agpt_hit> hits((size_t)n);
    const int rc = agpt_intersect_batch(s, rays, n, hits.data(), 0, nullptr);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        float* L = radiance3_out + 3 * (size_t)i;
        L[0] = L[1] = L[2] = 0.f;
        const agpt_hit& h = hits[i];
        if (!h.hit) continue;
        const agpt::HostPrim& hp = s->prims[h.prim];
        float u, v;
        if (hp.type == AGPT_PRIM_MESH) {
            const agpt::HostMesh& m = s->meshes[hp.index];
            float uv[3][2] = {{0, 0}, {1, 0}, {1, 1}};   // a mesh without texture coordinates (trianglemesh.cpp:52-56)
            if (!m.texcoords.empty())
                for (int k = 0; k < 3; ++k) {
                    const v2 t = m.texcoords[m.indices[3 * (h.tri + k) + 2]];
                    uv[k][0] = t.x;
                    uv[k][1] = t.y;
                }
            const float b0 = 1.f - h.b1 - h.b2;
            u = uv[0][0] * b0 + uv[1][0] * h.b1 + uv[2][0] * h.b2;
            v = uv[0][1] * b0 + uv[1][1] * h.b1 + uv[2][1] * h.b2;
        } else {
            const agpt::HostSphere& sp = s->spheres[hp.index];
            const v3 D = normalize(V3(rays[i].d[0], rays[i].d[1], rays[i].d[2]));   // the Ray ctor's (camera.h:6), as k_prepare_rays
            const v3 P = V3(rays[i].o[0], rays[i].o[1], rays[i].o[2]) + h.t * D;
            if (hp.type == AGPT_PRIM_PLANE) {   // centre = O, r / r2 = HalfSize.x / .y
                u = ((P.x - sp.center.x) / sp.r + 1) * .5f;
                v = ((P.z - sp.center.z) / sp.r2 + 1) * .5f;
            } else {
                v3 pHit = P - sp.center;
                if (pHit.x == 0 && pHit.y == 0) pHit.x = AGPT_EPSILON * sp.r;
                float phi = cr_atan2f(pHit.y, pHit.x);
                if (phi < 0) phi += AGPT_TWOPI;
                u = phi * AGPT_INV2PI;
                v = cr_acosf(tclampf(pHit.z / sp.r, -1.f, 1.f)) * AGPT_INVPI;
            }
        }
        if (u == 0 || v == 0) {
            L[0] = 1.f;
        } else {
            L[0] = u / 5;
            L[1] = v / 5;
        }
    }
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
// k_features: material colour + flag and shading normal + t.
int agpt_render_features(agpt_scene* s, const agpt_render_params* rp, float* albedo_dev, float* normal_depth_dev) {
    if (!rp) return fail(AGPT_ERR_INVALID, "agpt_render_features: NULL argument");
    if (rp->spp_begin != 0 || rp->spp_count != 0)
        return fail(AGPT_ERR_INVALID, "agpt_render_features: spp_begin and spp_count must be 0 (one unjittered ray per pixel)");
    if (rp->interleave_block != 0 || rp->interleave_world != 0 || rp->interleave_rank != 0)
        return fail(AGPT_ERR_INVALID, "agpt_render_features: the interleave fields must be 0");
    if (!s || !albedo_dev || !normal_depth_dev) return fail(AGPT_ERR_INVALID, "agpt_render_features: NULL argument");
    if (!s->committed || !s->has_camera) return fail(AGPT_ERR_INVALID, "agpt_render_features: scene not committed or camera not set");
    int rc;
    if ((rc = check_tile("agpt_render_features", rp))) return rc;
    if (albedo_dev == normal_depth_dev) return fail(AGPT_ERR_INVALID, "agpt_render_features: the two outputs are one buffer");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t np64 = (uint64_t)rp->w * (uint64_t)rp->h;
    if (np64 > 0x7FFFFFFFull) return fail(AGPT_ERR_LIMIT, "agpt_render_features: tile too large");
    const uint32_t NP = (uint32_t)np64;
    if ((rc = ensure_pool(c, (size_t)NP, s->dev.n_prims))) return rc;
    s->dev.cam = s->cam;
    const RenderConsts rcn = tile_consts(rp, NP);   // (the interleave fields are 0)
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, sizeof(DevCounters), c->stream));
    HIP_TRY(hipMemsetAsync(c->work.p, 0, AGPT_FRONTIERS * AGPT_QSTRIDE * sizeof(uint32_t), c->stream));
    agpt::launch_feature_rays(c->stream, s->dev, rcn, c->ext_o.p, c->ext_d.p);
    trace_rays(c, s->dev, NP, false, 0);
    agpt::launch_features(c->stream, s->dev, s->shade_level, rcn, s->d_colors.p, c->hit.p, c->ext_o.p, c->ext_d.p, (float4*)albedo_dev,
                          (float4*)normal_depth_dev);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(c->take_deferred());
    return AGPT_OK;
}

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
    agpt::launch_denoise_prepare(c->stream, dc, (const float4*)accum_dev, moment2_dev, (const float4*)albedo_dev, buf[cur]);
    for (int i = 0; i < p->iterations; ++i, cur ^= 1) {
        dc.step = 1 << i;
        dc.last = i == p->iterations - 1;
        agpt::launch_denoise_pass(c->stream, dc, buf[cur], (const float4*)albedo_dev, (const float4*)normal_depth_dev, buf[cur ^ 1]);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

int agpt_camera_vectors(const agpt_camera_desc* d, float out22[22]) {
    if (!d || !out22) return fail(AGPT_ERR_INVALID, "agpt_camera_vectors: NULL argument");
    const DevCamera cam = agpt::make_camera(*d);
    static_assert(sizeof(DevCamera) == 22 * sizeof(float), "origin, u, v, w, lower_left_corner, horizontal, vertical, lens_radius");
    std::memcpy(out22, &cam, sizeof(cam));
    return AGPT_OK;
}

// One k_temporal launch: this frame's buffers plus the previous frame's history, reprojected, into the history buffers the next
// agpt_denoise and the next frame's call read.
int agpt_temporal_accumulate(agpt_ctx* c, const agpt_temporal_params* p, const float* accum_cur_dev, const float* moment2_cur_dev,
                             const float* albedo_cur_dev, const float* normal_depth_cur_dev, const float* hist_accum_prev_dev,
                             const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
                             float* hist_accum_out_dev, float* hist_moment2_out_dev) {
    if (!p) return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: NULL argument");
    if (p->width <= 0 || p->height <= 0 || (uint64_t)p->width * (uint64_t)p->height > 0x7FFFFFFFull)
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: bad film size");
    if (!(p->max_history > 0.f) || std::isinf(p->max_history))
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: max_history must be positive and finite");
    if (!(p->depth_tol >= 0.f) || std::isinf(p->depth_tol))
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: depth_tol must be non-negative and finite");
    if (!(p->normal_cos >= -1.f && p->normal_cos <= 1.f))
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: normal_cos must be in [-1, 1]");
    if (!c || !accum_cur_dev || !moment2_cur_dev || !albedo_cur_dev || !normal_depth_cur_dev || !hist_accum_out_dev || !hist_moment2_out_dev)
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: NULL argument");
    const float* prev[4] = {hist_accum_prev_dev, hist_moment2_prev_dev, albedo_prev_dev, normal_depth_prev_dev};
    const int n_prev = (prev[0] != nullptr) + (prev[1] != nullptr) + (prev[2] != nullptr) + (prev[3] != nullptr);
    if (n_prev != 0 && n_prev != 4)
        return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: the four prev buffers must be all NULL (first frame) or all given");
    const float* in[8] = {accum_cur_dev, moment2_cur_dev, albedo_cur_dev, normal_depth_cur_dev, prev[0], prev[1], prev[2], prev[3]};
    for (const float* q : in)
        if (q && (q == hist_accum_out_dev || q == hist_moment2_out_dev))
            return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: an output aliases an input");
    if (hist_accum_out_dev == hist_moment2_out_dev) return fail(AGPT_ERR_INVALID, "agpt_temporal_accumulate: the two outputs are one buffer");
    HIP_TRY(hipSetDevice(c->device));
    TemporalConsts tc{};
    tc.W = p->width; tc.H = p->height;
    tc.identity = std::memcmp(&p->cam_prev, &p->cam_cur, sizeof(agpt_camera_desc)) == 0;
    tc.max_history = p->max_history; tc.depth_tol = p->depth_tol; tc.normal_cos = p->normal_cos;
    tc.cur = agpt::make_camera(p->cam_cur);
    tc.prev = agpt::make_camera(p->cam_prev);
    agpt::launch_temporal(c->stream, tc, (const float4*)accum_cur_dev, moment2_cur_dev, (const float4*)albedo_cur_dev,
                          (const float4*)normal_depth_cur_dev, (const float4*)hist_accum_prev_dev, hist_moment2_prev_dev,
                          (const float4*)albedo_prev_dev, (const float4*)normal_depth_prev_dev, (float4*)hist_accum_out_dev, hist_moment2_out_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
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
    HIP_TRY(hipMemcpyAsync(out_rgb, d.p, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

int agpt_resolve_counts(agpt_ctx* c, const float* accum_dev, int n_pixels, uint32_t* out_rgb) {
    if (!c || !accum_dev || !out_rgb || n_pixels <= 0) return fail(AGPT_ERR_INVALID, "agpt_resolve_counts: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> d;
    HIP_TRY(d.alloc((size_t)n_pixels));
    agpt::launch_resolve_counts(c->stream, (const float4*)accum_dev, n_pixels, d.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_rgb, d.p, (size_t)n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

// ---- known-answer entry points ------------------------------------------------------------------------------
int agpt_kat_bsdf_eval(agpt_scene* s, int material, int n, const float* wo3, const float* wi3, float* f3_out, float* pdf_out) {
    if (!s || !s->committed || material < 0 || material >= (int)s->materials.size() || n <= 0 || !wo3 || !wi3 || !f3_out || !pdf_out)
        return fail(AGPT_ERR_INVALID, "agpt_kat_bsdf_eval: bad argument");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_wo, d_wi, d_f, d_p;
    HIP_TRY(d_wo.alloc(3 * (size_t)n));
    HIP_TRY(d_wi.alloc(3 * (size_t)n));
    HIP_TRY(d_f.alloc(3 * (size_t)n));
    HIP_TRY(d_p.alloc((size_t)n));
    HIP_TRY(hipMemcpy(d_wo.p, wo3, 12 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_wi.p, wi3, 12 * (size_t)n, hipMemcpyHostToDevice));
    if (s->shading_arith == AGPT_SHADING_FAST)
        agpt::launch_kat_bsdf_eval_fast(c->stream, s->dev, material, n, d_wo.p, d_wi.p, d_f.p, d_p.p);
    else
        hipLaunchKernelGGL(k_kat_bsdf_eval, dim3((n + 63) / 64), dim3(64), 0, c->stream, s->dev, material, n, d_wo.p, d_wi.p, d_f.p, d_p.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(f3_out, d_f.p, 12 * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pdf_out, d_p.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return AGPT_OK;
}

int agpt_kat_bsdf_sample(agpt_scene* s, int material, int n, const float* wo3, const float* u2, float* wi3_out, float* f3_out,
                         float* pdf_out, int32_t* specular_out) {
    if (!s || !s->committed || material < 0 || material >= (int)s->materials.size() || n <= 0 || !wo3 || !u2 || !wi3_out ||
        !f3_out || !pdf_out || !specular_out)
        return fail(AGPT_ERR_INVALID, "agpt_kat_bsdf_sample: bad argument");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_wo, d_u, d_wi, d_f, d_p;
    DevBuf<int32_t> d_s;
    HIP_TRY(d_wo.alloc(3 * (size_t)n));
    HIP_TRY(d_u.alloc(2 * (size_t)n));
    HIP_TRY(d_wi.alloc(3 * (size_t)n));
    HIP_TRY(d_f.alloc(3 * (size_t)n));
    HIP_TRY(d_p.alloc((size_t)n));
    HIP_TRY(d_s.alloc((size_t)n));
    HIP_TRY(hipMemcpy(d_wo.p, wo3, 12 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_u.p, u2, 8 * (size_t)n, hipMemcpyHostToDevice));
    if (s->shading_arith == AGPT_SHADING_FAST)
        agpt::launch_kat_bsdf_sample_fast(c->stream, s->dev, material, n, d_wo.p, d_u.p, d_wi.p, d_f.p, d_p.p, d_s.p);
    else
        hipLaunchKernelGGL(k_kat_bsdf_sample, dim3((n + 63) / 64), dim3(64), 0, c->stream, s->dev, material, n, d_wo.p, d_u.p, d_wi.p, d_f.p,
                           d_p.p, d_s.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(wi3_out, d_wi.p, 12 * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(f3_out, d_f.p, 12 * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pdf_out, d_p.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(specular_out, d_s.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return AGPT_OK;
}

int agpt_kat_normal_map(agpt_ctx* c, int n, const float* ns3, const float* ss3, const float* rgb3, float scale, float* ns_out3) {
    if (!c || n <= 0 || !ns3 || !ss3 || !rgb3 || !ns_out3) return fail(AGPT_ERR_INVALID, "agpt_kat_normal_map: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_ns, d_ss, d_rgb, d_o;
    HIP_TRY(d_ns.alloc(3 * (size_t)n));
    HIP_TRY(d_ss.alloc(3 * (size_t)n));
    HIP_TRY(d_rgb.alloc(3 * (size_t)n));
    HIP_TRY(d_o.alloc(3 * (size_t)n));
    HIP_TRY(hipMemcpy(d_ns.p, ns3, 12 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ss.p, ss3, 12 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_rgb.p, rgb3, 12 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_kat_normal_map, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, d_ns.p, d_ss.p, d_rgb.p, scale, d_o.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(ns_out3, d_o.p, 12 * (size_t)n, hipMemcpyDeviceToHost));
    return AGPT_OK;
}

int agpt_kat_rng(agpt_ctx* c, uint32_t pixel, uint32_t wh, uint32_t sample, uint32_t seed_base, int n, float* out,
                 uint32_t* seed_out) {
    if (!c || n <= 0 || !out || !seed_out) return fail(AGPT_ERR_INVALID, "agpt_kat_rng: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_o;
    DevBuf<uint32_t> d_s;
    HIP_TRY(d_o.alloc((size_t)n));
    HIP_TRY(d_s.alloc(1));
    hipLaunchKernelGGL(k_kat_rng, dim3(1), dim3(64), 0, c->stream, pixel, wh, sample, seed_base, n, d_o.p, d_s.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, d_o.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(seed_out, d_s.p, 4, hipMemcpyDeviceToHost));
    return AGPT_OK;
}

int agpt_kat_distribution1d(agpt_ctx* c, const float* func, int n, const float* u, int k, float* cdf_out, float* func_int_out,
                            float* x_out, float* pdf_out) {
    if (!c || !func || n <= 0 || k < 0 || (k && (!u || !x_out || !pdf_out)))
        return fail(AGPT_ERR_INVALID, "agpt_kat_distribution1d: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float> cdf((size_t)n + 1);
    const float func_int = agpt::build_distribution1d(func, n, cdf.data());
    if (cdf_out) memcpy(cdf_out, cdf.data(), 4 * cdf.size());
    if (func_int_out) *func_int_out = func_int;
    if (k == 0) return AGPT_OK;
    DevBuf<float> d_f, d_c, d_u, d_x, d_p;
    HIP_TRY(d_f.alloc((size_t)n));
    HIP_TRY(d_c.alloc((size_t)n + 1));
    HIP_TRY(d_u.alloc((size_t)k));
    HIP_TRY(d_x.alloc((size_t)k));
    HIP_TRY(d_p.alloc((size_t)k));
    HIP_TRY(hipMemcpy(d_f.p, func, 4 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_c.p, cdf.data(), 4 * cdf.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_u.p, u, 4 * (size_t)k, hipMemcpyHostToDevice));
    DevEnv e{};
    e.func = d_f.p;
    e.cdf = d_c.p;
    e.n = n;
    e.funcInt = func_int;
    hipLaunchKernelGGL(k_kat_distribution1d, dim3((k + 63) / 64), dim3(64), 0, c->stream, e, d_u.p, k, d_x.p, d_p.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(x_out, d_x.p, 4 * (size_t)k, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pdf_out, d_p.p, 4 * (size_t)k, hipMemcpyDeviceToHost));
    return AGPT_OK;
}


// ---- multi-GPU: gather of the per-rank tile buffers ------------------------------------------------
// RCCL is bound at run time (dlopen of the librccl already in the process, else the ROCm one): a single-GPU host never
// loads it, and a host that also uses PyTorch shares PyTorch's copy instead of getting a second set of nccl* symbols.
}  // extern "C"

#include <dlfcn.h>
#include <rccl/rccl.h>

namespace {

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi* rccl() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api.lib ? &api : nullptr;
    tried = true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (api.lib) break;
    }
    if (!api.lib) return nullptr;
    bool ok = true;
    auto sym = [&](const char* n) {
        void* p = dlsym(api.lib, n);
        ok = ok && p != nullptr;
        return p;
    };
    api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.Send = (decltype(api.Send))sym("ncclSend");
    api.Recv = (decltype(api.Recv))sym("ncclRecv");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    if (!ok) {
        dlclose(api.lib);
        api.lib = nullptr;
        return nullptr;
    }
    return &api;
}

// compact rank buffer -> full accumulator.  Rank r owns the film's row blocks k with k % world == r; its j-th block sits at
// compact rows [j*block, j*block + h) with the rows flipped inside the block (agpt_render's interleave layout), the full
// accumulator is Accumulator::pixels: row (H-1-y) (myapp.h:17-19).  One thread per float4.
__global__ void k_deinterleave(const float4* __restrict__ compact, float4* __restrict__ full, int W, int H, int block, int world,
                               int rank, int rows_local) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows_local * (size_t)W) return;
    const int row = (int)(i / (size_t)W), x = (int)(i - (size_t)row * (size_t)W);
    const int j = row / block, r_in = row % block;
    const int yb = (j * world + rank) * block;      // first film row of the block
    const int hb = min(block, H - yb);
    if (r_in >= hb) return;
    const int y = yb + (hb - 1 - r_in);             // compact row j*block + (hb-1-within) holds film row yb + within
    full[(size_t)(H - 1 - y) * (size_t)W + (size_t)x] = compact[i];
}

}  // namespace

struct agpt_comm {
    agpt_ctx* ctx = nullptr;
    int world = 1, rank = 0;
    ncclComm_t comm = nullptr;
    DevBuf<float4> staging;   // rank 0: one compact buffer per peer
};

extern "C" {

int agpt_comm_unique_id(void* id128) {
    if (!id128) return fail(AGPT_ERR_INVALID, "agpt_comm_unique_id: NULL argument");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    RcclApi* R = rccl();
    if (!R) return fail(AGPT_ERR_DEVICE, "agpt_comm_unique_id: librccl.so could not be loaded");
    ncclResult_t e = R->GetUniqueId((ncclUniqueId*)id128);
    if (e != ncclSuccess) return fail(AGPT_ERR_DEVICE, std::string("ncclGetUniqueId: ") + R->GetErrorString(e));
    return AGPT_OK;
}

int agpt_comm_init(agpt_ctx* c, const void* id128, int world, int rank, agpt_comm** out) {
    if (!c || !out || world < 1 || rank < 0 || rank >= world || (world > 1 && !id128))
        return fail(AGPT_ERR_INVALID, "agpt_comm_init: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<agpt_comm> m(new agpt_comm());
    m->ctx = c;
    m->world = world;
    m->rank = rank;
    if (world > 1) {   // a single rank needs no communicator (and no RCCL)
        RcclApi* R = rccl();
        if (!R) return fail(AGPT_ERR_DEVICE, "agpt_comm_init: librccl.so could not be loaded");
        ncclUniqueId id;
        std::memcpy(&id, id128, sizeof(id));
        ncclResult_t e = R->CommInitRank(&m->comm, world, id, rank);
        if (e != ncclSuccess) return fail(AGPT_ERR_DEVICE, std::string("ncclCommInitRank: ") + R->GetErrorString(e));
    }
    *out = m.release();
    return AGPT_OK;
}

void agpt_comm_destroy(agpt_comm* m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    if (m->comm) (void)rccl()->CommDestroy(m->comm);
    delete m;
}

int agpt_deinterleave_tiles(agpt_ctx* c, const float* compact_dev, int width, int height, int block_rows, int world, int rank,
                            float* full_accum_dev) {
    if (!c || !compact_dev || !full_accum_dev || width <= 0 || height <= 0 || block_rows <= 0 || world < 1 || rank < 0 || rank >= world)
        return fail(AGPT_ERR_INVALID, "agpt_deinterleave_tiles: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const int rows = interleave_rows(height, block_rows, world, rank);
    if (!rows) return AGPT_OK;
    const size_t n = (size_t)rows * (size_t)width;
    hipLaunchKernelGGL(k_deinterleave, agpt_blocks(n), dim3(AGPT_BLOCK), 0, c->stream, (const float4*)compact_dev,
                       (float4*)full_accum_dev, width, height, block_rows, world, rank, rows);
    HIP_TRY(hipGetLastError());
    return AGPT_OK;
}

int agpt_gather_tiles(agpt_comm* m, const float* local_accum_dev, int width, int height, int block_rows, float* full_accum_dev) {
    if (!m || !local_accum_dev || width <= 0 || height <= 0 || block_rows <= 0 || (m->rank == 0 && !full_accum_dev))
        return fail(AGPT_ERR_INVALID, "agpt_gather_tiles: bad argument");
    agpt_ctx* c = m->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int world = m->world;
    int max_rows = 0;
    for (int r = 0; r < world; r++) max_rows = std::max(max_rows, interleave_rows(height, block_rows, world, r));
    const size_t slot = (size_t)max_rows * (size_t)width;   // float4 per rank buffer
    if (world > 1) {
        RcclApi* R = rccl();
        ncclResult_t e = ncclSuccess;
        if (m->rank == 0) {
            int rc = m->staging.ensure(slot * (size_t)(world - 1));
            if (rc) return rc;
            // grouped point-to-point: every peer's buffer travels its own direct xGMI link to rank 0 (not a ring)
            // (a group that was started is always ended, also when a call inside it fails: the first error is reported)
            e = R->GroupStart();
            if (e == ncclSuccess) {
                for (int r = 1; r < world && e == ncclSuccess; r++) {
                    const size_t n = (size_t)interleave_rows(height, block_rows, world, r) * (size_t)width * 4;
                    if (n) e = R->Recv(m->staging.p + slot * (size_t)(r - 1), n, ncclFloat, r, m->comm, c->stream);
                }
                const ncclResult_t e_end = R->GroupEnd();
                if (e == ncclSuccess) e = e_end;
            }
        } else {
            const size_t n = (size_t)interleave_rows(height, block_rows, world, m->rank) * (size_t)width * 4;
            e = R->GroupStart();
            if (e == ncclSuccess) {
                if (n) e = R->Send(local_accum_dev, n, ncclFloat, 0, m->comm, c->stream);
                const ncclResult_t e_end = R->GroupEnd();
                if (e == ncclSuccess) e = e_end;
            }
        }
        if (e != ncclSuccess) return fail(AGPT_ERR_DEVICE, std::string("agpt_gather_tiles: ") + R->GetErrorString(e));
    }
    if (m->rank == 0) {
        for (int r = 0; r < world; r++) {
            const float* src = r == 0 ? local_accum_dev : (const float*)(m->staging.p + slot * (size_t)(r - 1));
            int rc = agpt_deinterleave_tiles(c, src, width, height, block_rows, world, r, full_accum_dev);
            if (rc) return rc;
        }
    }
    return AGPT_OK;
}

}  // extern "C"
