// agpt_comm.hip -- the multi-GPU entry points of include/agpt.h: the communicator, and the gather of the per-rank tile buffers into
// rank 0's full accumulator with its own kernel (k_deinterleave).
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "agpt_internal.h"

using agpt::fail;

// ---- multi-GPU: gather of the per-rank tile buffers ------------------------------------------------
// RCCL is bound at run time (dlopen of the librccl already in the process, else the ROCm one): a single-GPU host never
// loads it, and a host that also uses PyTorch shares PyTorch's copy instead of getting a second set of nccl* symbols.
namespace {

// the nccl* functions the gather uses, listed once: X(name without the prefix)
#define AGPT_RCCL_FUNCTIONS(X) X(GetUniqueId) X(CommInitRank) X(CommDestroy) X(GroupStart) X(GroupEnd) X(Send) X(Recv) X(GetErrorString)

struct RcclApi {
    void* lib = nullptr;
#define X(name) decltype(&nccl##name) name = nullptr;
    AGPT_RCCL_FUNCTIONS(X)
#undef X
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
#define X(name) api.name = (decltype(api.name))sym("nccl" #name);
    AGPT_RCCL_FUNCTIONS(X)
#undef X
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
    const int rows = agpt::interleave_rows(height, block_rows, world, rank);
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
    for (int r = 0; r < world; r++) max_rows = std::max(max_rows, agpt::interleave_rows(height, block_rows, world, r));
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
                    const size_t n = (size_t)agpt::interleave_rows(height, block_rows, world, r) * (size_t)width * 4;
                    if (n) e = R->Recv(m->staging.p + slot * (size_t)(r - 1), n, ncclFloat, r, m->comm, c->stream);
                }
                const ncclResult_t e_end = R->GroupEnd();
                if (e == ncclSuccess) e = e_end;
            }
        } else {
            const size_t n = (size_t)agpt::interleave_rows(height, block_rows, world, m->rank) * (size_t)width * 4;
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
