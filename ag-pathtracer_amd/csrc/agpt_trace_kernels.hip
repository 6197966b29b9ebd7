// agpt_trace_kernels.hip -- translation unit of the trace kernels (agpt_trace_kernels.h) and their host-side launchers: launch_trace
// picks one of the 40 k_trace_fast, 8 k_trace and 3 k_candidates instantiations for a TraceLaunch (agpt_internal.h).  The only unit
// that includes agpt_trace_kernels.h.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "agpt_internal.h"
#include "agpt_trace_kernels.h"

static int trace_grid(const agpt_ctx* c) { return c->num_cus * c->blocks_per_cu; }           // generic kernel
static int fast_grid(const agpt_ctx* c) { return c->num_cus * c->fast_blocks_per_cu; }       // production kernel

namespace agpt {

bool use_fast_trace(const agpt_ctx* c, const DevScene& sc, int count) {
    return count != 1 && sc.n_prims <= 64 * AGPT_MAX_CHUNKS && !c->force_generic;
}

}  // namespace agpt
using agpt::TraceLaunch;
using agpt::use_fast_trace;

template <int MODE, bool COUNT, bool SPILL, bool PEEK>
static void launch_trace_fast(agpt_ctx* c, const DevScene& sc, const TraceLaunch& t) {
    const dim3 block(AGPT_BLOCK), g(fast_grid(c));
    const int refill = MODE == 0 ? c->refill : c->refill_any;
    // (developer knob, read at each launch: AGPT_ROOT_STEP=1 makes short-list launches enter every mesh at its root pair again)
    const bool root_entry = !getenv("AGPT_ROOT_STEP");
    if constexpr (MODE == 0 && !COUNT) {
        if (t.coherent && sc.n_prims <= 64) {   // (a wave takes a whole 64-ray chunk, and only when it is empty: refill = 64)
            hipLaunchKernelGGL((k_trace_fast<0, AGPT_FAST_STACK, false, false, SPILL, PEEK, true>), g, block, 0, t.stream, sc, t.queue,
                               t.count_ptr, t.count_imm, t.work_head, t.ro, t.rd, t.hits, t.occ, c->counters.p, 64, 0u, c->spill.p,
                               (const unsigned long long*)nullptr, (const uint32_t*)nullptr, t.recast, (const float4*)c->beta4.p, c->L4.p,
                               root_entry);
            return;
        }
    }
    if (sc.n_prims <= 64) {
        hipLaunchKernelGGL((k_trace_fast<MODE, AGPT_FAST_STACK, false, COUNT, SPILL, PEEK>), g, block, 0, t.stream, sc, t.queue, t.count_ptr,
                           t.count_imm, t.work_head, t.ro, t.rd, t.hits, t.occ, c->counters.p,
                           refill, 0u, c->spill.p, (const unsigned long long*)nullptr, (const uint32_t*)nullptr, MODE == 0 && t.recast,
                           (const float4*)c->beta4.p, c->L4.p, root_entry);
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
                       (float4*)nullptr, false);
}

template <bool ANY, bool COUNT, int DEPTH>
static void launch_trace_generic(agpt_ctx* c, int grid, const DevScene& sc, const TraceLaunch& t) {
    hipLaunchKernelGGL((k_trace<ANY, COUNT, DEPTH>), dim3(grid), dim3(AGPT_BLOCK), 0, t.stream, sc, t.queue, t.count_ptr, t.count_imm,
                       t.work_head, t.ro, t.rd, t.hits, t.occ, c->counters.p);
}

// MODE 0 closest, 1 any-hit, 2 MIS query (production kernel only; the generic kernel traces MIS rays as closest hits)
template <int MODE>
static void launch_trace_mode(agpt_ctx* c, const DevScene& sc, const TraceLaunch& t) {
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

void agpt::launch_trace(agpt_ctx* c, int mode, const DevScene& sc, const TraceLaunch& t) {
    switch (mode) {
        case 0: launch_trace_mode<0>(c, sc, t); break;
        case 1: launch_trace_mode<1>(c, sc, t); break;
        default: launch_trace_mode<2>(c, sc, t); break;
    }
}
