// agpt_adaptive.h -- host-side launchers of the adaptive-sampling unit (agpt_adaptive.hip, which also defines agpt_resolve_counts),
// used by agpt_render_adaptive in agpt_api.hip.
#pragma once

#include "agpt_wavefront.h"

// select / compact work split: a block of AGPT_BLOCK threads covers AGPT_ADAPT_PER_THREAD passes of AGPT_BLOCK tile pixels
#define AGPT_ADAPT_PER_THREAD 16u
#define AGPT_ADAPT_BLOCK_PIXELS (AGPT_BLOCK * AGPT_ADAPT_PER_THREAD)
// words of the select / compact passes the host reads back after each round's decision
enum {
    AGPT_AW_INVALID = 0,   // tile pixels whose count (accum.w) is not an integer in [0, 2^24] on the step_spp grid
    AGPT_AW_INV_MIN = 1,   // max over the valid pixels of ~n (= ~min n; 0 when there is none)
    AGPT_AW_MAX = 2,       // max n over the valid pixels
    AGPT_AW_STOPPED = 3,   // pixels with min_spp <= n < max_spp that pass the stop test
    AGPT_AW_ACTIVE = 4,    // length of the active list (k_adaptive_compact)
    AGPT_AW_COUNT = 8
};

struct AdaptiveConsts {
    int32_t min_spp, max_spp, step_spp;
    float rel_error, abs_floor;
};

namespace agpt {
// words[AGPT_AW_INVALID .. AGPT_AW_STOPPED] must be zero before the select pass
void launch_adaptive_select(hipStream_t stream, const RenderConsts& rc, const AdaptiveConsts& ac, const float4* accum, const float* moment2,
                            uint32_t* masks, uint32_t* block_counts, uint32_t* words);
void launch_adaptive_compact(hipStream_t stream, uint32_t np, const uint32_t* masks, const uint32_t* block_counts, uint32_t* list,
                             uint32_t* words);
// rc: the tile (rc.NP) and the samples per listed pixel of this batch (rc.S); the pixels are list[a0 .. a0 + na) (list NULL:
// the local pixels a0 .. a0 + na themselves)
void launch_generate_list(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, const uint32_t* list, uint32_t a0, uint32_t na,
                          const float4* accum, const PathBuffers& pb, const Queues& q);
void launch_accumulate_list(hipStream_t stream, const RenderConsts& rc, const uint32_t* list, uint32_t a0, uint32_t na, const PathBuffers& pb,
                            float4* accum, float* moment2, DevCounters* counters);
}  // namespace agpt
