// agpt_shade_kernels.hip -- translation unit of the shading kernels (agpt_shade_kernels.h) and their host-side launchers (the unit's own come with the header; launch_shading picks the unit).
// build.py compiles it with -mllvm -disable-machine-licm (see the header for why); the trace kernels are in agpt_trace_kernels.hip,
// the rest of the library in units of its own (build.py: SOURCES).
#define AGPT_SHADE_LEVEL 0
#define AGPT_SHADE_FAST 0
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"

namespace agpt {

bool shade_tables_fit_lds(int n_prims, int n_materials, int n_lights) {
    return n_prims <= AGPT_SHADE_LDS_PRIMS && n_materials <= AGPT_SHADE_LDS_MATERIALS && n_lights <= AGPT_SHADE_LDS_LIGHTS;
}

void launch_shading(hipStream_t stream, const ShadeVariant& v, int shade_grid, const DevScene& sc, const RenderConsts& rc,
                    const PathBuffers& pb, const Queues& qin, const Queues& qout, DevCounters* counters, uint32_t* tile_heads) {
#define X(level, suffix) {launch_shade##suffix, launch_shade##suffix##_fast},
    static ShadeLaunch* const table[SHADE_LEVELS][2] = {AGPT_SHADE_LEVEL_LIST(X)};   // (rows in level order)
#undef X
    table[v.level][v.fast](stream, shade_grid, v.lds_tables, v.env, sc, rc, pb, qin, qout, counters, tile_heads);
}

// The units above level 0 have no finishing kernels (no BSDF and no material in them): their batches use the plain
// unit's of the same arithmetic.
void launch_accumulate(hipStream_t stream, bool fast, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, float4* accum,
                       DevCounters* counters) {
    (fast ? finish_accumulate_fast : finish_accumulate)(stream, sc, rc, pb, accum, counters);
}
void launch_export_li(hipStream_t stream, bool fast, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t n,
                      float* radiance3, uint32_t* rng_out) {
    (fast ? finish_export_li_fast : finish_export_li)(stream, sc, rc, pb, n, radiance3, rng_out);
}
void launch_finish_paths(hipStream_t stream, bool fast, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t n) {
    (fast ? finish_paths_fast : finish_paths)(stream, sc, rc, pb, n);
}

}  // namespace agpt
