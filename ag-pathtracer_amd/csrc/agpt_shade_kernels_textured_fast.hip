// agpt_shade_kernels_textured_fast.hip -- k_shade_textured_fast: the TEXTURED variant of the shading kernel (AGPT_SHADE_TEXTURED, agpt_shade_kernels.h) in fast arithmetic (AGPT_SHADE_FAST, agpt_shade_arith.h).
// agpt_scene_set_material_texture on any material of a scene selects it at launch; scenes without textures never run it.  Same flags
// as agpt_shade_kernels_fast.hip (MachineLICM off, four waves per SIMD, -ffp-contract=off).
#define AGPT_SHADE_FAST 1
#define AGPT_SHADE_TEXTURED 1
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"

namespace agpt {

void launch_shade_textured_fast(hipStream_t stream, int grid, bool lds_tables, bool env, const DevScene& sc, const RenderConsts& rc,
                     const PathBuffers& pb, const Queues& qin, const Queues& qout, DevCounters* counters, uint32_t* tile_heads) {
    const dim3 g(grid), b(AGPT_BLOCK);
    if (lds_tables && env) hipLaunchKernelGGL((k_shade_textured_fast<true, true>), g, b, 0, stream, sc, rc, pb, qin, qout, counters, tile_heads);
    else if (lds_tables) hipLaunchKernelGGL((k_shade_textured_fast<true, false>), g, b, 0, stream, sc, rc, pb, qin, qout, counters, tile_heads);
    else if (env) hipLaunchKernelGGL((k_shade_textured_fast<false, true>), g, b, 0, stream, sc, rc, pb, qin, qout, counters, tile_heads);
    else hipLaunchKernelGGL((k_shade_textured_fast<false, false>), g, b, 0, stream, sc, rc, pb, qin, qout, counters, tile_heads);
}

}  // namespace agpt
