// agpt_motion.h -- the launchers of the motion-vector unit (agpt_motion.hip, which also defines agpt_scene_snapshot_positions and
// agpt_temporal_accumulate_motion) that agpt_render_features_motion (agpt_api.hip) calls.
#pragma once

#include "agpt_wavefront.h"

namespace agpt {
// gen[3 * gid ..] = the positions of the slot whose tri_verts record names triangle gid (w lanes 0), for the n_tris slots of the scene
void launch_snapshot_positions(hipStream_t stream, const float4* tri_verts, uint32_t n_tris, float4* gen);
// prev_point (indexed like k_features' outputs) from the hits and rays of the feature pass, the two generations of positions and the
// two of analytic records (agpt_analytic.h; n_prims == 0: none, a sphere or a plane then never counts as moved)
void launch_motion(hipStream_t stream, const RenderConsts& rc, const DevHit* hits, const float4* ray_o, const float4* ray_d,
                   const float4* gen_old, const float4* gen_new, uint32_t n_tris, const float4* an_old, const float4* an_new, uint32_t n_prims,
                   float4* prev_point);
}  // namespace agpt
