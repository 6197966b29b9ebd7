// agpt_temporal_clamp.h -- the constants of k_temporal_clamp (agpt_temporal_clamp.hip, which also defines
// agpt_temporal_accumulate_clamped): the clamp's parameters as the kernel takes them and the LDS tile its blocks stage.
#pragma once

#include "agpt_temporal.h"

#define AGPT_TC_RADIUS_MAX 3
#define AGPT_TC_ALBEDO_FLOOR 1e-3f   // agpt_denoise's demodulation floor
// a block's tile of k_denoise_pass' tiling plus a halo of the largest radius, one float4 per pixel: 70 x 10 x 16 B = 11200 B
#define AGPT_TC_TILE_W (AGPT_DN_TX + 2 * AGPT_TC_RADIUS_MAX)
#define AGPT_TC_TILE_H (AGPT_DN_TY + 2 * AGPT_TC_RADIUS_MAX)
#define AGPT_TC_LDS_BYTES (AGPT_TC_TILE_W * AGPT_TC_TILE_H * 16)

struct TemporalClampConsts {
    int32_t radius;
    int32_t demodulate;
    int32_t motion;        // 1: prev_point_cur is given (agpt_temporal_accumulate_motion's step 3), 0: it is NULL
    float gamma, clamped_max_history;
};
