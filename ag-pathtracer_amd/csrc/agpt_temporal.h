// agpt_temporal.h -- the constants of k_temporal (agpt_temporal.hip, which also defines agpt_temporal_accumulate).
#pragma once

#include "agpt_denoise.h"

struct TemporalConsts {
    int32_t W, H;
    int32_t identity;      // 1: the two camera descriptions are the same bytes -- every pixel reads its own history, no arithmetic
    float max_history, depth_tol, normal_cos;
    DevCamera cur, prev;   // make_camera of the two descriptions
};
