// agpt_shade_kernels_sampled_fast.hip -- k_shade_sampled_fast: the shading kernel of level 3 (SAMPLED) in fast arithmetic; see the table in agpt_shade_kernels.h.
#define AGPT_SHADE_LEVEL 3
#define AGPT_SHADE_FAST 1
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
