// agpt_shade_kernels_sampled.hip -- k_shade_sampled: the shading kernel of level 3 (SAMPLED) in exact arithmetic; see the table in agpt_shade_kernels.h.
#define AGPT_SHADE_LEVEL 3
#define AGPT_SHADE_FAST 0
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
