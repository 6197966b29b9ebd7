// agpt_shade_kernels_normal_fast.hip -- k_shade_normal_fast: the shading kernel of level 4 (NORMAL) in fast arithmetic; see the table in agpt_shade_kernels.h.
#define AGPT_SHADE_LEVEL 4
#define AGPT_SHADE_FAST 1
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
