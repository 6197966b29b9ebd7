// agpt_shade_kernels_normal.hip -- k_shade_normal: the shading kernel of level 4 (NORMAL) in exact arithmetic; see the table in agpt_shade_kernels.h.
#define AGPT_SHADE_LEVEL 4
#define AGPT_SHADE_FAST 0
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
