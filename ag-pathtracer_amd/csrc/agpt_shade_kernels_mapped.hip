// agpt_shade_kernels_mapped.hip -- k_shade_mapped: the shading kernel of level 2 (MAPPED) in exact arithmetic; see the table in agpt_shade_kernels.h.
#define AGPT_SHADE_LEVEL 2
#define AGPT_SHADE_FAST 0
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
