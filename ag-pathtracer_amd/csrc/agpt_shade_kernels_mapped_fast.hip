// agpt_shade_kernels_mapped_fast.hip -- k_shade_mapped_fast: the shading kernel of level 2 (MAPPED) in fast arithmetic; see the table in agpt_shade_kernels.h.
#define AGPT_SHADE_LEVEL 2
#define AGPT_SHADE_FAST 1
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
