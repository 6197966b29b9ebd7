// agpt_shade_kernels_textured_fast.hip -- k_shade_textured_fast: the shading kernel of level 1 (TEXTURED) in fast arithmetic; see the table in agpt_shade_kernels.h.
#define AGPT_SHADE_LEVEL 1
#define AGPT_SHADE_FAST 1
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
