// agpt_shade_kernels_textured.hip -- k_shade_textured: the shading kernel of level 1 (TEXTURED) in exact arithmetic; see the table in agpt_shade_kernels.h.
#define AGPT_SHADE_LEVEL 1
#define AGPT_SHADE_FAST 0
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
