// agpt_shade_kernels_sampled.hip -- k_shade_sampled: the SAMPLED variant of the shading kernel (AGPT_SHADE_TEXTURED 3, agpt_shade_kernels.h).
// agpt_scene_set_texture_sampler with a filter or a wrap mode other than the default, on a texture that a material of the scene names,
// selects it at launch; every other scene never runs it.  Same flags as agpt_shade_kernels.hip (MachineLICM off, four waves per SIMD,
// -ffp-contract=off).
#define AGPT_SHADE_TEXTURED 3
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
