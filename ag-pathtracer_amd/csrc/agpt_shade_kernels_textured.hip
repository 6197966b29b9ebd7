// agpt_shade_kernels_textured.hip -- k_shade_textured: the TEXTURED variant of the shading kernel (AGPT_SHADE_TEXTURED, agpt_shade_kernels.h).
// agpt_scene_set_material_texture on any material of a scene selects it at launch; scenes without textures never run it.  Same flags
// as agpt_shade_kernels.hip (MachineLICM off, four waves per SIMD, -ffp-contract=off).
#define AGPT_SHADE_TEXTURED 1
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
