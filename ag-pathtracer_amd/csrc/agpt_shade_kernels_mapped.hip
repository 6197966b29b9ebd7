// agpt_shade_kernels_mapped.hip -- k_shade_mapped: the MAPPED variant of the shading kernel (AGPT_SHADE_TEXTURED 2, agpt_shade_kernels.h).
// agpt_scene_set_material_param_texture on any material of a scene selects it at launch; scenes without roughness / metallic maps
// never run it.  Same flags as agpt_shade_kernels.hip (MachineLICM off, four waves per SIMD, -ffp-contract=off).
#define AGPT_SHADE_TEXTURED 2
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
