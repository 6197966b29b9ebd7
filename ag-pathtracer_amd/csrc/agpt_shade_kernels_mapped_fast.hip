// agpt_shade_kernels_mapped_fast.hip -- k_shade_mapped_fast: the MAPPED variant of the shading kernel (AGPT_SHADE_TEXTURED 2, agpt_shade_kernels.h) in fast arithmetic (AGPT_SHADE_FAST, agpt_shade_arith.h).
// agpt_scene_set_material_param_texture on any material of a scene selects it at launch; scenes without roughness / metallic maps
// never run it.  Same flags as agpt_shade_kernels_fast.hip (MachineLICM off, four waves per SIMD, -ffp-contract=off).
#define AGPT_SHADE_FAST 1
#define AGPT_SHADE_TEXTURED 2
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
