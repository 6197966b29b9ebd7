// agpt_shade_kernels_textured_fast.hip -- k_shade_textured_fast: the TEXTURED variant of the shading kernel (AGPT_SHADE_TEXTURED, agpt_shade_kernels.h) in fast arithmetic (AGPT_SHADE_FAST, agpt_shade_arith.h).
// agpt_scene_set_material_texture on any material of a scene selects it at launch; scenes without textures never run it.  Same flags
// as agpt_shade_kernels_fast.hip (MachineLICM off, four waves per SIMD, -ffp-contract=off).
#define AGPT_SHADE_FAST 1
#define AGPT_SHADE_TEXTURED 1
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
