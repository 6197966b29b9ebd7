// agpt_shade_kernels_normal_fast.hip -- k_shade_normal_fast: the NORMAL variant of the shading kernel (AGPT_SHADE_TEXTURED 4, agpt_shade_kernels.h) in fast arithmetic (AGPT_SHADE_FAST, agpt_shade_arith.h).
// agpt_scene_set_material_normal_texture on any material of a scene selects it at launch; every other scene never runs it.  Flags of
// agpt_shade_kernels_fast.hip (MachineLICM off, -ffp-contract=off), but three waves per SIMD: no spilled registers, and measured faster
// than four waves with spills (build.py).
#define AGPT_SHADE_FAST 1
#define AGPT_SHADE_TEXTURED 4
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"
