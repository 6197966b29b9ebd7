// agpt_shade_arith.h -- the value-only arithmetic of the shading code, behind device helpers whose body the translation unit
// chooses.  Value-only: what a BSDF's f and pdf are (lobe evaluation, Fresnel, the microfacet D and G), the pdfs of the lights,
// MIS weights and the path's contributions and throughput.
//
//   AGPT_SHADE_FAST 0 (default; agpt_api.hip, agpt_kat.hip, agpt_shade_kernels.hip): each helper is exactly the expression it replaces --
//     correctly rounded fp32 divide and square root.  Bit-exact parity with the oracle rests on this; the unit's code is the
//     code the plain expressions compile to.
//   AGPT_SHADE_FAST 1 (agpt_shade_kernels_fast.hip, agpt_scene_set_shading_arith(AGPT_SHADING_FAST)): a / b is a * v_rcp_f32(b),
//     square roots are v_sqrt_f32 and normalize uses v_rsq_f32 -- except the microfacet lobe's half vector, which keeps normalize's
//     bits (sh_normalize_rn): tr_D forms sin^2 as 1 - wh.z^2, about 1e-6 at the peak of a lobe at the alpha clamp of .001, so the ulp
//     v_rsq_f32 may be off in wh.z came back as 10 % of D and took 3 % of a render's pixels out of the 1e-3 rule.
//
// What decides where a ray goes or what a path draws stays exact in both modes and does not use these helpers: the sampled
// directions (BSDF and light sampling, with their fp64 trigonometry), the surface frames they are built in, the environment
// map's texel choices (sampling, Le and pdf lookups), every ray's origin, direction and tmax, agpt_trace.h (sphere_test_c included), camera rays, the RNG and the queue logic.
// A 1-ulp change to a direction moves the next hit point; on finely tessellated meshes that flips the hit triangle (its
// geometric normal) often enough that relaxing the sampling arithmetic left 2-14 % of the pixels of a 1-spp render more than
// 1e-3 away from the exact one.  With the directions exact a FAST render traces the same rays as the
// exact one and differs from it only by the rounding of the path weights.
#pragma once

#include "agpt_math.h"

#ifndef AGPT_SHADE_FAST
#define AGPT_SHADE_FAST 0
#endif

#define AGPT_SH __device__ __forceinline__

#if AGPT_SHADE_FAST
AGPT_SH float sh_rcp(float b) { return __builtin_amdgcn_rcpf(b); }
AGPT_SH float sh_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
AGPT_SH float sh_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
AGPT_SH v3 sh_div3(v3 a, float b) { return a * __builtin_amdgcn_rcpf(b); }
AGPT_SH v3 sh_normalize(v3 v) { return v * __builtin_amdgcn_rsqf(dot(v, v)); }
// normalize(v) (agpt_math.h) bit for bit, without the IEEE divide expansion: sqrtf is correctly rounded in this unit too, and 1 / s is
// the Newton-Raphson core of that expansion, operation by operation -- what v_div_scale_f32, v_div_fmas_f32 and v_div_fixup_f32 add to
// it are identities while s is a normal number within [2^-90, 2^90] (no operand is scaled, the result is no special case); the length
// of a sum of two unit vectors is, down to a pair that cancels to 2^-90.  For the one place where an ulp in a unit vector does not
// stay an ulp in the value: the half vector of the microfacet lobe (agpt_shade.h: lobe_eval).
AGPT_SH v3 sh_normalize_rn(v3 v) {
    const float s = sqrtf(dot(v, v));
    const float r0 = __builtin_amdgcn_rcpf(s);
    const float r1 = __builtin_fmaf(__builtin_fmaf(-s, r0, 1.f), r0, r0);
    const float q1 = __builtin_fmaf(__builtin_fmaf(-s, r1, 1.f), r1, r1);
    const float q = __builtin_fmaf(__builtin_fmaf(-s, q1, 1.f), r1, q1);
    return v * q;
}
#else
AGPT_SH float sh_rcp(float b) { return 1.f / b; }
// (a macro, not a function: through an always-inlined call the optimiser laid out env_sample_li's blocks differently, and
// this unit's code must stay the code the expressions themselves compile to)
#define sh_div(a, b) ((float)(a) / (float)(b))
AGPT_SH float sh_sqrt(float x) { return sqrtf(x); }
AGPT_SH v3 sh_div3(v3 a, float b) { return a / b; }
AGPT_SH v3 sh_normalize(v3 v) { return normalize(v); }
AGPT_SH v3 sh_normalize_rn(v3 v) { return normalize(v); }
#endif
