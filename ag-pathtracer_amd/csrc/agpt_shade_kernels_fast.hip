// agpt_shade_kernels_fast.hip -- the shading kernels again, with the path weights in fast arithmetic (AGPT_SHADE_FAST 1,
// agpt_shade_arith.h): k_shade_fast, the finishing kernels k_accumulate_fast, k_export_li_fast and k_resolve_pending_fast and the known-answer kernels k_kat_bsdf_*_fast and k_kat_env_light_fast, with their
// host-side launchers.  agpt_scene_set_shading_arith(AGPT_SHADING_FAST) selects them.  The unit keeps -ffp-contract=off
// -fno-fast-math like every other: agpt_trace.h, which it includes for sphere_test_c, must answer a ray as the trace kernels do.
#define AGPT_SHADE_LEVEL 0
#define AGPT_SHADE_FAST 1
#include <hip/hip_runtime.h>

#include "agpt_shade_kernels.h"

__global__ void k_kat_bsdf_eval_fast(DevScene sc, int material, int n, const float* __restrict__ wo3, const float* __restrict__ wi3,
                                     float* __restrict__ f3o, float* __restrict__ pdfo) {
    kat_bsdf_eval_lane(sc, material, n, wo3, wi3, f3o, pdfo);
}
__global__ void k_kat_bsdf_sample_fast(DevScene sc, int material, int n, const float* __restrict__ wo3, const float* __restrict__ u2,
                                       float* __restrict__ wi3o, float* __restrict__ f3o, float* __restrict__ pdfo,
                                       int32_t* __restrict__ speco) {
    kat_bsdf_sample_lane(sc, material, n, wo3, u2, wi3o, f3o, pdfo, speco);
}
__global__ void k_kat_env_light_fast(DevScene sc, int light, int n_dirs, const float* __restrict__ d3, float* __restrict__ le3o,
                                     float* __restrict__ pdf_li_o, int n_draws, const float* __restrict__ u, float* __restrict__ wi3o,
                                     float* __restrict__ pdfo, float* __restrict__ sle3o, int32_t* __restrict__ oko) {
    kat_env_light_lane(sc, light, n_dirs, d3, le3o, pdf_li_o, n_draws, u, wi3o, pdfo, sle3o, oko);
}

namespace agpt {

void launch_kat_bsdf_eval_fast(hipStream_t stream, const DevScene& sc, int material, int n, const float* wo3, const float* wi3, float* f3o,
                               float* pdfo) {
    hipLaunchKernelGGL(k_kat_bsdf_eval_fast, dim3((n + 63) / 64), dim3(64), 0, stream, sc, material, n, wo3, wi3, f3o, pdfo);
}

void launch_kat_bsdf_sample_fast(hipStream_t stream, const DevScene& sc, int material, int n, const float* wo3, const float* u2, float* wi3o,
                                 float* f3o, float* pdfo, int32_t* speco) {
    hipLaunchKernelGGL(k_kat_bsdf_sample_fast, dim3((n + 63) / 64), dim3(64), 0, stream, sc, material, n, wo3, u2, wi3o, f3o, pdfo, speco);
}

void launch_kat_env_light_fast(hipStream_t stream, const DevScene& sc, int light, int n_dirs, const float* d3, float* le3o, float* pdf_li_o,
                               int n_draws, const float* u, float* wi3o, float* pdfo, float* sle3o, int32_t* oko) {
    const int n = n_dirs + n_draws;
    hipLaunchKernelGGL(k_kat_env_light_fast, dim3((n + 63) / 64), dim3(64), 0, stream, sc, light, n_dirs, d3, le3o, pdf_li_o, n_draws, u, wi3o,
                       pdfo, sle3o, oko);
}

}  // namespace agpt
