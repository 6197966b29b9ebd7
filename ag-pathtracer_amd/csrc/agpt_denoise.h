// agpt_denoise.h -- what the feature-buffer / denoiser unit (agpt_denoise.hip, which also defines agpt_denoise) shares: the launchers
// agpt_render_features (agpt_api.hip) calls, and the tiling, constants and pixel-centre ray that agpt_temporal.hip uses as well.
#pragma once

#include "agpt_wavefront.h"

// a pass works on tiles of AGPT_DN_TX x AGPT_DN_TY pixels, one thread each: a wave is one 64-pixel row segment (1 KiB per float4 tap)
#define AGPT_DN_TX 64
#define AGPT_DN_TY 4

struct DenoiseConsts {
    int32_t W, H;
    int32_t step;          // tap spacing of this pass
    int32_t demodulate;
    int32_t last;          // 1: this pass writes the final image (re-modulated, w = 1)
    float sigma_z, sigma_n, sigma_l;
};

// The pixel-centre camera ray of film pixel (x, y): film position ((x + .5) / W, (y + .5) / H) -> Camera::GetRay (camera.h:58-64) with
// rd = 0 whatever the aperture (myapp.cpp:165-167); the Ray that Scene::Intersect then receives normalises the direction once more
// (camera.h:6), as the rays of agpt_intersect_device do (k_prepare_rays).  Shared by k_feature_rays and k_temporal (agpt_temporal.hip),
// which reprojects the point that ray hit: one arithmetic, so the two agree bit for bit.
__device__ __forceinline__ void feature_ray(const DevCamera& c, int x, int y, int32_t W, int32_t H, v3& O, v3& D) {
    const float px = x + 0.5f, py = y + 0.5f;
    const float s = px / W, t = py / H;
    camera_ray(c, s, t, 0.f, 0.f, O, D);
    D = normalize(D);
}

namespace agpt {
// the pixel-centre camera rays of the tile (rc.NP pixels in pixel_of order), ready for a closest-hit trace launch
void launch_feature_rays(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, float4* ray_o, float4* ray_d);
// colors: one float4 per material, rgb = the colour agpt_scene_add_material was given; level: the scene's texturing
// level (agpt_scene_commit), which picks the feature kernel
void launch_features(hipStream_t stream, const DevScene& sc, ShadeLevel level, const RenderConsts& rc, const float4* colors,
                     const DevHit* hits, const float4* ray_o, const float4* ray_d, float4* albedo, float4* normal_depth);
// launch_features through the kernels' PREV siblings (agpt_render_features_surface_motion): prev_normal as well, from prev_point -- which
// launch_motion (agpt_motion.h) wrote for the same hits, earlier on the stream -- and the older generation of tri_shade records.
// tri_shade_old is read for pixels whose prev_point.w is 1 on a triangle only; NULL for a scene without triangles.
void launch_features_prev(hipStream_t stream, const DevScene& sc, ShadeLevel level, const RenderConsts& rc, const float4* colors,
                          const DevHit* hits, const float4* ray_o, const float4* ray_d, float4* albedo, float4* normal_depth,
                          const float4* tri_shade_old, const float4* prev_point, float4* prev_normal);
}  // namespace agpt
