// denoise_scene.cpp -- the denoising call sequence through the C++ adapter (include/agpt_host.hpp): a uniform 16-spp render with
// the adaptive entry point (which keeps the luminance second moment), the first-hit feature buffers, the a-trous filter, resolve.
//
//   g++ -std=c++17 -Iinclude examples/denoise_scene.cpp -o denoise_scene libagpt_hip.so
//   ./denoise_scene out.bin [width height]      -> albedo, normal_depth, denoised float4 planes and the resolved 0x00RRGGBB words
#include <cstdio>
#include <cstdlib>

#include "agpt_host.hpp"
using namespace agpt;

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s out.bin [width height]\n", argv[0]);
        return 2;
    }
    const int W = argc > 3 ? std::atoi(argv[2]) : 96, H = argc > 3 ? std::atoi(argv[3]) : 64;
    try {
        Context ctx(0);
        Scene scene(ctx);
        int gold = DisneyMaterial::Make(scene, float3{0.944f, 0.776f, 0.373f}, .5f, 1.f);
        int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, 1.f, 0.f);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1, 20}, float3{40, 20, 40}, 7.5f, 32), floor, 1);
        scene.primitives_push_back(Sphere{float3{0, 0, 0}, 1.f}, gold);
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 1.16f, -4.64f}, {0, 0, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        AdaptiveAccumulator acc(ctx, W, H);
        agpt_adaptive_params uniform{16, 16, 16, 0.f, 0.f};   // rel_error <= 0, min_spp = max_spp: every pixel gets 16 samples
        integrator.RenderAdaptive(scene, acc, uniform);
        FeatureBuffers features(ctx, W, H);
        integrator.RenderFeatures(scene, features);
        Accumulator denoised(ctx, W, H);
        acc.Denoise(features, denoised);                       // 5 passes, demodulated, default sigmas
        const std::vector<float> albedo = features.DownloadAlbedo(), nd = features.DownloadNormalDepth(), out = denoised.Download();
        const std::vector<uint32_t> rgb = denoised.CopyToSurface();

        FILE* f = std::fopen(argv[1], "wb");
        if (!f) {
            std::fprintf(stderr, "cannot write %s\n", argv[1]);
            return 1;
        }
        std::fwrite(albedo.data(), 4, albedo.size(), f);
        std::fwrite(nd.data(), 4, nd.size(), f);
        std::fwrite(out.data(), 4, out.size(), f);
        std::fwrite(rgb.data(), 4, rgb.size(), f);
        std::fclose(f);
        std::printf("denoised %dx%d samples=%d\n", W, H, denoised.NumSamples());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
