// normal_scene.cpp -- a tangent-space normal map through the C++ adapter (include/agpt_host.hpp): filtered_scene.cpp's backdrop with a
// procedural bump image in its material's normal slot, read with bilinear filtering; the scene is rendered and its first-hit normal
// buffer -- which carries the perturbed normal -- written beside it.
//
//   g++ -std=c++17 -Iinclude examples/normal_scene.cpp -o normal_scene libagpt_hip.so
//   ./normal_scene out.bin [width height]      -> accum and normal_depth float4 planes
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
        int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, .6f, 0.f);
        // an 8 x 8 map of studs: each 4 x 4 cell tilts away from its centre, by eighths (exact in fp32) -- rgb = n / 2 + 1 / 2, not
        // normalized: the library normalizes the sum it forms
        const int TW = 8, TH = 8;
        std::vector<float> texels((size_t)TW * TH * 3);
        for (int y = 0; y < TH; y++)
            for (int x = 0; x < TW; x++) {
                const float dx = (float)(x % 4) - 1.5f, dy = (float)(y % 4) - 1.5f;
                float* t = &texels[3 * ((size_t)y * TW + x)];
                t[0] = .5f + .125f * dx;
                t[1] = .5f + .125f * dy;
                t[2] = 1.f;
            }
        const int bumps = scene.textures_push_back(texels.data(), TW, TH);
        scene.SetTextureSampler(bumps, AGPT_FILTER_BILINEAR, AGPT_WRAP_REPEAT, AGPT_WRAP_REPEAT);
        scene.SetMaterialNormalTexture(floor, bumps, 1.5f);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1, 20}, float3{40, 20, 40}, 7.5f, 32), floor, 1);
        scene.primitives_push_back(Sphere{float3{0, 0, 0}, 1.f}, gold);
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 1.16f, -4.64f}, {0, 0, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        Accumulator acc(ctx, W, H);
        integrator.Render(scene, acc, 4);
        FeatureBuffers features(ctx, W, H);
        integrator.RenderFeatures(scene, features);
        const std::vector<float> img = acc.Download(), normal_depth = features.DownloadNormalDepth();

        FILE* f = std::fopen(argv[1], "wb");
        if (!f) {
            std::fprintf(stderr, "cannot write %s\n", argv[1]);
            return 1;
        }
        std::fwrite(img.data(), 4, img.size(), f);
        std::fwrite(normal_depth.data(), 4, normal_depth.size(), f);
        std::fclose(f);
        std::printf("normal-mapped %dx%d samples=%d\n", W, H, acc.NumSamples());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
