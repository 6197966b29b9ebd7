// filtered_scene.cpp -- a texture sampler through the C++ adapter (include/agpt_host.hpp): textured_scene.cpp's checker on the backdrop,
// read with bilinear filtering, mirrored across and clamped along the sweep; the scene is rendered and its first-hit albedo buffer
// written beside it.
//
//   g++ -std=c++17 -Iinclude examples/filtered_scene.cpp -o filtered_scene libagpt_hip.so
//   ./filtered_scene out.bin [width height]      -> accum and albedo float4 planes
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
        // a 16 x 8 checker of two linear colours, darker towards the bottom rows (a decoded sRGB image would be linearised first)
        const int TW = 16, TH = 8;
        std::vector<float> texels((size_t)TW * TH * 3);
        for (int y = 0; y < TH; y++)
            for (int x = 0; x < TW; x++) {
                const bool odd = ((x / 2) + (y / 2)) % 2 == 1;
                const float shade = 1.f - 0.0625f * (float)y;
                float* t = &texels[3 * ((size_t)y * TW + x)];
                t[0] = (odd ? 0.125f : 0.75f) * shade;
                t[1] = (odd ? 0.25f : 0.75f) * shade;
                t[2] = (odd ? 0.5f : 0.625f) * shade;
            }
        const int checker = scene.textures_push_back(texels.data(), TW, TH);
        scene.SetMaterialTexture(floor, checker);
        scene.SetTextureSampler(checker, AGPT_FILTER_BILINEAR, AGPT_WRAP_MIRROR, AGPT_WRAP_CLAMP);
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
        const std::vector<float> img = acc.Download(), albedo = features.DownloadAlbedo();

        FILE* f = std::fopen(argv[1], "wb");
        if (!f) {
            std::fprintf(stderr, "cannot write %s\n", argv[1]);
            return 1;
        }
        std::fwrite(img.data(), 4, img.size(), f);
        std::fwrite(albedo.data(), 4, albedo.size(), f);
        std::fclose(f);
        std::printf("filtered %dx%d samples=%d\n", W, H, acc.NumSamples());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
