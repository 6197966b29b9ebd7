// mapped_scene.cpp -- roughness and metallic maps through the C++ adapter (include/agpt_host.hpp): the backdrop of the simple test
// scene takes one metallic-roughness image laid out as glTF does (roughness in g, metallic in b) -- a checker of rough dielectric and
// polished metal cells -- beside its constant colour; the scene is rendered and the accumulator written out.
//
//   g++ -std=c++17 -Iinclude examples/mapped_scene.cpp -o mapped_scene libagpt_hip.so
//   ./mapped_scene out.bin [width height]      -> the accum float4 plane
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
        // 16 x 8 texels: r unused, g = roughness (smoother towards the bottom rows), b = metallic (0 or 1 in 2 x 2 cells)
        const int TW = 16, TH = 8;
        std::vector<float> texels((size_t)TW * TH * 3);
        for (int y = 0; y < TH; y++)
            for (int x = 0; x < TW; x++) {
                const bool metal = ((x / 2) + (y / 2)) % 2 == 1;
                float* t = &texels[3 * ((size_t)y * TW + x)];
                t[0] = 0.f;
                t[1] = (metal ? 0.5f : 1.f) - 0.0625f * (float)y;
                t[2] = metal ? 1.f : 0.f;
            }
        const int mr = scene.textures_push_back(texels.data(), TW, TH);
        scene.SetMaterialParamTexture(floor, AGPT_PARAM_ROUGHNESS, mr, 1);
        scene.SetMaterialParamTexture(floor, AGPT_PARAM_METALLIC, mr, 2);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1, 20}, float3{40, 20, 40}, 7.5f, 32), floor, 1);
        scene.primitives_push_back(Sphere{float3{0, 0, 0}, 1.f}, gold);
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 1.16f, -4.64f}, {0, 0, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        Accumulator acc(ctx, W, H);
        integrator.Render(scene, acc, 4);
        const std::vector<float> img = acc.Download();

        FILE* f = std::fopen(argv[1], "wb");
        if (!f) {
            std::fprintf(stderr, "cannot write %s\n", argv[1]);
            return 1;
        }
        std::fwrite(img.data(), 4, img.size(), f);
        std::fclose(f);
        std::printf("mapped %dx%d samples=%d\n", W, H, acc.NumSamples());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
