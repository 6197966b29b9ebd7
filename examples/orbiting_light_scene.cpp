// orbiting_light_scene.cpp -- a light that moves in a committed scene, through the C++ adapter (include/agpt_host.hpp): the card scene
// -- a floor, a card, a sphere light -- with the light circling the card, a quarter of its way in four frames.  Per frame
//     Scene::updateSphere -> SnapshotPositions -> RenderAdaptive -> RenderFeaturesMotion -> TemporalAccumulate (clamped) -> Denoise
// The update rewrites 20 bytes of one device record; no mesh is uploaded again.  The light's own pixels follow it (prev_point.w = 1 on
// them), and the shadows it moves across the unmoved floor are what the clamp is for.  With a file name as last argument the last
// frame's history, prev_point and denoised image go there as raw floats (W * H * 4 each), for comparison with another route.
//
//   g++ -std=c++17 -Iinclude examples/orbiting_light_scene.cpp -o orbiting_light_scene libagpt_hip.so
//   ./orbiting_light_scene [width height [frames [out.bin]]]   -> "frames 4 light_pixels 38 history 31"
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "agpt_host.hpp"
using namespace agpt;

static TriangleMesh floor_mesh() {
    TriangleMesh m;
    m.vertices = {-5, 0, -5, 5, 0, -5, -5, 0, 5, 5, 0, 5};
    for (int v : {0, 2, 1, 1, 2, 3}) m.indices.insert(m.indices.end(), {v, 0, 0});   // (vertex, normal, texcoord): no normals, no texcoords
    return m;
}

// a 6 x 6-quad card of side 1 in the plane z = 0 around (0, 1, 0)
static TriangleMesh card_mesh() {
    const int n = 6;
    TriangleMesh m;
    for (int i = 0; i <= n; i++)
        for (int j = 0; j <= n; j++) m.vertices.insert(m.vertices.end(), {-0.5f + (float)i / n, 0.5f + (float)j / n, 0.f});
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const int a = i * (n + 1) + j, b = (i + 1) * (n + 1) + j, c = a + 1, d = b + 1;
            for (int v : {a, b, c, c, b, d}) m.indices.insert(m.indices.end(), {v, 0, 0});
        }
    return m;
}

// the light's (x, z) on its circle about the vertical axis, frame by frame (a table: the same floats on every route)
static const float orbit[4][2] = {{1.6f, 1.0f}, {1.8f, 0.4f}, {1.85f, -0.25f}, {1.7f, -0.9f}};

int main(int argc, char** argv) {
    const int W = argc > 2 ? std::atoi(argv[1]) : 64, H = argc > 2 ? std::atoi(argv[2]) : 48;
    const int frames = argc > 3 ? std::atoi(argv[3]) : 4;
    const char* out_path = argc > 4 ? argv[4] : nullptr;
    if (W < 1 || H < 1 || frames < 1) return 2;
    try {
        Context ctx(0);
        Scene scene(ctx);
        const int grey = scene.add_material(AGPT_MAT_DIFFUSE_ONLY, float3{0.6f, 0.6f, 0.6f}, 0.f, 0.f);
        const int red = scene.add_material(AGPT_MAT_DIFFUSE_ONLY, float3{0.7f, 0.2f, 0.15f}, 0.f, 0.f);
        scene.primitives_push_back(floor_mesh(), grey, 1);
        scene.primitives_push_back(card_mesh(), red, 1);
        const int light = scene.addAreaLight(Sphere{float3{orbit[0][0], 2.f, orbit[0][1]}, 0.3f}, float3{40.f, 40.f, 40.f});
        scene.camera = CameraDesc{{0.f, 1.f, -4.f}, {0.f, 1.f, 0.f}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        const agpt_adaptive_params uniform{4, 4, 4, 0.f, 0.f};        // rel_error <= 0, min_spp = max_spp: every pixel gets 4 samples
        const agpt_temporal_clamp_params clamp{2, 1, 1.f, 8.f};       // a 5 x 5 window on demodulated radiance, one sigma, at most 8 samples kept
        AdaptiveAccumulator current(ctx, W, H);
        std::unique_ptr<AdaptiveAccumulator> history[2] = {std::make_unique<AdaptiveAccumulator>(ctx, W, H),
                                                           std::make_unique<AdaptiveAccumulator>(ctx, W, H)};
        std::unique_ptr<FeatureBuffers> features[2] = {std::make_unique<FeatureBuffers>(ctx, W, H), std::make_unique<FeatureBuffers>(ctx, W, H)};
        Accumulator denoised(ctx, W, H);
        for (int k = 0; k < frames; ++k) {
            const int cur = k & 1, prev = cur ^ 1;
            scene.updateSphere(light, Sphere{float3{orbit[k % 4][0], 2.f, orbit[k % 4][1]}, 0.3f});
            scene.SnapshotPositions();
            current.Clear();
            integrator.RenderAdaptive(scene, current, uniform, (uint32_t)k);
            integrator.RenderFeaturesMotion(scene, *features[cur]);
            current.TemporalAccumulate(*features[cur], scene.camera, k ? history[prev].get() : nullptr, k ? features[prev].get() : nullptr,
                                       scene.camera, *history[cur], 32.f, AGPT_TEMPORAL_DEPTH_TOL, AGPT_TEMPORAL_NORMAL_COS, Motion::Follow, &clamp);
            history[cur]->Denoise(*features[cur], denoised);
        }
        const int last = (frames - 1) & 1;
        const std::vector<float> hist = history[last]->Download(), point = features[last]->DownloadPrevPoint(), image = denoised.Download();
        int light_pixels = 0, with_history = 0;
        for (size_t i = 0; i < (size_t)W * H; ++i)
            if (point[4 * i + 3] == 1.f) {
                light_pixels++;
                with_history += hist[4 * i + 3] > 4.f;
            }
        std::printf("frames %d light_pixels %d history %d\n", frames, light_pixels, with_history);
        if (out_path) {
            std::FILE* f = std::fopen(out_path, "wb");
            if (!f) return 3;
            for (const std::vector<float>* a : {&hist, &point, &image}) std::fwrite(a->data(), sizeof(float), a->size(), f);
            std::fclose(f);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
