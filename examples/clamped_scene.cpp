// clamped_scene.cpp -- neighbourhood clamping of temporal history, through the C++ adapter (include/agpt_host.hpp): a card stands on a
// floor before a sphere light and throws a shadow onto the floor.  Frame 0 renders 64 samples per pixel; then the card slides half its
// width sideways (Scene::UpdateMesh, a snapshot behind it) and frame 1 renders 4.  The floor the shadow left is geometrically what it
// was -- same flag, depth and normal --, so the plain temporal call blends frame 0's 32 samples of shadow into it: the shadow trails
// behind the card.  With a clamp (AdaptiveAccumulator::TemporalAccumulate's last argument -> agpt_temporal_accumulate_clamped) that
// history is pulled into the range the frame's own samples span around each pixel.  Printed for clamp off and on: the number of floor
// pixels the shadow left (their 256-sample luminance at least doubled between the two poses) and the mean absolute luminance error of
// the accumulated history there against the 256-sample render of frame 1.
//
//   g++ -std=c++17 -Iinclude examples/clamped_scene.cpp -o clamped_scene libagpt_hip.so
//   ./clamped_scene [width height]   -> "clamp 0 uncovered 124 error 0.044580", "clamp 1 uncovered 124 error 0.011350"
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "agpt_host.hpp"
using namespace agpt;

static TriangleMesh floor_mesh() {
    TriangleMesh m;
    m.vertices = {-5, 0, -5, 5, 0, -5, -5, 0, 5, 5, 0, 5};
    for (int v : {0, 2, 1, 1, 2, 3}) m.indices.insert(m.indices.end(), {v, 0, 0});   // (vertex, normal, texcoord): no normals, no texcoords
    return m;
}

// a 6 x 6-quad card of side 1 in the plane z = 0 around (dx, 1, 0)
static TriangleMesh card_mesh(float dx) {
    const int n = 6;
    TriangleMesh m;
    for (int i = 0; i <= n; i++)
        for (int j = 0; j <= n; j++) m.vertices.insert(m.vertices.end(), {-0.5f + (float)i / n + dx, 0.5f + (float)j / n, 0.f});
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const int a = i * (n + 1) + j, b = (i + 1) * (n + 1) + j, c = a + 1, d = b + 1;
            for (int v : {a, b, c, c, b, d}) m.indices.insert(m.indices.end(), {v, 0, 0});
        }
    return m;
}

static float luminance(const float* rgb, float n) { return (0.212671f * rgb[0] + 0.715160f * rgb[1] + 0.072169f * rgb[2]) / n; }

int main(int argc, char** argv) {
    const int W = argc > 2 ? std::atoi(argv[1]) : 64, H = argc > 2 ? std::atoi(argv[2]) : 48;
    if (W < 1 || H < 1) return 2;
    const int long_spp = 256;
    try {
        Context ctx(0);
        Scene scene(ctx);
        const int grey = scene.add_material(AGPT_MAT_DIFFUSE_ONLY, float3{0.6f, 0.6f, 0.6f}, 0.f, 0.f);
        const int red = scene.add_material(AGPT_MAT_DIFFUSE_ONLY, float3{0.7f, 0.2f, 0.15f}, 0.f, 0.f);
        scene.primitives_push_back(floor_mesh(), grey, 1);
        const int card = scene.primitives_push_back(card_mesh(0.f), red, 1);
        scene.addAreaLight(Sphere{float3{1.6f, 2.f, 1.f}, 0.3f}, float3{40.f, 40.f, 40.f});
        scene.camera = CameraDesc{{0.f, 1.f, -4.f}, {0.f, 1.f, 0.f}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        AdaptiveAccumulator current(ctx, W, H), history0(ctx, W, H), history1(ctx, W, H);
        FeatureBuffers features0(ctx, W, H), features1(ctx, W, H);
        Accumulator reference(ctx, W, H);
        std::vector<float> ref[2];

        // frame 0: the card at rest, 64 samples; its history is the frame itself
        scene.SnapshotPositions();
        const agpt_adaptive_params first{64, 64, 64, 0.f, 0.f};   // rel_error <= 0, min_spp = max_spp: every pixel gets all of them
        integrator.RenderAdaptive(scene, current, first, 1u);
        integrator.RenderFeaturesMotion(scene, features0);
        current.TemporalAccumulate(features0, scene.camera, nullptr, nullptr, scene.camera, history0);
        integrator.Render(scene, reference, long_spp);
        ref[0] = reference.Download();

        // frame 1: the card half its width to the side, 4 samples
        scene.UpdateMesh(card, card_mesh(-0.5f));
        scene.SnapshotPositions();
        const agpt_adaptive_params few{4, 4, 4, 0.f, 0.f};
        current.Clear();
        integrator.RenderAdaptive(scene, current, few, 2u);
        integrator.RenderFeaturesMotion(scene, features1);
        reference.Clear();
        integrator.Render(scene, reference, long_spp);
        ref[1] = reference.Download();

        // the floor the shadow left: grey floor in both frames, at least twice as bright in the second long render
        const std::vector<float> a0 = features0.DownloadAlbedo(), a1 = features1.DownloadAlbedo();
        std::vector<char> uncovered((size_t)W * H, 0);
        for (size_t i = 0; i < (size_t)W * H; ++i) {
            const bool is_floor = a0[4 * i + 3] == 1.f && a1[4 * i + 3] == 1.f && a0[4 * i] == 0.6f && a1[4 * i] == 0.6f;
            const float y0 = luminance(&ref[0][4 * i], (float)long_spp), y1 = luminance(&ref[1][4 * i], (float)long_spp);
            uncovered[i] = is_floor && y1 >= 2.f * y0 && y1 > y0;
        }

        const agpt_temporal_clamp_params clamp{2, 1, 1.f, 8.f};   // a 5 x 5 window on demodulated radiance, one sigma, at most 8 samples kept
        for (int on = 0; on < 2; ++on) {
            current.TemporalAccumulate(features1, scene.camera, &history0, &features0, scene.camera, history1, 32.f, AGPT_TEMPORAL_DEPTH_TOL,
                                       AGPT_TEMPORAL_NORMAL_COS, Motion::Follow, on ? &clamp : nullptr);
            const std::vector<float> hist = history1.Download();
            int count = 0;
            double error = 0;
            for (size_t i = 0; i < (size_t)W * H; ++i)
                if (uncovered[i]) {
                    count++;
                    error += std::fabs((double)luminance(&hist[4 * i], hist[4 * i + 3]) - (double)luminance(&ref[1][4 * i], (float)long_spp));
                }
            std::printf("clamp %d uncovered %d error %.6f\n", on, count, count ? error / count : 0.0);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
