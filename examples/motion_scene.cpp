// motion_scene.cpp -- temporal history that follows a moving mesh, through the C++ adapter (include/agpt_host.hpp): an octahedron over
// a backdrop turns 8 degrees and comes 0.45 closer to the camera every frame (Scene::TransformMesh).  Every frame renders 4 fresh
// samples per pixel, adds the reprojected history of the previous frame and filters the result.  The sequence runs twice: with the motion
// calls -- Scene::SnapshotPositions after the frame's update, PathTracer::RenderFeaturesMotion, TemporalAccumulate(..., Motion::Follow)
// --, where the octahedron keeps its history, and with the plain TemporalAccumulate, whose depth test rejects all of it (the mesh moves
// by a tenth of its depth per frame).  Printed per run: the octahedron's pixels in the last frame and how many of them took history.
//
//   g++ -std=c++17 -Iinclude examples/motion_scene.cpp -o motion_scene libagpt_hip.so
//   ./motion_scene [width height frames]   -> "motion 1 mesh_pixels 412 history 398 coverage 0.966", "motion 0 ... coverage 0.000"
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "agpt_host.hpp"
using namespace agpt;

static TriangleMesh octahedron() {
    TriangleMesh m;
    m.vertices = {1, 0, 0, -1, 0, 0, 0, 1.5f, 0, 0, -1.5f, 0, 0, 0, 1, 0, 0, -1};
    const int tris[8][3] = {{0, 2, 4}, {2, 1, 4}, {1, 3, 4}, {3, 0, 4}, {2, 0, 5}, {1, 2, 5}, {3, 1, 5}, {0, 3, 5}};
    for (const auto& t : tris)
        for (int v : t)
            for (int k = 0; k < 3; k++) m.indices.push_back(v);   // (vertex, normal, texcoord): no normals, no texcoords
    return m;
}

int main(int argc, char** argv) {
    const int W = argc > 2 ? std::atoi(argv[1]) : 96, H = argc > 2 ? std::atoi(argv[2]) : 64, frames = argc > 3 ? std::atoi(argv[3]) : 4;
    if (W < 1 || H < 1 || frames < 2) return 2;
    const int spp = 4;
    // (cos, sin) of 0, 8, 16 and 24 degrees
    const float turns[4][2] = {{1.0f, 0.0f}, {0.99026807f, 0.13917310f}, {0.96126170f, 0.27563736f}, {0.91354546f, 0.40673664f}};
    try {
        Context ctx(0);
        for (const Motion motion : {Motion::Follow, Motion::Ignore}) {
            Scene scene(ctx);
            int gold = DisneyMaterial::Make(scene, float3{0.944f, 0.776f, 0.373f}, .4f, 1.f);
            int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, 1.f, 0.f);
            scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1.5f, 20}, float3{40, 20, 40}, 7.5f, 8), floor, 1);
            const int spinner = scene.primitives_push_back(octahedron(), gold, 1);
            scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
            scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
            scene.camera = CameraDesc{{0.f, 0.5f, -6.f}, {0, 0, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
            scene.commit();

            PathTracer integrator;
            const agpt_adaptive_params uniform{spp, spp, spp, 0.f, 0.f};   // rel_error <= 0, min_spp = max_spp: every pixel gets 4 samples
            AdaptiveAccumulator current(ctx, W, H);
            std::unique_ptr<AdaptiveAccumulator> history[2] = {std::make_unique<AdaptiveAccumulator>(ctx, W, H),
                                                               std::make_unique<AdaptiveAccumulator>(ctx, W, H)};
            std::unique_ptr<FeatureBuffers> features[2] = {std::make_unique<FeatureBuffers>(ctx, W, H), std::make_unique<FeatureBuffers>(ctx, W, H)};
            Accumulator denoised(ctx, W, H);
            for (int k = 0; k < frames; ++k) {
                const int cur = k & 1, prev = cur ^ 1;
                const float c = turns[k % 4][0], s = turns[k % 4][1], nearer = -0.45f * (float)(k % 4);
                const float m[16] = {c, 0, s, 0, 0, 1, 0, 0, -s, 0, c, nearer, 0, 0, 0, 1};
                // the per-frame order: update -> snapshot -> render -> features_motion -> temporal_accumulate_motion -> denoise
                scene.TransformMesh(spinner, m);
                scene.SnapshotPositions();
                current.Clear();
                integrator.RenderAdaptive(scene, current, uniform, (uint32_t)k);
                integrator.RenderFeaturesMotion(scene, *features[cur]);   // (in both runs: prev_point.w also tells which pixels moved)
                current.TemporalAccumulate(*features[cur], scene.camera, k ? history[prev].get() : nullptr, k ? features[prev].get() : nullptr,
                                           scene.camera, *history[cur], 32.f, AGPT_TEMPORAL_DEPTH_TOL, AGPT_TEMPORAL_NORMAL_COS, motion);
                history[cur]->Denoise(*features[cur], denoised);
            }
            const int last = (frames - 1) & 1;
            const std::vector<float> hist = history[last]->Download(), point = features[last]->DownloadPrevPoint();
            int mesh_pixels = 0, with_history = 0;
            for (size_t i = 0; i < (size_t)W * H; ++i)
                if (point[4 * i + 3] == 1.f) {
                    mesh_pixels++;
                    with_history += hist[4 * i + 3] > (float)spp;
                }
            std::printf("motion %d mesh_pixels %d history %d coverage %.3f\n", motion == Motion::Follow ? 1 : 0, mesh_pixels, with_history,
                        mesh_pixels ? (double)with_history / mesh_pixels : 0.0);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
