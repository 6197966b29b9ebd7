// turning_scene.cpp -- temporal history that follows a turning surface, through the C++ adapter (include/agpt_host.hpp): a flat card
// over a floor, seen from 4 away, is turned 40 degrees about its vertical axis between frame 0 and frame 1 (Scene::TransformMesh).  Both
// frames render 4 samples per pixel; frame 1 adds the reprojected history of frame 0 twice: with TemporalAccumulate(..., Motion::Follow)
// -- agpt_temporal_accumulate_motion, which finds the card's previous pixels and then compares the card's normal NOW with the stored one:
// cos 40 = 0.766 < normal_cos = 0.9, so every card pixel loses its history -- and with Motion::FollowSurfaces --
// agpt_temporal_accumulate_surface_motion with the features of RenderFeaturesSurfaceMotion after Scene::SnapshotSurfaces --, which
// compares the normal the card had a frame ago.  Printed: the card's pixels and the share of them that took history, per call.
//
//   g++ -std=c++17 -Iinclude examples/turning_scene.cpp -o turning_scene libagpt_hip.so
//   ./turning_scene   -> "card_pixels=162 share_motion=0.000000 share_surface_motion=1.000000"
#include <cstdio>
#include <cstdlib>

#include "agpt_host.hpp"
using namespace agpt;

// an n x n-quad card of side 1 in the plane z = 0 around (0, 1, 0)
static TriangleMesh card(int n) {
    TriangleMesh m;
    for (int i = 0; i <= n; i++)
        for (int j = 0; j <= n; j++) {
            m.vertices.push_back((float)(-0.5 + (double)i / n));
            m.vertices.push_back((float)(-0.5 + (double)j / n + 1.0));
            m.vertices.push_back(0.f);
        }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const int a = i * (n + 1) + j, b = (i + 1) * (n + 1) + j, c = i * (n + 1) + j + 1, d = (i + 1) * (n + 1) + j + 1;
            for (int v : {a, b, c, c, b, d}) {
                m.indices.push_back(v);   // (vertex, normal, texcoord): no normals, no texcoords
                m.indices.push_back(0);
                m.indices.push_back(0);
            }
        }
    return m;
}

static TriangleMesh floor_mesh() {
    TriangleMesh m;
    m.vertices = {-5, 0, -5, 5, 0, -5, -5, 0, 5, 5, 0, 5};
    for (int v : {0, 2, 1, 1, 2, 3}) {
        m.indices.push_back(v);
        m.indices.push_back(0);
        m.indices.push_back(0);
    }
    return m;
}

int main() {
    const int W = 64, H = 48, spp = 4;
    const float c = 0.76604444f, s = 0.64278764f;   // 40 degrees
    const float turn[16] = {c, 0, s, 0, 0, 1, 0, 0, -s, 0, c, 0, 0, 0, 0, 1};
    try {
        Context ctx(0);
        Scene scene(ctx);
        const int grey = scene.add_material(AGPT_MAT_DIFFUSE_ONLY, float3{0.6f, 0.6f, 0.6f}, 0.f, 0.f);
        const int red = scene.add_material(AGPT_MAT_DIFFUSE_ONLY, float3{0.7f, 0.2f, 0.15f}, 0.f, 0.f);
        scene.primitives_push_back(floor_mesh(), grey, 1);
        const int card_prim = scene.primitives_push_back(card(6), red, 1);
        scene.addAreaLight(Sphere{float3{1.6f, 2.0f, 1.0f}, 0.3f}, float3{40.f, 40.f, 40.f});
        scene.camera = CameraDesc{{0.f, 1.f, -4.f}, {0.f, 1.f, 0.f}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        const agpt_adaptive_params uniform{spp, spp, spp, 0.f, 0.f};
        AdaptiveAccumulator frame0(ctx, W, H), frame1(ctx, W, H), followed(ctx, W, H), surfaces(ctx, W, H);
        FeatureBuffers features0(ctx, W, H), features1(ctx, W, H);
        // frame 0: its history is the frame itself
        scene.SnapshotSurfaces();
        integrator.RenderAdaptive(scene, frame0, uniform, 1u);
        integrator.RenderFeatures(scene, features0);
        // frame 1: update -> snapshot -> render -> features -> temporal accumulation, once per call
        scene.TransformMesh(card_prim, turn);
        scene.SnapshotSurfaces();
        integrator.RenderAdaptive(scene, frame1, uniform, 2u);
        integrator.RenderFeaturesSurfaceMotion(scene, features1);
        frame1.TemporalAccumulate(features1, scene.camera, &frame0, &features0, scene.camera, followed, 32.f, AGPT_TEMPORAL_DEPTH_TOL,
                                  AGPT_TEMPORAL_NORMAL_COS, Motion::Follow);
        frame1.TemporalAccumulate(features1, scene.camera, &frame0, &features0, scene.camera, surfaces, 32.f, AGPT_TEMPORAL_DEPTH_TOL,
                                  AGPT_TEMPORAL_NORMAL_COS, Motion::FollowSurfaces);
        const std::vector<float> a = followed.Download(), b = surfaces.Download(), point = features1.DownloadPrevPoint();
        int card_pixels = 0, with_a = 0, with_b = 0;
        for (size_t i = 0; i < (size_t)W * H; ++i)
            if (point[4 * i + 3] == 1.f) {
                card_pixels++;
                with_a += a[4 * i + 3] > (float)spp;
                with_b += b[4 * i + 3] > (float)spp;
            }
        std::printf("card_pixels=%d share_motion=%.6f share_surface_motion=%.6f\n", card_pixels,
                    card_pixels ? (double)with_a / card_pixels : 0.0, card_pixels ? (double)with_b / card_pixels : 0.0);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
