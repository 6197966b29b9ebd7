// morphed_scene.cpp -- morph targets (blend shapes) through the C++ adapter (include/agpt_host.hpp): skinned_scene's strip of 16 segments
// over simple_test_scene's backdrop with two targets -- a bulge that lifts the middle of the strip and a twist that raises one edge and
// lowers the other towards the far end, both with normal deltas -- driven over four frames by two weights; the last two frames are also
// bent by the strip's two joints.  The deltas are given once (Scene::SetMeshMorphTargets); the host then sends two weights (and two
// matrices) per frame, and morph and skin run in one kernel on the GPU from the strip's rest pose (absolute, so the frames do not
// accumulate rounding).  Each frame clears the accumulator, renders and prints the FNV-1a hash of the resolved pixels; with a path
// prefix it also writes one PNG per frame.
//
//   g++ -std=c++17 -Iinclude examples/morphed_scene.cpp -o morphed_scene libagpt_hip.so
//   ./morphed_scene [frames width height [prefix]]    -> "frame 0 hash 0123456789abcdef", ... (prefix_000.png, ...)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "agpt_host.hpp"
using namespace agpt;

constexpr int kSegments = 16;
constexpr int kVertices = 2 * (kSegments + 1);

// 2 x 17 vertices along x in [-2, 2], one normal (0, 1, 0) per vertex; every coordinate, weight and delta is a dyadic fraction
static TriangleMesh strip(std::vector<int32_t>& joints, std::vector<float>& weights, std::vector<float>& position_deltas,
                          std::vector<float>& normal_deltas) {
    TriangleMesh m;
    position_deltas.assign(2 * kVertices * 3, 0.f);   // [target][vertex][xyz]: target 0 the bulge, target 1 the twist
    normal_deltas.assign(2 * kVertices * 3, 0.f);
    for (int i = 0; i <= kSegments; i++)
        for (int side = 0; side < 2; side++) {
            const float x = 0.25f * (float)i - 2.f, z = side ? 0.5f : -0.5f, t = (float)i / (float)kSegments;
            const int v = 2 * i + side;
            m.vertices.insert(m.vertices.end(), {x, 0.f, z});
            m.normals.insert(m.normals.end(), {0.f, 1.f, 0.f});
            joints.insert(joints.end(), {0, 1});
            weights.insert(weights.end(), {1.f - t, t});
            const float hump = 1.f - (float)(i < 8 ? 8 - i : i - 8) / 8.f;                       // 0 at both ends, 1 in the middle
            position_deltas[3 * v + 1] = 0.75f * hump;                                           // the bulge: up
            normal_deltas[3 * v + 0] = i < 8 ? -0.375f : (i > 8 ? 0.375f : 0.f);                 //   and its normals lean outwards
            position_deltas[3 * (kVertices + v) + 1] = (side ? 0.5f : -0.5f) * t;                // the twist: one edge up, one down
            normal_deltas[3 * (kVertices + v) + 2] = -0.5f * t;
        }
    for (int i = 0; i < kSegments; i++) {
        const int a = 2 * i, b = 2 * i + 1, c = 2 * i + 2, d = 2 * i + 3;
        for (int v : {a, b, c, b, d, c}) m.indices.insert(m.indices.end(), {v, v, -1});   // (vertex, normal, texcoord)
    }
    return m;
}

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 4;
    const int W = argc > 3 ? std::atoi(argv[2]) : 96, H = argc > 3 ? std::atoi(argv[3]) : 64;
    const std::string prefix = argc > 4 ? argv[4] : "";
    // (bulge, twist) per frame, four to a cycle; the second half of a cycle is also bent: (cos, sin) of the second joint's turn,
    // Pythagorean pairs, so that every host writes the same floats
    const float morphs[4][2] = {{0.5f, 0.f}, {1.f, 0.25f}, {0.75f, 0.5f}, {-0.25f, 1.f}};
    const float turns[4][2] = {{1.0f, 0.0f}, {1.0f, 0.0f}, {0.96f, 0.28f}, {0.8f, 0.6f}};
    try {
        Context ctx(0);
        Scene scene(ctx);
        int red = DisneyMaterial::Make(scene, float3{0.8f, 0.1f, 0.12f}, .6f, 0.f);
        int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, 1.f, 0.f);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1.5f, 20}, float3{40, 20, 40}, 7.5f, 8), floor, 1);
        std::vector<int32_t> joints;
        std::vector<float> weights, position_deltas, normal_deltas;
        const int ribbon = scene.primitives_push_back(strip(joints, weights, position_deltas, normal_deltas), red, 1);
        scene.SetMeshMorphTargets(ribbon, 2, position_deltas, normal_deltas);
        scene.SetMeshSkin(ribbon, 2, 2, joints, weights);   // normals: as many as vertices, the same influences
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 2.16f, -5.64f}, {0, 0.5f, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        Accumulator acc(ctx, W, H);
        for (int frame = 0; frame < frames; frame++) {
            const int k = frame % 4;
            const std::vector<float> w = {morphs[k][0], morphs[k][1]};
            if (k < 2) {
                scene.MorphMesh(ribbon, w);   // the per-frame loop: morph (and pose), zero the accumulator, render, resolve
            } else {
                const float c = turns[k][0], s = turns[k][1], lift = 0.125f * (float)frame;
                // joint 0 stays; joint 1 turns about the z axis and rises
                scene.MorphMesh(ribbon, w, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1,
                                            c, -s, 0, 0, s, c, 0, lift, 0, 0, 1, 0, 0, 0, 0, 1});
            }
            acc.Clear();
            integrator.Render(scene, acc, 4);
            const std::vector<uint32_t> rgb = acc.CopyToSurface();
            unsigned long long h = 1469598103934665603ull;
            for (uint32_t word : rgb) h = (h ^ word) * 1099511628211ull;
            std::printf("frame %d hash %016llx\n", frame, h);
            if (!prefix.empty()) {
                char name[32];
                std::snprintf(name, sizeof name, "_%03d.png", frame);
                if (agpt_write_png((prefix + name).c_str(), rgb.data(), W, H) != AGPT_OK) {
                    std::fprintf(stderr, "cannot write %s%s: %s\n", prefix.c_str(), name, agpt_last_error());
                    return 1;
                }
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
