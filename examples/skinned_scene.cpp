// skinned_scene.cpp -- an articulated object moved between frames through the C++ adapter (include/agpt_host.hpp): a strip of 16
// segments over simple_test_scene's backdrop, bound to two joints -- the weight of the second grows from 0 at one end to 1 at the
// other -- and bent upwards a little more every frame with Scene::PoseMesh.  The binding is given once (Scene::SetMeshSkin); the host
// then sends two matrices per frame, and the blend runs on the GPU from the strip's rest pose (absolute, so the frames do not
// accumulate rounding), the BVH keeps its topology and the mesh's records are rewritten in place.  Each frame clears the accumulator,
// renders and prints the FNV-1a hash of the resolved pixels; with a path prefix it also writes one PNG per frame.
//
//   g++ -std=c++17 -Iinclude examples/skinned_scene.cpp -o skinned_scene libagpt_hip.so
//   ./skinned_scene [frames width height [prefix]]    -> "frame 0 hash 0123456789abcdef", ... (prefix_000.png, ...)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "agpt_host.hpp"
using namespace agpt;

constexpr int kSegments = 16;

// 2 x 17 vertices along x in [-2, 2], one normal (0, 1, 0) per vertex; every coordinate and weight is a dyadic fraction
static TriangleMesh strip(std::vector<int32_t>& joints, std::vector<float>& weights) {
    TriangleMesh m;
    for (int i = 0; i <= kSegments; i++)
        for (int side = 0; side < 2; side++) {
            const float x = 0.25f * (float)i - 2.f, z = side ? 0.5f : -0.5f, t = (float)i / (float)kSegments;
            m.vertices.insert(m.vertices.end(), {x, 0.f, z});
            m.normals.insert(m.normals.end(), {0.f, 1.f, 0.f});
            joints.insert(joints.end(), {0, 1});
            weights.insert(weights.end(), {1.f - t, t});
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
    // (cos, sin) of the second joint's turn, four to a cycle: Pythagorean pairs, so that every host writes the same floats
    const float turns[4][2] = {{1.0f, 0.0f}, {0.96f, 0.28f}, {0.8f, 0.6f}, {0.6f, 0.8f}};
    try {
        Context ctx(0);
        Scene scene(ctx);
        int red = DisneyMaterial::Make(scene, float3{0.8f, 0.1f, 0.12f}, .6f, 0.f);
        int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, 1.f, 0.f);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1.5f, 20}, float3{40, 20, 40}, 7.5f, 8), floor, 1);
        std::vector<int32_t> joints;
        std::vector<float> weights;
        const int bender = scene.primitives_push_back(strip(joints, weights), red, 1);
        scene.SetMeshSkin(bender, 2, 2, joints, weights);   // normals: as many as vertices, the same influences
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 2.16f, -5.64f}, {0, 0.5f, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        Accumulator acc(ctx, W, H);
        for (int frame = 0; frame < frames; frame++) {
            const float c = turns[frame % 4][0], s = turns[frame % 4][1], lift = 0.125f * (float)frame;
            // joint 0 stays; joint 1 turns about the z axis and rises
            const std::vector<float> pose = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1,
                                             c, -s, 0, 0, s, c, 0, lift, 0, 0, 1, 0, 0, 0, 0, 1};
            scene.PoseMesh(bender, pose);   // the per-frame loop: pose, zero the accumulator, render, resolve
            acc.Clear();
            integrator.Render(scene, acc, 4);
            const std::vector<uint32_t> rgb = acc.CopyToSurface();
            unsigned long long h = 1469598103934665603ull;
            for (uint32_t w : rgb) h = (h ^ w) * 1099511628211ull;
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
