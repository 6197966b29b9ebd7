// rigid_scene.cpp -- a rigid object moved between frames through the C++ adapter (include/agpt_host.hpp): an octahedron over
// simple_test_scene's backdrop, turned about the vertical axis and lifted a little every frame with Scene::TransformMesh.  The host
// sends 16 floats per frame; the matrix is applied on the GPU to the mesh's rest pose (absolute, so the turns do not accumulate
// rounding), the BVH keeps its topology and the mesh's records are rewritten in place.  Each frame clears the accumulator, renders
// and prints the FNV-1a hash of the resolved pixels; with a path prefix it also writes one PNG per frame.
//
//   g++ -std=c++17 -Iinclude examples/rigid_scene.cpp -o rigid_scene libagpt_hip.so
//   ./rigid_scene [frames width height [prefix]]      -> "frame 0 hash 0123456789abcdef", ... (prefix_000.png, ...)
#include <cstdio>
#include <cstdlib>
#include <string>

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
    const int frames = argc > 1 ? std::atoi(argv[1]) : 4;
    const int W = argc > 3 ? std::atoi(argv[2]) : 96, H = argc > 3 ? std::atoi(argv[3]) : 64;
    const std::string prefix = argc > 4 ? argv[4] : "";
    // (cos, sin) of the turn, four to a cycle: Pythagorean pairs, so that every host writes the same floats
    const float turns[4][2] = {{1.0f, 0.0f}, {0.8f, 0.6f}, {0.28f, 0.96f}, {-0.352f, 0.936f}};
    try {
        Context ctx(0);
        Scene scene(ctx);
        int gold = DisneyMaterial::Make(scene, float3{0.944f, 0.776f, 0.373f}, .4f, 1.f);
        int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, 1.f, 0.f);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1.5f, 20}, float3{40, 20, 40}, 7.5f, 8), floor, 1);
        const int spinner = scene.primitives_push_back(octahedron(), gold, 1);
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 1.16f, -4.64f}, {0, 0, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        Accumulator acc(ctx, W, H);
        for (int frame = 0; frame < frames; frame++) {
            const float c = turns[frame % 4][0], s = turns[frame % 4][1], lift = 0.25f * (float)frame;
            const float m[16] = {c, 0, s, 0, 0, 1, 0, lift, -s, 0, c, 0, 0, 0, 0, 1};
            scene.TransformMesh(spinner, m);   // the per-frame loop: place, zero the accumulator, render, resolve
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
