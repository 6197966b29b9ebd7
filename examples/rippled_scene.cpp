// rippled_scene.cpp -- a surface whose positions alone change per frame, through the C++ adapter (include/agpt_host.hpp): a 17 x 17 grid
// over simple_test_scene's backdrop whose heights are rewritten every frame by a travelling ripple, as a simulation step would.  The host
// has no normals to give: the mesh is put in MeshNormals::Smooth mode once (Scene::SetMeshNormalsMode), and every Scene::UpdateMesh then
// recomputes its vertex normals on the GPU from the new positions (agpt_vertex_normals_arrays' definition), ahead of the refit.  The
// normals the mesh was added with are never read again.  Each frame clears the accumulator, renders and prints the FNV-1a hash of the
// resolved pixels; with a path prefix it also writes one PNG per frame.
//
//   g++ -std=c++17 -Iinclude examples/rippled_scene.cpp -o rippled_scene libagpt_hip.so
//   ./rippled_scene [frames width height [prefix]]    -> "frame 0 hash 0123456789abcdef", ... (prefix_000.png, ...)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "agpt_host.hpp"
using namespace agpt;

constexpr int kSide = 17;

// a triangle wave of period 8 and height 4 in whole steps: every height below is a dyadic fraction, the same float on every host
static int wave(int k) {
    const int r = ((k % 8) + 8) % 8;
    return r < 4 ? r : 8 - r;
}

static float height(int i, int j, int frame) { return 0.0625f * (float)wave(i + 2 * frame) + 0.03125f * (float)wave(2 * j + 3 * frame); }

// 17 x 17 vertices over [-2, 2] x [-2, 2], one normal per vertex ((0, 1, 0): never used after the first update)
static TriangleMesh grid() {
    TriangleMesh m;
    for (int i = 0; i < kSide; i++)
        for (int j = 0; j < kSide; j++) {
            m.vertices.insert(m.vertices.end(), {0.25f * (float)i - 2.f, 0.f, 0.25f * (float)j - 2.f});
            m.normals.insert(m.normals.end(), {0.f, 1.f, 0.f});
        }
    for (int i = 0; i + 1 < kSide; i++)
        for (int j = 0; j + 1 < kSide; j++) {
            const int a = i * kSide + j, b = a + 1, c = a + kSide, d = c + 1;
            for (int v : {a, b, c, b, d, c}) m.indices.insert(m.indices.end(), {v, v, -1});   // (vertex, normal, texcoord)
        }
    return m;
}

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 4;
    const int W = argc > 3 ? std::atoi(argv[2]) : 96, H = argc > 3 ? std::atoi(argv[3]) : 64;
    const std::string prefix = argc > 4 ? argv[4] : "";
    try {
        Context ctx(0);
        Scene scene(ctx);
        int blue = DisneyMaterial::Make(scene, float3{0.15f, 0.35f, 0.8f}, .3f, 0.f);
        int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, 1.f, 0.f);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1.5f, 20}, float3{40, 20, 40}, 7.5f, 8), floor, 1);
        TriangleMesh surface = grid();
        const int water = scene.primitives_push_back(surface, blue, 4);
        scene.SetMeshNormalsMode(water, MeshNormals::Smooth);
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 2.16f, -5.64f}, {0, 0.f, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        Accumulator acc(ctx, W, H);
        for (int frame = 0; frame < frames; frame++) {
            for (int i = 0; i < kSide; i++)
                for (int j = 0; j < kSide; j++) surface.vertices[3 * (i * kSide + j) + 1] = height(i, j, frame);
            scene.UpdateMesh(water, surface);   // the per-frame loop: positions only, zero the accumulator, render, resolve
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
