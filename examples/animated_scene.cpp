// animated_scene.cpp -- a mesh that changes shape between frames through the C++ adapter (include/agpt_host.hpp): simple_test_scene's
// backdrop with a blob whose bumps travel around it.  Every frame hands the new positions and normals to Scene::UpdateMesh -- the
// BVH keeps its topology and the blob's records are rewritten on the GPU --, clears the accumulator, renders and writes a PNG; the
// last frame rebuilds the tree instead, which is what a host does once the shape has drifted far from the pose the tree was built for.
//
//   g++ -std=c++17 -Iinclude examples/animated_scene.cpp -o animated_scene libagpt_hip.so
//   ./animated_scene frame [frames width height]      -> frame_000.png, frame_001.png, ...
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "agpt_host.hpp"
using namespace agpt;

// a unit sphere displaced along its radius by two travelling waves; the same indices and texture coordinates for every phase
static TriangleMesh blob(int n_seg, int n_ring, float phase) {
    TriangleMesh m;
    const float pi = 3.14159265358979f;
    auto radius = [&](float theta, float phi) {
        return 1.f + .14f * std::sin(3 * phi + phase) * std::sin(2 * theta) + .07f * std::sin(5 * phi - 2 * phase) * std::sin(4 * theta);
    };
    auto position = [&](float theta, float phi, float* p) {
        const float r = radius(theta, phi);
        p[0] = r * std::sin(theta) * std::cos(phi);
        p[1] = r * std::cos(theta);
        p[2] = r * std::sin(theta) * std::sin(phi);
    };
    for (int i = 0; i <= n_ring; i++)
        for (int j = 0; j <= n_seg; j++) {
            const float theta = pi * (float)i / (float)n_ring, phi = 2 * pi * (float)j / (float)n_seg;
            float p[3], a[3], b[3], c[3], d[3];
            position(theta, phi, p);
            const float e = 1e-3f;   // normal = cross of the central differences (the poles keep the radial direction)
            position(theta + e, phi, a);
            position(theta - e, phi, b);
            position(theta, phi + e, c);
            position(theta, phi - e, d);
            const float t[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]}, s[3] = {c[0] - d[0], c[1] - d[1], c[2] - d[2]};
            float n[3] = {s[1] * t[2] - s[2] * t[1], s[2] * t[0] - s[0] * t[2], s[0] * t[1] - s[1] * t[0]};
            float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (i == 0 || i == n_ring || len < 1e-12f) {
                n[0] = p[0]; n[1] = p[1]; n[2] = p[2];
                len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            }
            for (int k = 0; k < 3; k++) {
                m.vertices.push_back(p[k]);
                m.normals.push_back(n[k] / len);
            }
            m.texcoords.push_back((float)j / (float)n_seg);
            m.texcoords.push_back((float)i / (float)n_ring);
        }
    auto corner = [&](int v) {
        for (int k = 0; k < 3; k++) m.indices.push_back(v);
    };
    for (int i = 0; i < n_ring; i++)
        for (int j = 0; j < n_seg; j++) {
            const int a = i * (n_seg + 1) + j, b = a + 1, c = a + n_seg + 1, d = c + 1;
            if (i > 0) { corner(a); corner(b); corner(c); }            // (the pole rows would be zero-area triangles)
            if (i < n_ring - 1) { corner(b); corner(d); corner(c); }
        }
    return m;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s frame [frames width height]\n", argv[0]);
        return 2;
    }
    const int frames = argc > 2 ? std::atoi(argv[2]) : 4;
    const int W = argc > 4 ? std::atoi(argv[3]) : 96, H = argc > 4 ? std::atoi(argv[4]) : 64;
    try {
        Context ctx(0);
        Scene scene(ctx);
        int gold = DisneyMaterial::Make(scene, float3{0.944f, 0.776f, 0.373f}, .4f, 1.f);
        int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, 1.f, 0.f);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1.3f, 20}, float3{40, 20, 40}, 7.5f, 32), floor, 1);
        const int blob_prim = scene.primitives_push_back(blob(48, 32, 0.f), gold, 1);
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 1.16f, -4.64f}, {0, 0, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        Accumulator acc(ctx, W, H);
        for (int frame = 0; frame < frames; frame++) {
            if (frame > 0) {   // the per-frame loop: update, zero the accumulator, render, resolve
                const bool last = frame == frames - 1;
                scene.UpdateMesh(blob_prim, blob(48, 32, .6f * (float)frame), last ? MeshUpdate::Rebuild : MeshUpdate::Refit);
                acc.Clear();
            }
            integrator.Render(scene, acc, 8);
            const std::vector<uint32_t> rgb = acc.CopyToSurface();
            char name[32];
            std::snprintf(name, sizeof name, "_%03d.png", frame);
            const std::string path = std::string(argv[1]) + name;
            if (agpt_write_png(path.c_str(), rgb.data(), W, H) != AGPT_OK) {
                std::fprintf(stderr, "cannot write %s: %s\n", path.c_str(), agpt_last_error());
                return 1;
            }
            std::printf("%s samples=%d\n", path.c_str(), acc.NumSamples());
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
