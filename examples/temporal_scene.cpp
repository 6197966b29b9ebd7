// temporal_scene.cpp -- the frame loop of an interactive sequence through the C++ adapter (include/agpt_host.hpp): a short orbit
// around the sphere; every frame renders 4 fresh samples per pixel and the first-hit feature buffers, adds the reprojected history
// of the previous frame (agpt_temporal_accumulate), filters the result (agpt_denoise) and resolves it.  Between frames the host keeps
// two things: the history buffers this frame wrote and this frame's feature buffers (and the camera they were rendered with).
//
//   g++ -std=c++17 -Iinclude examples/temporal_scene.cpp -o temporal_scene libagpt_hip.so
//   ./temporal_scene out.bin [width height frames]  -> the last frame's history (float4 plane, moment plane), its denoised float4
//                                                      plane and resolved 0x00RRGGBB words, then every frame's lookfrom (3 floats)
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "agpt_host.hpp"
using namespace agpt;

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s out.bin [width height frames]\n", argv[0]);
        return 2;
    }
    const int W = argc > 3 ? std::atoi(argv[2]) : 96, H = argc > 3 ? std::atoi(argv[3]) : 64, frames = argc > 4 ? std::atoi(argv[4]) : 4;
    if (frames < 1) return 2;
    try {
        Context ctx(0);
        Scene scene(ctx);
        int gold = DisneyMaterial::Make(scene, float3{0.944f, 0.776f, 0.373f}, .5f, 1.f);
        int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, 1.f, 0.f);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1, 20}, float3{40, 20, 40}, 7.5f, 32), floor, 1);
        scene.primitives_push_back(Sphere{float3{0, 0, 0}, 1.f}, gold);
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 1.16f, -4.64f}, {0, 0, 0}, {0, 1, 0}, (float)W / (float)H, 45.f, 0.f};
        scene.commit();

        PathTracer integrator;
        const agpt_adaptive_params uniform{4, 4, 4, 0.f, 0.f};   // rel_error <= 0, min_spp = max_spp: every pixel gets 4 samples
        AdaptiveAccumulator current(ctx, W, H);
        // ping-pong: what frame k writes, frame k + 1 reads as `prev`
        std::unique_ptr<AdaptiveAccumulator> history[2] = {std::make_unique<AdaptiveAccumulator>(ctx, W, H),
                                                           std::make_unique<AdaptiveAccumulator>(ctx, W, H)};
        std::unique_ptr<FeatureBuffers> features[2] = {std::make_unique<FeatureBuffers>(ctx, W, H), std::make_unique<FeatureBuffers>(ctx, W, H)};
        Accumulator denoised(ctx, W, H);
        CameraDesc cam_prev = scene.camera;
        std::vector<float> lookfroms;
        std::vector<uint32_t> rgb;
        const float c = 0.99875026f, s = 0.04997917f;            // one step of the orbit: 0.05 rad about the y axis
        for (int k = 0; k < frames; ++k) {
            const int cur = k & 1, prev = cur ^ 1;
            if (k > 0) {
                const float x = scene.camera.lookfrom[0], z = scene.camera.lookfrom[2];
                scene.camera.lookfrom[0] = c * x + s * z;
                scene.camera.lookfrom[2] = c * z - s * x;
                scene.set_camera();
            }
            for (int a = 0; a < 3; ++a) lookfroms.push_back(scene.camera.lookfrom[a]);
            current.Clear();
            integrator.RenderAdaptive(scene, current, uniform, (uint32_t)k);
            integrator.RenderFeatures(scene, *features[cur]);
            current.TemporalAccumulate(*features[cur], scene.camera, k ? history[prev].get() : nullptr, k ? features[prev].get() : nullptr,
                                       cam_prev, *history[cur]);
            history[cur]->Denoise(*features[cur], denoised);
            rgb = denoised.CopyToSurface();                      // the frame a viewer would show
            cam_prev = scene.camera;
        }
        const AdaptiveAccumulator& last = *history[(frames - 1) & 1];
        const std::vector<float> hist = last.Download(), m2 = last.DownloadMoment2(), out = denoised.Download();

        FILE* f = std::fopen(argv[1], "wb");
        if (!f) {
            std::fprintf(stderr, "cannot write %s\n", argv[1]);
            return 1;
        }
        std::fwrite(hist.data(), 4, hist.size(), f);
        std::fwrite(m2.data(), 4, m2.size(), f);
        std::fwrite(out.data(), 4, out.size(), f);
        std::fwrite(rgb.data(), 4, rgb.size(), f);
        std::fwrite(lookfroms.data(), 4, lookfroms.size(), f);
        std::fclose(f);
        std::printf("temporal %dx%d frames=%d\n", W, H, frames);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
