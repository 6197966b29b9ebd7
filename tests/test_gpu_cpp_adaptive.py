"""The C++ adapter's adaptive path (include/agpt_host.hpp: AdaptiveAccumulator, PathTracer::RenderAdaptive): a small program
compiled with g++ against libagpt_hip.so renders adaptively in two calls, and must give the bytes the Python path gives."""
import re
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import build_cpp_example, gpu_scene

W, H = 96, 64

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "agpt_host.hpp"
using namespace agpt;

int main(int argc, char** argv) {
    const int W = %(W)d, H = %(H)d;
    try {
        Context ctx(0);
        Scene scene(ctx);
        int gold = DisneyMaterial::Make(scene, float3{0.944f, 0.776f, 0.373f}, .5f, 1.f);
        int floor = DisneyMaterial::Make(scene, float3{0.6f, 0.62f, 0.45f}, 1.f, 0.f);
        scene.primitives_push_back(TriangleMesh::CreateBackdrop(float3{0, -1, 20}, float3{40, 20, 40}, 7.5f, 32), floor, 1);
        scene.primitives_push_back(Sphere{float3{0, 0, 0}, 1.f}, gold);
        scene.addAreaLight(Sphere{float3{0, 25, -20}, 1.f}, float3{200.f, .941f * 200, .914f * 200});
        scene.lights_push_back(UniformInfiniteLight{float3{.4f, .45f, .5f}});
        scene.camera = CameraDesc{{-1.46f, 1.16f, -4.64f}, {0, 0, 0}, {0, 1, 0}, 1.5f, 45.f, 0.f};
        scene.commit();
        PathTracer integrator;
        AdaptiveAccumulator acc(ctx, W, H);
        agpt_adaptive_params p{4, 16, 4, 0.1f, 0.01f};
        agpt_adaptive_stats a1{}, a2{};
        integrator.RenderAdaptive(scene, acc, p, 0u, &a1);
        p.max_spp = 32;   // continue the frame
        agpt_stats st = integrator.RenderAdaptive(scene, acc, p, 0u, &a2);
        std::vector<float> pix = acc.Download(), m2 = acc.DownloadMoment2();
        std::vector<uint32_t> rgb = acc.CopyToSurface();
        FILE* f = std::fopen(argv[1], "wb");
        std::fwrite(pix.data(), 4, pix.size(), f);
        std::fwrite(m2.data(), 4, m2.size(), f);
        std::fwrite(rgb.data(), 4, rgb.size(), f);
        std::fclose(f);
        std::printf("samples=%%llu %%llu stats=%%llu rounds=%%d\n", (unsigned long long)a1.samples, (unsigned long long)a2.samples,
                    (unsigned long long)st.samples, a2.rounds);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%%s\n", e.what());
        return 1;
    }
    return 0;
}
"""


def build_program(tmp_path):
    src = tmp_path / "adaptive.cpp"
    src.write_text(PROGRAM % dict(W=W, H=H))
    return build_cpp_example(tmp_path, str(src))


def test_cpp_adaptive_program_compiles_and_links(tmp_path):
    build_program(tmp_path)


@pytest.mark.gpu
def test_cpp_adaptive_matches_python(tmp_path):
    exe = build_program(tmp_path)
    out_path = str(tmp_path / "out.bin")
    out = subprocess.check_output([exe, out_path], timeout=300).decode()
    m = re.search(r"samples=(\d+) (\d+) stats=(\d+) rounds=(\d+)", out)
    assert m, out
    raw = np.fromfile(out_path, np.uint8)
    acc_c = raw[:W * H * 16].view(np.float32).reshape(H, W, 4)
    m2_c = raw[W * H * 16:W * H * 20].view(np.float32).reshape(H, W)
    rgb_c = raw[W * H * 20:].view(np.uint32)

    d = ag.SceneDesc("cpp-adaptive")
    gold = d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], .5, 1.)
    floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
    d.add_mesh(*ag.create_backdrop([0, -1, 20], [40, 20, 40], 7.5, 32), floor, 1)
    d.add_sphere([0, 0, 0], 1.0, gold)
    d.add_area_light([0, 25, -20], 1.0, [200., np.float32(.941) * np.float32(200), np.float32(.914) * np.float32(200)])
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], 1.5, 45.0, 0.0)
    g = gpu_scene(d)
    try:
        acc, m2, st, ast = ag.PathTracer(5).render_adaptive_to_host(g, W, H, 4, 32, 4, 0.1, abs_floor=0.01)
        ctx = g.ctx
        p = ctx.alloc(acc.nbytes)
        try:
            ctx.upload(p, acc)
            rgb = ctx.resolve_counts(p, W * H)
        finally:
            ctx.free(p)
    finally:
        g.close()
    assert acc_c.tobytes() == acc.tobytes()
    assert m2_c.tobytes() == m2.tobytes()
    assert np.array_equal(rgb_c, rgb)
    assert int(m.group(1)) + int(m.group(2)) == ast.samples == int(acc[..., 3].sum())
    assert int(m.group(3)) == int(m.group(2))
    assert len(np.unique(acc[..., 3])) >= 2
