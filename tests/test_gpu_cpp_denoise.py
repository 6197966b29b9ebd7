"""The C++ adapter's denoising path (include/agpt_host.hpp: FeatureBuffers, PathTracer::RenderFeatures,
AdaptiveAccumulator::Denoise): examples/denoise_scene.cpp compiled with g++ against libagpt_hip.so must give the bytes the
Python path gives."""
import re
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import build_cpp_example, gpu_scene

W, H = 96, 64


def test_cpp_denoise_program_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "denoise_scene")


@pytest.mark.gpu
def test_cpp_denoise_matches_python(tmp_path):
    exe = build_cpp_example(tmp_path, "denoise_scene")
    out_path = str(tmp_path / "out.bin")
    out = subprocess.check_output([exe, out_path, str(W), str(H)], timeout=300).decode()
    assert re.search(r"denoised %dx%d samples=1" % (W, H), out), out
    raw = np.fromfile(out_path, np.uint8)
    n = W * H * 16
    albedo_c, nd_c, den_c = (raw[k * n:(k + 1) * n].view(np.float32).reshape(H, W, 4) for k in range(3))
    rgb_c = raw[3 * n:].view(np.uint32)

    d = ag.SceneDesc("cpp-denoise")
    d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], .5, 1.)
    floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
    d.add_mesh(*ag.create_backdrop([0, -1, 20], [40, 20, 40], 7.5, 32), floor, 1)
    d.add_sphere([0, 0, 0], 1.0, 0)
    d.add_area_light([0, 25, -20], 1.0, [200., np.float32(.941) * np.float32(200), np.float32(.914) * np.float32(200)])
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], np.float32(W) / np.float32(H), 45.0, 0.0)
    g = gpu_scene(d)
    try:
        pt = ag.PathTracer(5)
        acc, m2, _, _ = pt.render_adaptive_to_host(g, W, H, 16, 16, 16, 0.0)
        albedo, nd = pt.render_features_to_host(g, W, H)
        den = g.ctx.denoise_to_host(acc, m2, albedo, nd)
        p = g.ctx.alloc(den.nbytes)
        try:
            g.ctx.upload(p, den)
            rgb = g.ctx.resolve(p, W * H, 1)
        finally:
            g.ctx.free(p)
    finally:
        g.close()
    assert albedo_c.tobytes() == albedo.tobytes()
    assert nd_c.tobytes() == nd.tobytes()
    assert den_c.tobytes() == den.tobytes()
    assert np.array_equal(rgb_c, rgb)
    assert len(np.unique(albedo[..., 3])) >= 2 and (den[..., 3] == 1).all()
