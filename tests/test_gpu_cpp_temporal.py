"""The C++ adapter's frame loop (include/agpt_host.hpp: AdaptiveAccumulator::TemporalAccumulate): examples/temporal_scene.cpp
compiled with g++ against libagpt_hip.so must leave the history bytes the Python path leaves after the same frames."""
import re
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import build_cpp_example, gpu_scene

W, H, FRAMES = 48, 40, 3


def test_cpp_temporal_program_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "temporal_scene")


@pytest.mark.gpu
def test_cpp_temporal_matches_python(tmp_path):
    exe = build_cpp_example(tmp_path, "temporal_scene")
    out_path = str(tmp_path / "out.bin")
    out = subprocess.check_output([exe, out_path, str(W), str(H), str(FRAMES)], timeout=300).decode()
    assert re.search(r"temporal %dx%d frames=%d" % (W, H, FRAMES), out), out
    raw = np.fromfile(out_path, np.uint8)
    n = W * H * 4
    assert raw.size == n * 4 + n + n * 4 + n + FRAMES * 12
    hist_c = raw[:4 * n].view(np.float32).reshape(H, W, 4)
    m2_c = raw[4 * n:5 * n].view(np.float32).reshape(H, W)
    den_c = raw[5 * n:9 * n].view(np.float32).reshape(H, W, 4)
    rgb_c = raw[9 * n:10 * n].view(np.uint32)
    lookfroms = raw[10 * n:].view(np.float32).reshape(FRAMES, 3)
    assert lookfroms[0].tobytes() == np.array([-1.46, 1.16, -4.64], np.float32).tobytes()
    assert len(np.unique(lookfroms[:, 0])) == FRAMES and (lookfroms[:, 1] == lookfroms[0, 1]).all()

    d = ag.SceneDesc("cpp-temporal")
    d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], .5, 1.)
    floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
    d.add_mesh(*ag.create_backdrop([0, -1, 20], [40, 20, 40], 7.5, 32), floor, 1)
    d.add_sphere([0, 0, 0], 1.0, 0)
    d.add_area_light([0, 25, -20], 1.0, [200., np.float32(.941) * np.float32(200), np.float32(.914) * np.float32(200)])
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera(lookfroms[0], [0, 0, 0], [0, 1, 0], np.float32(W) / np.float32(H), 45.0, 0.0)
    g = gpu_scene(d)
    try:
        pt = ag.PathTracer(5)
        prev, cam_prev = None, None
        for k in range(FRAMES):
            cam = (lookfroms[k], [0, 0, 0], [0, 1, 0], np.float32(W) / np.float32(H), 45.0, 0.0)
            g.set_camera(*cam)
            acc, m2, _, _ = pt.render_adaptive_to_host(g, W, H, 4, 4, 4, 0.0, seed_base=k)
            albedo, nd = pt.render_features_to_host(g, W, H)
            hist, hm2 = g.ctx.temporal_to_host(cam, cam_prev if prev is not None else cam, acc, m2, albedo, nd, prev=prev)
            prev, cam_prev = (hist, hm2, albedo, nd), cam
        den = g.ctx.denoise_to_host(hist, hm2, albedo, nd)
        p = g.ctx.alloc(den.nbytes)
        try:
            g.ctx.upload(p, den)
            rgb = g.ctx.resolve(p, W * H, 1)
        finally:
            g.ctx.free(p)
    finally:
        g.close()
    assert (hist[..., 3] > 4).any(), "history was taken"
    assert hist_c.tobytes() == hist.tobytes()
    assert m2_c.tobytes() == hm2.tobytes()
    assert den_c.tobytes() == den.tobytes()
    assert np.array_equal(rgb_c, rgb)
