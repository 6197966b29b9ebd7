"""The C++ adapter's calls that move a light (include/agpt_host.hpp: Scene::updateSphere): examples/orbiting_light_scene.cpp compiled
with g++ against libagpt_hip.so.  The history, prev_point and denoised image it writes for its last frame are, byte for byte, those of
the same frames through the Python binding."""
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import build_cpp_example, gpu_context, gpu_scene

F = np.float32
W, H, FRAMES = 64, 48, 4
ORBIT = ((1.6, 1.0), (1.8, 0.4), (1.85, -0.25), (1.7, -0.9))
CAMERA = ([0.0, 1.0, -4.0], [0.0, 1.0, 0.0], [0, 1, 0], F(W) / F(H), 45.0, 0.0)


def example_scene():
    """the program's scene, its card in the program's own float32 arithmetic"""
    n = 6
    g = np.arange(n + 1, dtype=F) / F(n)
    X, Y = np.meshgrid(F(-0.5) + g, F(0.5) + g, indexing="ij")
    verts = np.stack([X, Y, np.zeros_like(X)], -1).reshape(-1, 3).astype(F)
    tri = []
    for i in range(n):
        for j in range(n):
            a, b = i * (n + 1) + j, (i + 1) * (n + 1) + j
            tri += [a, b, a + 1, a + 1, b, b + 1]
    idx = np.zeros((len(tri), 3), np.int32)
    idx[:, 0] = tri
    floor = np.array([[-5, 0, -5], [5, 0, -5], [-5, 0, 5], [5, 0, 5]], F)
    fidx = np.zeros((6, 3), np.int32)
    fidx[:, 0] = [0, 2, 1, 1, 2, 3]
    d = ag.SceneDesc("orbiting-light")
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.6, 0.6, 0.6), 0.0, 0.0)
    red = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.7, 0.2, 0.15), 0.0, 0.0)
    d.add_mesh(floor, None, None, fidx, grey)
    d.add_mesh(verts, None, None, idx, red)
    light = d.add_area_light((ORBIT[0][0], 2.0, ORBIT[0][1]), 0.3, (40.0, 40.0, 40.0))
    d.set_camera(*CAMERA)
    return d, light


def test_cpp_orbiting_light_program_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "orbiting_light_scene")


@pytest.mark.gpu
def test_cpp_orbiting_light_writes_the_python_routes_bytes(tmp_path):
    exe = build_cpp_example(tmp_path, "orbiting_light_scene")
    path = tmp_path / "frames.bin"
    out = subprocess.check_output([exe, str(W), str(H), str(FRAMES), str(path)], timeout=300).decode()
    print(out)
    hist, point, image = np.fromfile(str(path), F).reshape(3, H, W, 4)
    ctx = gpu_context()
    pt = ag.PathTracer(5)
    desc, light = example_scene()
    g = gpu_scene(desc)
    clamp = ag.TemporalClampParams(2, 1, 1.0, 8.0)
    prev = None
    try:
        for k in range(FRAMES):
            g.update_sphere(light, (ORBIT[k % 4][0], 2.0, ORBIT[k % 4][1]), 0.3)
            g.snapshot_positions()
            acc, m2, _, _ = pt.render_adaptive_to_host(g, W, H, 4, 4, 4, 0.0, seed_base=k)
            albedo, nd, pp = pt.render_features_motion_to_host(g, W, H)
            h_acc, h_m2 = ctx.temporal_to_host(CAMERA, CAMERA, acc, m2, albedo, nd, prev=prev, prev_point=pp, clamp=clamp)
            den = ctx.denoise_to_host(h_acc, h_m2, albedo, nd)
            prev = (h_acc, h_m2, albedo, nd)
    finally:
        g.close()
    assert point.tobytes() == pp.tobytes()
    assert hist.tobytes() == h_acc.tobytes()
    assert image.tobytes() == den.tobytes()
    on_light = pp[..., 3] == 1
    assert 10 <= on_light.sum() <= 200                                  # the light moved, and only the light
    assert out.split() == ["frames", str(FRAMES), "light_pixels", str(int(on_light.sum())), "history", str(int((h_acc[on_light, 3] > 4).sum()))]
