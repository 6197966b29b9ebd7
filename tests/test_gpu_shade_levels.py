"""launch_shading's table of shading units, cell by cell: a ladder of scenes S0 .. S4 on one quad, each needing exactly its texturing
level (agpt_shade_kernels.h), rendered in both arithmetics.  The exact kernels of every level are pinned to the oracle in their
<LDS tables, no ENV> instantiation by the tests of their own features (test_gpu_textures, _material_maps, _texture_filter, _normal_map),
and in the instantiations with an environment map or with the scene tables in global memory by test_gpu_shade_matrix.py (every level
against the oracle under ENV, global tables byte for byte against LDS tables and at the three count limits) and the textured fuzz of
test_gpu_fuzz.py; here they are the reference: FAST must land
within the project's L2 rule (test_gpu_shading_fast: >= 99 % of pixels with every channel within 1e-3 |exact| + 1e-6) of the EXACT
render of the same level, and the EXACT renders of neighbouring levels must be far apart under that rule (fewer than 90 % of pixels
agree), so a launcher one level off cannot pass.

Share of pixels on which the EXACT render of S_L agrees with that of S_{L-1} under that rule, observed on an MI355X: L=1 0.0000,
L=2 0.0004, L=3 0.0000, L=4 0.0004 (the quad fills the frame and every level changes every hit); FAST against EXACT of the same
level: 1.0000 at every level, never bit-identical."""
import functools

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import bits, close_fraction, gpu_scene

pytestmark = pytest.mark.gpu
F = np.float32
W = H = 48
SPP, DEPTH, SEED = 4, 3, 0x5EED


def colour_image():
    """4 x 4, high contrast: neighbouring texels differ in every channel"""
    rng = np.random.RandomState(3)
    img = np.where((np.add.outer(np.arange(4), np.arange(4)) % 2)[..., None] == 0, rng.uniform(.7, .95, (4, 4, 3)), rng.uniform(.05, .2, (4, 4, 3)))
    return img.astype(F)


def param_image():
    """3 x 5 (its texel borders are not the colour image's): r = metallic 0 / 1, g = roughness .15 .. .95, far from the constants"""
    y, x = np.mgrid[0:5, 0:3]
    metal = ((x + y) % 2).astype(F)
    rough = (0.15 + 0.8 * ((3 * x + 2 * y) % 5) / 4).astype(F)
    return np.stack([metal, rough, np.zeros_like(rough)], -1).astype(F)


def normal_image():
    """4 x 4 texels tilted 25 .. 40 degrees from +z, each in another direction: rgb = n / 2 + 1 / 2"""
    k = np.arange(16).reshape(4, 4)
    theta, phi = np.radians(25 + 15 * ((5 * k) % 16) / 15), 2 * np.pi * k / 16 + 0.3
    n = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)
    return (0.5 * n + 0.5).astype(F)


def ladder_scene(level):
    """S_level: one quad (two triangles, unit normal at the four vertices, uvs 0 .. 1) that fills the frame, under a sphere light and a sky"""
    d = ag.SceneDesc("shade-level-%d" % level)
    m = d.add_material(ag.MAT_DISNEY, [.8, .7, .6], .6, .1)
    corners = np.array([[-2.5, 0, -2.5], [2.5, 0, -2.5], [2.5, 0, 2.5], [-2.5, 0, 2.5]], F)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)
    tris = np.array([0, 2, 1, 0, 3, 2], np.int32)
    d.add_mesh(corners, np.broadcast_to(np.array([0, 1, 0], F), (4, 3)).copy(), uv, np.stack([tris, tris, tris], 1), m, 1)
    if level >= 1:
        colour = d.add_texture(colour_image())
        d.set_material_texture(m, colour)
    if level >= 2:
        params = d.add_texture(param_image())
        d.set_material_param_texture(m, ag.PARAM_METALLIC, params, 0)
        d.set_material_param_texture(m, ag.PARAM_ROUGHNESS, params, 1)
    if level >= 3:
        d.set_texture_sampler(colour, ag.FILTER_BILINEAR, ag.WRAP_REPEAT, ag.WRAP_REPEAT)
    if level >= 4:
        d.set_material_normal_texture(m, d.add_texture(normal_image()), 1.0)
    d.add_area_light([0.5, 5, -1], 0.7, ag.scenes.KEY_LIGHT * F(40))
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([0.2, 4.0, -0.6], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    return d


@functools.lru_cache(None)
def renders(level):
    """S_level's images: {"exact": two renders, "fast": two renders, "features": (albedo, normal_depth)}"""
    g = gpu_scene(ladder_scene(level))
    try:
        pt = ag.PathTracer(DEPTH)
        out = {}
        assert g.shade_variant()[0] == level
        for arith in ("exact", "fast"):
            g.set_shading_arith(arith)
            out[arith] = [pt.render_to_host(g, W, H, SPP, seed_base=SEED)[0][..., :3].reshape(-1, 3) for _ in range(2)]
        g.set_shading_arith("exact")
        out["features"] = pt.render_features_to_host(g, W, H)
    finally:
        g.close()
    return out


@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_each_level_runs_its_own_kernels_in_both_arithmetics(level):
    r, below = renders(level), renders(level - 1)
    exact, fast = r["exact"][0], r["fast"][0]
    apart = close_fraction(exact, below["exact"][0], 1e-3)
    close = close_fraction(fast, exact, 1e-3)
    print("level %d: EXACT agrees with level %d's on %.4f of the pixels, FAST with EXACT on %.4f" % (level, level - 1, apart, close))
    assert apart < 0.90                                   # the precondition: the level below is another image
    assert r["exact"][1].tobytes() == exact.tobytes()
    assert r["fast"][1].tobytes() == fast.tobytes()
    assert fast.tobytes() != exact.tobytes()
    assert close >= 0.99


def test_features_come_from_the_levels_own_kernel():
    (a1, n1), (a3, n3), (a4, n4) = (renders(level)["features"] for level in (1, 3, 4))
    quad = a1[..., 3] == 1
    assert quad.mean() > 0.9 and np.array_equal(a3[..., 3], a1[..., 3]) and np.array_equal(a4[..., 3], a1[..., 3])
    texels = {t.tobytes() for t in colour_image().reshape(-1, 3)}
    nearest = np.array([px.tobytes() in texels for px in a1[..., :3].reshape(-1, 3)]).reshape(H, W)
    blended = np.array([px.tobytes() not in texels for px in a3[..., :3].reshape(-1, 3)]).reshape(H, W)
    moved = (bits(n4[..., :3]) != bits(n3[..., :3])).any(-1)
    print("features: S1 albedo is a texel on %.4f of the quad, S3 albedo is a blend on %.4f, S4 moves the normal on %.4f" % (
        nearest[quad].mean(), blended[quad].mean(), moved[quad].mean()))
    assert nearest[quad].all()                                  # k_features_textured: the nearest texel
    assert blended[quad].mean() > 0.9                           # k_features_sampled: a bilinear blend, away from the texel centres
    assert n3.tobytes() == n1.tobytes()                         # ... with the normal untouched
    assert a4.tobytes() == a3.tobytes()                         # k_features_normal: the same albedo
    assert moved[quad].all() and not moved[~quad].any()         # ... and the normal map's normal
