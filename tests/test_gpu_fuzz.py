"""Seeded random scenes: every primitive kind, material kind and light kind the path supports, mixed at random (including
degenerate, tiny and huge triangles, overlapping spheres, multi-triangle leaves, sphere-only and light-less scenes, thin-lens
cameras and varying MaxDepth), rendered and ray-cast on the GPU and compared with the oracle bit for bit.  A second family decorates
such scenes with the material features the oracle did not know when the family was written -- colour images, roughness / metallic maps, samplers, normal maps --
in forms that change nothing (a constant image of the material's own value, a flat normal map), so the oracle's render of the undecorated
scene is still the reference while the shading kernels of every texturing level run, from LDS tables and from global memory.  A third
family decorates them with random images that do change the picture, and compares with the textured oracle's render of the same
decorated scene."""
import copy
import os

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import bits, gpu_scene, oracle_render, oracle_scene, random_rays
from oracle import binding as ob
from texture_cases import FLAT

F = np.float32


def random_scene(seed, textured=False):
    """the scene of `seed`; textured: decorated by with_noop_textures (the undecorated scene is what it is without the flag)"""
    rng = np.random.RandomState(seed)
    d = ag.SceneDesc("fuzz-%d" % seed)
    mats = []
    for _ in range(rng.randint(1, 6)):
        kind = rng.choice([ag.MAT_DISNEY, ag.MAT_DISNEY, ag.MAT_DISNEY, ag.MAT_MIRROR, ag.MAT_DIFFUSE_ONLY])
        mats.append(d.add_material(kind, rng.uniform(0.05, 1.0, 3), float(rng.choice([0.0, 0.02, 0.3, 0.7, 1.0, rng.uniform()])),
                                   float(rng.choice([0.0, 1.0, rng.uniform()]))))
    n_mesh = rng.randint(0, 5)
    for mi in range(n_mesh):
        style = rng.randint(4)
        if style == 0:      # smooth patch with normals and uvs
            n = rng.randint(2, 14)
            v, nn, t, idx = ag.scenes.heightfield(n, S=float(rng.uniform(0.5, 2.5)))
            v = v + rng.uniform(-1, 1, 3).astype(np.float32)
        elif style == 1:    # triangle soup without normals, sizes over six orders of magnitude, some degenerate
            k = rng.randint(1, 60)
            c = rng.uniform(-2, 2, (k, 1, 3))
            size = 10.0 ** rng.uniform(-4, 1, (k, 1, 1))
            v = (c + rng.normal(size=(k, 3, 3)) * size).astype(np.float32).reshape(-1, 3)
            deg = rng.uniform(size=k) < 0.1
            v.reshape(k, 3, 3)[deg, 2] = v.reshape(k, 3, 3)[deg, 1]     # two equal vertices
            nn, t = None, None
            idx = np.stack([np.arange(3 * k, dtype=np.int32)] * 3, 1)
        elif style == 2:    # blob with shared vertices
            v, nn, t, idx = ag.scenes.blob_mesh(rng.randint(4, 12), rng.randint(3, 10), center=tuple(rng.uniform(-1.5, 1.5, 3)),
                                                radius=float(rng.uniform(0.2, 1.2)), seed=int(rng.randint(1 << 30)))
        else:               # stacked triangles: one multi-triangle leaf
            k = rng.randint(2, 14)
            c = rng.randint(-8, 8, 3).astype(np.float32) / np.float32(4)
            v = []
            for _ in range(k):
                a, b, h = (rng.randint(1, 16, 3) / np.float32(8.0)).astype(np.float32)
                v += [c + np.float32([-a, -b, -h]), c + np.float32([a, -b, h]), c + np.float32([rng.choice([-a, a]), b, 0])]
            v = np.array(v, np.float32)
            nn, t = None, None
            idx = np.stack([np.arange(3 * k, dtype=np.int32)] * 3, 1)
        d.add_mesh(v, nn, t, idx, mats[rng.randint(len(mats))], int(rng.choice([1, 1, 2, 4])))
    for _ in range(rng.randint(0, 4) + (1 if n_mesh == 0 else 0)):
        d.add_sphere(rng.uniform(-2, 2, 3), float(rng.uniform(0.1, 1.2)), mats[rng.randint(len(mats))])
    if rng.uniform() < 0.12:   # a long primitive list: top-level tree + candidate words per chunk of 64
        for i in range(rng.randint(60, 150)):
            c = rng.uniform(-3, 3, 3)
            if rng.uniform() < 0.5:
                d.add_sphere(c, float(rng.uniform(0.05, 0.3)), mats[rng.randint(len(mats))])
            else:
                k = rng.randint(1, 5)
                v = (c + rng.normal(size=(k, 3, 3)) * 0.3).astype(np.float32).reshape(-1, 3)
                d.add_mesh(v, None, None, np.stack([np.arange(3 * k, dtype=np.int32)] * 3, 1), mats[rng.randint(len(mats))], 1)
    if rng.uniform() < 0.4:
        d.add_plane([float(rng.uniform(-1, 1)), float(rng.uniform(-2.5, -1)), float(rng.uniform(-1, 1))],
                    [float(rng.uniform(1, 6)), float(rng.uniform(1, 6))], mats[rng.randint(len(mats))])
    for _ in range(rng.randint(0, 3)):
        d.add_area_light(rng.uniform(-3, 3, 3) + np.array([0, 3, 0]), float(rng.uniform(0.1, 0.8)), rng.uniform(2, 40, 3))
    if rng.uniform() < 0.5:
        d.add_uniform_infinite_light(rng.uniform(0.05, 1.0, 3))
    if rng.uniform() < 0.3:
        d.add_infinite_area_light(ag.scenes.synthetic_hdr(16, 8, seed=int(rng.randint(1 << 30))))
    eye = rng.uniform(-1, 1, 3) * 2 + np.array([0, 1, -5])
    d.set_camera(eye, rng.uniform(-0.5, 0.5, 3), [0, 1, 0], float(rng.choice([1.0, 16 / 9])), float(rng.uniform(25, 70)),
                 float(rng.choice([0.0, 0.0, 0.15])))
    return with_noop_textures(d, seed) if textured else d


def mesh_only_materials(desc):
    analytic = {op[3] for op in desc.ops if op[0] in ("sphere", "plane")}
    return sorted({op[5] for op in desc.ops if op[0] == "mesh"} - analytic)


def with_noop_textures(desc, seed):
    """desc with, at random, on the materials that only meshes use: a constant colour image of the material's colour, ONE constant
    image (0, roughness, metallic) serving both parameter slots of a Disney material, a random sampler on each of those images, and a
    flat normal map at a random scale -- each proven to change nothing (test_gpu_textures, _material_maps, _texture_filter, _normal_map).
    `top` caps the features of a scene, so that the seeds spread over the texturing levels."""
    rng = np.random.RandomState(77000 + seed)
    d = copy.copy(desc)
    d.ops = list(desc.ops)
    materials = [op for op in desc.ops if op[0] == "material"]
    top = int(rng.randint(1, 5))

    def image(value):
        t = d.add_texture(np.broadcast_to(np.asarray(value, F), (int(rng.randint(1, 5)), int(rng.randint(1, 6)), 3)))
        if top >= 3 and rng.uniform() < 0.7:
            d.set_texture_sampler(t, int(rng.randint(2)), int(rng.randint(3)), int(rng.randint(3)))
        return t

    for m in mesh_only_materials(desc):
        _, kind, colour, roughness, metallic = materials[m]
        if rng.uniform() < 0.7:
            d.set_material_texture(m, image(colour))
        if top >= 2 and kind == ag.MAT_DISNEY and rng.uniform() < 0.7:
            t = image([0, roughness, metallic])
            d.set_material_param_texture(m, ag.PARAM_ROUGHNESS, t, 1)
            d.set_material_param_texture(m, ag.PARAM_METALLIC, t, 2)
        if top >= 4 and rng.uniform() < 0.7:
            d.set_material_normal_texture(m, image(FLAT[0, 0]), float(rng.choice([0.25, 1.0, 3.0, rng.uniform(0, 4)])))
    return d


def with_random_textures(desc, seed):
    """desc with, at random, on the materials that only meshes use: a random colour image, ONE random image (0, roughness, metallic)
    serving both parameter slots of a Disney material -- its texels exact 0s and 1s among random values --, a random sampler on each
    image, and a normal map of random tilts around (.5, .5, 1), a few texels exactly flat, at a random scale of either sign.  Images are
    1 to 8 texels a side with values in (.05, .95).  `top` caps the features of a scene as in with_noop_textures, from the same draw."""
    rng = np.random.RandomState(77000 + seed)
    d = copy.copy(desc)
    d.ops = list(desc.ops)
    materials = [op for op in desc.ops if op[0] == "material"]
    top = int(rng.randint(1, 5))
    rng = np.random.RandomState(88000 + seed)

    def image(texels):
        h, w = int(rng.randint(1, 9)), int(rng.randint(1, 9))
        t = d.add_texture(texels(h, w))
        if top >= 3 and rng.uniform() < 0.8:
            d.set_texture_sampler(t, int(rng.randint(2)), int(rng.randint(3)), int(rng.randint(3)))
        return t

    def colour(h, w):
        return rng.uniform(0.05, 0.95, (h, w, 3))

    def params(h, w):
        img = rng.uniform(0.05, 0.95, (h, w, 3))
        edge = rng.uniform(size=(h, w, 3))
        return np.where(edge < 0.25, 0.0, np.where(edge < 0.5, 1.0, img))

    def normal(h, w):
        img = np.stack([0.5 + rng.uniform(-0.3, 0.3, (h, w)), 0.5 + rng.uniform(-0.3, 0.3, (h, w)), rng.uniform(0.7, 0.95, (h, w))], -1)
        return np.where((rng.uniform(size=(h, w)) < 0.15)[..., None], FLAT[0, 0], img)

    for m in mesh_only_materials(desc):
        kind = materials[m][1]
        if rng.uniform() < 0.8:
            d.set_material_texture(m, image(colour))
        if top >= 2 and kind == ag.MAT_DISNEY and rng.uniform() < 0.8:
            t = image(params)
            d.set_material_param_texture(m, ag.PARAM_ROUGHNESS, t, 1)
            d.set_material_param_texture(m, ag.PARAM_METALLIC, t, 2)
        if top >= 4 and rng.uniform() < 0.8:
            d.set_material_normal_texture(m, image(normal), float(rng.choice([0.25, 1.0, 3.0, -1.0, rng.uniform(-4, 4)])))
    return d


def texturing_level(desc):
    """the level agpt_scene_commit derives (agpt_shade_kernels.h): the highest one a material needs"""
    sampled = {op[1] for op in desc.ops if op[0] == "texture_sampler" and tuple(op[2:]) != (0, 0, 0)}
    named = {op[2] for op in desc.ops if op[0] == "material_texture"} | {op[3] for op in desc.ops if op[0] == "material_param_texture"}
    if any(op[0] == "material_normal_texture" and op[2] >= 0 for op in desc.ops):
        return 4
    if sampled & named:
        return 3
    if any(op[0] == "material_param_texture" for op in desc.ops):
        return 2
    return 1 if named else 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(int(os.environ.get("AGPT_FUZZ_SEEDS", "24"))))
def test_random_scene_matches_oracle(seed):
    d = random_scene(1000 + seed)
    rng = np.random.RandomState(seed)
    W, H, spp = int(rng.choice([24, 40, 64])), int(rng.choice([24, 36])), int(rng.choice([1, 3]))
    if os.environ.get("AGPT_FUZZ_BIG"):
        W, H, spp = 8 * W, 8 * H, 4
    depth = int(rng.choice([0, 1, 2, 5, 5, 8]))
    g = gpu_scene(d)
    o = oracle_scene(d, depth)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        oacc, ost = o.render(W, H, spp, seed_base=seed, rng_mode=ob.RNG_PER_SAMPLE, threads=8)
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    pt = ag.PathTracer(depth)
    gacc, gst = pt.render_to_host(g, W, H, spp, seed_base=seed)
    gcnt, gcst = pt.render_to_host(g, W, H, spp, seed_base=seed, counters=True)
    assert gacc.tobytes() == gcnt.tobytes()
    assert np.array_equal(gacc[..., :3].view(np.uint32), oacc[..., :3].view(np.uint32)), d.name
    assert (gst.closest_rays, gst.anyhit_rays, gst.outliers) == (ost.closest_rays, ost.anyhit_rays, ost.outliers)
    assert (gcst.interior_visits, gcst.tri_tests) == (ost.interior_visits, ost.tri_tests)
    if any(op[0] == "mesh" for op in d.ops):
        rays = random_rays(d, 4000, seed=seed)
        gh, _ = g.Intersect(rays)
        oh, _ = o.intersect(rays, any_hit=False)
        m = oh["hit"] == 1
        assert np.array_equal(gh["hit"], oh["hit"]) and np.array_equal(gh["prim"], oh["prim"]) and np.array_equal(gh["tri"], oh["tri"])
        assert np.array_equal(bits(gh["t"][m]), bits(oh["t"][m]))
        gp, _ = g.IntersectP(rays)
        op_, _ = o.intersect(rays, any_hit=True)
        assert np.array_equal(gp["hit"], op_["hit"])
    g.close()


# ---- the same, decorated with material features that change nothing ----------------------------------------------------------------
# seeds of random_scene chosen on the CPU (test_textured_seeds_cover_levels_placements_and_env): a mesh-only material in each, the
# texturing levels 1 .. 4 twice, once with and once without an environment map
TEXTURED_SEEDS = [2001, 2029, 2006, 2021, 2011, 2028, 2049, 2027]


def textured_case(seed):
    """(decorated scene, plain scene, W, H, spp, depth, whether AGPT_SHADE_GLOBAL_TABLES is set, the variant the render must report)"""
    plain, d = random_scene(seed), random_scene(seed, textured=True)
    rng = np.random.RandomState(seed)
    W, H, spp = int(rng.choice([24, 40, 64])), int(rng.choice([24, 36])), int(rng.choice([1, 3]))
    depth = int(rng.choice([1, 2, 5, 5, 8]))
    knob = bool(rng.uniform() < 0.5)
    assert d.n_prims <= 256 and d.n_materials <= 128 and d.n_lights <= 64      # (below the limits: the knob alone decides the placement)
    variant = (texturing_level(d), 0, int(not knob), int(any(op[0] == "env_light" for op in d.ops)))
    return d, plain, W, H, spp, depth, knob, variant


def varied_case(seed):
    """textured_case with with_random_textures in place of with_noop_textures: (decorated scene, W, H, spp, depth, knob, variant)"""
    _, plain, W, H, spp, depth, knob, _ = textured_case(seed)
    d = with_random_textures(plain, seed)
    variant = (texturing_level(d), 0, int(not knob), int(any(op[0] == "env_light" for op in d.ops)))
    return d, W, H, spp, depth, knob, variant


def slot_counters(desc):
    """the census counters (oracle.binding.CENSUS_NAMES) whose slot some material of desc has filled"""
    out = set()
    for op in desc.ops:
        if op[0] == "material_texture" and op[2] >= 0:
            out.add("lookup_colour")
        elif op[0] == "material_param_texture" and op[3] >= 0:
            out.add("lookup_roughness" if op[2] == ag.PARAM_ROUGHNESS else "lookup_metallic")
        elif op[0] == "material_normal_texture" and op[2] >= 0:
            out.add("lookup_normal")
    return sorted(out)


def test_varied_seeds_cover_levels_placements_and_env():
    """on the CPU, for the family with images that vary: the same spread as the no-op family's, and per seed the textured oracle's
    census -- every kind of slot the decoration fills is looked up along the seed's paths"""
    variants = []
    for seed in TEXTURED_SEEDS:
        d, W, H, spp, depth, knob, variant = varied_case(seed)
        plain = random_scene(seed)
        kinds = [op[0] for op in d.ops]       # the plain scene's calls, then texture calls alone
        assert kinds[:len(plain.ops)] == [op[0] for op in plain.ops] and d.n_textures >= 1
        assert set(kinds[len(plain.ops):]) <= {"texture", "material_texture", "material_param_texture", "material_normal_texture", "texture_sampler"}
        for op in d.ops:
            if op[0] == "texture":
                assert 1 <= op[1].shape[0] <= 8 and 1 <= op[1].shape[1] <= 8
        oracle_render(d, W, H, spp, depth, seed_base=seed)
        census = ob.census()
        print("varied fuzz %d: variant (level, fast, lds, env) = %s, census %s" % (seed, variant, census))
        for name in slot_counters(d):
            assert census[name] > 0, (seed, name)
        assert slot_counters(d)
        variants.append(variant)
    assert len({v[0] for v in variants}) >= 3
    assert {v[2] for v in variants} == {0, 1}
    assert any(v[3] for v in variants)


def test_textured_seeds_cover_levels_placements_and_env():
    """on the CPU: what the eight cases will run (each asserts on the GPU that it does)"""
    variants = []
    for seed in TEXTURED_SEEDS:
        d, plain, *_, variant = textured_case(seed)
        assert any(op[0] == "mesh" for op in plain.ops) and mesh_only_materials(plain) and d.n_textures >= 1
        kinds = [op[0] for op in d.ops]       # the plain scene's calls, then texture calls alone
        assert kinds[:len(plain.ops)] == [op[0] for op in plain.ops]
        assert set(kinds[len(plain.ops):]) <= {"texture", "material_texture", "material_param_texture", "material_normal_texture", "texture_sampler"}
        variants.append(variant)
    print("textured fuzz variants (level, fast, lds, env):", variants)
    assert len({v[0] for v in variants}) >= 3
    assert {v[2] for v in variants} == {0, 1}
    assert any(v[3] for v in variants)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", TEXTURED_SEEDS)
def test_random_textured_scene_matches_oracle(seed, monkeypatch):
    d, plain, W, H, spp, depth, knob, variant = textured_case(seed)
    oacc, ost = oracle_render(plain, W, H, spp, depth, seed_base=seed)
    monkeypatch.delenv("AGPT_SHADE_GLOBAL_TABLES", raising=False)
    if knob:
        monkeypatch.setenv("AGPT_SHADE_GLOBAL_TABLES", "1")
    g = gpu_scene(d)
    try:
        print("textured fuzz %d: shade variant (level, fast, lds, env) = %s, %d textures" % (seed, g.shade_variant(), d.n_textures))
        assert g.shade_variant() == variant
        gacc, gst = ag.PathTracer(depth).render_to_host(g, W, H, spp, seed_base=seed)
    finally:
        g.close()
    assert np.array_equal(bits(gacc[..., :3]), bits(oacc[..., :3])), d.name
    assert (gst.closest_rays, gst.anyhit_rays, gst.outliers, gst.shaded_vertices) == (ost.closest_rays, ost.anyhit_rays, ost.outliers, ost.shaded_vertices)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", TEXTURED_SEEDS)
def test_random_varied_textured_scene_matches_oracle(seed, monkeypatch):
    """images that vary inside triangles: the textured oracle renders the same decorated scene"""
    d, W, H, spp, depth, knob, variant = varied_case(seed)
    oacc, ost = oracle_render(d, W, H, spp, depth, seed_base=seed)
    monkeypatch.delenv("AGPT_SHADE_GLOBAL_TABLES", raising=False)
    if knob:
        monkeypatch.setenv("AGPT_SHADE_GLOBAL_TABLES", "1")
    g = gpu_scene(d)
    try:
        print("varied fuzz %d: shade variant (level, fast, lds, env) = %s, %d textures" % (seed, g.shade_variant(), d.n_textures))
        assert g.shade_variant() == variant
        gacc, gst = ag.PathTracer(depth).render_to_host(g, W, H, spp, seed_base=seed)
    finally:
        g.close()
    same = (bits(gacc[..., :3]) == bits(oacc[..., :3])).all(-1)
    print("varied fuzz %d: %d of %d pixels bit-identical" % (seed, same.sum(), same.size))
    assert same.all(), d.name
    assert (gst.closest_rays, gst.anyhit_rays, gst.outliers, gst.shaded_vertices) == (ost.closest_rays, ost.anyhit_rays, ost.outliers, ost.shaded_vertices)
