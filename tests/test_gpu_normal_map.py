"""Tangent-space normal maps on the GPU (agpt_scene_set_material_normal_texture).  The tests below go back to when the CPU
oracle knew neither textures nor normal maps (whole textured paths against it: test_gpu_textured_paths.py); every test is built so that
the untextured oracle is still the yardstick: the perturbation alone against the numpy model (tests/normal_map_model.py)
bit for bit, a flat map against no map, the first-hit normal against the model fed the oracle's hits, and invariance of the render."""
import functools
import re
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import denoise_model as dm
import normal_map_model as nm
import texture_filter_model as fm
import texture_model as tm
from denoise_features import host_features, primitive_table
from helpers import bits, build_cpp_example, close_fraction, compare_with_model, gpu_context, gpu_scene, oracle_scene, render
from oracle import binding as ob
from texture_cases import FLAT, varying_lights_and_camera, varying_mesh

F = np.float32
BILINEAR, NEAREST = ag.FILTER_BILINEAR, ag.FILTER_NEAREST
KINDS = {"disney": ag.MAT_DISNEY, "mirror": ag.MAT_MIRROR, "diffuse": ag.MAT_DIFFUSE_ONLY}


# ---- 1. the perturbation alone ---------------------------------------------------------------------------------------------
def kat_items():
    rng = np.random.RandomState(7)
    n = 4096
    ns = rng.normal(size=(n, 3))
    ns = (ns / np.linalg.norm(ns, axis=1, keepdims=True)).astype(F)
    ss = rng.normal(size=(n, 3))                    # deliberately not orthogonal to ns (as for an interpolated normal)
    ss = (ss / np.linalg.norm(ss, axis=1, keepdims=True)).astype(F)
    rgb = rng.uniform(0, 1, (n, 3)).astype(F)
    z, x = [0, 0, 1], [1, 0, 0]
    edge = [(z, x, [.5, .5, 1]),                    # the flat texel
            ([-0.0, .6, .8], x, [.5, .5, 1]),       # ... on a normal with a -0 component: untouched, sign included
            ([-0.0, .6, .8], x, [.25, .75, .9]),
            (z, x, [0, 0, 0]),
            (z, x, [.5, .5, .5]),                   # m cancels to zero
            ([0, 0, 1], [0, 0, 1], [1, .5, 0]),     # ... through ss = ns: ss * tx + ns * tz = 0 at scale 1
            (z, x, [np.inf, .5, 1]), (z, x, [.5, -np.inf, 1]), (z, x, [.5, .5, np.inf]), (z, x, [np.nan, .5, 1]), (z, x, [.5, .5, np.nan]),
            (z, x, [.5, .5, 0]),                    # straight down: tz < 0 is not the no-op case
            (z, x, [1e30, .5, 1])]                  # sqrlen(m) overflows
    e = np.array(edge, F)
    return np.concatenate([ns, e[:, 0]]), np.concatenate([ss, e[:, 1]]), np.concatenate([rgb, e[:, 2]])


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 0.25, 3.0])
def test_kat_is_the_model_bit_for_bit(scale):
    ns, ss, rgb = kat_items()
    want = nm.perturb(ns, ss, rgb, scale)
    got = gpu_context().kat_normal_map(ns, ss, rgb, scale)
    same = (bits(got) == bits(want)).all(-1)
    print("normal-map KAT scale %g: %d of %d items bit-identical; %d of them untouched" % (
        scale, same.sum(), same.size, (bits(want) == bits(ns)).all(-1).sum()))
    assert same.all()
    assert (bits(want) != bits(ns)).any(-1).mean() > 0.99      # the random items are all perturbed


# ---- shared scenes -----------------------------------------------------------------------------------------------------------
def varying_scene(kind="disney", normal=None, with_normals=True):
    """the varying mesh with one material of `kind`, a gold sphere beside it (its material has no map) and two lights; normal: None or
    (image, filter, wrap_u, wrap_v, scale)"""
    d = ag.SceneDesc("varying-normal")
    m = d.add_material(KINDS[kind], [.5, .5, .5], .7, .2)
    gold = d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], .5, 1.)
    d.add_mesh(*varying_mesh(with_normals), m, 1)
    d.add_sphere([0.9, 1.0, 0.2], 0.35, gold)
    if normal is not None:
        image, filter, wu, wv, scale = normal
        t = d.add_texture(image)
        d.set_texture_sampler(t, filter, wu, wv)
        d.set_material_normal_texture(m, t, scale)
    return varying_lights_and_camera(d)


# ---- 2. a flat map is no map -----------------------------------------------------------------------------------------------
W2 = H2 = 64
SPP2 = 2
N_LI = 1000


@functools.lru_cache(None)
def plain_references(kind):
    """the scene without a map: the oracle's render and Li values, the GPU's own FAST render (FAST is compared with FAST) and features"""
    plain = varying_scene(kind)
    o = oracle_scene(plain, 5)
    rng = np.random.RandomState(11)
    rays, states = np.zeros(N_LI, ag.RAY_DTYPE), np.zeros(N_LI, np.uint32)
    for i in range(N_LI):
        rays[i], states[i] = o.camera_ray(float(rng.uniform()), float(rng.uniform()), rng=int(rng.randint(1, 2 ** 31 - 1)))
    li, after = np.zeros((N_LI, 3), F), np.zeros(N_LI, np.uint32)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        oacc, ost = o.render(W2, H2, SPP2, rng_mode=ob.RNG_PER_SAMPLE, threads=8)
        for i in range(N_LI):
            li[i], after[i], _ = o.li(rays[i], int(states[i]))
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    g = gpu_scene(plain)
    try:
        fast, fst = render(g, W2, H2, SPP2, arith="fast")
        g.set_shading_arith("exact")
        features = ag.PathTracer(5).render_features_to_host(g, W2, H2)
    finally:
        g.close()
    return dict(oacc=oacc, ost=ost, rays=rays, states=states, li=li, after=after, fast=fast, fst=fst, features=features)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("filter", [NEAREST, BILINEAR])
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_flat_map_equals_no_map(kind, filter, scale):
    ref = plain_references(kind)
    g = gpu_scene(varying_scene(kind, (FLAT, filter, ag.WRAP_REPEAT, ag.WRAP_MIRROR, scale)))
    try:
        acc, st = render(g, W2, H2, SPP2)
        fast, fst = render(g, W2, H2, SPP2, arith="fast")
        g.set_shading_arith("exact")
        li, after, _ = ag.PathTracer(5).Li(g, ref["rays"], ref["states"])
        albedo, nd = ag.PathTracer(5).render_features_to_host(g, W2, H2)
    finally:
        g.close()
    same = (bits(acc[..., :3]) == bits(ref["oacc"][..., :3])).all(-1)
    print("flat map %s filter %d scale %g: %d of %d pixels equal the oracle's plain render" % (kind, filter, scale, same.sum(), same.size))
    assert same.all()
    for name in ("closest_rays", "anyhit_rays", "shaded_vertices", "samples"):
        assert getattr(st, name) == getattr(ref["ost"], name), name
    assert np.array_equal(bits(fast), bits(ref["fast"]))
    for name in ("closest_rays", "anyhit_rays", "shaded_vertices", "samples"):
        assert getattr(fst, name) == getattr(ref["fst"], name), ("fast", name)
    assert np.array_equal(bits(li), bits(ref["li"])) and np.array_equal(after, ref["after"])
    assert albedo.tobytes() == ref["features"][0].tobytes() and nd.tobytes() == ref["features"][1].tobytes()


# ---- 3. first-hit normal = the model -----------------------------------------------------------------------------------------
def tilt_image(w, h, seed, max_deg=40.0):
    """texels that tilt up to max_deg from +z in every direction: rgb = n / 2 + 1 / 2"""
    rng = np.random.RandomState(seed)
    theta, phi = np.radians(rng.uniform(0, max_deg, (h, w))), rng.uniform(0, 2 * np.pi, (h, w))
    n = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)
    return (0.5 * n + 0.5).astype(F)


IMAGES = {"16x16": tilt_image(16, 16, 21), "5x3": tilt_image(5, 3, 22)}
SAMPLERS = {"bilinear": (BILINEAR, ag.WRAP_MIRROR, ag.WRAP_CLAMP), "nearest": (NEAREST, ag.WRAP_REPEAT, ag.WRAP_REPEAT)}
FIRST_HIT_CASES = [(i, s, scale) for i in IMAGES for s in SAMPLERS for scale in (1.0, 0.5)]


@functools.lru_cache(None)
def first_hits(W, H):
    """the oracle's pixel-centre hits on the varying mesh (the same with and without vertex normals: hits are geometry), and per mesh-hit
    pixel the model's uv and the hit triangle's tangent: u, v [H, W], ss [H, W, 3], mask, host normal_depth, host albedo"""
    plain = varying_scene()
    albedo, nd, _, hits = host_features(plain, W, H)
    prims, _ = primitive_table(plain)
    mesh = varying_mesh()
    u, v, mask, ss = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), bool), np.zeros((H, W, 3), F)
    cache = {}
    for y in range(H):
        for x in range(W):
            h = hits[y, x]
            if not h["hit"] or prims[h["prim"]][0][0] != "mesh":
                continue
            uvs, idx, tri = mesh[2], mesh[3], int(h["tri"])
            uv0, uv1, uv2 = (uvs[idx[tri + k, 2]] for k in range(3))
            u[H - 1 - y, x], v[H - 1 - y, x] = tm.interpolate_uv(uv0, uv1, uv2, h["b1"], h["b2"])
            if tri not in cache:
                cache[tri] = nm.triangle_ss(mesh, tri)
            ss[H - 1 - y, x] = cache[tri]
            mask[H - 1 - y, x] = True
    return u, v, ss, mask, nd, albedo


def expected_first_hit_normal(ns_plain, image, sampler, scale, W=64, H=64):
    u, v, ss, mask, _, _ = first_hits(W, H)
    tex = IMAGES[image]
    want = nm.perturb(ns_plain, ss, fm.value(tex, u, v, *SAMPLERS[sampler]), scale)
    skip = mask & (fm.floor_flip_distance(tex, u, v) < 1e-5)
    return want, mask, skip


def test_first_hit_construction_on_the_cpu():
    """oracle and model alone: at most 0.5 % of more than 1500 hit pixels are skipped, and the maps move the normal nearly everywhere"""
    u, v, ss, mask, nd, _ = first_hits(64, 64)
    assert np.allclose(np.linalg.norm(ss[mask], axis=-1), 1, atol=1e-6)
    for image, sampler, scale in FIRST_HIT_CASES:
        want, mask, skip = expected_first_hit_normal(nd[..., :3], image, sampler, scale)
        check = mask & ~skip
        moved = (bits(want) != bits(nd[..., :3])).any(-1)[check].mean()
        tilt = np.degrees(np.arccos(np.clip((want * nd[..., :3]).sum(-1)[check], -1, 1)))
        print("%s %s %g: hit pixels %d, skipped %d, moved %.1f %%, tilt up to %.1f deg" % (image, sampler, scale, mask.sum(), skip.sum(), 100 * moved, tilt.max()))
        assert mask.sum() > 1500 and skip.sum() <= 0.005 * mask.sum()
        assert moved > 0.95


@pytest.mark.gpu
@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("image,sampler,scale", FIRST_HIT_CASES)
def test_first_hit_normal_is_the_model(image, sampler, scale, with_normals):
    W = H = 64
    p = gpu_scene(varying_scene(with_normals=with_normals))
    g = gpu_scene(varying_scene(normal=(IMAGES[image],) + SAMPLERS[sampler] + (scale,), with_normals=with_normals))
    try:
        albedo_p, nd_p = ag.PathTracer(5).render_features_to_host(p, W, H)
        albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
    finally:
        p.close()
        g.close()
    want, mask, skip = expected_first_hit_normal(nd_p[..., :3], image, sampler, scale, W, H)
    assert mask.sum() > 1500 and skip.sum() <= 0.005 * mask.sum()
    check = mask & ~skip
    same = (bits(nd[..., :3]) == bits(want)).all(-1)
    moved = (bits(nd[..., :3]) != bits(nd_p[..., :3])).any(-1)
    print("first-hit normal %s %s %g normals=%s: %d pixels checked, %d skipped, %d differ from the model, %d moved" % (
        image, sampler, scale, with_normals, check.sum(), skip.sum(), (check & ~same).sum(), (check & moved).sum()))
    assert same[check].all()
    assert moved[check].mean() > 0.95
    assert np.array_equal(bits(nd[..., :3])[~mask], bits(nd_p[..., :3])[~mask])       # the sphere and the misses: untouched
    assert nd[..., 3].tobytes() == nd_p[..., 3].tobytes() and albedo.tobytes() == albedo_p.tobytes()


# ---- 5. invariance -----------------------------------------------------------------------------------------------------------
def bump_image(size=16):
    """a procedural bump field as a normal map: the gradient of a product of sines, rgb = n / 2 + 1 / 2"""
    y, x = np.mgrid[0:size, 0:size]
    gx = 0.7 * np.cos(2 * np.pi * (x + .5) / size * 2) * np.sin(2 * np.pi * (y + .5) / size * 2)
    gy = 0.7 * np.sin(2 * np.pi * (x + .5) / size * 2) * np.cos(2 * np.pi * (y + .5) / size * 2)
    n = np.stack([-gx, -gy, np.ones_like(gx)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return (0.5 * n + 0.5).astype(F)


def scene_mapped_bilinear_normal(normal=True):
    """scenes.scene_mapped() -- colour, roughness and metallic images on both mesh materials -- all BILINEAR, plus a normal map on both:
    the floor's an image of its own, the blob's the metallic-roughness image again (a slot that shares its taps)"""
    d = ag.scenes.scene_mapped()
    shared = d.n_textures - 1
    own = d.add_texture(bump_image())
    for t in range(d.n_textures):
        d.set_texture_sampler(t, BILINEAR, ag.WRAP_MIRROR, ag.WRAP_REPEAT)
    if normal:
        d.set_material_normal_texture(0, own, 1.0)
        d.set_material_normal_texture(2, shared, 0.5)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_normal_mapped_render_does_not_depend_on_the_split(arith):
    from ag_pathtracer_amd import tiles
    W, H, spp = 64, 64, 4
    g = gpu_scene(scene_mapped_bilinear_normal())
    g.set_shading_arith(arith)
    ctx = g.ctx
    try:
        pt = ag.PathTracer(5)
        full, st = pt.render_to_host(g, W, H, spp)
        again, st2 = pt.render_to_host(g, W, H, spp)
        assert again.tobytes() == full.tobytes() and st2.rays == st.rays
        for spb in (1, 3):
            a, sa = pt.render_to_host(g, W, H, spp, samples_per_batch=spb)
            assert a.tobytes() == full.tobytes() and sa.rays == st.rays
        ptr = ctx.alloc(W * H * 16)
        try:
            ctx.memset(ptr, 0, W * H * 16)
            for ty in range(2):
                for tx in range(2):
                    pt.render(g, W, H, spp, ptr, tile=(tx * W // 2, ty * H // 2, W // 2, H // 2))
            assert ctx.download(ptr, (H, W, 4)).tobytes() == full.tobytes()
            bufs = []
            for r in range(2):
                ctx.memset(ptr, 0, W * H * 16)
                pt.render(g, W, H, spp, ptr, interleave=(tiles.BLOCK_ROWS, 2, r))
                bufs.append(ctx.download(ptr, (H, W, 4))[:tiles.max_local_rows(H, 2)].copy())
            assert tiles.deinterleave(bufs, W, H, 2).tobytes() == full.tobytes()
        finally:
            ctx.free(ptr)
        acc, m2, _, ast = pt.render_adaptive_to_host(g, W, H, spp, spp, 2, 0.0)
        assert (acc[..., 3] == spp).all() and acc[..., :3].tobytes() == full[..., :3].tobytes()
        # the maps are seen: the same scene without them renders another image
        p = gpu_scene(scene_mapped_bilinear_normal(False))
        try:
            p.set_shading_arith(arith)
            plain, _ = pt.render_to_host(p, W, H, spp)
        finally:
            p.close()
        share = (bits(plain[..., :3]) != bits(full[..., :3])).any(-1).mean()
        print("normal-mapped against unmapped (%s): %.1f %% of the pixels differ" % (arith, 100 * share))
        assert share > 0.3
    finally:
        g.close()


# ---- 4. whole paths against the oracle ---------------------------------------------------------------------------------------
NQ = 8
QUAD_KINDS = [(ag.MAT_DISNEY, .6, .1), (ag.MAT_MIRROR, 0., 0.), (ag.MAT_DIFFUSE_ONLY, 0., 0.)]
QUAD_KIND_OF = [0, 2, 1, 0, 2, 0, 2, 0]    # (one mirror: under the uniform sky most of what a mirror shows does not depend on its normal)
QUAD_SCALE = 1.0


def quad_texels():
    """one texel per quad: tilts of 10 .. 30 degrees from +z, each in another direction"""
    k = np.arange(NQ)
    theta, phi = np.radians(10 + 20 * ((3 * k) % NQ) / (NQ - 1)), 2 * np.pi * k / NQ + 0.3
    n = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)
    return (0.5 * n + 0.5).astype(F).reshape(1, NQ, 3)


def quad_meshes():
    """NQ flat quads (two triangles each, a mesh of its own) in a 4 x 2 arrangement that fills the frame, each tipped a little in its own direction, with its
    unit normal at all four vertices and uvs whose NEAREST lookup position lies strictly inside texel k of an NQ x 1 image (a fifth of a
    texel from its edges)"""
    rng = np.random.RandomState(17)
    out = []
    for k in range(NQ):
        c = np.array([0.62 * (-2.7 + 1.8 * (k % 4)), 0.0, -1.05 + 2.1 * (k // 4)])
        a, b = rng.uniform(-0.25, 0.25, 2)
        ex = np.array([np.cos(a), np.sin(a), 0.0])
        ez = np.array([0.0, np.sin(b), np.cos(b)])
        corners = np.array([c - .54 * ex - ez, c + .54 * ex - ez, c + .54 * ex + ez, c - .54 * ex + ez]).astype(F)
        n = np.cross(ez, ex)
        n = (n / np.linalg.norm(n)).astype(F)
        u0, u1 = (k + .7) / NQ, (k + 1.3) / NQ       # (the lookup position is u * NQ - .5: k + .2 .. k + .8)
        uv = np.array([[u0, .2], [u1, .2], [u1, .8], [u0, .8]], F)
        tris = np.array([[0, 2, 1], [0, 3, 2]], np.int32).reshape(-1)
        out.append((corners, np.broadcast_to(n, (4, 3)).copy(), uv, np.stack([tris, tris, tris], 1).astype(np.int32)))
    return out


def quad_normals(ulps=0):
    """per quad the model's perturbed normal: perturb(vertex normal, the first triangle's tangent, the quad's texel) -- what the GPU
    forms at every hit of the quad up to the last bits of the frame it rebuilds there -- optionally moved by `ulps` in every component"""
    tex = quad_texels()
    out = []
    for k, mesh in enumerate(quad_meshes()):
        n = nm.perturb(mesh[1][0], nm.triangle_ss(mesh, 0), tex[0, k], QUAD_SCALE)
        for _ in range(ulps):
            n = np.nextafter(n, F(np.inf), dtype=F)
        out.append(n)
    return out


def quad_scene(mode):
    """mode "mapped": shared materials with the plateau image as NEAREST normal map (the GPU's scene); "baked": no map, each quad's
    vertex normals replaced by quad_normals() (the oracle's scene); "baked+1": those moved by one ulp; "flat": no map, the quads as built"""
    d = ag.SceneDesc("quads-" + mode)
    mats = [d.add_material(t, [.8, .7, .6], r, m) for (t, r, m) in QUAD_KINDS]
    baked = {"baked": quad_normals(0), "baked+1": quad_normals(1)}.get(mode)
    for k, (v, n, uv, idx) in enumerate(quad_meshes()):
        if baked is not None:
            n = np.broadcast_to(baked[k], (4, 3)).copy()
        d.add_mesh(v, n, uv, idx, mats[QUAD_KIND_OF[k]], 1)
    if mode == "mapped":
        t = d.add_texture(quad_texels())
        for m in mats:
            d.set_material_normal_texture(m, t, QUAD_SCALE)
    d.add_area_light([0, 6, -1], 0.7, ag.scenes.KEY_LIGHT * F(40))
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([0.1, 4.6, -1.6], [0, 0, 0.1], [0, 1, 0], 1.0, 45.0, 0.0)
    return d


@functools.lru_cache(None)
def quad_oracle(mode, spp):
    o = oracle_scene(quad_scene(mode), 5)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        acc, _ = o.render(64, 64, spp, rng_mode=ob.RNG_PER_SAMPLE, threads=8)
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    return acc[..., :3].reshape(-1, 3)


def mean_rel(a, b):
    ma, mb = a.mean(0, dtype=np.float64), b.mean(0, dtype=np.float64)
    return np.abs(ma - mb) / np.maximum(np.abs(mb), 1e-12)


def test_quad_construction_on_the_cpu():
    """the oracle alone: one ulp on the baked normals stays inside the criteria (the reference's own sensitivity), the untilted quads fail
    them by a wide margin (the test can see the feature); the tilts are 10 .. 30 degrees and stay above every quad's plane"""
    for k, mesh in enumerate(quad_meshes()):
        uv = mesh[2]
        assert (bits(fm.value(quad_texels(), uv[:, 0], uv[:, 1], NEAREST, ag.WRAP_REPEAT, ag.WRAP_REPEAT)) == bits(quad_texels()[0, k])).all()
        assert (fm.floor_flip_distance(quad_texels(), uv[:, 0], np.full(4, 1, F)) > 0.15).all()      # (v = 1: mid-texel on the one-row axis, the u axis alone decides)
    for mesh, n in zip(quad_meshes(), quad_normals()):
        tilt = np.degrees(np.arccos(np.clip(float(np.dot(n.astype(np.float64), mesh[1][0].astype(np.float64))), -1, 1)))
        assert 9.5 < tilt < 30.5
    frac = close_fraction(quad_oracle("baked+1", 2), quad_oracle("baked", 2), 1e-3)
    rel = mean_rel(quad_oracle("baked+1", 16), quad_oracle("baked", 16))
    flat = close_fraction(quad_oracle("flat", 2), quad_oracle("baked", 2), 1e-3)
    print("oracle, baked normals moved by one ulp: %.5f of the pixels within 1e-3, mean rel %s; untilted quads: %.5f" % (frac, rel, flat))
    assert frac >= 0.99 and (rel <= 1e-3).all()
    assert flat < 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_whole_paths_match_the_oracle_on_baked_normals(arith):
    g = gpu_scene(quad_scene("mapped"))
    try:
        got2, _ = render(g, 64, 64, 2, arith=arith)
        got16, _ = render(g, 64, 64, 16, arith=arith)
    finally:
        g.close()
    frac = close_fraction(got2[..., :3].reshape(-1, 3), quad_oracle("baked", 2), 1e-3)
    rel = mean_rel(got16[..., :3].reshape(-1, 3), quad_oracle("baked", 16))
    print("normal-mapped quads (%s) against the oracle on baked normals: %.5f of the pixels within 1e-3 at 2 spp, mean rel %s at 16 spp" % (arith, frac, rel))
    assert frac >= 0.99
    assert (rel <= 1e-3).all()


# ---- 6. adaptive sampling and the denoiser ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adaptive_render_features_and_denoise_match_the_model():
    W = H = 64
    g = gpu_scene(scene_mapped_bilinear_normal())
    p = gpu_scene(scene_mapped_bilinear_normal(False))
    try:
        pt = ag.PathTracer(5)
        for rel in (0.1, 0.2, 0.05, 0.3):
            acc, m2, _, _ = pt.render_adaptive_to_host(g, W, H, 4, 32, 4, rel, abs_floor=0.01)
            if len(np.unique(acc[..., 3])) >= 3:
                break
        assert len(np.unique(acc[..., 3])) >= 3
        albedo, nd = pt.render_features_to_host(g, W, H)
        albedo_p, nd_p = pt.render_features_to_host(p, W, H)
        # the guide buffers carry the map: the normals of the mapped materials moved, the albedo and the depth did not
        moved = (bits(nd[..., :3]) != bits(nd_p[..., :3])).any(-1)
        assert moved.mean() > 0.3 and albedo.tobytes() == albedo_p.tobytes() and nd[..., 3].tobytes() == nd_p[..., 3].tobytes()
        ctx = gpu_context()
        for iterations in (1, 5):
            for demod in (False, True):
                out = ctx.denoise_to_host(acc, m2, albedo, nd, iterations, demod)
                assert (out[..., 3] == 1).all()
                compare_with_model(out, dm.denoise(acc, m2, albedo, nd, iterations, demod), "normal-mapped, iterations %d demodulate %d" % (iterations, demod))
        # ... and the filter sees it: with the unmapped scene's guide normals the result is another image
        other = ctx.denoise_to_host(acc, m2, albedo, nd_p, 5, True)
        assert (bits(other[..., :3]) != bits(out[..., :3])).any(-1).mean() > 0.1
    finally:
        g.close()
        p.close()


# ---- 7. the C++ adapter ------------------------------------------------------------------------------------------------------
def test_cpp_normal_example_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "normal_scene")


@pytest.mark.gpu
def test_cpp_normal_example_matches_python(tmp_path):
    W, H = 64, 48
    exe = build_cpp_example(tmp_path, "normal_scene")
    out_path = str(tmp_path / "out.bin")
    out = subprocess.check_output([exe, out_path, str(W), str(H)], timeout=300).decode()
    assert re.search(r"normal-mapped %dx%d samples=4" % (W, H), out), out
    raw = np.fromfile(out_path, np.uint8)
    n = W * H * 16
    acc_c, nd_c = (raw[k * n:(k + 1) * n].view(F).reshape(H, W, 4) for k in range(2))
    y, x = np.mgrid[0:8, 0:8]
    tex = np.stack([F(.5) + F(.125) * ((x % 4).astype(F) - F(1.5)), F(.5) + F(.125) * ((y % 4).astype(F) - F(1.5)),
                    np.ones((8, 8), F)], -1).astype(F)

    def scene(mapped):
        d = ag.SceneDesc("cpp-normal")
        d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], .5, 1.)
        floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], .6, 0.)
        t = d.add_texture(tex)
        d.set_texture_sampler(t, ag.FILTER_BILINEAR, ag.WRAP_REPEAT, ag.WRAP_REPEAT)
        if mapped:
            d.set_material_normal_texture(floor, t, 1.5)
        d.add_mesh(*ag.create_backdrop([0, -1, 20], [40, 20, 40], 7.5, 32), floor, 1)
        d.add_sphere([0, 0, 0], 1.0, 0)
        d.add_area_light([0, 25, -20], 1.0, [200., F(.941) * F(200), F(.914) * F(200)])
        d.add_uniform_infinite_light([.4, .45, .5])
        d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], F(W) / F(H), 45.0, 0.0)
        return d

    g, p = gpu_scene(scene(True)), gpu_scene(scene(False))
    try:
        acc, _ = ag.PathTracer(5).render_to_host(g, W, H, 4)
        _, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
        _, nd_p = ag.PathTracer(5).render_features_to_host(p, W, H)
    finally:
        g.close()
        p.close()
    assert nd_c.tobytes() == nd.tobytes() and acc_c.tobytes() == acc.tobytes()
    assert nd.tobytes() != nd_p.tobytes()      # the map is at work
