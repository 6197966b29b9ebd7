"""Texture samplers on the GPU (agpt_scene_set_texture_sampler: bilinear filtering, clamp and mirror wrap).  The tests below go back
to when the CPU oracle knew no textures (whole textured paths against it: test_gpu_textured_paths.py); as for the nearest lookup
(test_gpu_textures.py, test_gpu_material_maps.py) every test is built so that the untextured oracle is still the
yardstick: a constant image must equal no image, the blended value -- a pure fp32 function of (image, u, v) that the numpy model
(tests/texture_filter_model.py) evaluates -- handed to the oracle as a plain material must render the same bits."""
import copy
import functools
import re
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import texture_filter_model as fm
import texture_model as tm
from denoise_features import host_features, primitive_table
from helpers import bits, build_cpp_example, gpu_scene, oracle_render, render
from texture_cases import (K, KINDS, OUTSIDE, PALETTE, PARAM_TEXELS, PARAMS, check_li_against_oracle, matrix_samplers, palette_lights_and_camera, plateau,
                           plateau_meshes, plateau_values, varying_lights_and_camera, varying_mesh, without_textures)

F = np.float32
R, M = ag.PARAM_ROUGHNESS, ag.PARAM_METALLIC
BILINEAR, NEAREST = ag.FILTER_BILINEAR, ag.FILTER_NEAREST
WRAPS = {"repeat": ag.WRAP_REPEAT, "clamp": ag.WRAP_CLAMP, "mirror": ag.WRAP_MIRROR}


# ---- 1. a constant image is no image, whatever the sampler -------------------------------------------------------------------
C1 = dict(W=64, H=64, spp=3)


@functools.lru_cache(None)
def c1_references():
    """the untextured C1: the oracle's render and the GPU's own FAST render (FAST is compared with FAST)"""
    plain = ag.scenes.scene_c1()
    oacc, ost = oracle_render(plain, C1["W"], C1["H"], C1["spp"])
    g = gpu_scene(plain)
    try:
        exact, _ = render(g, C1["W"], C1["H"], C1["spp"])
        fast, fst = render(g, C1["W"], C1["H"], C1["spp"], arith="fast")
    finally:
        g.close()
    assert not np.array_equal(bits(fast), bits(exact))
    return oacc, ost.rays, fast, fst.rays


def with_constant_images(desc, slot, tw, th, wrap):
    """desc; every material that only meshes use gets tw x th BILINEAR images that hold its own constants -- slot "colour": its colour
    in the colour slot; slot "maps" (Disney only): ONE image (roughness, metallic, 0) serving both parameter slots"""
    d = copy.copy(desc)
    d.ops = list(desc.ops)
    analytic = {op[3] for op in d.ops if op[0] in ("sphere", "plane")}
    n = 0
    for m, op in enumerate([op for op in desc.ops if op[0] == "material"]):
        if m in analytic or (slot == "maps" and op[1] != ag.MAT_DISNEY):
            continue
        if slot == "colour":
            t = d.add_texture(np.broadcast_to(np.asarray(op[2], F), (th, tw, 3)))
            d.set_material_texture(m, t)
        else:
            t = d.add_texture(np.broadcast_to(np.array([op[3], op[4], 0], F), (th, tw, 3)))
            d.set_material_param_texture(m, R, t, 0)
            d.set_material_param_texture(m, M, t, 1)
        d.set_texture_sampler(t, BILINEAR, wrap, wrap)
        n += 1
    assert n >= 1
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("slot", ["colour", "maps"])
@pytest.mark.parametrize("wrap", list(WRAPS))
@pytest.mark.parametrize("size", [(1, 1), (1, 4), (5, 3)])
def test_constant_image_equals_no_image(slot, wrap, size):
    oacc, orays, fast, fast_rays = c1_references()
    g = gpu_scene(with_constant_images(ag.scenes.scene_c1(), slot, size[0], size[1], WRAPS[wrap]))
    try:
        a, sa = render(g, C1["W"], C1["H"], C1["spp"])
        fa, fsa = render(g, C1["W"], C1["H"], C1["spp"], arith="fast")
    finally:
        g.close()
    same = (bits(a[..., :3]) == bits(oacc[..., :3])).all(-1)
    print("constant %s image %s %s: %d of %d pixels equal the oracle's untextured render, rays %d / %d" % (
        slot, size, wrap, same.sum(), same.size, sa.rays, orays))
    assert same.all() and sa.rays == orays
    assert np.array_equal(bits(fa), bits(fast)) and fsa.rays == fast_rays


# ---- 2. first-hit albedo = the model ---------------------------------------------------------------------------------------
IMAGES = {"16x16": np.random.RandomState(21).uniform(0.05, 0.95, (16, 16, 3)).astype(F),
          "5x3": np.random.RandomState(22).uniform(0.05, 0.95, (3, 5, 3)).astype(F)}     # (width x height)
# (a wrap "a/b" is wrap_u = a, wrap_v = b: the axes take different modes, on the non-square image too, so that a sampler whose two
# modes were stored or read the wrong way round cannot pass)
MIXED_CASES = [("5x3", BILINEAR, "clamp/mirror"), ("5x3", BILINEAR, "mirror/repeat"), ("16x16", NEAREST, "repeat/clamp")]
FIRST_HIT_CASES = ([(i, BILINEAR, w) for i in IMAGES for w in WRAPS] + [("16x16", NEAREST, "clamp"), ("16x16", NEAREST, "mirror")] +
                   MIXED_CASES)


def wrap_pair(wrap):
    """"clamp" -> (CLAMP, CLAMP), "clamp/mirror" -> (CLAMP, MIRROR): (wrap_u, wrap_v)"""
    names = wrap.split("/")
    return WRAPS[names[0]], WRAPS[names[-1]]


def varying_scene(tex, filter, wrap_u, wrap_v):
    """test_gpu_textures.varying_scene's construction, the image with a sampler"""
    d = ag.SceneDesc("varying-filtered")
    m = d.add_material(ag.MAT_DISNEY, [.5, .5, .5], .7, .2)
    d.add_mesh(*varying_mesh(), m, 1)
    ti = d.add_texture(tex)
    d.set_material_texture(m, ti)
    d.set_texture_sampler(ti, filter, wrap_u, wrap_v)
    return varying_lights_and_camera(d)


@functools.lru_cache(None)
def first_hit_uv(W, H):
    """the oracle's pixel-centre hits on the varying scene and texture_model's uv interpolation: u[H, W], v[H, W], hit-the-mesh mask"""
    plain = without_textures(varying_scene(IMAGES["5x3"], NEAREST, 0, 0))
    _, _, _, hits = host_features(plain, W, H)
    prims, _ = primitive_table(plain)
    u, v, mask = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            h = hits[y, x]
            if not h["hit"] or prims[h["prim"]][0][0] != "mesh":
                continue
            op = prims[h["prim"]][0]
            uvs, idx, tri = op[3], op[4], h["tri"]
            uv0, uv1, uv2 = (uvs[idx[tri + k, 2]] for k in range(3))
            u[H - 1 - y, x], v[H - 1 - y, x] = tm.interpolate_uv(uv0, uv1, uv2, h["b1"], h["b2"])
            mask[H - 1 - y, x] = True
    return u, v, mask


def expected_first_hit_albedo(image, filter, wrap, W=64, H=64):
    """the model on the oracle's hits: rgb[H, W, 3], the mask of mesh hits, and the pixels within 1e-5 texels of an integer position
    (where floor, the tap choice of both filters, flips on a last-bit difference of the position)"""
    u, v, mask = first_hit_uv(W, H)
    tex = IMAGES[image]
    want = fm.value(tex, u, v, filter, *wrap_pair(wrap))
    skip = mask & (fm.floor_flip_distance(tex, u, v) < 1e-5)
    return want, mask, skip


def test_first_hit_skipped_share_on_the_cpu():
    """oracle and model alone: the uvs leave [0, 1] (u on both sides, v above), and at most 0.5 % of the hit pixels lie within 1e-5 texels of an
    integer position for either image"""
    u, v, mask = first_hit_uv(64, 64)
    assert u[mask].min() < -0.05 and u[mask].max() > 1.05 and v[mask].max() > 1.05
    for image in IMAGES:
        _, mask, skip = expected_first_hit_albedo(image, BILINEAR, "repeat")
        print("%s: hit pixels %d, skipped %d" % (image, mask.sum(), skip.sum()))
        assert mask.sum() > 1500 and skip.sum() <= 0.005 * mask.sum()
    # the wrap modes disagree on these inputs: the test below can tell them apart
    a, b, c = (expected_first_hit_albedo("16x16", BILINEAR, w)[0][mask] for w in WRAPS)
    assert (a != b).any(-1).mean() > 0.05 and (a != c).any(-1).mean() > 0.05 and (b != c).any(-1).mean() > 0.05
    # ... and the axes: with the two modes of a mixed case exchanged the model gives another image
    for image, filter, wrap in MIXED_CASES:
        wu, wv = wrap.split("/")
        a, b = (expected_first_hit_albedo(image, filter, w)[0][mask] for w in (wrap, wv + "/" + wu))
        assert (a != b).any(-1).mean() > 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("image,filter,wrap", FIRST_HIT_CASES)
def test_first_hit_albedo_is_the_model(image, filter, wrap):
    W = H = 64
    want, mask, skip = expected_first_hit_albedo(image, filter, wrap, W, H)
    assert mask.sum() > 1500 and skip.sum() <= 0.005 * mask.sum()
    g = gpu_scene(varying_scene(IMAGES[image], filter, *wrap_pair(wrap)))
    try:
        albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
    finally:
        g.close()
    assert ((albedo[..., 3] == 1) == mask).all()
    check = mask & ~skip
    same = (bits(albedo[..., :3]) == bits(want)).all(-1)
    distinct = len(np.unique(bits(albedo[..., :3])[mask], axis=0))
    print("first-hit albedo %s %s %s: %d pixels checked, %d skipped, %d differ, %d distinct values" % (
        image, filter, wrap, check.sum(), skip.sum(), (check & ~same).sum(), distinct))
    assert same[check].all()
    if filter == BILINEAR:
        assert distinct > 1000     # blends, not texels (the 16 x 16 image has 256 of those, the 5 x 3 one 15)
    assert (albedo[~mask][:, :3] == 1).all()


# ---- 3. tap selection along whole paths ------------------------------------------------------------------------------------
def test_plateau_footprints():
    """the construction, checked on the CPU with the model"""
    got = {w: plateau_values(PALETTE, WRAPS[w]) for w in WRAPS}
    for w in WRAPS:
        assert np.array_equal(got[w][:K], PALETTE)                        # inside [0, 1]: the mesh's own plateau in every mode
    for i, (j, shift) in enumerate(OUTSIDE):
        rep, cla, mir = (got[w][K + i] for w in WRAPS)
        assert np.array_equal(rep, PALETTE[j])
        assert np.array_equal(cla, PALETTE[K - 1 if shift > 0 else 0])
        assert np.array_equal(mir, PALETTE[K - 1 - j if shift % 2 else j])
        if shift % 2:
            assert len({rep.tobytes(), cla.tobytes(), mir.tobytes()}) == 3   # each mode picks another pair
    assert sum(shift % 2 for _, shift in OUTSIDE) >= 3
    # a NEAREST lookup picks the same plateau: floor of a position inside (2k, 2k + 1)
    for v, n, uv, idx in plateau_meshes():
        for w in WRAPS.values():
            assert np.array_equal(fm.value(plateau(PALETTE), uv[:, 0], uv[:, 1], NEAREST, w, w), fm.value(plateau(PALETTE), uv[:, 0], uv[:, 1], BILINEAR, w, w))


    # the stacked scenes of test_gpu_shade_matrix.py: one value per mesh (plateau_values asserts it) under every sampler they use, the
    # colour from the plateau MIRROR picks, the parameters from the one CLAMP picks
    for level in (1, 2, 3, 4):
        (cf, cw), (pf, pw) = matrix_samplers(level)
        colour, params = plateau_values(PALETTE, cw, cf), plateau_values(PARAM_TEXELS, pw, pf)[:, 1:]
        assert colour.shape == (K + len(OUTSIDE), 3) and params.shape == (K + len(OUTSIDE), 2)
        assert np.array_equal(colour[:K], PALETTE) and np.array_equal(params[:K], PARAMS)
        for i, (j, shift) in enumerate(OUTSIDE):
            assert np.array_equal(colour[K + i], PALETTE[(K - 1 - j if shift % 2 else j) if cw == ag.WRAP_MIRROR else j])
            assert np.array_equal(params[K + i], PARAMS[(K - 1 if shift > 0 else 0) if pw == ag.WRAP_CLAMP else j])
    assert {matrix_samplers(level) for level in (1, 2, 3, 4)} == {((NEAREST, ag.WRAP_REPEAT),) * 2, ((BILINEAR, ag.WRAP_MIRROR), (BILINEAR, ag.WRAP_CLAMP))}


def plateau_scene(slot, wrap, textured, filter=BILINEAR):
    """textured: shared materials that read plateau images -- slot "colour": one material per kind, all with the plateau palette as
    colour; slot "params": ONE Disney material with the parameter plateaus in g and b of one image.  Otherwise one plain material per
    mesh with the model's value (what the oracle renders)."""
    d = ag.SceneDesc("plateau-%s-%d" % (slot, wrap))
    meshes = plateau_meshes()
    if textured and slot == "colour":
        mats = [d.add_material(t, [.5, .5, .5], r, m) for (t, r, m) in KINDS]
        tex = d.add_texture(plateau(PALETTE))
        d.set_texture_sampler(tex, filter, wrap, wrap)
        for m in mats:
            d.set_material_texture(m, tex)
        for k, (v, n, uv, idx) in enumerate(meshes):
            d.add_mesh(v, n, uv, idx, mats[k % len(KINDS)], 1)
    elif textured:
        m = d.add_material(ag.MAT_DISNEY, PALETTE[3], .45, .5)
        tex = d.add_texture(plateau(np.concatenate([np.zeros((K, 1), F), PARAMS], 1)))
        d.set_texture_sampler(tex, filter, wrap, wrap)
        d.set_material_param_texture(m, R, tex, 1)
        d.set_material_param_texture(m, M, tex, 2)
        for v, n, uv, idx in meshes:
            d.add_mesh(v, n, uv, idx, m, 1)
    elif slot == "colour":
        colour = plateau_values(PALETTE, wrap)
        for k, (v, n, uv, idx) in enumerate(meshes):
            t, r, m = KINDS[k % len(KINDS)]
            d.add_mesh(v, n, uv, idx, d.add_material(t, colour[k], r, m), 1)
    else:
        params = plateau_values(PARAMS, wrap)
        for k, (v, n, uv, idx) in enumerate(meshes):
            d.add_mesh(v, n, uv, idx, d.add_material(ag.MAT_DISNEY, PALETTE[3], float(params[k, 0]), float(params[k, 1])), 1)
    return palette_lights_and_camera(d)


@pytest.mark.gpu
@pytest.mark.parametrize("slot", ["colour", "params"])
@pytest.mark.parametrize("wrap", list(WRAPS))
def test_plateau_per_mesh_equals_material_per_mesh(slot, wrap):
    W, H, spp, depth = 64, 64, 3, 5
    plain = plateau_scene(slot, WRAPS[wrap], False)
    oacc, ost = oracle_render(plain, W, H, spp, depth)
    g = gpu_scene(plateau_scene(slot, WRAPS[wrap], True))
    try:
        acc, st = ag.PathTracer(depth).render_to_host(g, W, H, spp)
        same = (bits(acc[..., :3]) == bits(oacc[..., :3])).all(-1)
        print("plateau %s %s: %d of %d pixels bit-identical, rays %d / %d" % (slot, wrap, same.sum(), same.size, st.rays, ost.rays))
        assert same.all() and st.rays == ost.rays
        assert len(np.unique(bits(acc[..., :3]).reshape(-1, 3), axis=0)) > W * H // 2
        check_li_against_oracle(g, plain, depth, 1000 if slot == "colour" else 300)
    finally:
        g.close()


# ---- 4. weights along whole paths ------------------------------------------------------------------------------------------
def corner_images():
    """per mesh two images of its own, 2 x 2 or 3 x 2 (width x height): a colour image, and (0, roughness, metallic).  The metallic
    texels are 0 or 1 with texel (0, 0) at 1 for half of the meshes: a blend of them has a diffuse lobe, that texel alone has none."""
    rng = np.random.RandomState(31)
    out = []
    for k in range(K):
        w = 2 + k % 2
        colour = rng.uniform(0.05, 0.95, (2, w, 3)).astype(F)
        params = np.zeros((2, w, 3), F)
        params[..., 1] = rng.uniform(0.05, 1.0, (2, w))
        params[..., 2] = rng.randint(0, 2, (2, w))
        params[0, 0, 2] = k % 2
        params[1, w - 1, 2] = 1 - k % 2     # (u = v = 0 under REPEAT blends the four CORNER texels: make them differ)
        out.append((colour, params))
    return out


def corner_values(wrap):
    """the model at u = v = 0: per mesh (colour, roughness, metallic)"""
    out = []
    for colour, params in corner_images():
        c = fm.value(colour, F(0), F(0), BILINEAR, wrap, wrap)
        p = fm.value(params, F(0), F(0), BILINEAR, wrap, wrap)
        out.append((c, p[1], p[2]))
    return out


def test_corner_values_are_blends_under_repeat_and_texels_otherwise():
    for k, (colour, params) in enumerate(corner_images()):
        x0, x1, y0, y1, fx, fy = fm.taps(colour, F(0), F(0), BILINEAR, ag.WRAP_REPEAT, ag.WRAP_REPEAT)
        assert (int(x0), int(x1), int(y0), int(y1), float(fx), float(fy)) == (colour.shape[1] - 1, 0, 1, 0, .5, .5)
    rep, cla, mir = (corner_values(w) for w in WRAPS.values())
    for k, (colour, params) in enumerate(corner_images()):
        for got in (cla[k], mir[k]):
            assert np.array_equal(got[0], colour[0, 0]) and got[1] == params[0, 0, 1] and got[2] == params[0, 0, 2]
        assert not (rep[k][0] == colour.reshape(-1, 3)).all(-1).any()           # no texel: a blend
        assert 0 < rep[k][2] < 1                                                # metallic texels 0 / 1 -> a blend has both lobe sets' lobes
    assert {float(c[2]) for c in cla} == {0.0, 1.0}


def corner_scene(wrap, textured):
    """K meshes whose uvs are all exactly (0, 0): the interpolated uv is exactly 0, the position -.5 on both axes, the weights 1/2"""
    d = ag.SceneDesc("corner-%d" % wrap)
    values = corner_values(wrap)
    for k, ((v, n, uv, idx), (colour, params)) in enumerate(zip(plateau_meshes()[:K], corner_images())):
        if textured:
            m = d.add_material(ag.MAT_DISNEY, [.5, .5, .5], .45, .5)
            ct, pt = d.add_texture(colour), d.add_texture(params)
            d.set_material_texture(m, ct)
            d.set_material_param_texture(m, R, pt, 1)
            d.set_material_param_texture(m, M, pt, 2)
            d.set_texture_sampler(ct, BILINEAR, wrap, wrap)
            d.set_texture_sampler(pt, BILINEAR, wrap, wrap)
        else:
            c, r, mt = values[k]
            m = d.add_material(ag.MAT_DISNEY, c, float(r), float(mt))
        d.add_mesh(v, n, np.zeros_like(uv), idx, m, 1)
    return palette_lights_and_camera(d)


@pytest.mark.gpu
@pytest.mark.parametrize("wrap", list(WRAPS))
def test_half_weights_equal_the_model_along_whole_paths(wrap):
    W, H, spp, depth = 64, 64, 3, 5
    oacc, ost = oracle_render(corner_scene(WRAPS[wrap], False), W, H, spp, depth)
    g = gpu_scene(corner_scene(WRAPS[wrap], True))
    try:
        acc, st = ag.PathTracer(depth).render_to_host(g, W, H, spp)
    finally:
        g.close()
    same = (bits(acc[..., :3]) == bits(oacc[..., :3])).all(-1)
    print("corner %s: %d of %d pixels bit-identical, rays %d / %d" % (wrap, same.sum(), same.size, st.rays, ost.rays))
    assert same.all() and st.rays == ost.rays


# ---- 5. invariance ---------------------------------------------------------------------------------------------------------
def scene_mapped_bilinear(wrap=ag.WRAP_MIRROR):
    d = ag.scenes.scene_mapped()
    for t in range(d.n_textures):
        d.set_texture_sampler(t, BILINEAR, wrap, ag.WRAP_REPEAT)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_bilinear_render_does_not_depend_on_the_split(arith):
    from ag_pathtracer_amd import tiles
    W, H, spp = 64, 64, 4
    g = gpu_scene(scene_mapped_bilinear())
    g.set_shading_arith(arith)
    ctx = g.ctx
    try:
        pt = ag.PathTracer(5)
        full, st = pt.render_to_host(g, W, H, spp)
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
        # the filter is seen: the same scene with the default samplers renders another image
        p = gpu_scene(ag.scenes.scene_mapped())
        try:
            p.set_shading_arith(arith)
            nearest, _ = pt.render_to_host(p, W, H, spp)
        finally:
            p.close()
        share = (bits(nearest[..., :3]) != bits(full[..., :3])).any(-1).mean()
        print("bilinear against nearest (%s): %.1f %% of the pixels differ" % (arith, 100 * share))
        assert share > 0.3
    finally:
        g.close()


# ---- 6. NEAREST textures in a sampled scene --------------------------------------------------------------------------------
def mixed_scene(third, bilinear):
    """Three groups of meshes: A reads a 16 x 16 colour image at varying uvs, B a parameter image, C -- plateau footprints -- the image
    `third` (1 x 2K).  A's and B's textures keep the default sampler; C's is BILINEAR (repeat, as the default) if `bilinear`, default otherwise."""
    d = ag.SceneDesc("mixed")
    rng = np.random.RandomState(41)
    ma = d.add_material(ag.MAT_DISNEY, [.5, .5, .5], .6, .1)
    d.set_material_texture(ma, d.add_texture(IMAGES["16x16"]))
    mb = d.add_material(ag.MAT_DISNEY, PALETTE[0], .45, .5)
    tb = d.add_texture(np.stack([np.zeros((4, 4), F), rng.uniform(.05, 1, (4, 4)), rng.randint(0, 2, (4, 4))], -1).astype(F))
    d.set_material_param_texture(mb, R, tb, 1)
    d.set_material_param_texture(mb, M, tb, 2)
    mc = d.add_material(ag.MAT_DISNEY, [.5, .5, .5], .8, 0.)
    tc = d.add_texture(third)
    d.set_material_texture(mc, tc)
    if bilinear:
        d.set_texture_sampler(tc, BILINEAR, ag.WRAP_REPEAT, ag.WRAP_REPEAT)     # (only the filter differs from the default)
    for k, (v, n, uv, idx) in enumerate(plateau_meshes()):
        if k % 3 == 2:
            d.add_mesh(v, n, uv, idx, mc, 1)
        else:
            d.add_mesh(v, n, rng.uniform(-1.5, 2.5, uv.shape).astype(F), idx, ma if k % 3 == 0 else mb, 1)
    return palette_lights_and_camera(d)


@pytest.mark.gpu
def test_nearest_textures_in_a_sampled_scene():
    W, H, spp = 64, 64, 3
    flat, ramp = plateau(PALETTE), np.random.RandomState(42).uniform(.05, .95, (1, 2 * K, 3)).astype(F)
    scenes = {name: gpu_scene(mixed_scene(img, bil)) for name, img, bil in (
        ("plateau_bilinear", flat, True), ("plateau_nearest", flat, False), ("ramp_bilinear", ramp, True), ("ramp_nearest", ramp, False))}
    try:
        for arith in ("exact", "fast"):
            img = {k: render(g, W, H, spp, arith=arith) for k, g in scenes.items()}
            # the plateau image: BILINEAR returns what NEAREST returns, so the sampled scene -- one tap for the two default textures, four
            # equal ones for the third -- is the all-NEAREST scene, bit for bit
            assert np.array_equal(bits(img["plateau_bilinear"][0]), bits(img["plateau_nearest"][0]))
            assert img["plateau_bilinear"][1].rays == img["plateau_nearest"][1].rays
            # ... and the filter is at work: with an image that varies between neighbours the two differ
            assert (bits(img["ramp_bilinear"][0]) != bits(img["ramp_nearest"][0])).any(-1).mean() > 0.02
        # first hits: the default textures' albedo is what it is in the unsampled scene, pixel by pixel; the third one's differs
        a, _ = ag.PathTracer(5).render_features_to_host(scenes["ramp_bilinear"], W, H)
        b, _ = ag.PathTracer(5).render_features_to_host(scenes["ramp_nearest"], W, H)
        c, _ = ag.PathTracer(5).render_features_to_host(scenes["plateau_bilinear"], W, H)
        e, _ = ag.PathTracer(5).render_features_to_host(scenes["plateau_nearest"], W, H)
        assert c.tobytes() == e.tobytes()
        third = (bits(c[..., :3]) != bits(b[..., :3])).any(-1)      # (the pixels that show group C: the two images differ everywhere)
        assert 0.02 < third.mean() < 0.6
        assert np.array_equal(bits(a)[~third], bits(b)[~third])
        assert (bits(a[..., :3]) != bits(b[..., :3])).any(-1)[third].mean() > 0.9
    finally:
        for g in scenes.values():
            g.close()


# ---- 7. the C++ adapter ----------------------------------------------------------------------------------------------------
def test_cpp_filtered_example_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "filtered_scene")


@pytest.mark.gpu
def test_cpp_filtered_example_matches_python(tmp_path):
    W, H = 64, 48
    exe = build_cpp_example(tmp_path, "filtered_scene")
    out_path = str(tmp_path / "out.bin")
    out = subprocess.check_output([exe, out_path, str(W), str(H)], timeout=300).decode()
    assert re.search(r"filtered %dx%d samples=4" % (W, H), out), out
    raw = np.fromfile(out_path, np.uint8)
    n = W * H * 16
    acc_c, albedo_c = (raw[k * n:(k + 1) * n].view(F).reshape(H, W, 4) for k in range(2))
    y, x = np.mgrid[0:8, 0:16]
    odd = ((x // 2) + (y // 2)) % 2 == 1
    shade = (F(1) - F(0.0625) * y.astype(F)).astype(F)
    tex = np.stack([np.where(odd, F(.125), F(.75)) * shade, np.where(odd, F(.25), F(.75)) * shade,
                    np.where(odd, F(.5), F(.625)) * shade], -1).astype(F)

    def scene(filtered):
        d = ag.SceneDesc("cpp-filtered")
        d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], .5, 1.)
        floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
        t = d.add_texture(tex)
        d.set_material_texture(floor, t)
        if filtered:
            d.set_texture_sampler(t, ag.FILTER_BILINEAR, ag.WRAP_MIRROR, ag.WRAP_CLAMP)
        d.add_mesh(*ag.create_backdrop([0, -1, 20], [40, 20, 40], 7.5, 32), floor, 1)
        d.add_sphere([0, 0, 0], 1.0, 0)
        d.add_area_light([0, 25, -20], 1.0, [200., F(.941) * F(200), F(.914) * F(200)])
        d.add_uniform_infinite_light([.4, .45, .5])
        d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], F(W) / F(H), 45.0, 0.0)
        return d

    g, p = gpu_scene(scene(True)), gpu_scene(scene(False))
    try:
        acc, _ = ag.PathTracer(5).render_to_host(g, W, H, 4)
        albedo, _ = ag.PathTracer(5).render_features_to_host(g, W, H)
        albedo_p, _ = ag.PathTracer(5).render_features_to_host(p, W, H)
    finally:
        g.close()
        p.close()
    assert albedo_c.tobytes() == albedo.tobytes() and acc_c.tobytes() == acc.tobytes()
    assert albedo.tobytes() != albedo_p.tobytes()      # the sampler is at work
