"""Roughness / metallic maps on the GPU (agpt_scene_set_material_param_texture).  The tests below go back to when the CPU
oracle knew no textures (whole textured paths against it: test_gpu_textured_paths.py); as for colour textures
(test_gpu_textures.py) every test is built so that the untextured oracle is still the yardstick: a map of one value must equal the plain
material, a texel per mesh must equal a material per mesh -- lobe set, alpha clamp and all -- bit for bit."""
import copy
import re
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import texture_cases as tc
import texture_model as tm
from helpers import bits, build_cpp_example, gpu_scene, oracle_render, oracle_scene, render
from oracle import binding as ob
from texture_cases import K, PALETTE, SOUP, palette_meshes, soup_excluded_pixels, without, without_textures

F = np.float32
R, M = ag.PARAM_ROUGHNESS, ag.PARAM_METALLIC


def without_maps(desc):
    """desc with its colour textures and without its roughness / metallic maps (their images stay: texture ids do not move)"""
    return without(desc, ("material_param_texture",))


def mesh_only_disney_materials(desc):
    """[(id, colour, roughness, metallic)] of the Disney materials that no sphere or plane uses (a map there is refused at commit)"""
    analytic = {op[3] for op in desc.ops if op[0] in ("sphere", "plane")}
    mats = [op for op in desc.ops if op[0] == "material"]
    return [(m, op[2], op[3], op[4]) for m, op in enumerate(mats) if op[1] == ag.MAT_DISNEY and m not in analytic]


def with_constant_maps(desc, tw, th, constant_colour_too=False):
    """desc; every Disney material that only meshes use gets a tw x th image filled with (its roughness, its metallic, 0) as both of
    its maps (constant_colour_too: and one filled with its colour as its colour texture)"""
    d = copy.copy(desc)
    d.ops = list(desc.ops)
    todo = mesh_only_disney_materials(d)
    assert todo
    for m, c, r, mt in todo:
        image = d.add_texture(np.broadcast_to(np.array([r, mt, 0], F), (th, tw, 3)))
        d.set_material_param_texture(m, R, image, 0)
        d.set_material_param_texture(m, M, image, 1)
        if constant_colour_too:
            d.set_material_texture(m, d.add_texture(np.broadcast_to(np.asarray(c, F), (th, tw, 3))))
    return d


# ---- 1. a map of one value is no map ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["c1", "textured"])
@pytest.mark.parametrize("size", [(1, 1), (7, 5)])
def test_constant_map_equals_no_map(which, size):
    base = ag.scenes.scene_c1() if which == "c1" else ag.scenes.scene_textured()
    W, H, spp = 96, 64, 3
    # (a) no image left that is not constant: the oracle renders the plain scene
    plain = without_textures(base)
    const = with_constant_maps(plain, *size, constant_colour_too=(which == "textured"))
    oacc, ost = oracle_render(plain, W, H, spp)
    gp, gc = gpu_scene(plain), gpu_scene(const)
    try:
        a, sa = render(gp, W, H, spp)
        b, sb = render(gc, W, H, spp)
        same = (bits(a) == bits(b)).all(-1)
        print("constant maps %s %s: %d of %d pixels equal the unmapped render, rays %d / %d / oracle %d" % (
            which, size, same.sum(), same.size, sb.rays, sa.rays, ost.rays))
        assert same.all() and sa.rays == sb.rays
        assert np.array_equal(bits(b[..., :3]), bits(oacc[..., :3])) and sb.rays == ost.rays
        fa, fsa = render(gp, W, H, spp, arith="fast")
        fb, fsb = render(gc, W, H, spp, arith="fast")
        assert np.array_equal(bits(fa), bits(fb)) and fsa.rays == fsb.rays
        assert not np.array_equal(bits(fa), bits(a))    # (FAST is another arithmetic: the comparison above is FAST with FAST)
    finally:
        gp.close()
        gc.close()
    if which != "textured":
        return
    # (b) the scene's own colour images stay: constant maps beside varying colour texels, GPU against GPU
    gp, gc = gpu_scene(base), gpu_scene(with_constant_maps(base, *size))
    try:
        for arith in ("exact", "fast"):
            a, sa = render(gp, W, H, spp, arith=arith)
            b, sb = render(gc, W, H, spp, arith=arith)
            assert np.array_equal(bits(a), bits(b)) and sa.rays == sb.rays
    finally:
        gp.close()
        gc.close()


# ---- 2. one texel per mesh = one material per mesh -----------------------------------------------------------------------------
# (roughness, metallic) per texel: metallic 0, 1 and .5 -- the lobe set changes per hit --, roughness 0 and .02 -- both below the
# .001 clamp of alpha = r * r --, .35 and 1
PARAMS = np.array([[1.0, 0.0], [.35, 1.0], [0.0, .5], [.02, 0.0], [.6, .5], [0.0, 1.0], [.02, 1.0], [.5, .3]], F)
CONST_COLOUR, CONST_ROUGH, CONST_METAL = PALETTE[3], F(.45), F(.5)
VARIANTS = ["all", "rough_only", "metal_only", "three_images", "swapped", "one_image"]


def test_parameter_palette_has_the_required_values():
    assert {0.0, 1.0, 0.5} <= set(PARAMS[:, 1].tolist())
    assert {F(0.0), F(.02), F(.35), F(1.0)} <= set(PARAMS[:, 0])
    assert (PARAMS[:, 0][PARAMS[:, 0] <= F(.02)] ** 2 < F(.001)).all()


def variant_values(variant):
    """per mesh k the (colour, roughness, metallic) the variant's textures and constants give it"""
    colour = np.broadcast_to(CONST_COLOUR, (K, 3)) if variant in ("rough_only", "metal_only") else PALETTE
    rough = np.full(K, CONST_ROUGH) if variant == "metal_only" else PARAMS[:, 0]
    metal = np.full(K, CONST_METAL) if variant == "rough_only" else PARAMS[:, 1]
    if variant == "one_image":     # the colour image serves all three slots: roughness = its r, metallic = its g
        rough, metal = PALETTE[:, 0], PALETTE[:, 1]
    return colour, rough, metal


def palette_scene(degenerate_uv, variant, mapped):
    """mapped: K meshes sharing ONE Disney material whose colour / roughness / metallic come from K x 1 images as `variant` says;
    otherwise one plain material per mesh with those values (what the oracle renders)"""
    d = ag.SceneDesc("palette-" + variant)
    colour, rough, metal = variant_values(variant)
    if mapped:
        m = d.add_material(ag.MAT_DISNEY, CONST_COLOUR, CONST_ROUGH, CONST_METAL)
        zero = np.zeros(K, F)
        if variant not in ("rough_only", "metal_only"):
            ctex = d.add_texture(PALETTE[None])
            d.set_material_texture(m, ctex)
        if variant in ("all", "rough_only", "metal_only"):     # roughness in g, metallic in b of one image (glTF's layout)
            image = d.add_texture(np.stack([zero, PARAMS[:, 0], PARAMS[:, 1]], -1)[None])
            if variant != "metal_only":
                d.set_material_param_texture(m, R, image, 1)
            if variant != "rough_only":
                d.set_material_param_texture(m, M, image, 2)
        elif variant == "three_images":                         # colour, roughness and metallic each from an image of its own
            d.set_material_param_texture(m, R, d.add_texture(np.stack([PARAMS[:, 0], zero, zero], -1)[None]), 0)
            d.set_material_param_texture(m, M, d.add_texture(np.stack([zero, zero, PARAMS[:, 1]], -1)[None]), 2)
        elif variant == "swapped":                              # the two parameters swapped between the channels
            image = d.add_texture(np.stack([zero, PARAMS[:, 1], PARAMS[:, 0]], -1)[None])
            d.set_material_param_texture(m, R, image, 2)
            d.set_material_param_texture(m, M, image, 1)
        else:                                                    # one_image
            d.set_material_param_texture(m, R, ctex, 0)
            d.set_material_param_texture(m, M, ctex, 1)
        return tc.palette_scene(d, palette_meshes(degenerate_uv), lambda k: m)
    return tc.palette_scene(d, palette_meshes(degenerate_uv),
                            lambda k: d.add_material(ag.MAT_DISNEY, colour[k], float(rough[k]), float(metal[k])))


def test_palette_footprints():
    """the construction, checked on the CPU with the model: every vertex uv of mesh k reads texel k, at least 0.05 of a texel from
    its ends"""
    for degenerate in (False, True):
        for k, (v, n, uv, idx) in enumerate(palette_meshes(degenerate)):
            x, y = tm.texel_index((1, K), uv[:, 0], uv[:, 1])
            assert (x == k).all() and (y == 0).all()
            pos, _ = tm.texel_position((1, K), uv[:, 0], uv[:, 1])
            assert (pos - np.floor(pos) > 0.05).all() and (pos - np.floor(pos) < 0.95).all()


def test_variants_describe_what_they_say():
    for variant in VARIANTS:
        ops = palette_scene(False, variant, True).ops
        slots = sorted(op[2] for op in ops if op[0] == "material_param_texture")
        assert slots == {"rough_only": [R], "metal_only": [M]}.get(variant, [R, M])
        assert sum(op[0] == "material" for op in ops) == 1
        assert sum(op[0] == "material" for op in palette_scene(False, variant, False).ops) == K


def check_against_per_mesh_oracle(degenerate_uv, variant, with_li):
    tex_desc, plain_desc = palette_scene(degenerate_uv, variant, True), palette_scene(degenerate_uv, variant, False)
    W, H, spp, depth = 64, 64, 3, 5
    oacc, ost = oracle_render(plain_desc, W, H, spp, depth)
    g = gpu_scene(tex_desc)
    try:
        acc, st = ag.PathTracer(depth).render_to_host(g, W, H, spp)
        same = (bits(acc[..., :3]) == bits(oacc[..., :3])).all(-1)
        print("palette %s (degenerate uv %s): %d of %d pixels bit-identical, rays %d / %d" % (
            variant, degenerate_uv, same.sum(), same.size, st.rays, ost.rays))
        assert same.all() and st.rays == ost.rays
        assert len(np.unique(bits(acc[..., :3]).reshape(-1, 3), axis=0)) > W * H // 2
        if not with_li:
            return
        # Li on camera rays, same streams
        o = oracle_scene(plain_desc, depth)
        n = 1000
        rng = np.random.RandomState(11)
        rays, states = np.zeros(n, ag.RAY_DTYPE), np.zeros(n, np.uint32)
        for i in range(n):
            rays[i], states[i] = o.camera_ray(float(rng.uniform()), float(rng.uniform()), rng=int(rng.randint(1, 2 ** 31 - 1)))
        want, after = np.zeros((n, 3), F), np.zeros(n, np.uint32)
        ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
        try:
            for i in range(n):
                want[i], after[i], _ = o.li(rays[i], int(states[i]))
        finally:
            ob.set_trig_mode(ob.TRIG_LIBM)
        got, got_after, _ = ag.PathTracer(depth).Li(g, rays, states)
        print("palette %s: %d of %d Li values bit-identical, %d RNG end states" % (
            variant, (bits(got) == bits(want)).all(-1).sum(), n, (got_after == after).sum()))
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(got_after, after)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("degenerate_uv", [False, True])
def test_one_texel_per_mesh_equals_one_material_per_mesh(degenerate_uv):
    check_against_per_mesh_oracle(degenerate_uv, "all", with_li=True)


# ---- 3. the slots are independent -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS[1:])
def test_slots_are_independent(variant):
    check_against_per_mesh_oracle(False, variant, with_li=False)


# ---- 4. variation inside one mesh, whole paths ----------------------------------------------------------------------------
def soup_scene(mode):
    """mode "mapped": the single mesh, roughness and metallic per triangle through the parameter palette; "single" / "grouped": the
    single mesh / the triangles regrouped into K meshes by texel, all with ONE material; "grouped_params": regrouped with K plain
    materials"""
    def material(d, k):
        r, mt = (float(PARAMS[k, 0]), float(PARAMS[k, 1])) if mode == "grouped_params" else (0.5, 0.3)
        m = d.add_material(ag.MAT_DISNEY, PALETTE[0], r, mt)
        if mode == "mapped":
            image = d.add_texture(np.stack([np.zeros(K, F), PARAMS[:, 0], PARAMS[:, 1]], -1)[None])
            d.set_material_param_texture(m, R, image, 1)
            d.set_material_param_texture(m, M, image, 2)
        return m

    return tc.soup_scene("soup-" + mode, material, grouped=mode.startswith("grouped"))


def test_regrouping_changes_few_pixels_for_the_oracle():
    """the reference alone: one mesh against the same triangles regrouped into K meshes (other BVHs), both with one material -- the
    pixels test_parameters_per_triangle_match_regrouped_oracle leaves out.  At most 1 %."""
    ex = soup_excluded_pixels()
    print("regrouped oracle render differs in %d of %d pixels" % (ex.sum(), ex.size))
    assert ex.sum() <= 0.01 * ex.size


@pytest.mark.gpu
def test_parameters_per_triangle_match_regrouped_oracle():
    """One mesh, roughness and metallic per triangle through the parameter palette, against the oracle rendering the triangles
    regrouped by texel with K plain materials.  Pixels where the oracle itself renders the one-material single mesh and the
    one-material regrouped meshes differently (a grazing hit decided differently by the two trees) are excluded."""
    ex = soup_excluded_pixels()
    assert ex.sum() <= 0.01 * ex.size
    want, _ = oracle_render(soup_scene("grouped_params"), SOUP["W"], SOUP["H"], SOUP["spp"], SOUP["depth"])
    g = gpu_scene(soup_scene("mapped"))
    try:
        acc, _ = ag.PathTracer(SOUP["depth"]).render_to_host(g, SOUP["W"], SOUP["H"], SOUP["spp"])
    finally:
        g.close()
    same = (bits(acc[..., :3]) == bits(want[..., :3])).all(-1)
    print("parameters per triangle: %d excluded, %d of the remaining %d pixels differ" % (ex.sum(), (~same & ~ex).sum(), (~ex).sum()))
    assert same[~ex].all()


# ---- 5. the feature buffers do not see the maps ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_features_are_untouched():
    W, H = 96, 64
    d = ag.scenes.scene_mapped()
    g, p = gpu_scene(d), gpu_scene(without_maps(d))
    try:
        albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
        albedo_p, nd_p = ag.PathTracer(5).render_features_to_host(p, W, H)
    finally:
        g.close()
        p.close()
    assert albedo.tobytes() == albedo_p.tobytes() and nd.tobytes() == nd_p.tobytes()
    assert len(np.unique(bits(albedo[..., :3])[albedo[..., 3] == 1], axis=0)) > 20      # (the colour texels are there)
    # ... also where the material has maps and no colour texture: the albedo is its constant colour
    d = palette_scene(False, "rough_only", True)
    g, p = gpu_scene(d), gpu_scene(without_textures(d))
    try:
        albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
        albedo_p, nd_p = ag.PathTracer(5).render_features_to_host(p, W, H)
    finally:
        g.close()
        p.close()
    assert albedo.tobytes() == albedo_p.tobytes() and nd.tobytes() == nd_p.tobytes()


# ---- 6. invariance -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_mapped_render_does_not_depend_on_the_split(arith):
    from ag_pathtracer_amd import tiles
    W, H, spp = 80, 64, 4
    g = gpu_scene(ag.scenes.scene_mapped())
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
        # agpt_render_adaptive with the stop test off = agpt_render at the pixel's count
        acc, m2, _, ast = pt.render_adaptive_to_host(g, W, H, spp, spp, 2, 0.0)
        assert (acc[..., 3] == spp).all() and acc[..., :3].tobytes() == full[..., :3].tobytes()
        # the maps are seen: the scene without them renders another image
        p = gpu_scene(without_maps(ag.scenes.scene_mapped()))
        try:
            p.set_shading_arith(arith)
            unmapped, _ = pt.render_to_host(p, W, H, spp)
        finally:
            p.close()
        share = (bits(unmapped[..., :3]) != bits(full[..., :3])).any(-1).mean()
        print("mapped against unmapped (%s): %.1f %% of the pixels differ" % (arith, 100 * share))
        assert share > 0.3
    finally:
        g.close()


# ---- 7. FAST --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("degenerate_uv", [False, True])
def test_fast_mapped_equals_fast_per_mesh_materials(degenerate_uv):
    """FAST against FAST on the GPU (the oracle is exact arithmetic): the maps decide what is read, not how it is multiplied"""
    W, H, spp, depth = 64, 64, 3, 5
    g, p = gpu_scene(palette_scene(degenerate_uv, "all", True)), gpu_scene(palette_scene(degenerate_uv, "all", False))
    try:
        exact, _ = render(g, W, H, spp, depth)
        fm, sm = render(g, W, H, spp, depth, arith="fast")
        fp, sp = render(p, W, H, spp, depth, arith="fast")
        same = (bits(fm) == bits(fp)).all(-1)
        print("FAST palette: %d of %d pixels bit-identical, rays %d / %d" % (same.sum(), same.size, sm.rays, sp.rays))
        assert same.all() and sm.rays == sp.rays
        assert not np.array_equal(bits(fm), bits(exact))
    finally:
        g.close()
        p.close()


# ---- 8. the C++ adapter ---------------------------------------------------------------------------------------------------
def test_cpp_mapped_example_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "mapped_scene")


@pytest.mark.gpu
def test_cpp_mapped_example_matches_python(tmp_path):
    W, H = 96, 64
    exe = build_cpp_example(tmp_path, "mapped_scene")
    out_path = str(tmp_path / "out.bin")
    out = subprocess.check_output([exe, out_path, str(W), str(H)], timeout=300).decode()
    assert re.search(r"mapped %dx%d samples=4" % (W, H), out), out
    acc_c = np.fromfile(out_path, F).reshape(H, W, 4)
    y, x = np.mgrid[0:8, 0:16]
    metal = ((x // 2) + (y // 2)) % 2 == 1
    rough = (np.where(metal, F(.5), F(1)) - F(0.0625) * y.astype(F)).astype(F)
    image = np.stack([np.zeros_like(rough), rough, metal.astype(F)], -1).astype(F)
    d = ag.SceneDesc("cpp-mapped")
    d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], .5, 1.)
    floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
    mr = d.add_texture(image)
    d.set_material_param_texture(floor, R, mr, 1)
    d.set_material_param_texture(floor, M, mr, 2)
    d.add_mesh(*ag.create_backdrop([0, -1, 20], [40, 20, 40], 7.5, 32), floor, 1)
    d.add_sphere([0, 0, 0], 1.0, 0)
    d.add_area_light([0, 25, -20], 1.0, [200., F(.941) * F(200), F(.914) * F(200)])
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], F(W) / F(H), 45.0, 0.0)
    g = gpu_scene(d)
    try:
        acc, _ = ag.PathTracer(5).render_to_host(g, W, H, 4)
    finally:
        g.close()
    assert acc_c.tobytes() == acc.tobytes()
