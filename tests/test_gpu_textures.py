"""Image-textured materials on the GPU (agpt_scene_add_texture / agpt_scene_set_material_texture).  The tests below go
back to when the CPU oracle knew no textures (whole textured paths against it: test_gpu_textured_paths.py); every test is built so
that the untextured oracle is still the yardstick: a texture of one colour must equal the plain material,
a texel per mesh must equal a material per mesh, first hits are checked through the oracle's intersections and the numpy model
of the lookup (tests/texture_model.py)."""
import re
import subprocess

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import denoise_model as dm
import texture_cases as tc
import texture_model as tm
from denoise_features import host_features, primitive_table
from helpers import bits, build_cpp_example, gpu_context, gpu_scene, oracle_render, oracle_scene
from oracle import binding as ob
from texture_cases import (K, PALETTE, SOUP, palette_meshes, soup_excluded_pixels, varying_lights_and_camera, varying_mesh,
                           without_textures)

F = np.float32


def with_constant_textures(desc, tw, th):
    """desc without its textures; then every material that only meshes use (a textured material on a sphere or a plane is
    refused at commit) gets a tw x th texture filled with its own colour"""
    d = without_textures(desc)
    d.ops = list(d.ops)
    analytic = {op[3] for op in d.ops if op[0] in ("sphere", "plane")}
    colors = [op[2] for op in d.ops if op[0] == "material"]
    n = 0
    for m, c in enumerate(colors):
        if m in analytic:
            continue
        d.set_material_texture(m, d.add_texture(np.broadcast_to(np.asarray(c, F), (th, tw, 3))))
        n += 1
    assert n >= 1
    return d


# ---- 3. a texture of one colour is no texture ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["c1", "textured"])
@pytest.mark.parametrize("size", [(1, 1), (7, 5)])
def test_constant_texture_equals_no_texture(which, size):
    base = ag.scenes.scene_c1() if which == "c1" else ag.scenes.scene_textured()
    plain, const = without_textures(base), with_constant_textures(base, *size)
    W, H, spp = 96, 64, 3
    oacc, ost = oracle_render(plain, W, H, spp)
    gp, gc = gpu_scene(plain), gpu_scene(const)
    try:
        pt = ag.PathTracer(5)
        a, sa = pt.render_to_host(gp, W, H, spp)
        b, sb = pt.render_to_host(gc, W, H, spp)
        assert np.array_equal(bits(a), bits(b)) and sa.rays == sb.rays
        assert np.array_equal(bits(b[..., :3]), bits(oacc[..., :3])) and sb.rays == ost.rays
        gp.set_shading_arith("fast")
        gc.set_shading_arith("fast")
        fa, _ = pt.render_to_host(gp, W, H, spp)
        fb, _ = pt.render_to_host(gc, W, H, spp)
        assert np.array_equal(bits(fa), bits(fb))
        assert not np.array_equal(bits(fa), bits(a))    # (FAST is another arithmetic: the comparison above is FAST with FAST)
    finally:
        gp.close()
        gc.close()


# ---- 4. one texel per mesh = one material per mesh ---------------------------------------------------------------------
KINDS = [(ag.MAT_DISNEY, 1.0, 0.0), (ag.MAT_DISNEY, 0.35, 1.0), (ag.MAT_MIRROR, 0.0, 0.0), (ag.MAT_DIFFUSE_ONLY, 0.0, 0.0),
         (ag.MAT_DISNEY, 0.6, 0.5)]


def palette_scene(degenerate_uv, textured):
    d = ag.SceneDesc("palette")
    if textured:   # the materials are shared: one per kind, all pointing at the palette
        mats = [d.add_material(t, [.5, .5, .5], r, m) for (t, r, m) in KINDS]
        tex = d.add_texture(PALETTE[None])
        for m in mats:
            d.set_material_texture(m, tex)

    def material(k):
        if textured:
            return mats[k % len(KINDS)]
        t, r, m = KINDS[k % len(KINDS)]
        return d.add_material(t, PALETTE[k], r, m)     # one plain material per mesh, its colour the texel

    return tc.palette_scene(d, palette_meshes(degenerate_uv), material)


def test_palette_footprints():
    """the construction, checked on the CPU with the model: every vertex uv of mesh k reads texel k"""
    for degenerate in (False, True):
        for k, (v, n, uv, idx) in enumerate(palette_meshes(degenerate)):
            x, y = tm.texel_index((1, K), uv[:, 0], uv[:, 1])
            assert (x == k).all() and (y == 0).all()
            pos, _ = tm.texel_position((1, K), uv[:, 0], uv[:, 1])
            assert (pos - np.floor(pos) > 0.05).all() and (pos - np.floor(pos) < 0.95).all()


@pytest.mark.gpu
@pytest.mark.parametrize("degenerate_uv", [False, True])
def test_one_texel_per_mesh_equals_one_material_per_mesh(degenerate_uv):
    tex_desc, plain_desc = palette_scene(degenerate_uv, True), palette_scene(degenerate_uv, False)
    W, H, spp, depth = 64, 64, 3, 5
    oacc, ost = oracle_render(plain_desc, W, H, spp, depth)
    g = gpu_scene(tex_desc)
    try:
        acc, st = ag.PathTracer(depth).render_to_host(g, W, H, spp)
        same = (bits(acc[..., :3]) == bits(oacc[..., :3])).all(-1)
        print("palette render: %d of %d pixels bit-identical, rays %d / %d" % (same.sum(), same.size, st.rays, ost.rays))
        assert same.all() and st.rays == ost.rays
        assert len(np.unique(bits(acc[..., :3]).reshape(-1, 3), axis=0)) > W * H // 2
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
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(got_after, after)
    finally:
        g.close()


# ---- 5. variation inside a mesh, first hit ------------------------------------------------------------------------------
def varying_scene():
    d = ag.SceneDesc("varying")
    m = d.add_material(ag.MAT_DISNEY, [.5, .5, .5], .7, .2)
    d.add_mesh(*varying_mesh(), m, 1)
    tex = np.random.RandomState(21).uniform(0.05, 0.95, (16, 16, 3)).astype(F)
    d.set_material_texture(m, d.add_texture(tex))
    return varying_lights_and_camera(d), tex


def expected_first_hit_albedo(desc, tex, W, H):
    """the model applied to the oracle's pixel-centre hits: albedo rgb[H, W, 3], hit-a-textured-mesh mask, boundary distance"""
    plain = without_textures(desc)     # (the oracle takes the geometry and the texture coordinates, not the image)
    _, _, _, hits = host_features(plain, W, H)
    prims, _ = primitive_table(plain)
    rgb = np.zeros((H, W, 3), F)
    mask = np.zeros((H, W), bool)
    dist = np.ones((H, W))
    for y in range(H):
        for x in range(W):
            h = hits[y, x]
            if not h["hit"] or prims[h["prim"]][0][0] != "mesh":
                continue
            op = prims[h["prim"]][0]
            uvs, idx, tri = op[3], op[4], h["tri"]
            uv0, uv1, uv2 = (uvs[idx[tri + k, 2]] for k in range(3))
            u, v = tm.interpolate_uv(uv0, uv1, uv2, h["b1"], h["b2"])
            row = H - 1 - y
            rgb[row, x] = tm.value(tex, u, v)
            mask[row, x] = True
            dist[row, x] = tm.boundary_distance(tex.shape, u, v)
    return rgb, mask, dist


def test_first_hit_boundary_share_on_the_cpu():
    """the share of hit pixels within 1e-5 texels of a texel boundary, from the oracle and the model alone: at most 0.5 %"""
    d, tex = varying_scene()
    _, mask, dist = expected_first_hit_albedo(d, tex, 64, 64)
    near = mask & (dist < 1e-5)
    print("hit pixels %d, near a boundary %d" % (mask.sum(), near.sum()))
    assert mask.sum() > 1500 and near.sum() <= 0.005 * mask.sum()


@pytest.mark.gpu
def test_first_hit_albedo_is_the_texel():
    d, tex = varying_scene()
    W = H = 64
    want, mask, dist = expected_first_hit_albedo(d, tex, W, H)
    skip = mask & (dist < 1e-5)
    assert mask.sum() > 1500 and skip.sum() <= 0.005 * mask.sum()
    g = gpu_scene(d)
    try:
        albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
    finally:
        g.close()
    assert ((albedo[..., 3] == 1) == mask).all()
    check = mask & ~skip
    same = (bits(albedo[..., :3]) == bits(want)).all(-1)
    print("first-hit albedo: %d pixels checked, %d skipped, %d differ" % (check.sum(), skip.sum(), (check & ~same).sum()))
    assert same[check].all()
    assert len(np.unique(bits(albedo[..., :3])[mask], axis=0)) > 100     # many texels seen
    assert (albedo[~mask][:, :3] == 1).all()


# ---- 6. variation inside a mesh, whole paths -----------------------------------------------------------------------------
def soup_scene(mode):
    """mode "textured": the single mesh with the palette; "single" / "grouped": the single mesh / the triangles regrouped into K
    meshes by colour, all in ONE colour; "grouped_colours": regrouped with K plain materials"""
    def material(d, k):
        m = d.add_material(ag.MAT_DISNEY, PALETTE[k] if mode == "grouped_colours" else PALETTE[0], 0.5, 0.3)
        if mode == "textured":
            d.set_material_texture(m, d.add_texture(PALETTE[None]))
        return m

    return tc.soup_scene("soup-" + mode, material, grouped=mode.startswith("grouped"))


def test_regrouping_changes_few_pixels_for_the_oracle():
    """the reference alone: one mesh against the same triangles regrouped into K meshes (other BVHs), both in one colour.
    Found on the CPU: 0 pixels of 4096 differ (see test_colour_per_triangle_matches_regrouped_oracle)."""
    ex = soup_excluded_pixels()
    print("regrouped oracle render differs in %d of %d pixels" % (ex.sum(), ex.size))
    assert ex.sum() <= 0.01 * ex.size


@pytest.mark.gpu
def test_colour_per_triangle_matches_regrouped_oracle():
    """One mesh, colour per triangle through the palette texture, against the oracle rendering the triangles regrouped by colour
    with K plain materials.  Pixels where the oracle itself renders the one-colour single mesh and the one-colour regrouped meshes
    differently (a grazing hit decided differently by the two trees) are excluded: 0 of 4096 when this was written (CPU, oracle only)."""
    ex = soup_excluded_pixels()
    assert ex.sum() <= 0.01 * ex.size
    want, _ = oracle_render(soup_scene("grouped_colours"), SOUP["W"], SOUP["H"], SOUP["spp"], SOUP["depth"])
    g = gpu_scene(soup_scene("textured"))
    try:
        acc, _ = ag.PathTracer(SOUP["depth"]).render_to_host(g, SOUP["W"], SOUP["H"], SOUP["spp"])
    finally:
        g.close()
    same = (bits(acc[..., :3]) == bits(want[..., :3])).all(-1)
    print("colour per triangle: %d excluded, %d of the remaining %d pixels differ" % (ex.sum(), (~same & ~ex).sum(), (~ex).sum()))
    assert same[~ex].all()


# ---- 7. invariance ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_textured_render_does_not_depend_on_the_split(arith):
    from ag_pathtracer_amd import tiles
    W, H, spp = 80, 64, 4
    g = gpu_scene(ag.scenes.scene_textured())
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
        # the texture is seen: the plain scene renders another image
        p = gpu_scene(without_textures(ag.scenes.scene_textured()))
        try:
            p.set_shading_arith(arith)
            plain, _ = pt.render_to_host(p, W, H, spp)
        finally:
            p.close()
        assert (bits(plain[..., :3]) != bits(full[..., :3])).any(-1).mean() > 0.3
    finally:
        g.close()


# ---- 8. the textured albedo flows through the denoiser ------------------------------------------------------------------
@pytest.mark.gpu
def test_denoise_demodulates_the_textured_albedo():
    W, H = 96, 64
    g = gpu_scene(ag.scenes.scene_textured())
    try:
        pt = ag.PathTracer(5)
        acc, m2, _, _ = pt.render_adaptive_to_host(g, W, H, 8, 8, 8, 0.0)
        albedo, nd = pt.render_features_to_host(g, W, H)
    finally:
        g.close()
    surface = albedo[..., 3] == 1
    assert len(np.unique(bits(albedo[..., :3])[surface], axis=0)) > 20      # texels, not one colour per material
    out = gpu_context().denoise_to_host(acc, m2, albedo, nd, 5, True)
    model = dm.denoise(acc, m2, albedo, nd, 5, True)
    differ = (out != model).any(-1)
    print("denoise on the textured scene: %d of %d pixels differ from the model" % (differ.sum(), differ.size))
    assert not differ.any()


# ---- 9. the C++ adapter ---------------------------------------------------------------------------------------------------
def test_cpp_textured_example_compiles_and_links(tmp_path):
    build_cpp_example(tmp_path, "textured_scene")


@pytest.mark.gpu
def test_cpp_textured_example_matches_python(tmp_path):
    W, H = 96, 64
    exe = build_cpp_example(tmp_path, "textured_scene")
    out_path = str(tmp_path / "out.bin")
    out = subprocess.check_output([exe, out_path, str(W), str(H)], timeout=300).decode()
    assert re.search(r"textured %dx%d samples=4" % (W, H), out), out
    raw = np.fromfile(out_path, np.uint8)
    n = W * H * 16
    acc_c, albedo_c = (raw[k * n:(k + 1) * n].view(F).reshape(H, W, 4) for k in range(2))
    y, x = np.mgrid[0:8, 0:16]
    odd = ((x // 2) + (y // 2)) % 2 == 1
    shade = (F(1) - F(0.0625) * y.astype(F)).astype(F)
    tex = np.stack([np.where(odd, F(.125), F(.75)) * shade, np.where(odd, F(.25), F(.75)) * shade,
                    np.where(odd, F(.5), F(.625)) * shade], -1).astype(F)
    d = ag.SceneDesc("cpp-textured")
    d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], .5, 1.)
    floor = d.add_material(ag.MAT_DISNEY, [0.6, 0.62, 0.45], 1., 0.)
    d.set_material_texture(floor, d.add_texture(tex))
    d.add_mesh(*ag.create_backdrop([0, -1, 20], [40, 20, 40], 7.5, 32), floor, 1)
    d.add_sphere([0, 0, 0], 1.0, 0)
    d.add_area_light([0, 25, -20], 1.0, [200., F(.941) * F(200), F(.914) * F(200)])
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], F(W) / F(H), 45.0, 0.0)
    g = gpu_scene(d)
    try:
        acc, _ = ag.PathTracer(5).render_to_host(g, W, H, 4)
        albedo, _ = ag.PathTracer(5).render_features_to_host(g, W, H)
    finally:
        g.close()
    assert albedo_c.tobytes() == albedo.tobytes() and acc_c.tobytes() == acc.tobytes()
    assert len(np.unique(bits(albedo[..., :3]).reshape(-1, 3), axis=0)) > 10
