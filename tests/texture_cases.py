"""The scene construction the texture-family GPU tests share (test_gpu_textures.py, test_gpu_material_maps.py,
test_gpu_texture_filter.py, test_gpu_normal_map.py): the palette meshes, the triangle soup and the varying heightfield with their lights
and cameras, and descriptions with texture ops taken out.  What a feature attaches -- materials, images, samplers -- stays in its file and
comes in as a callback, or is applied to the description before or after."""
import copy

import numpy as np

import ag_pathtracer_amd as ag
import texture_filter_model as fm
from helpers import bits, oracle_render, oracle_scene
from oracle import binding as ob

F = np.float32
K = 8
PALETTE = np.array([[.80, .78, .70], [.85, .30, .25], [.20, .55, .80], [.95, .93, .88], [.35, .70, .30], [.90, .75, .35],
                    [.55, .35, .75], [.25, .25, .28]], F)
TEXTURE_OPS = ("texture", "material_texture", "material_param_texture", "texture_sampler")
BILINEAR, NEAREST = ag.FILTER_BILINEAR, ag.FILTER_NEAREST
FLAT = np.broadcast_to(np.array([.5, .5, 1], F), (4, 4, 3))      # a normal map that tilts nothing


# ---- descriptions without their texture ops ----------------------------------------------------------------------------------
def without(desc, kinds):
    d = copy.copy(desc)
    d.ops = [op for op in desc.ops if op[0] not in kinds]
    d.n_textures = sum(op[0] == "texture" for op in d.ops)
    return d


def without_textures(desc):
    """desc without images, the colour and parameter slots that name them and their samplers (normal-map slots are not taken out)"""
    return without(desc, TEXTURE_OPS)


# ---- K meshes, one palette texel each ----------------------------------------------------------------------------------------
def palette_meshes(degenerate_uv):
    """K meshes -- a floor and K - 1 blobs around the origin -- whose texture coordinates all lie inside texel k's footprint
    [(k + .5) / K, (k + 1.5) / K) of a K x 1 palette, a tenth of a texel away from its ends"""
    rng = np.random.RandomState(5)
    meshes = []
    for k in range(K):
        if k == 0:
            v, n, t, idx = ag.scenes.grid_mesh(lambda U, V: np.stack([-6 + 12 * U, -1 + 0 * U, -6 + 12 * V], -1), 6, 6)
        else:
            a = 2 * np.pi * k / (K - 1)
            v, n, t, idx = ag.scenes.blob_mesh(10, 8, center=(2.4 * np.cos(a), -0.2 + 0.5 * (k % 3), 2.4 * np.sin(a)), radius=0.85, seed=k)
        if degenerate_uv:
            uv = np.broadcast_to(np.array([(k + 1.0) / K, 0.5], F), (len(v), 2)).copy()
        else:
            uv = np.stack([(k + 0.6 + 0.8 * rng.uniform(size=len(v))) / K, rng.uniform(0.1, 0.9, len(v))], 1).astype(F)
        meshes.append((v, n, uv, idx))
    return meshes


def palette_lights_and_camera(d):
    d.add_area_light([0, 9, -2], 1.0, ag.scenes.KEY_LIGHT * F(60))
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([0.5, 4.5, -7.5], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    return d


def palette_scene(d, meshes, material_of):
    """d -- with whatever materials and images the meshes share already in it -- completed: mesh k of `meshes` with material
    material_of(k), which may add one per mesh, then the palette scene's lights and camera"""
    for k, (v, n, uv, idx) in enumerate(meshes):
        d.add_mesh(v, n, uv, idx, material_of(k), 1)
    return palette_lights_and_camera(d)


# ---- K + 4 meshes, one PAIR of texels each ------------------------------------------------------------------------------------
# (roughness, metallic) per plateau: metallic 0, 1 and .5 -- a wrong tap changes the lobe set and the ray count --, roughness below the
# .001 clamp of alpha, .35 and 1
PARAMS = np.array([[1.0, 0.0], [.35, 1.0], [0.0, .5], [.02, 0.0], [.6, .5], [0.0, 1.0], [.02, 1.0], [.5, .3]], F)
KINDS = [(ag.MAT_DISNEY, 1.0, 0.0), (ag.MAT_DISNEY, 0.35, 1.0), (ag.MAT_MIRROR, 0.0, 0.0), (ag.MAT_DIFFUSE_ONLY, 0.0, 0.0),
         (ag.MAT_DISNEY, 0.6, 0.5)]
# meshes beyond the first K: (plateau their footprint would have inside [0, 1], whole periods it is shifted by).  REPEAT reads the
# plateau itself, CLAMP the last (shift > 0) or the first (shift < 0) texel, MIRROR with an odd shift plateau K - 1 - j
OUTSIDE = [(2, 1), (5, -1), (1, 2), (3, -3)]


def plateau(values):
    """[K, C] -> image [1, 2K, 3]: texels 2k and 2k + 1 both hold values[k] (C < 3: zero-filled)"""
    values = np.asarray(values, F)
    img = np.zeros((1, 2 * len(values), 3), F)
    img[0, :, :values.shape[1]] = np.repeat(values, 2, axis=0)
    return img


def plateau_meshes():
    """K + len(OUTSIDE) meshes -- a floor, K - 1 blobs around the origin, more blobs above them.  Mesh k < K has every u strictly
    between the centres of texels 2k and 2k + 1 of a 2K x 1 image (a tenth of a texel from both), so both horizontal taps of a
    BILINEAR lookup are that pair; the others have such a footprint shifted by whole periods, outside [0, 1].  v is anywhere in
    [-2, 3]: the image has one row."""
    rng = np.random.RandomState(5)
    meshes = []
    for k in range(K + len(OUTSIDE)):
        if k == 0:
            v, n, t, idx = ag.scenes.grid_mesh(lambda U, V: np.stack([-6 + 12 * U, -1 + 0 * U, -6 + 12 * V], -1), 6, 6)
        elif k < K:
            a = 2 * np.pi * k / (K - 1)
            v, n, t, idx = ag.scenes.blob_mesh(10, 8, center=(2.4 * np.cos(a), -0.2 + 0.5 * (k % 3), 2.4 * np.sin(a)), radius=0.85, seed=k)
        else:
            a = 2 * np.pi * (k - K + .5) / len(OUTSIDE)
            v, n, t, idx = ag.scenes.blob_mesh(10, 8, center=(1.1 * np.cos(a), 1.5, 1.1 * np.sin(a)), radius=0.6, seed=k)
        j, shift = (k, 0) if k < K else OUTSIDE[k - K]
        u = (2 * j + 0.6 + 0.8 * rng.uniform(size=len(v))) / (2 * K) + shift
        meshes.append((v, n, np.stack([u, rng.uniform(-2, 3, len(v))], 1).astype(F), idx))
    return meshes


def plateau_values(values, wrap, filter=BILINEAR):
    """per mesh the value a lookup of plateau(values) under (filter, wrap) gives at EVERY vertex uv of the mesh, from the model (asserts
    that it is one value per mesh, and that the position keeps 0.05 texels from both centres: both taps of a BILINEAR lookup are the
    plateau's pair, the floor of a NEAREST one its first texel)"""
    img = plateau(values)
    out = []
    for v, n, uv, idx in plateau_meshes():
        c = fm.value(img, uv[:, 0], uv[:, 1], filter, wrap, wrap)
        assert (bits(c) == bits(c[0])).all()
        x0, x1, y0, y1, fx, fy = fm.taps(img, uv[:, 0], uv[:, 1], BILINEAR, wrap, wrap)
        assert (fx > 0.05).all() and (fx < 0.95).all() and (y0 == 0).all() and (y1 == 0).all()
        out.append(c[0, :np.asarray(values).shape[1]])
    return np.array(out, F)


# what tests/test_gpu_shade_matrix.py stacks on the plateau meshes: the parameter plateaus in channels 1 and 2 of ONE image, and per
# texturing level the (filter, wrap) of the colour image and of the parameter image -- the default sampler below SAMPLED
PARAM_TEXELS = np.concatenate([np.zeros((K, 1), F), PARAMS], 1)


def matrix_samplers(level):
    if level >= 3:
        return (BILINEAR, ag.WRAP_MIRROR), (BILINEAR, ag.WRAP_CLAMP)
    return (NEAREST, ag.WRAP_REPEAT), (NEAREST, ag.WRAP_REPEAT)


def check_li_against_oracle(g, plain_desc, depth, n=1000):
    """agpt_li_batch on camera rays against the oracle's Li on the plain scene: values and RNG end states"""
    o = oracle_scene(plain_desc, depth)
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
    print("Li: %d of %d values bit-identical, %d RNG end states" % ((bits(got) == bits(want)).all(-1).sum(), n, (got_after == after).sum()))
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(got_after, after)


# ---- one mesh of unshared triangles, one palette texel each ------------------------------------------------------------------
def triangle_soup():
    """a bumpy floor and a blob as ONE mesh of T unshared triangles, each with its three uvs inside one palette texel: positions,
    normals, uvs [3T, .] and the texel [T]"""
    parts = [ag.scenes.heightfield(10, S=3.0), ag.scenes.blob_mesh(10, 8, center=(0.2, 1.3, 0.1), radius=0.9, seed=2)]
    V, N, UV, texel = [], [], [], []
    rng = np.random.RandomState(8)
    for v, n, t, idx in parts:
        tri = idx[:, 0].reshape(-1, 3)
        for a in tri:
            k = int(rng.randint(K))
            V.append(v[a])
            N.append(n[a])
            UV.append(np.stack([(k + 0.6 + 0.8 * rng.uniform(size=3)) / K, rng.uniform(0.1, 0.9, 3)], 1))
            texel.append(k)
    return np.concatenate(V).astype(F), np.concatenate(N).astype(F), np.concatenate(UV).astype(F), np.array(texel)


def soup_material(d, k):
    """the ONE material of the soup scenes that vary nothing"""
    return d.add_material(ag.MAT_DISNEY, PALETTE[0], 0.5, 0.3)


def soup_scene(name, material_of, grouped):
    """the triangle soup as the single mesh, with material material_of(d, None), or -- grouped -- its triangles regrouped into K meshes
    by texel, group k with material_of(d, k)"""
    v, n, uv, texel = triangle_soup()
    d = ag.SceneDesc(name)

    def mesh(sel, material):
        ids = np.repeat(3 * np.nonzero(sel)[0], 3) + np.tile(np.arange(3), int(sel.sum()))
        ix = np.arange(len(ids), dtype=np.int32)
        d.add_mesh(v[ids], n[ids], uv[ids], np.stack([ix, ix, ix], 1), material, 1)

    if grouped:
        for k in range(K):
            mesh(texel == k, material_of(d, k))
    else:
        mesh(np.ones(len(texel), bool), material_of(d, None))
    d.add_area_light([1, 7, -2], 0.8, ag.scenes.KEY_LIGHT * F(50))
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([0.4, 3.4, -5.2], [0, 0.4, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    return d


SOUP = dict(W=64, H=64, spp=2, depth=5)


def soup_excluded_pixels():
    """the pixels the oracle itself renders differently for the single mesh and for the regrouped meshes, both with the one material"""
    a, _ = oracle_render(soup_scene("soup-single", soup_material, False), SOUP["W"], SOUP["H"], SOUP["spp"], SOUP["depth"])
    b, _ = oracle_render(soup_scene("soup-grouped", soup_material, True), SOUP["W"], SOUP["H"], SOUP["spp"], SOUP["depth"])
    return (bits(a[..., :3]) != bits(b[..., :3])).any(-1)


# ---- variation inside one mesh ---------------------------------------------------------------------------------------------------
def varying_mesh(with_normals=True):
    """a heightfield whose uvs are a rotated, scaled copy of the grid's own: they vary smoothly and leave [0, 1]"""
    v, n, t, idx = ag.scenes.heightfield(24)
    c, s = np.cos(0.4), np.sin(0.4)
    uv = np.stack([1.7 * (c * t[:, 0] - s * t[:, 1]) - 0.3, 1.3 * (s * t[:, 0] + c * t[:, 1]) + 0.2], 1).astype(F)
    return v, (n if with_normals else None), uv, idx


def varying_lights_and_camera(d):
    d.add_area_light([0, 6, 0], 0.5, ag.scenes.KEY_LIGHT * F(30))
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([0.3, 3.2, -3.6], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    return d
