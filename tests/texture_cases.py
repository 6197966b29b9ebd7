"""The scene construction the texture-family GPU tests share (test_gpu_textures.py, test_gpu_material_maps.py,
test_gpu_texture_filter.py, test_gpu_normal_map.py): the palette meshes, the triangle soup and the varying heightfield with their lights
and cameras, and descriptions with texture ops taken out.  What a feature attaches -- materials, images, samplers -- stays in its file and
comes in as a callback, or is applied to the description before or after."""
import copy

import numpy as np

import ag_pathtracer_amd as ag
from helpers import bits, oracle_render

F = np.float32
K = 8
PALETTE = np.array([[.80, .78, .70], [.85, .30, .25], [.20, .55, .80], [.95, .93, .88], [.35, .70, .30], [.90, .75, .35],
                    [.55, .35, .75], [.25, .25, .28]], F)
TEXTURE_OPS = ("texture", "material_texture", "material_param_texture", "texture_sampler")


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
