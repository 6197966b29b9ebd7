"""The meshes the smooth-normal tests share (test_vertex_normals_arrays.py on the host, test_gpu_smooth_normals.py on the GPU).  A case
is (vertices[n, 3], corners[k, 3], n_normals): corners are (vertex, normal, texcoord) triplets as for Scene.add_mesh."""
import numpy as np

import device_update_cases as dc

F = np.float32
ZOO_WITH_NORMALS = [p for p in dc.PRIMS if dc.ZOO[p - 1][2]]   # the four zoo meshes that have normals


def zoo_case(prim, pose=0):
    _, make, wn, _, _ = dc.ZOO[prim - 1]
    v, n = dc.zoo_arrays(prim, pose)
    return v, make(wn)[2], len(n)


def grid(n, offset=(0.0, 0.0, 0.0), height=None):
    """n x n vertices over [-1, 1]^2, one normal per vertex, 2 (n - 1)^2 triangles"""
    x, z = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing="ij")
    y = 0.2 * np.sin(2.7 * x + 0.3) * np.cos(3.1 * z) if height is None else height(x, z)
    v = (np.stack([x, y + 0.5, z], -1).reshape(-1, 3) + np.array(offset)).astype(F)
    tris = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, i * n + j + 1, (i + 1) * n + j, (i + 1) * n + j + 1
            tris += [(a, b, c), (b, d, c)]
    return v, dc._corners(tris, True), n * n


def flat_grid():
    """bumpy_grid with one normal per triangle, named by its three corners: 170 vertices, 288 normals"""
    v, _, ix = dc.bumpy_grid(False)
    corners = ix.copy()
    corners[:, 1] = np.repeat(np.arange(len(ix) // 3, dtype=np.int32), 3)
    return v, corners, len(ix) // 3


def plane_grid(n=9, flip=False):
    """a grid in the xz-plane with spacing 2^-3: every difference, product and square is exact, every referenced normal (0, +1, 0) --
    (0, -1, 0) with the winding flipped"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([0.125 * i, np.zeros_like(i, float), 0.125 * j], -1).reshape(-1, 3).astype(F)
    tris = []
    for a in range(n - 1):
        for b in range(n - 1):
            p, q, r, s = a * n + b, a * n + b + 1, (a + 1) * n + b, (a + 1) * n + b + 1
            tris += [(p, r, q), (q, r, s)] if flip else [(p, q, r), (q, s, r)]
    return v, dc._corners(tris, True), n * n


def shared_normal():
    """the 288-triangle grid with ONE normal, named by all 864 corners"""
    v, _, ix = dc.bumpy_grid(True)
    corners = ix.copy()
    corners[:, 1] = 0
    return v, corners, 1


def fan(k=200):
    """k triangles around vertex 0 (valence k), the rim a wavy circle; one normal per vertex"""
    a = 2 * np.pi * np.arange(k) / k
    rim = np.stack([np.cos(a), 0.15 * np.sin(5 * a) + 0.05 * np.cos(13 * a), np.sin(a)], 1)
    v = np.concatenate([[[0.0, 0.3, 0.0]], rim]).astype(F)
    tris = [(0, 1 + (i + 1) % k, 1 + i) for i in range(k)]
    return v, dc._corners(tris, True), k + 1


def _extended(extra_v, extra_corners, extra_normals):
    """bumpy_grid (170 vertices and normals; vertex and normal 169 are referenced by nothing) plus vertices, corners and normals of a
    case's own; the corners index the extra vertices from 170 and the extra normals from 170"""
    v, _, ix = dc.bumpy_grid(True)
    if len(extra_v):
        v = np.concatenate([v, np.asarray(extra_v, F).reshape(-1, 3)]).astype(F)
    if len(extra_corners):
        ix = np.concatenate([ix, np.asarray(extra_corners, np.int32).reshape(-1, 3)])
    return v, ix, 170 + extra_normals


def _tri(verts, normals):
    return [(170 + a, 170 + b, -1) for a, b in zip(verts, normals)]


def specials():
    """{name: (case, the normal items that must come out as exact zeros)}; every item below 169 that is not listed must keep the bits it
    has in bumpy_grid alone"""
    out = {}
    # normal 169 has items on both sides (170 is named by the extra triangle), 171 is the last item: neither is named by a corner
    out["unreferenced"] = (_extended([[0, 2, 0], [1, 2, 0], [0, 2, 1]], _tri((0, 1, 2), (0, 0, 0)), 2), [169, 171])
    out["zero_area"] = (_extended([[0, 2, 0], [0, 2, 0], [1, 2, 3]], _tri((0, 1, 2), (0, 1, 2)), 3), [169, 170, 171, 172])
    out["cancelling"] = (_extended([[0, 2, 0], [1, 2.5, 0], [0.25, 2, 1]], _tri((0, 1, 2), (0, 1, 2)) + _tri((0, 2, 1), (0, 2, 1)), 3),
                         [169, 170, 171, 172])
    s = 2.0 ** -70    # g = 2^-140 (a denormal), its square underflows to 0
    out["underflow"] = (_extended([[0, 0, 0], [s, 0, 0], [0, s, 0]], _tri((0, 1, 2), (0, 1, 2)), 3), [169, 170, 171, 172])
    b = 2.0 ** 40     # g = 2^80, its square overflows to Inf
    out["overflow"] = (_extended([[0, 0, 0], [b, 0, 0], [0, b, 0]], _tri((0, 1, 2), (0, 1, 2)), 3), [169, 170, 171, 172])
    for name, bad in (("nan", np.nan), ("inf", np.inf)):
        v, ix, nn = _extended([], [], 0)
        v[dc.REFERENCED, 1] = bad
        touched = sorted({int(j) for t in range(len(ix) // 3) if dc.REFERENCED in ix[3 * t:3 * t + 3, 0] for j in ix[3 * t:3 * t + 3, 1]})
        out[name] = ((v, ix, nn), touched + [169])
    return out
