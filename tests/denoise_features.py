"""What agpt_render_features must produce, computed on the host from the CPU oracle: one oracle_camera_ray through every pixel
centre of an aperture-0 copy of the camera, oracle_intersect_batch, then the material colour of the hit primitive and the
shading normal expected for its type.  Buffers are [H, W, 4] in Accumulator::pixels order (row H-1-y), like the device's."""
import copy

import numpy as np

from helpers import oracle_scene
from oracle import binding as ob

F = np.float32


def pinhole(desc):
    """a copy of the scene description whose camera has aperture 0"""
    d = copy.copy(desc)
    d.camera = tuple(desc.camera[:5]) + (0.0,)
    return d


def primitive_table(desc):
    """per primitive in Scene::primitives order: (op, material index or -1); and the material colours"""
    prims, colors = [], []
    for op in desc.ops:
        if op[0] == "material":
            colors.append(np.asarray(op[2], F))
        elif op[0] == "mesh":
            prims.append((op, op[5]))
        elif op[0] in ("sphere", "plane"):
            prims.append((op, op[3]))
        elif op[0] == "area_light":
            prims.append((op, -1))
    return prims, colors


def _unit(v):
    return v / np.linalg.norm(v)


def host_features(desc, W, H):
    """-> (albedo[H, W, 4], normal_depth[H, W, 4] with the EXPECTED normal in float64 precision rounded to float32,
    either_sign[H, W]: pixels whose normal is defined up to its sign (meshes without normals), hits[H, W])"""
    o = oracle_scene(pinhole(desc))
    rays = np.zeros(W * H, ob.RAY_DTYPE)
    for y in range(H):
        for x in range(W):
            rays[y * W + x], _ = o.camera_ray(F(x + 0.5) / F(W), F(y + 0.5) / F(H))
    hits, _ = o.intersect(rays, False)
    prims, colors = primitive_table(desc)
    albedo = np.zeros((H, W, 4), F)
    nd = np.zeros((H, W, 4), F)
    either = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            h, r = hits[y * W + x], rays[y * W + x]
            row = H - 1 - y
            if not h["hit"]:
                albedo[row, x] = (1, 1, 1, 0)
                continue
            op, mat = prims[h["prim"]]
            albedo[row, x, :3] = colors[mat] if mat >= 0 else 1.0
            albedo[row, x, 3] = 1 if mat >= 0 else 2
            if op[0] == "mesh":
                verts, normals, idx, tri = op[1].astype(np.float64), op[2], op[4], h["tri"]
                if normals is not None:
                    n0, n1, n2 = (normals[idx[tri + k, 1]].astype(np.float64) for k in range(3))
                    b1, b2 = float(h["b1"]), float(h["b2"])
                    ns = _unit((1.0 - b1 - b2) * n0 + b1 * n1 + b2 * n2)
                else:
                    v0, v1, v2 = (verts[idx[tri + k, 0]] for k in range(3))
                    ns = _unit(np.cross(v2 - v0, v1 - v0))
                    either[row, x] = True
            elif op[0] == "plane":
                ns = np.array([0.0, 1.0, 0.0])
            else:
                d = _unit(r["d"].astype(np.float64))
                p = r["o"].astype(np.float64) + float(h["t"]) * d
                ns = (p - op[1].astype(np.float64)) / float(op[2])
            nd[row, x, :3] = ns
            nd[row, x, 3] = h["t"]
    return albedo, nd, either, hits.reshape(H, W)
