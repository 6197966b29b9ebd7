"""numpy model of agpt_bvh_refit: the bounds of a BVH in the reference layout recomputed for new vertices, topology kept.  A leaf is
the +-1e34 box grown over its primitives' three vertices in slot order, an interior node (left, right) of its child pair; min / max
are the builder's comparisons (a < b ? a : b, a > b ? a : b), written with np.where -- not np.minimum -- so that +-0 come out as the
library's do."""
import numpy as np

F = np.float32


def tmin(a, b):
    return np.where(a < b, a, b)


def tmax(a, b):
    return np.where(a > b, a, b)


def refit(nodes, prim_index, verts, indices):
    """nodes: NODE_DTYPE[total + 1] (slot 1 unused), prim_index: int32[n_tris] (3 * triangle per slot), verts: [n, 3] float32,
    indices: [3 * n_tris, 3] (v, n, t) rows -> a new nodes array."""
    out = nodes.copy()
    v = np.ascontiguousarray(verts, F).reshape(-1, 3)
    vid = np.asarray(indices, np.int32).reshape(-1, 3)[:, 0]
    for i in range(len(out) - 1, -1, -1):
        if i == 1:
            continue
        first, count = int(out["first"][i]), int(out["count"][i])
        if count > 0:
            lo, hi = np.full(3, 1e34, F), np.full(3, -1e34, F)
            for s in range(first, first + count):
                for k in range(3):
                    p = v[vid[prim_index[s] + k]]
                    lo, hi = tmin(lo, p), tmax(hi, p)
        else:
            lo = tmin(out["bmin"][first], out["bmin"][first + 1])
            hi = tmax(out["bmax"][first], out["bmax"][first + 1])
        out["bmin"][i], out["bmax"][i] = lo, hi
    return out


def subtree_vertices(nodes, prim_index, indices, i):
    """vertex ids below node i"""
    first, count = int(nodes["first"][i]), int(nodes["count"][i])
    vid = np.asarray(indices, np.int32).reshape(-1, 3)[:, 0]
    if count > 0:
        return np.concatenate([vid[prim_index[s]:prim_index[s] + 3] for s in range(first, first + count)])
    return np.concatenate([subtree_vertices(nodes, prim_index, indices, first), subtree_vertices(nodes, prim_index, indices, first + 1)])
