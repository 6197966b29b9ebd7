"""The definition of agpt_vertex_normals_arrays in numpy (include/agpt.h, csrc/agpt_normals.h): float32 scalars, operation by operation,
the corners in their order.  Slow and plain on purpose: it is what the twin and the kernels are compared with, bit for bit."""
import numpy as np

F = np.float32


def _sub(a, b):
    return [F(a[0] - b[0]), F(a[1] - b[1]), F(a[2] - b[2])]


def _cross(a, b):
    return [F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0]))]


def _dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def face_vectors(vertices, indices):
    """g[t] = cross(p_b - p_a, p_c - p_a) of the corners 3t, 3t+1, 3t+2"""
    v = np.asarray(vertices, F).reshape(-1, 3)
    ix = np.asarray(indices, np.int32).reshape(-1, 3)
    g = []
    for t in range(len(ix) // 3):
        a, b, c = (v[ix[3 * t + k, 0]] for k in range(3))
        g.append(_cross(_sub(b, a), _sub(c, a)))
    return g


def corner_lists(indices, n_normals):
    """per normal item the corners that name it, ascending"""
    lists = [[] for _ in range(n_normals)]
    for q, j in enumerate(np.asarray(indices, np.int32).reshape(-1, 3)[:, 1]):
        lists[j].append(q)
    return lists


def vertex_normals_arrays(vertices, indices, n_normals, reverse=False):
    """-> normals[n_normals, 3].  reverse: every item's corners walked backwards -- NOT the definition; it exists so that a test can
    show that the order is observable."""
    with np.errstate(all="ignore"):
        g = face_vectors(vertices, indices)
        out = np.zeros((n_normals, 3), F)
        for j, corners in enumerate(corner_lists(indices, n_normals)):
            if not corners:
                continue
            if reverse:
                corners = corners[::-1]
            acc = list(g[corners[0] // 3])
            for q in corners[1:]:
                gt = g[q // 3]
                acc = [F(acc[0] + gt[0]), F(acc[1] + gt[1]), F(acc[2] + gt[2])]
            l2 = _dot(acc, acc)
            if not (l2 > 0) or not np.isfinite(l2):
                continue
            inv = F(F(1.0) / F(np.sqrt(l2)))
            out[j] = [F(acc[0] * inv), F(acc[1] * inv), F(acc[2] * inv)]
        return out
