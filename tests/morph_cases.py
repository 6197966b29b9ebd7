"""Targets and weights the morph tests share (test_morph_arrays.py on the host, test_gpu_morph_mesh.py on the GPU)."""
import numpy as np

F = np.float32
SINGLE_ITEM = 0      # the item that the single-item target moves


def zero_target(T):
    """the target whose deltas are all zero (T >= 2), or None"""
    return 1 if T >= 2 else None


def single_target(T):
    """the target that touches item SINGLE_ITEM only (T >= 3), or None"""
    return 2 if T >= 3 else None


def targets(n, T, seed, extent=2.0):
    """deltas[T, n, 3]: seeded, about a tenth of `extent` (the mesh's size); target zero_target(T) is all zero and target
    single_target(T) moves item SINGLE_ITEM alone"""
    rs = np.random.RandomState(seed)
    d = (rs.uniform(-1, 1, (T, n, 3)) * (0.1 * extent)).astype(F)
    if zero_target(T) is not None:
        d[zero_target(T)] = 0
    if single_target(T) is not None:
        keep = d[single_target(T), SINGLE_ITEM].copy()
        d[single_target(T)] = 0
        d[single_target(T), SINGLE_ITEM] = keep
    return d


def weights(T, seed, active):
    """w[T]: the targets of `active` non-zero -- the first of them negative, the second above 1, the others in (0.2, 0.9) --, every other
    one zero, the first of those -0.0"""
    rs = np.random.RandomState(seed)
    w = np.zeros(T, F)
    values = [F(-0.625), F(1.375)] + list(rs.uniform(0.2, 0.9, T).astype(F))
    active = list(active)
    for k, t in enumerate(active):
        w[t] = values[k]
    idle = [t for t in range(T) if t not in active]
    if idle:
        w[idle[0]] = F(-0.0)
        assert np.signbit(w[idle[0]])
    assert np.isfinite(w).all() and int((w != 0).sum()) == len(active)
    return w


ACTIVE_SETS = {"none": lambda T: [], "first": lambda T: [0], "last": lambda T: [T - 1], "all": lambda T: list(range(T))}
