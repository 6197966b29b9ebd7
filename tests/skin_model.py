"""A numpy model of linear-blend skinning as include/agpt.h defines it for agpt_skin_arrays / agpt_scene_pose_mesh: float32 throughout,
one rounding per operation, sums left to right.  It calls nothing of the library; tests compare the library's bytes with its."""
import numpy as np

F = np.float32


def transform_point(M, v):
    """rows 0..2 of M applied to (x, y, z, 1); divided by row 3's w unless w == 1"""
    M = np.asarray(M, F)
    x, y, z = (v[:, i].astype(F) for i in range(3))
    with np.errstate(all="ignore"):
        r = [M[i, 0] * x + M[i, 1] * y + M[i, 2] * z + M[i, 3] for i in range(4)]
        out = np.stack(r[:3], 1).astype(F)
        m = r[3] != 1
        out[m] = out[m] * (F(1) / r[3][m])[:, None]
    return out


def transform_vector(N, v):
    N = np.asarray(N, F)
    x, y, z = (v[:, i].astype(F) for i in range(3))
    with np.errstate(all="ignore"):
        return np.stack([N[i, 0] * x + N[i, 1] * y + N[i, 2] * z for i in range(3)], 1).astype(F)


def inverse_transpose(M):
    """the 3x3 transpose of the inverse of M by the cofactor expansion (gluInvertMatrix's, on the row-major cells): the cofactors the
    3x3 and the determinant need, det = cell[0] * inv[0] + cell[1] * inv[4] + cell[2] * inv[8] + cell[3] * inv[12], each cofactor times
    1 / det; the identity when det is exactly 0"""
    cell = [F(x) for x in np.asarray(M, F).reshape(16)]
    inv = {}
    with np.errstate(all="ignore"):
        inv[0] = cell[5] * cell[10] * cell[15] - cell[5] * cell[11] * cell[14] - cell[9] * cell[6] * cell[15] + cell[9] * cell[7] * cell[14] + cell[13] * cell[6] * cell[11] - cell[13] * cell[7] * cell[10]
        inv[1] = -cell[1] * cell[10] * cell[15] + cell[1] * cell[11] * cell[14] + cell[9] * cell[2] * cell[15] - cell[9] * cell[3] * cell[14] - cell[13] * cell[2] * cell[11] + cell[13] * cell[3] * cell[10]
        inv[2] = cell[1] * cell[6] * cell[15] - cell[1] * cell[7] * cell[14] - cell[5] * cell[2] * cell[15] + cell[5] * cell[3] * cell[14] + cell[13] * cell[2] * cell[7] - cell[13] * cell[3] * cell[6]
        inv[4] = -cell[4] * cell[10] * cell[15] + cell[4] * cell[11] * cell[14] + cell[8] * cell[6] * cell[15] - cell[8] * cell[7] * cell[14] - cell[12] * cell[6] * cell[11] + cell[12] * cell[7] * cell[10]
        inv[5] = cell[0] * cell[10] * cell[15] - cell[0] * cell[11] * cell[14] - cell[8] * cell[2] * cell[15] + cell[8] * cell[3] * cell[14] + cell[12] * cell[2] * cell[11] - cell[12] * cell[3] * cell[10]
        inv[6] = -cell[0] * cell[6] * cell[15] + cell[0] * cell[7] * cell[14] + cell[4] * cell[2] * cell[15] - cell[4] * cell[3] * cell[14] - cell[12] * cell[2] * cell[7] + cell[12] * cell[3] * cell[6]
        inv[8] = cell[4] * cell[9] * cell[15] - cell[4] * cell[11] * cell[13] - cell[8] * cell[5] * cell[15] + cell[8] * cell[7] * cell[13] + cell[12] * cell[5] * cell[11] - cell[12] * cell[7] * cell[9]
        inv[9] = -cell[0] * cell[9] * cell[15] + cell[0] * cell[11] * cell[13] + cell[8] * cell[1] * cell[15] - cell[8] * cell[3] * cell[13] - cell[12] * cell[1] * cell[11] + cell[12] * cell[3] * cell[9]
        inv[10] = cell[0] * cell[5] * cell[15] - cell[0] * cell[7] * cell[13] - cell[4] * cell[1] * cell[15] + cell[4] * cell[3] * cell[13] + cell[12] * cell[1] * cell[7] - cell[12] * cell[3] * cell[5]
        inv[12] = -cell[4] * cell[9] * cell[14] + cell[4] * cell[10] * cell[13] + cell[8] * cell[5] * cell[14] - cell[8] * cell[6] * cell[13] - cell[12] * cell[5] * cell[10] + cell[12] * cell[6] * cell[9]
        det = cell[0] * inv[0] + cell[1] * inv[4] + cell[2] * inv[8] + cell[3] * inv[12]
        if det == 0:
            return np.eye(3, dtype=F)
        invdet = F(1) / det
        full = {i: c * invdet for i, c in inv.items()}
    # the transpose: N[r][c] = inverse[c][r]
    return np.array([[full[0], full[4], full[8]], [full[1], full[5], full[9]], [full[2], full[6], full[10]]], F)


_INVERSES = {}


def joint_normal_matrix(M):
    key = np.asarray(M, F).tobytes()
    if key not in _INVERSES:
        _INVERSES[key] = inverse_transpose(M)
    return _INVERSES[key]


def blend(apply, mats, rest, joints, weights):
    """the walk over the slots: apply(mats[j], rows) is the joint's transform of the rest rows"""
    rest = np.ascontiguousarray(rest, F)
    joints, weights = np.asarray(joints), np.asarray(weights, F)
    acc = rest.copy()
    started = np.zeros(len(rest), bool)
    for k in range(joints.shape[1]):
        w = weights[:, k]
        use = w != 0                       # -0.0 == 0: skipped as well
        q = np.zeros_like(rest)
        for j in np.unique(joints[use, k]):
            s = use & (joints[:, k] == j)
            q[s] = apply(mats[j], rest[s])
        with np.errstate(all="ignore"):
            term = (w[:, None] * q).astype(F)
            first, later = use & ~started, use & started
            acc[first] = term[first]
            acc[later] = (acc[later] + term[later]).astype(F)
        started |= use
    return acc


def skin_arrays(matrices, verts, joints, weights, normals=None, normal_joints=None, normal_weights=None):
    mats = np.asarray(matrices, F).reshape(-1, 4, 4)
    v = blend(transform_point, mats, verts, joints, weights)
    if normals is None:
        return v, None
    if normal_joints is None:
        assert len(normals) == len(verts)
        normal_joints, normal_weights = joints, weights
    used = np.unique(np.asarray(normal_joints)[np.asarray(normal_weights, F) != 0])
    nmats = {int(j): joint_normal_matrix(mats[j]) for j in used}
    return v, blend(transform_vector, nmats, normals, normal_joints, normal_weights)
