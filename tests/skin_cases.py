"""Joints, bindings and meshes the skinning tests share (test_skin_arrays.py on the host, test_gpu_pose_mesh.py on the GPU)."""
import numpy as np

from transform_cases import MATRICES

F = np.float32
# a rotation + translation, a scale + shear and the identity
JOINTS3 = np.stack([MATRICES["rotation+translation"], MATRICES["scale+shear"], MATRICES["identity"]]).astype(F)
ALL_ZERO, MINUS_ZERO = 1, 0     # the vertices that binding() makes special


def binding(n, K, seed, n_joints=3):
    """(joints[n, K], weights[n, K]): seeded, about 30 % of the slots zeroed, the rest normalised in float32; vertex ALL_ZERO has
    no used slot and vertex MINUS_ZERO the value -0.0 in its last slot"""
    rs = np.random.RandomState(seed)
    J = rs.randint(0, n_joints, (n, K)).astype(np.int32)
    W = rs.rand(n, K).astype(F)
    W[rs.rand(n, K) < 0.3] = 0
    total = W.sum(1, dtype=F, keepdims=True)
    W = (W / np.where(total > 0, total, F(1))).astype(F)
    W[ALL_ZERO] = 0
    W[MINUS_ZERO, K - 1] = F(-0.0)
    assert np.signbit(W[MINUS_ZERO, K - 1]) and (W >= 0).all() and np.isfinite(W).all()
    return J, W


def single_slot(n, K, joint, slots, weight):
    """every vertex bound to `joint` with `weight` in each of `slots`, the other slots zero (and naming other joints)"""
    J = np.full((n, K), (joint + 1) % 3, np.int32)
    W = np.zeros((n, K), F)
    for s in slots:
        J[:, s] = joint
        W[:, s] = weight
    return J, W


def flat_shaded(v, tris):
    """one normal per triangle of the corner list `tris`: n_normals = n_triangles != n_vertices"""
    t = np.asarray(tris, np.int32).reshape(-1, 3)
    p = v.astype(np.float64)
    n = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)
