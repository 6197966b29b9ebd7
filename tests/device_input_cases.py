"""Joint matrices and morph weights for the tests of the palette and the active list (test_skin_palette.py and test_morph_active.py on
the host, test_gpu_device_inputs.py on the GPU), and the numpy models of both: skin_model's inverse transpose laid out as the palette,
morph_model's skip rule as the list."""
import numpy as np

import skin_model

F = np.float32
NONE = 0xFFFFFFFF           # a status word without an offender
SUBNORMAL_DET, ZERO_DET = "tiny", "underflow"


def _affine(m3, t=(0, 0, 0)):
    m = np.eye(4)
    m[:3, :3] = m3
    m[:3, 3] = t
    return m.astype(F)


def _rotation(rs):
    q, r = np.linalg.qr(rs.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def joint_of(kind, rs):
    """one matrix of a class, last row (0, 0, 0, 1); every class but ZERO_DET has a palette of finite numbers"""
    if kind == "rotation":
        return _affine(_rotation(rs), rs.uniform(-8, 8, 3))
    if kind == "scale+shear":
        return _affine(np.diag(rs.uniform(0.2, 3.0, 3)) + np.triu(rs.uniform(-0.8, 0.8, (3, 3)), 1), rs.uniform(-2, 2, 3))
    if kind == "mirror":            # negative determinant
        return _affine(_rotation(rs) @ np.diag([-1.0, 1.3, 0.7]), rs.uniform(-1, 1, 3))
    if kind == SUBNORMAL_DET:       # det = 2^-127, a subnormal: its reciprocal 2^127 is finite, and so is N (2^42, 2^42, 2^43)
        return _affine(np.diag([2.0 ** -42, 2.0 ** -42, 2.0 ** -43]))
    if kind == ZERO_DET:            # det = 2^-150 rounds to exactly 0: singular, N is the identity
        return _affine(np.diag([2.0 ** -50] * 3))
    raise KeyError(kind)


REGULAR = ("rotation", "scale+shear", "mirror", SUBNORMAL_DET)


def joints(n, seed, kinds=REGULAR):
    """n matrices, the classes scattered over them by the seed (every class present from n = len(kinds) on) -> (mats[n, 4, 4], kinds[n])"""
    rs = np.random.RandomState(seed)
    order = [kinds[i] for i in rs.permutation(len(kinds))]
    names = [order[j % len(order)] if j < len(order) else kinds[rs.randint(len(kinds))] for j in range(n)]
    return np.stack([joint_of(k, rs) for k in names]), names


def model_palette(mats, with_normals):
    """skin_pack_palette's layout from skin_model.inverse_transpose: rows 0 .. 2 of M, then the 3x3 of N (21 floats), or M and a pad (13)"""
    mats = np.asarray(mats, F).reshape(-1, 4, 4)
    out = np.zeros((len(mats), 21 if with_normals else 13), F)
    out[:, :12] = mats[:, :3, :].reshape(-1, 12)
    if with_normals:
        for j, m in enumerate(mats):
            out[j, 12:] = skin_model.joint_normal_matrix(m).reshape(9)
    return out


def model_det(m):
    """the determinant the cofactor expansion computes for a DIAGONAL affine matrix, in float32: cell[0] * (cell[5] * cell[10] * cell[15])"""
    m = np.asarray(m, F)
    assert (m[:3, :3] == np.diag(np.diag(m[:3, :3]))).all() and (m[:3, 3] == 0).all()
    with np.errstate(under="ignore"):
        return m[0, 0] * (m[1, 1] * m[2, 2] * m[3, 3])


def model_active(weights):
    """morph_model.blend's rule as a list: the targets whose weight is not 0 (-0.0 == 0), in order"""
    w = np.asarray(weights, F).reshape(-1)
    t = np.flatnonzero(w != 0).astype(np.int32)
    return t, w[t]


def weight_patterns(T, seed=0):
    """name -> weights[T]: the patterns of the active-list tests"""
    rs = np.random.RandomState(seed + T)
    mixed = rs.uniform(-2.0, 3.0, T).astype(F)          # negative weights and weights above 1
    mixed[rs.rand(T) < 0.4] = 0
    mixed[::7] = F(-0.0)
    last = np.zeros(T, F)
    last[-1] = 0.75
    other = np.zeros(T, F)                              # every other target: crosses every wave and block boundary
    other[::2] = np.linspace(0.1, 1.9, len(other[::2]), dtype=F)
    return {"all-zero": np.zeros(T, F), "minus-zero": np.full(T, -0.0, F), "mixed": mixed, "last-only": last,
            "all-active": np.linspace(-1.5, 2.5, T, dtype=F) + F(0.001), "every-other": other}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
