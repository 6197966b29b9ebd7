"""The matrices the transform, skinning and morph tests share (test_transform_arrays.py on the host, the mesh-update tests on the GPU)."""
import numpy as np

F = np.float32


def rotation_translation():
    a, b = 0.7, -1.9
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = rz @ rx
    m[:3, 3] = [1.25, -0.3, 7.1]
    return m.astype(F)


MATRICES = {
    "rotation+translation": rotation_translation(),
    "scale+shear": np.array([[2.5, 0.3, 0, 0], [0, 0.4, -0.7, 0], [0.1, 0, -1.75, 0], [0, 0, 0, 1]], F),
    "projective": np.array([[1, 0.2, 0, 0.5], [0, 1.1, 0, 0], [0.3, 0, 0.9, -2], [0.01, -0.02, 0.03, 1.5]], F),   # w != 1
    "identity": np.eye(4, dtype=F),
}
