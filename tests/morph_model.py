"""A numpy model of morph targets as include/agpt.h defines them for agpt_morph_arrays / agpt_scene_morph_mesh: float32 throughout, one
rounding per operation, the targets in order, a target of weight 0 (either sign) skipped.  It calls nothing of the library; tests compare
the library's bytes with its.  morph_then_skin composes it with skin_model.skin_arrays: glTF's order."""
import numpy as np

import skin_model

F = np.float32


def blend(rest, deltas, weights):
    """acc = rest; for every target t with w[t] != 0, in order: acc = acc + w[t] * deltas[t] (the product rounds, then the sum)"""
    acc = np.array(rest, F).reshape(-1, 3)
    deltas = np.asarray(deltas, F).reshape(len(weights), len(acc), 3)
    for t, w in enumerate(np.asarray(weights, F)):
        if w == 0:                          # -0.0 == 0: skipped as well
            continue
        with np.errstate(all="ignore"):
            term = (w * deltas[t]).astype(F)
            acc = (acc + term).astype(F)
    return acc


def morph_arrays(weights, verts, position_deltas, normals=None, normal_deltas=None):
    v = blend(verts, position_deltas, weights)
    if normals is None:
        return v, None
    if normal_deltas is None:
        return v, np.array(normals, F).reshape(-1, 3)      # the rest normals
    return v, blend(normals, normal_deltas, weights)


def morph_then_skin(weights, matrices, verts, position_deltas, joints, skin_weights, normals=None, normal_deltas=None, normal_joints=None,
                    normal_weights=None):
    v, n = morph_arrays(weights, verts, position_deltas, normals, normal_deltas)
    return skin_model.skin_arrays(matrices, v, joints, skin_weights, n, normal_joints, normal_weights)
