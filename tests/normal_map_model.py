"""numpy model of tangent-space normal maps (include/agpt.h: agpt_scene_set_material_normal_texture), fp32 operation by operation,
every operation rounded on its own: the perturbation of the shading normal and the tangent agpt_host_scene.cpp stores per triangle."""
import numpy as np

F = np.float32


def _dot(a, b):
    """agpt_math.h dot: a.x * b.x + a.y * b.y + a.z * b.z, summed left to right"""
    return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)


def normalize(v):
    """agpt_math.h normalize: v * (1.0f / sqrtf(dot(v, v)))"""
    with np.errstate(all="ignore"):
        inv = (F(1) / np.sqrt(_dot(v, v).astype(F)).astype(F)).astype(F)
        return (v * inv[..., None]).astype(F)


def cross(a, b):
    """agpt_math.h cross"""
    def c(i, j):
        return ((a[..., i] * b[..., j]).astype(F) - (a[..., j] * b[..., i]).astype(F)).astype(F)
    return np.stack([c(1, 2), c(2, 0), c(0, 1)], -1)


def perturb(ns, ss, rgb, scale):
    """the perturbed shading normal [..., 3] of hits with shading normal ns, tangent ss (Surface::ss_bsdf) and texel rgb"""
    ns, ss, rgb = (np.asarray(a, F) for a in np.broadcast_arrays(np.asarray(ns, F), np.asarray(ss, F), np.asarray(rgb, F)))
    scale = F(scale)
    with np.errstate(all="ignore"):
        tx = (((F(2) * rgb[..., 0]).astype(F) - F(1)).astype(F) * scale).astype(F)
        ty = (((F(2) * rgb[..., 1]).astype(F) - F(1)).astype(F) * scale).astype(F)
        tz = ((F(2) * rgb[..., 2]).astype(F) - F(1)).astype(F)
        ts = cross(ns, ss)
        m = (((ss * tx[..., None]).astype(F) + (ts * ty[..., None]).astype(F)).astype(F) + (ns * tz[..., None]).astype(F)).astype(F)
        noop = (tx == 0) & (ty == 0) & (tz > 0)
        noop |= ~np.isfinite(m).all(-1)
        noop |= _dot(m, m).astype(F) == 0
        out = normalize(m)
    return np.where(noop[..., None], ns, out).astype(F)


def triangle_ss(mesh, tri):
    """normalize(dpdu) of the triangle whose index rows are tri, tri + 1, tri + 2 of mesh = (verts, normals, uvs, indices), as
    agpt_host_scene.cpp forms it (trianglemesh.cpp:46-80) for a triangle whose uvs are not degenerate"""
    verts, _, uvs, idx = mesh
    v0, v1, v2 = (np.asarray(verts, F)[idx[tri + k, 0]] for k in range(3))
    if uvs is None:
        uv0, uv1, uv2 = np.array([0, 0], F), np.array([1, 0], F), np.array([1, 1], F)
    else:
        uv0, uv1, uv2 = (np.asarray(uvs, F)[idx[tri + k, 2]] for k in range(3))
    du02, du12 = (uv0 - uv2).astype(F), (uv1 - uv2).astype(F)
    dp02, dp12 = (v0 - v2).astype(F), (v1 - v2).astype(F)
    det = F(F(du02[0] * du12[1]) - F(du02[1] * du12[0]))
    if not abs(float(det)) >= 1e-8:
        raise ValueError("triangle %d has degenerate uvs" % tri)
    invdet = F(F(1) / det)
    dpdu = (((du12[1] * dp02).astype(F) - (du02[1] * dp12).astype(F)).astype(F) * invdet).astype(F)
    return normalize(dpdu)
