"""numpy model of image-texture lookups (include/agpt.h: agpt_scene_set_material_texture), fp32 operation by operation:
TriangleIntersect's uv interpolation (trianglemesh.cpp:46-57) and HDRTexture::value (texture.h:59-79: nearest texel, wrapped)."""
import numpy as np

F = np.float32


def interpolate_uv(uv0, uv1, uv2, b1, b2):
    """uv = uv0 * b0 + uv1 * b1 + uv2 * b2 with b0 = 1 - b1 - b2, every product and sum rounded to fp32, summed left to right.
    uv0..2: [..., 2], b1 / b2: [...] -> (u, v)"""
    uv0, uv1, uv2 = (np.asarray(a, F) for a in (uv0, uv1, uv2))
    b1, b2 = np.asarray(b1, F), np.asarray(b2, F)
    b0 = F(1) - b1 - b2
    u = uv0[..., 0] * b0 + uv1[..., 0] * b1 + uv2[..., 0] * b2
    v = uv0[..., 1] * b0 + uv1[..., 1] * b1 + uv2[..., 1] * b2
    return u.astype(F), v.astype(F)


def mod(a, b):
    """HDRTexture::Mod: a - (a / b) * b with C's truncating division, + b if negative"""
    a = np.asarray(a, np.int64)
    q = np.trunc(a / float(b)).astype(np.int64)
    r = a - q * b
    return np.where(r < 0, r + b, r)


def texel_position(shape, u, v):
    """(u * width - .5, v * height - .5) in fp32: the values whose floor picks the texel"""
    height, width = shape[:2]
    return (np.asarray(u, F) * F(width) - F(.5)).astype(F), (np.asarray(v, F) * F(height) - F(.5)).astype(F)


def texel_index(shape, u, v):
    """(x, y) of value(u, v); a non-finite coordinate reads texel (0, 0)"""
    height, width = shape[:2]
    s, t = texel_position(shape, u, v)
    ok = np.isfinite(np.asarray(u, F)) & np.isfinite(np.asarray(v, F))
    x = mod(np.floor(np.where(ok, s, 0)).astype(np.int64), width)
    y = mod(np.floor(np.where(ok, t, 0)).astype(np.int64), height)
    return np.where(ok, x, 0), np.where(ok, y, 0)


def value(tex, u, v):
    """tex[H, W, 3] -> rgb[..., 3]"""
    tex = np.asarray(tex, F)
    x, y = texel_index(tex.shape, u, v)
    return tex[y, x]


def boundary_distance(shape, u, v):
    """distance, in texel units, of the lookup position from the nearest texel boundary along either axis"""
    s, t = texel_position(shape, u, v)
    s, t = s.astype(np.float64), t.astype(np.float64)
    return np.minimum(np.abs(s - np.round(s)), np.abs(t - np.round(t)))
