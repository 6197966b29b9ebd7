"""numpy model of sampled texture lookups (include/agpt.h: agpt_scene_set_texture_sampler), fp32 operation by operation: the wrap
modes, the tap choice and the bilinear blend.  Builds on texture_model.py (uv interpolation, position, Mod)."""
import numpy as np

import texture_model as tm

F = np.float32
NEAREST, BILINEAR = 0, 1
REPEAT, CLAMP, MIRROR = 0, 1, 2
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def wrap(x, n, mode):
    """integer coordinate(s) x on an axis of n texels -> 0 .. n - 1"""
    x = np.asarray(x, np.int64)
    if mode == REPEAT:
        return tm.mod(x, n)
    if mode == CLAMP:
        return np.minimum(np.maximum(x, 0), n - 1)
    if mode == MIRROR:
        m = tm.mod(x, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    raise ValueError("wrap mode %r" % (mode,))


def _axis(s, n, mode, ok):
    """position s (fp32) -> the first tap's integer coordinate as the saturating float-to-int conversion gives it, the two wrapped
    tap coordinates, and fx = s - floor(s) in fp32 (0 where the conversion saturated, or the uv is not finite)"""
    with np.errstate(invalid="ignore", over="ignore"):
        fl = np.floor(s).astype(F)
        inside = ok & (np.abs(fl) < F(2.0 ** 31))
        f = np.where(inside, (s - fl).astype(F), F(0)).astype(F)
        x0 = np.where(ok, np.clip(np.where(np.isnan(fl), 0, fl).astype(np.float64), INT_MIN, INT_MAX), 0).astype(np.int64)
    return np.where(ok, wrap(x0, n, mode), 0), np.where(ok, wrap(x0 + 1, n, mode), 0), f


def taps(tex, u, v, filter=BILINEAR, wrap_u=REPEAT, wrap_v=REPEAT):
    """(x0, x1, y0, y1, fx, fy): the wrapped coordinates of the four taps (x0 | x1, y0 | y1) and the two weights.  NEAREST: x1 = x0,
    y1 = y0 and both weights 0.  A non-finite u or v: texel (0, 0) four times."""
    height, width = np.asarray(tex).shape[:2]
    u, v = np.asarray(u, F), np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore"):
        s, t = tm.texel_position((height, width), u, v)
    ok = np.isfinite(u) & np.isfinite(v)
    x0, x1, fx = _axis(s, width, wrap_u, ok)
    y0, y1, fy = _axis(t, height, wrap_v, ok)
    if filter == NEAREST:
        return x0, x0, y0, y0, np.zeros_like(fx), np.zeros_like(fy)
    if filter != BILINEAR:
        raise ValueError("filter %r" % (filter,))
    return x0, x1, y0, y1, fx, fy


def value(tex, u, v, filter=NEAREST, wrap_u=REPEAT, wrap_v=REPEAT):
    """tex[H, W, 3] -> rgb[..., 3]: NEAREST the texel; BILINEAR top = c00 + fx * (c10 - c00), bot = c01 + fx * (c11 - c01),
    c = top + fy * (bot - top), every operation rounded to fp32"""
    tex = np.asarray(tex, F)
    x0, x1, y0, y1, fx, fy = taps(tex, u, v, filter, wrap_u, wrap_v)
    c00 = tex[y0, x0]
    if filter == NEAREST:
        return c00
    c10, c01, c11 = tex[y0, x1], tex[y1, x0], tex[y1, x1]
    fx, fy = np.asarray(fx, F)[..., None], np.asarray(fy, F)[..., None]
    top = (c00 + (fx * (c10 - c00).astype(F)).astype(F)).astype(F)
    bot = (c01 + (fx * (c11 - c01).astype(F)).astype(F)).astype(F)
    return (top + (fy * (bot - top).astype(F)).astype(F)).astype(F)


def floor_flip_distance(tex, u, v):
    """distance, in texel units, of the lookup position from the nearest INTEGER position along either axis: where floor -- the tap
    choice of both filters -- flips (texture_model.boundary_distance under its other name)"""
    return tm.boundary_distance(np.asarray(tex).shape, u, v)
