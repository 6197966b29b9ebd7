"""A numpy model of agpt_denoise's contract (include/agpt.h): float32 operation by operation, a loop over the 25 taps in the
contract's order, vectorised over the pixels.  Buffers are [H, W, ...] in Accumulator::pixels order like the device's."""
import numpy as np

from adaptive_model import luminance

F = np.float32
KERNEL = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
ALBEDO_FLOOR = F(1e-3)
DEPTH_FLOOR = F(1e-3)
LUM_EPS = F(1e-6)
SIGMA_Z, SIGMA_N, SIGMA_L = 1.0, 0.25, 4.0   # AGPT_DENOISE_SIGMA_*


def expc(x):
    """(float)exp((double)x)"""
    return np.exp(np.asarray(x, F).astype(np.float64)).astype(F)


def albedo_floor(albedo):
    """max(albedo.rgb, 1e-3) as fmaxf: a NaN channel gives the floor"""
    return np.fmax(np.asarray(albedo, F)[..., :3], ALBEDO_FLOOR)


def prepare(accum, moment2, albedo, demodulate):
    """-> (c[H, W, 3], v[H, W]); v = -1 marks an excluded pixel (not n > 0)."""
    accum = np.asarray(accum, F)
    moment2 = np.asarray(moment2, F)
    n = accum[..., 3]
    with np.errstate(all="ignore"):
        c = accum[..., :3] / n[..., None]
        mu = luminance(accum[..., :3]) / n
        var = np.fmax(F(0), moment2 / n - mu * mu) * n / (n - F(1))   # (fmaxf: a NaN moment2 gives 0)
        v = np.where(n >= 2, var / n, F(0)).astype(F)
        if demodulate:
            al = albedo_floor(albedo)
            c = c / al
            la = luminance(al)
            v = v / (la * la)
    excluded = ~(n > 0)
    c = np.where(excluded[..., None], F(0), c).astype(F)
    v = np.where(excluded, F(-1), v).astype(F)
    return c, v


def shifted(a, oy, ox):
    """a[y + oy, x + ox] (wrapped: the caller masks the taps outside the film)"""
    return np.roll(a, (-oy, -ox), axis=(0, 1))


def run_pass(c, v, albedo, normal_depth, step, sigma_z=SIGMA_Z, sigma_n=SIGMA_N, sigma_l=SIGMA_L, return_weights=False,
             return_taps=False, expc=expc):
    """One a-trous pass at tap spacing `step` -> (c', v'); excluded pixels stay (0, -1).
    return_weights: also w[25, H, W], 0 where the tap is not used.  return_taps: also a dict of bool [25, H, W] masks in tap order
    -- inside (the tap lies on the film), mismatch (inside, another flag), excluded (inside, same flag, q without samples), use --
    and zden[H, W], ez's denominator.  expc: the exp to use (tests/denoise_cases.py passes one that flushes subnormals)."""
    c = np.asarray(c, F)
    v = np.asarray(v, F)
    albedo = np.asarray(albedo, F)
    nd = np.asarray(normal_depth, F)
    H, W = v.shape
    flag = albedo[..., 3]
    ns, t = nd[..., :3], nd[..., 3]
    Y = luminance(c)
    yy, xx = np.mgrid[0:H, 0:W]
    geometry = flag != 0
    with np.errstate(all="ignore"):
        lden = F(sigma_l) * np.sqrt(np.maximum(v, F(0))) + LUM_EPS
        zden = F(sigma_z) * F(step) * np.fmax(t, DEPTH_FLOOR)   # (fmaxf: a NaN t gives the floor)
        nden = F(sigma_n) * F(sigma_n)
        sw = np.zeros((H, W), F)
        sc = np.zeros((H, W, 3), F)
        sv = np.zeros((H, W), F)
        weights = []
        taps = dict(inside=[], mismatch=[], excluded=[], use=[])
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                inside = (yy + oy >= 0) & (yy + oy < H) & (xx + ox >= 0) & (xx + ox < W)
                cq, vq = shifted(c, oy, ox), shifted(v, oy, ox)
                same = shifted(flag, oy, ox) == flag
                use = inside & same & ~(vq < 0)
                if return_taps:
                    taps["inside"].append(inside)
                    taps["mismatch"].append(inside & ~same)
                    taps["excluded"].append(inside & same & (vq < 0))
                    taps["use"].append(use)
                ez = np.abs(t - shifted(t, oy, ox)) / zden
                d = ns - shifted(ns, oy, ox)
                en = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / nden
                ez = np.where(geometry, ez, F(0)).astype(F)
                en = np.where(geometry, en, F(0)).astype(F)
                el = np.abs(Y - shifted(Y, oy, ox)) / lden
                w = (KERNEL[dx + 2] * KERNEL[dy + 2]) * expc(-((ez + en) + el))
                w = np.where(use, w, F(0)).astype(F)
                weights.append(w)
                sw = np.where(use, sw + w, sw)
                sc = np.where(use[..., None], sc + w[..., None] * cq, sc)
                sv = np.where(use, sv + (w * w) * vq, sv)
        c2 = sc / sw[..., None]
        v2 = sv / (sw * sw)
    excluded = v < 0
    c2 = np.where(excluded[..., None], F(0), c2).astype(F)
    v2 = np.where(excluded, F(-1), v2).astype(F)
    extra = ()
    if return_weights:
        extra += (np.stack(weights),)
    if return_taps:
        extra += (dict({k: np.stack(m) for k, m in taps.items()}, zden=zden),)
    return (c2, v2) + extra


def finish(c, v, albedo, demodulate):
    """the state after the last pass -> out[H, W, 4]: re-modulated with demodulate, w = 1"""
    if demodulate:
        c = np.where((v < 0)[..., None], F(0), c * albedo_floor(albedo)).astype(F)
    out = np.ones(c.shape[:2] + (4,), F)
    out[..., :3] = c
    return out


def denoise(accum, moment2, albedo, normal_depth, iterations=5, demodulate=True, sigma_z=SIGMA_Z, sigma_n=SIGMA_N, sigma_l=SIGMA_L):
    """agpt_denoise -> out[H, W, 4]: rgb = the denoised mean radiance, w = 1."""
    assert 1 <= iterations <= 8
    c, v = prepare(accum, moment2, albedo, demodulate)
    for i in range(iterations):
        c, v = run_pass(c, v, albedo, normal_depth, 1 << i, sigma_z, sigma_n, sigma_l)
    return finish(c, v, albedo, demodulate)


def display_rmse(mean_rgb, reference_rgb):
    """RMSE on the display range (both clamped to [0, 1]), the metric of DESIGN.md section 5.4"""
    a = np.clip(np.asarray(mean_rgb, np.float64), 0, 1)
    b = np.clip(np.asarray(reference_rgb, np.float64), 0, 1)
    return float(np.sqrt(np.mean((a - b) ** 2)))
