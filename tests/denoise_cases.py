"""Seeded synthetic inputs of agpt_denoise and a census of what they exercise (no GPU needed): the denoiser's counterpart of
ray_edge_cases.py / shade_edge_cases.py.

Render buffers choose their own values, so the filter tests on rendered scenes (tests/test_gpu_denoise.py) never see a floor of the
contract (include/agpt.h) hit exactly, a count that is not a positive integer, a clamped variance, flags mixed pixel by pixel, a tap
weight that is an fp32 subnormal, or a film narrower than the tap reach.  synthetic_inputs() builds all of that into films of any
size, down to one pixel; census() runs tests/denoise_model.py pass by pass and counts how often each case occurs, so that
tests/test_denoise_cases.py can demand that none of them is empty before tests/test_gpu_denoise_edges.py compares the kernels with the
model on them.
"""
import numpy as np

import denoise_model as dm
from adaptive_model import luminance

F = np.float32
TINY = np.finfo(F).tiny                      # the smallest normal fp32
FLOOR = F(1e-3)                              # the albedo floor and the depth floor
BELOW, ABOVE = np.nextafter(FLOOR, F(0)), np.nextafter(FLOOR, F(1))
COUNTS = np.array([0.0, -0.0, -1.0, 0.5, 1.0, 1.5, 2.0, 2.75, 4.0, 16.0, 1024.0], F)
ALBEDO_CASES = (F(0), F(-0.5), F(5e-4), BELOW, FLOOR, ABOVE)
DEPTH_CASES = (F(0), F(1e-30), F(5e-4), FLOOR, ABOVE)
BLACK_DEPTHS = (F(0.04), F(0.02))            # against depths near 4: ez = 99 / spacing and 198 / spacing
HUGE_MOMENT2 = F(1e30)
MAIN = (37, 29)                             # the main film: (W, H)
MAIN_ITERATIONS = 5
SIGMAS = (dm.SIGMA_Z, dm.SIGMA_N, dm.SIGMA_L)
# (W, H) of tests/test_gpu_denoise_edges.py: one pixel, one row, one column, below / at / one past the 64-pixel tile of k_denoise_pass,
# heights that are no multiple of its 4 rows, films narrower than the reach of the wider spacings
SHAPES = ((1, 1), (1, 9), (9, 1), (2, 2), (5, 3), (63, 5), (64, 4), (65, 5), MAIN, (130, 3), (3, 130), (129, 9))


def shape_seed(W, H):
    return 1000 * W + H


def synthetic_inputs(W, H, seed):
    """-> (accum[H, W, 4], moment2[H, W], albedo[H, W, 4], normal_depth[H, W, 4]), fp32, read-only"""
    rng = np.random.RandomState(seed)
    u = lambda *shape: rng.uniform(size=shape)
    # flags mixed pixel by pixel; colour (1, 1, 1) where the flag is not 1
    flag = rng.choice([0.0, 1.0, 2.0], size=(H, W), p=[0.2, 0.6, 0.2]).astype(F)
    albedo = np.ones((H, W, 4), F)
    albedo[..., :3] = np.where((flag == 1)[..., None], rng.uniform(0.05, 0.95, (H, W, 3)), 1.0)
    albedo[..., 3] = flag
    # normals near one direction, 15 % anywhere on the sphere: en from 0 to 4 / sigma_n^2
    base = np.array([0.3, 0.8, 0.52])
    ns = base + rng.normal(0, 0.05, (H, W, 3))
    anywhere = u(H, W) < 0.15
    ns = np.where(anywhere[..., None], rng.normal(size=(H, W, 3)), ns)
    ns /= np.linalg.norm(ns, axis=-1, keepdims=True)
    # depths within 3 % of 4, 20 % anywhere in [0.5, 400]: ez from 0 to a hundred at spacing 1
    t = 4.0 * (1.0 + rng.uniform(-0.03, 0.03, (H, W)))
    t = np.where(u(H, W) < 0.2, rng.uniform(0.5, 400.0, (H, W)), t)
    nd = np.zeros((H, W, 4), F)
    nd[..., :3] = ns
    nd[..., 3] = t
    nd[flag == 0] = 0                        # a miss: zero normal, t = 0
    # counts, mean radiance (a tenth of the pixels 50 times brighter), second moment mu^2 + a spread in [0, 30] (skewed to 0)
    n = COUNTS[rng.randint(len(COUNTS), size=(H, W))]
    mean = rng.uniform(0.1, 1.0, (H, W, 3)) * np.where(u(H, W) < 0.1, 50.0, 1.0)[..., None]
    accum = np.zeros((H, W, 4), F)
    accum[..., :3] = mean * np.where(n > 0, n, 1.0)[..., None]
    accum[..., 3] = n
    with np.errstate(all="ignore"):
        mu = luminance(accum[..., :3]).astype(np.float64) / np.where(n > 0, n, 1.0)
    spread = 30.0 * u(H, W) ** 4
    moment2 = ((mu * mu + spread) * np.where(n > 0, n, 1.0)).astype(F)
    moment2[u(H, W) < 0.15] = 0              # moment2 / n below mu^2: the clamp
    # the floor cases, last, into cells of their own (as many as the film has room for): flag 1, 4 samples
    cells = rng.permutation(W * H)[:len(ALBEDO_CASES) + len(DEPTH_CASES) + len(BLACK_DEPTHS) + 1]
    ys, xs = np.unravel_index(cells, (H, W))
    for k, (y, x) in enumerate(zip(ys, xs)):
        albedo[y, x, 3] = 1
        if nd[y, x, 3] == 0:
            nd[y, x] = (*(base / np.linalg.norm(base)), 4.0)
        accum[y, x] = (*(4.0 * mean[y, x]), 4.0)
        moment2[y, x] = 4.0 * (luminance(mean[y, x].astype(F)) ** 2 + 0.5)
        if k < len(ALBEDO_CASES):
            albedo[y, x, :3] = rng.uniform(0.05, 0.95, 3)
            albedo[y, x, k % 3] = ALBEDO_CASES[k]
        elif k < len(ALBEDO_CASES) + len(DEPTH_CASES):
            nd[y, x, 3] = DEPTH_CASES[k - len(ALBEDO_CASES)]
        elif k == len(ALBEDO_CASES) + len(DEPTH_CASES) + len(BLACK_DEPTHS):
            moment2[y, x] = HUGE_MOMENT2             # v about 1e29: sv / (sw * sw) and w * w * v_q far from 1, still finite
        else:
            # black, noisy (el small) and a hundred times nearer than the pixels around it: at one spacing ez is about 99 for them,
            # every tap but the centre weighs an fp32 subnormal, and the pixel's output is those weights times their radiance
            # alone -- a subnormal itself, zero if anything on the way flushes
            accum[y, x] = (0, 0, 0, 2)
            moment2[y, x] = 60
            nd[y, x] = (*(base / np.linalg.norm(base)), BLACK_DEPTHS[k - len(ALBEDO_CASES) - len(DEPTH_CASES)])
    out = (accum, moment2, albedo, nd)
    for a in out:
        a.setflags(write=False)
    return out


def _pass_with_flushed_exp(*args):
    """dm.run_pass with an expc whose subnormal results are zero: what a flushing device would compute from the same state"""
    def flushing_expc(x):
        e = dm.expc(x)
        return np.where(e < TINY, F(0), e).astype(F)
    return dm.run_pass(*args, expc=flushing_expc)


def census(inputs, iterations, demodulate, sigmas=SIGMAS):
    """{class: count} over the model's `iterations` passes on `inputs`, and the model's output under "output"."""
    accum, moment2, albedo, nd = inputs
    n, flag, t = accum[..., 3], albedo[..., 3], nd[..., 3]
    H, W = n.shape
    out = {}
    c, v = dm.prepare(accum, moment2, albedo, demodulate)
    live = ~(v < 0)                          # pixels that run their taps (k_denoise_pass returns early for the others)
    out["variance_huge"] = int((v > F(1e20)).sum())
    out["variance_huge_after_the_passes"] = 0
    names = ("taps_flag_mismatch", "taps_excluded", "weights_subnormal", "weights_zero", "weights_small")
    out.update({k: 0 for k in names})
    neighbour = np.zeros((H, W), bool)
    out["weights_subnormal_on_bright_taps"] = 0
    for i in range(iterations):
        s = 1 << i
        bright = np.stack([dm.shifted(luminance(c) > 10, dy * s, dx * s) for dy in range(-2, 3) for dx in range(-2, 3)])
        flushed = _pass_with_flushed_exp(c, v, albedo, nd, s, *sigmas)
        c, v, w, m = dm.run_pass(c, v, albedo, nd, s, *sigmas, return_weights=True, return_taps=True)
        if i < len(BLACK_DEPTHS):              # (the spacings the black cells are made for; a later pass swamps what they left)
            out["pixels_decided_by_subnormal_weights_at_spacing_%d" % s] = int(((flushed[0] != c).any(-1) | (flushed[1] != v)).sum())
        out["variance_huge_after_the_passes"] += int((v > F(1e20)).sum())
        out["taps_flag_mismatch"] += int((m["mismatch"] & live).sum())
        out["taps_excluded"] += int((m["excluded"] & live).sum())
        out["taps_outside_spacing_%d" % (1 << i)] = int((~m["inside"]).sum())
        use = m["use"] & live
        out["weights_subnormal"] += int((use & (w > 0) & (w < TINY)).sum())
        out["weights_subnormal_on_bright_taps"] += int((use & (w > 0) & (w < TINY) & bright).sum())
        out["weights_zero"] += int((use & (w == 0)).sum())
        out["weights_small"] += int((use & (w >= TINY) & (w < F(1e-3))).sum())
        off_centre = np.ones(25, bool)
        off_centre[12] = False
        neighbour |= use[off_centre].any(0)
    rgb = albedo[..., :3]
    out["albedo_zero"] = int((rgb == 0).sum())
    out["albedo_negative"] = int((rgb < 0).sum())
    out["albedo_below_floor"] = int((rgb < FLOOR).sum())
    out["albedo_at_floor"] = int((rgb == FLOOR).sum())
    out["albedo_above_floor"] = int((rgb > FLOOR).sum())
    out["albedo_next_below_floor"] = int((rgb == BELOW).sum())
    out["albedo_next_above_floor"] = int((rgb == ABOVE).sum())
    geometry = flag != 0
    out["depth_zero_on_geometry"] = int((geometry & (t == 0)).sum())
    out["depth_below_floor"] = int((geometry & (t < FLOOR)).sum())
    out["depth_at_floor"] = int((geometry & (t == FLOOR)).sum())
    out["depth_above_floor"] = int((geometry & (t > FLOOR)).sum())
    out["depth_next_above_floor"] = int((geometry & (t == ABOVE)).sum())
    out["count_le_0"] = int((n <= 0).sum())
    out["count_minus_zero"] = int(((n == 0) & np.signbit(n)).sum())
    out["count_negative"] = int((n < 0).sum())
    out["count_0_to_1"] = int(((n > 0) & (n < 1)).sum())
    out["count_1"] = int((n == 1).sum())
    out["count_1_to_2"] = int(((n > 1) & (n < 2)).sum())
    out["count_ge_2"] = int((n >= 2).sum())
    with np.errstate(all="ignore"):
        mu = luminance(accum[..., :3]) / n
        out["variance_clamped"] = int(((n >= 2) & (moment2 / n - mu * mu < 0)).sum())
    for f in (0, 1, 2):
        out["flag_%d" % f] = int((flag == f).sum())
        out["flag_%d_with_a_used_neighbour" % f] = int(((flag == f) & neighbour).sum())
    out["output"] = dm.finish(c, v, albedo, demodulate)
    return out


def nan_case(kind, W=MAIN[0], H=MAIN[1]):
    """-> (inputs with one NaN, the same inputs with the value the contract states in its place, the pixel)"""
    accum, moment2, albedo, nd = [a.copy() for a in synthetic_inputs(W, H, shape_seed(W, H))]
    ok = (albedo[..., 3] == 1) & (accum[..., 3] >= 2) & (moment2 > 0) & (nd[..., 3] > 1)
    y, x = np.argwhere(ok)[len(np.argwhere(ok)) // 2]
    stated = [accum.copy(), moment2.copy(), albedo.copy(), nd.copy()]
    if kind == "count":
        accum[y, x, 3] = np.nan
        stated[0][y, x, 3] = 0                          # not n > 0: excluded
    elif kind == "albedo":
        albedo[y, x, 1] = np.nan
        stated[2][y, x, 1] = FLOOR
    elif kind == "moment2":
        moment2[y, x] = np.nan
        stated[1][y, x] = 0                             # max(0, -mu^2) = 0: a variance of 0
    else:
        nd[y, x, 3] = np.nan
        stated[3][y, x, 3] = FLOOR
    return (accum, moment2, albedo, nd), tuple(stated), (y, x)


def same_but_for_nan_payloads(a, b):
    """the same non-finite mask, and the same bytes wherever finite"""
    bad = ~np.isfinite(a)
    return np.array_equal(bad, ~np.isfinite(b)) and np.where(bad, F(0), a).tobytes() == np.where(bad, F(0), b).tobytes()
