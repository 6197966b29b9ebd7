"""Seeded inputs for the tests of agpt_temporal_accumulate_clamped: the stale-shadow frame (a uniformly lit flat film whose history
still holds a shadow on a disc) and synthetic frames that hold every case of the contract's step 5' -- chosen here, on the CPU, so
that the census the GPU test takes from the model's masks holds."""
import numpy as np

import ag_pathtracer_amd as ag
import motion_model as mm
import temporal_model as tm
from adaptive_model import luminance
from helpers import film_point, unit

F = np.float32

# ---- the stale-shadow frame ------------------------------------------------------------------------------------------------------
SW, SH = 37, 29
SHADOW_CAM = ([0.3, 1.4, -6.0], [0, 0, 0], [0, 1, 0], SW / float(SH), 42.0, 0.0)
SHADOW_DISC = ((18, 14), 6)          # centre (column, buffer row) and radius: 113 pixels
LIT, SHADOWED, SAMPLE_SD, N_CUR, N_HIST = 1.0, 0.1, 0.3, 4, 32


def stale_shadow(seed=11):
    """(cur, prev, disc): flat grey geometry seen by a static camera.  Now: 4 samples a pixel of mean 1.0 and standard deviation 0.3
    (grey: r = g = b).  The history: 32 samples a pixel of mean 1.0, except 0.1 on the disc -- the shadow that is no longer there."""
    rng = np.random.RandomState(seed)
    samples = rng.normal(LIT, SAMPLE_SD, (N_CUR, SH, SW)).clip(0, None).astype(F)
    accum = np.zeros((SH, SW, 4), F)
    accum[..., :3] = samples.sum(0, dtype=F)[..., None]
    accum[..., 3] = N_CUR
    grey = luminance(np.ones(3, F))
    m2 = ((samples * grey) ** 2).sum(0, dtype=F)
    albedo = np.ones((SH, SW, 4), F)
    nd = np.zeros((SH, SW, 4), F)
    nd[..., 1] = 1
    nd[..., 3] = 5
    (cx, cy), rad = SHADOW_DISC
    rr, cc = np.mgrid[0:SH, 0:SW]
    disc = (rr - cy) ** 2 + (cc - cx) ** 2 <= rad * rad
    mean = np.where(disc, F(SHADOWED), F(LIT)).astype(F)
    h_acc = np.zeros((SH, SW, 4), F)
    h_acc[..., :3] = (mean * F(N_HIST))[..., None]
    h_acc[..., 3] = N_HIST
    sd = np.where(disc, F(SAMPLE_SD * SHADOWED), F(SAMPLE_SD))
    h_m2 = (F(N_HIST) * ((mean * grey) ** 2 + (sd * grey) ** 2)).astype(F)
    return (accum, m2, albedo, nd), (h_acc, h_m2, albedo.copy(), nd.copy()), disc


def mean_luminance(hist_accum, where):
    a = np.asarray(hist_accum, np.float64)
    return float((luminance((a[..., :3] / a[..., 3:4]).astype(F))[where]).mean())


# ---- synthetic frames ------------------------------------------------------------------------------------------------------------
CAM_CUR = ([0.3, 1.4, -6.0], [0.0, 0.0, 0.0], [0, 1, 0], 37 / 19.0, 42.0, 0.0)
CAM_PREV = ([0.45, 1.3, -5.7], [0.2, 0.1, 0.0], [0.02, 1, 0], 37 / 19.0, 42.0, 0.0)
MAX_HISTORY, DEPTH_TOL, NORMAL_COS = 10.0, 0.0625, 0.9
GAMMA, CLAMPED_MAX_HISTORY = 1.0, 6.0
FILMS = [(1, 1), (5, 3), (37, 19), (70, 9)]
LONE_FLAG = 5.0


def synthetic(W, H, cameras, motion, seed=20251020):
    """(cur, prev, prev_point or None, cam_prev).  cameras: "equal" / "different"; motion: whether prev_point is given (w = 1 on some
    40 % of the pixels, their points on the previous film).  The previous frame's features are made coherent where most pixels land,
    so that their history is accepted.  On films of 30 pixels or more, planted by hand: an empty pixel in an empty 7 x 7 patch (k == 0
    with history), a pixel with a flag of its own (k == 1, sd == 0), a NaN current pixel (NaN bounds around it) and a NaN history
    channel."""
    rng = np.random.RandomState(seed + 131 * W + H)
    cam_prev = CAM_PREV if cameras == "different" else CAM_CUR
    va, vb = ag.camera_vectors(CAM_CUR), ag.camera_vectors(cam_prev)
    P = tm.camera(vb)
    big = W * H >= 30
    flag = rng.choice([0.0, 1.0, 2.0], size=(H, W), p=[0.15, 0.7, 0.15]).astype(F)
    n_c = np.where(rng.uniform(size=(H, W)) < 0.08, 0.0, 4.0).astype(F)
    if W * H == 1:
        flag[...], n_c[...] = 1, 4
    lone = empty = nan_cur = None
    if big:
        empty = (W // 4, H // 2)                             # (column, row) of the pixel whose whole window is empty
        n_c[max(empty[1] - 3, 0):empty[1] + 4, empty[0] - 3:empty[0] + 4] = 0
        lone = (W // 2, H // 2)
        flag[lone[1], lone[0]] = LONE_FLAG
        n_c[lone[1], lone[0]] = 4
        nan_cur = (3 * W // 4, H // 2)
        n_c[nan_cur[1], nan_cur[0]] = 4
        flag[nan_cur[1] - 1:nan_cur[1] + 2, nan_cur[0] - 1:nan_cur[0] + 2] = 1
    geometry = flag != 0
    albedo = np.ones((H, W, 4), F)
    albedo[..., :3] = rng.uniform(0.1, 1.0, (H, W, 3))
    albedo[..., :3][rng.uniform(size=(H, W)) < 0.05] = 0      # below the demodulation floor
    albedo[..., 3] = flag
    nd = np.zeros((H, W, 4), F)
    nd[..., :3] = np.where(geometry[..., None], unit(rng.normal(size=(H, W, 3))), 0)
    nd[..., 3] = np.where(geometry, rng.uniform(3.0, 9.0, (H, W)), 0)
    accum = np.zeros((H, W, 4), F)
    accum[..., :3] = rng.uniform(0.5, 1.5, (H, W, 3)) * albedo[..., :3].clip(0.05, None) * n_c[..., None]
    accum[..., 3] = n_c
    m2 = (rng.uniform(0, 6, (H, W)) * n_c).astype(F)
    if big:
        accum[nan_cur[1], nan_cur[0], :3] = np.nan

    p_albedo = np.ones((H, W, 4), F)
    p_albedo[..., 3] = rng.choice([0.0, 1.0, 2.0], size=(H, W))
    p_nd = np.zeros((H, W, 4), F)
    p_nd[..., :3] = unit(rng.normal(size=(H, W, 3)))
    p_nd[..., 3] = rng.uniform(3.0, 9.0, (H, W))
    n_q = rng.choice([0.0, 1.5, 3.0, 8.0, 12.25], size=(H, W), p=[0.08, 0.23, 0.23, 0.23, 0.23]).astype(F)
    # the history's mean: close to what the frame says now for some 40 % of the pixels (kept), anywhere in [0, 2] x albedo for the rest
    close = rng.uniform(size=(H, W, 1)) < 0.4
    level = np.where(close, rng.uniform(0.97, 1.03, (H, W, 3)), rng.uniform(0.0, 2.0, (H, W, 3)))
    h_acc = np.zeros((H, W, 4), F)
    h_acc[..., :3] = level * albedo[..., :3].clip(0.05, None) * n_q[..., None]
    h_acc[..., 3] = n_q
    h_m2 = (rng.uniform(0, 6, (H, W)) * n_q).astype(F)

    pp = None
    if motion:
        pp = np.zeros((H, W, 4), F)
        pp[..., 3] = rng.choice(np.array([0.0, 1.0, 2.0], F), size=(H, W), p=[0.1, 0.4, 0.5])
        if W * H == 1:
            pp[..., 3] = 1
        for r in range(H):
            for c in range(W):
                pp[r, c, :3] = film_point(P, rng.uniform(0.02, 0.98), rng.uniform(0.02, 0.98), rng.uniform(3.0, 9.0))
        pos, _ = mm.position(va, vb, cameras == "equal", flag, nd[..., 3], pp, W, H)
    else:
        pos = tm.position(va, vb, cameras == "equal", flag, nd[..., 3], W, H)
    planted = [p for p in (lone, empty) if p is not None]
    coherent = pos["found"] & (rng.uniform(size=(H, W)) < 0.85)
    order = [(r, c) for r, c in zip(*np.nonzero(coherent)) if (c, r) not in planted] + [(r, c) for c, r in planted if pos["found"][r, c]]
    one = F(1)
    weights = ((one - pos["fx"]) * (one - pos["fy"]), pos["fx"] * (one - pos["fy"]), (one - pos["fx"]) * pos["fy"], pos["fx"] * pos["fy"])
    for r, c in order:                                        # (the planted pixels last: nobody overwrites their taps)
        for tap in range(4):
            qx, qy = pos["x0"][r, c] + (tap & 1), pos["y0"][r, c] + (tap >> 1)
            if 0 <= qx < W and 0 <= qy < H and weights[tap][r, c] > 0:
                q = (H - 1 - qy, qx)
                p_albedo[q][3] = flag[r, c]
                p_nd[q][3] = pos["te"][r, c] * F(1 + rng.uniform(-0.03, 0.03))
                p_nd[q][:3] = unit(nd[r, c, :3] + rng.normal(size=3) * 0.08) if geometry[r, c] else 0
                if h_acc[q][3] == 0 and (c, r) in planted:
                    h_acc[q] = (3.0, 2.0, 1.0, 8.0)
    if big:                                                   # a NaN history channel under three pixels that land on history
        landed = [(r, c) for r, c in order if 0 <= pos["x0"][r, c] < W and 0 <= pos["y0"][r, c] < H and weights[0][r, c] > 0
                  and h_acc[H - 1 - pos["y0"][r, c], pos["x0"][r, c], 3] > 0]
        for r, c in landed[len(landed) // 4::len(landed) // 4][:3]:
            h_acc[H - 1 - pos["y0"][r, c], pos["x0"][r, c], 2] = np.nan
    return (accum, m2, albedo, nd), (h_acc, h_m2, p_albedo, p_nd), pp, cam_prev


CENSUS_20 = ("unclamped", "at_lo", "at_hi", "clamped_capped", "clamped_uncapped", "cut", "flag_drop", "empty_drop")
CENSUS_1 = ("k0", "sd0", "nan_bound_unclamped", "nan_history")


# ---- the card scene (tests/motion_model.py) with the card moved sideways ---------------------------------------------------------
# The light stands at x = 1.6 behind the card and throws its shadow onto the floor before it; sliding the card by -0.5 in x drags
# the shadow along and uncovers some 120 floor pixels of the 64 x 48 film (the CPU oracle at 256 spp: test_temporal_clamp_model.py).
CARD_SLIDE = (-0.5, 0.0, 0.0)
CARD_CLAMP = dict(radius=2, demodulate=1, gamma=1.0, clamped_max_history=8.0)
FLOOR_ALBEDO = F(0.6)


def floor_pixels(albedo, normal_depth):
    """the pixels of a card-scene feature buffer that show the grey floor"""
    return (albedo[..., 3] == 1) & (albedo[..., :3] == FLOOR_ALBEDO).all(-1) & (normal_depth[..., 3] > 0)


def uncovered_pixels(floor, y_before, y_after):
    """floor pixels whose reference luminance at least doubled between the two poses (a pixel that stayed black did not)"""
    return floor & (y_after >= 2 * y_before) & (y_after > y_before)
