"""A numpy model of agpt_temporal_accumulate_clamped's contract (include/agpt.h): float32 operation by operation like
tests/temporal_model.py and tests/motion_model.py, whose position() it uses for step 3 and whose gather() for step 4.  It adds the
neighbourhood statistics in the contract's tap order (dy = -r .. r outermost in FILM rows, dx = -r .. r) and step 5', and returns
the masks the tests take their census from.  Buffers are [H, W, ...] in Accumulator::pixels order (buffer row r holds film
row y = H - 1 - r)."""
import numpy as np

import motion_model as mm
import temporal_model as tm
from adaptive_model import luminance

F = np.float32
ALBEDO_FLOOR = F(1e-3)


def demodulated_means(accum, albedo, demodulate):
    """x[H, W, 3] = accum.rgb / n (/ fmaxf(albedo.rgb, 1e-3) with demodulate) and whether n > 0"""
    n = accum[..., 3]
    with np.errstate(all="ignore"):
        x = accum[..., :3] / n[..., None]
        if demodulate:
            x = x / np.fmax(albedo[..., :3], ALBEDO_FLOOR)
    return x.astype(F), n > 0


def statistics(accum, albedo, radius, demodulate):
    """-> dict: k[H, W], s1, s2 [H, W, 3] summed in tap order from +0, and per pixel whether its window is cut by the film edge, drops
    a tap for its flag, drops a tap for n_q <= 0"""
    H, W = accum.shape[:2]
    r = int(radius)
    x, valid = demodulated_means(accum, albedo, demodulate)
    flag = albedo[..., 3]
    pad = ((r, r), (r, r))
    xp = np.pad(x, pad + ((0, 0),))
    vp = np.pad(valid, pad)
    fp = np.pad(flag, pad)
    ip = np.pad(np.ones((H, W), bool), pad)
    k = np.zeros((H, W), F)
    s1 = np.zeros((H, W, 3), F)
    s2 = np.zeros((H, W, 3), F)
    cut = np.zeros((H, W), bool)
    flag_drop = np.zeros((H, W), bool)
    empty_drop = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            rows = slice(r - dy, r - dy + H)                 # film row y + dy is buffer row `row - dy`
            for dx in range(-r, r + 1):
                cols = slice(r + dx, r + dx + W)
                inside, xq = ip[rows, cols], xp[rows, cols]
                same = fp[rows, cols] == flag
                use = inside & vp[rows, cols] & same
                k = np.where(use, k + F(1), k)
                s1 = np.where(use[..., None], s1 + xq, s1)
                s2 = np.where(use[..., None], s2 + xq * xq, s2)
                cut |= ~inside
                flag_drop |= inside & vp[rows, cols] & ~same
                empty_drop |= inside & ~vp[rows, cols]
    return dict(k=k, s1=s1.astype(F), s2=s2.astype(F), cut=cut, flag_drop=flag_drop, empty_drop=empty_drop)


def accumulate_clamped(cam_cur, cam_prev, accum, moment2, albedo, normal_depth, prev=None, prev_point=None, radius=2, demodulate=0,
                       gamma=1.0, clamped_max_history=8.0, max_history=32.0, depth_tol=tm.DEPTH_TOL, normal_cos=tm.NORMAL_COS,
                       identity=None, return_masks=False):
    """agpt_temporal_accumulate_clamped -> (hist_accum[H, W, 4], hist_moment2[H, W]) (+ a dict of masks).  prev as for tm.accumulate;
    prev_point None: step 3 is tm.position's, else mm.position's."""
    accum, moment2, albedo, nd = (np.asarray(a, F) for a in (accum, moment2, albedo, normal_depth))
    H, W = moment2.shape
    if prev is None:
        return (accum.copy(), moment2.copy()) + (({},) if return_masks else ())
    prev = tuple(np.asarray(a, F) for a in prev)
    if identity is None:
        identity = np.asarray(cam_cur, F).tobytes() == np.asarray(cam_prev, F).tobytes()
    flag = albedo[..., 3]
    if prev_point is None:
        pos = tm.position(cam_cur, cam_prev, identity, flag, nd[..., 3], W, H)
    else:
        pos, _ = mm.position(cam_cur, cam_prev, identity, flag, nd[..., 3], prev_point, W, H)
    sb, sn, sc, sm, history = tm.gather(pos, flag, nd[..., :3], prev, depth_tol, normal_cos)      # step 4
    g, cmh = F(gamma), F(clamped_max_history)
    with np.errstate(all="ignore"):
        # the statistics of the current frame
        st = statistics(accum, albedo, radius, demodulate)
        k = st["k"]
        has_k = k > 0
        mu = st["s1"] / k[..., None]
        var = np.fmax(st["s2"] / k[..., None] - mu * mu, F(0))
        sd = np.sqrt(var)
        lo = mu - g * sd
        hi = mu + g * sd
        # step 5'
        n_raw = np.fmin(sn / sb, F(max_history))
        c_h = (sc / sb[..., None]).astype(F)
        m_h = sm / sb
        a = np.fmax(albedo[..., :3], ALBEDO_FLOOR)
        d = c_h / a if demodulate else c_h
        e = np.fmin(np.fmax(d, lo), hi)
        channel = has_k[..., None] & ~(e == d)
        c_new = np.where(channel, e * a if demodulate else e, c_h).astype(F)
        clamped = channel.any(-1)
        y_old, y_new = luminance(c_h), luminance(c_new)
        m_new = np.where(clamped, np.fmax(m_h - y_old * y_old, F(0)) + y_new * y_new, m_h)
        n_h = np.where(clamped, np.fmin(n_raw, cmh), n_raw)
        out, m_out = tm.blend(accum, moment2, history, c_new, m_new, n_h)
        if return_masks:
            nan_bound = np.isnan(lo) | np.isnan(hi)
            masks = dict(
                history=history, clamped=history & clamped, unclamped=history & ~clamped,
                at_lo=history & (channel & (d < lo)).any(-1), at_hi=history & (channel & (d > hi)).any(-1),
                clamped_capped=history & clamped & (n_raw > cmh), clamped_uncapped=history & clamped & (n_raw < cmh),
                cut=history & st["cut"], flag_drop=history & st["flag_drop"], empty_drop=history & st["empty_drop"],
                k0=history & ~has_k, sd0=history & has_k & (sd == 0).any(-1),
                nan_bound_unclamped=history & has_k & (nan_bound & ~channel).any(-1) & ~clamped,
                nan_history=history & np.isnan(c_h).any(-1), k=k)
            return out, m_out, masks
    return out, m_out
