"""A numpy model of agpt_temporal_accumulate's contract (include/agpt.h): float32 operation by operation, a loop over the four
taps in the contract's order, vectorised over the pixels.  Buffers are [H, W, ...] in Accumulator::pixels order like the device's
(buffer row r holds film row y = H - 1 - r); the cameras come as the 22 floats of agpt_camera_vectors, so the model derives no
camera of its own."""
import numpy as np

F = np.float32
DEPTH_TOL, NORMAL_COS, MIN_WEIGHT = 0.05, 0.9, 1e-2   # AGPT_TEMPORAL_*
DEPTH_FLOOR = F(1e-3)


def camera(vec22):
    """origin, u, v, w, lower_left_corner, horizontal, vertical as float32[3] each"""
    v = np.asarray(vec22, F)
    assert v.shape == (22,)
    return {k: v[3 * i:3 * i + 3] for i, k in enumerate(("origin", "u", "v", "w", "llc", "horizontal", "vertical"))}


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(v):
    inv = F(1) / np.sqrt(dot(v, v))
    return v * inv[..., None]


def feature_directions(cam, W, H):
    """D[H, W, 3] in buffer order: the direction of agpt_render_features' ray through each pixel (k_feature_rays)"""
    c = camera(cam)
    x = np.arange(W).astype(F)[None, :]
    y = (H - 1 - np.arange(H)).astype(F)[:, None]
    s = ((x + F(0.5)) / F(W))[..., None] + np.zeros((H, 1, 1), F)
    t = ((y + F(0.5)) / F(H))[..., None] + np.zeros((1, W, 1), F)
    offset = c["u"] * F(0) + c["v"] * F(0)
    pixel = (c["llc"] + s * c["horizontal"]) + t * c["vertical"]
    return normalize(normalize((pixel - c["origin"]) - offset)).astype(F)


def project(cam_prev, Q, W, H):
    """The projection half of step 3.  Q[H, W, 3]: the point relative to the previous camera's origin (a direction for a point at
    infinity) -> dict: found[H, W] (False: no history), x0, y0 (int, film coordinates), fx, fy, te, and the two reasons a pixel is
    not found: behind (not in front of the previous camera), off_film."""
    P = camera(cam_prev)
    with np.errstate(all="ignore"):
        Q = np.asarray(Q, F)
        te = np.sqrt(dot(Q, Q))
        L = P["llc"] - P["origin"]
        dw = dot(Q, P["w"])
        behind = ~(dw < 0)
        k = dot(L, P["w"]) / dw
        R = Q * k[..., None] - L
        s = dot(R, P["horizontal"]) / dot(P["horizontal"], P["horizontal"])
        t = dot(R, P["vertical"]) / dot(P["vertical"], P["vertical"])
        sx = s * F(W) - F(0.5)
        sy = t * F(H) - F(0.5)
        inside = (sx > -1) & (sx < W) & (sy > -1) & (sy < H)
        found = ~behind & inside
        flx, fly = np.floor(sx), np.floor(sy)
        fx, fy = sx - flx, sy - fly
    x0 = np.where(found, flx, 0).astype(np.int64)
    y0 = np.where(found, fly, 0).astype(np.int64)
    return dict(found=found, x0=x0, y0=y0, fx=fx.astype(F), fy=fy.astype(F), te=te.astype(F), behind=behind, off_film=~behind & ~inside)


def position(cam_cur, cam_prev, identity, flag, depth, W, H):
    """Step 3 -> project's dict for the point each pixel sees now (a miss: the point at infinity along its ray); identity: every pixel
    lands on itself, no arithmetic."""
    yy = (H - 1 - np.arange(H))[:, None] + np.zeros((1, W), np.int64)
    xx = np.arange(W)[None, :] + np.zeros((H, 1), np.int64)
    if identity:
        z = np.zeros((H, W), F)
        no = np.zeros((H, W), bool)
        return dict(found=~no, x0=xx, y0=yy, fx=z, fy=z.copy(), te=np.asarray(depth, F), behind=no, off_film=no.copy())
    C, P = camera(cam_cur), camera(cam_prev)
    D = feature_directions(cam_cur, W, H)
    with np.errstate(all="ignore"):
        hit = (C["origin"] + np.asarray(depth, F)[..., None] * D) - P["origin"]
        Q = np.where((flag != 0)[..., None], hit, D).astype(F)
    return project(cam_prev, Q, W, H)


def gather(pos, flag, normal, prev, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS, masks=None):
    """Step 4: the four taps around the positions `pos` (position's dict, or motion_model.position's) in the contract's order.  flag[H, W]
    and normal[H, W, 3]: the current frame's, compared with each tap's; prev = (hist_accum, hist_moment2, albedo, normal_depth) of the
    previous frame -> (sb, sn, sc[H, W, 3], sm, history): the sums over the accepted taps and step 5's test on sb.
    masks: a dict that receives, per tap, why it was used or rejected (accumulate's return_masks)."""
    h_acc, h_m2, p_albedo, p_nd = prev
    H, W = flag.shape
    geometry = flag != 0
    found, x0, y0, fx, fy, te = (pos[k] for k in ("found", "x0", "y0", "fx", "fy", "te"))
    one = F(1)
    weights = ((one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy)
    sb = np.zeros((H, W), F)
    sn = np.zeros((H, W), F)
    sc = np.zeros((H, W, 3), F)
    sm = np.zeros((H, W), F)
    if masks is not None:
        masks.update(used=[], flag_mismatch=[], empty_tap=[], depth_on=[], depth_out=[], normal_on=[], normal_out=[])
    with np.errstate(all="ignore"):
        zmax = F(depth_tol) * np.fmax(te, DEPTH_FLOOR)
        for tap in range(4):
            qx, qy = x0 + (tap & 1), y0 + (tap >> 1)
            b = weights[tap].astype(F)
            inside = found & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (b > 0)
            r, c = np.clip(H - 1 - qy, 0, H - 1), np.clip(qx, 0, W - 1)
            n_q = h_acc[r, c, 3]
            flag_ok = p_albedo[r, c, 3] == flag
            dz = np.abs(te - p_nd[r, c, 3])
            near = dz <= zmax
            cosine = dot(normal, p_nd[r, c, :3])
            facing = cosine >= F(normal_cos)
            candidate = inside & (n_q > 0) & flag_ok
            use = candidate & (~geometry | (near & facing))
            sb = np.where(use, sb + b, sb)
            sn = np.where(use, sn + b * n_q, sn)
            sc = np.where(use[..., None], sc + b[..., None] * (h_acc[r, c, :3] / n_q[..., None]), sc)
            sm = np.where(use, sm + b * (h_m2[r, c] / n_q), sm)
            if masks is not None:
                masks["used"].append(use)
                masks["flag_mismatch"].append(inside & (n_q > 0) & ~flag_ok)
                masks["empty_tap"].append(inside & ~(n_q > 0))
                masks["depth_on"].append(use & geometry & (dz == zmax))
                masks["depth_out"].append(candidate & geometry & ~near)
                masks["normal_on"].append(use & geometry & (cosine == F(normal_cos)))
                masks["normal_out"].append(candidate & geometry & near & ~facing)
        history = found & (sb >= F(MIN_WEIGHT))
    return sb, sn, sc, sm, history


def blend(accum, moment2, history, c_h, m_h, n_h):
    """Step 6: the history's mean colour c_h[H, W, 3] and mean squared luminance m_h, n_h times each, added where `history`"""
    with np.errstate(all="ignore"):
        out = accum.copy()
        out[..., :3] = np.where(history[..., None], accum[..., :3] + c_h * n_h[..., None], accum[..., :3])
        out[..., 3] = np.where(history, accum[..., 3] + n_h, accum[..., 3])
        m_out = np.where(history, moment2 + m_h * n_h, moment2).astype(F)
    return out.astype(F), m_out


def accumulate(cam_cur, cam_prev, accum, moment2, albedo, normal_depth, prev=None, max_history=32.0, depth_tol=DEPTH_TOL,
               normal_cos=NORMAL_COS, identity=None, return_masks=False):
    """agpt_temporal_accumulate -> (hist_accum[H, W, 4], hist_moment2[H, W]) (+ a dict of masks).  prev: None (first frame) or
    (hist_accum, hist_moment2, albedo, normal_depth) of the previous frame.  identity: whether the two camera DESCRIPTIONS are the
    same bytes (the library compares those, not the vectors); default: the vectors are."""
    accum, moment2, albedo, nd = (np.asarray(a, F) for a in (accum, moment2, albedo, normal_depth))
    H, W = moment2.shape
    if prev is None:
        return (accum.copy(), moment2.copy()) + (({},) if return_masks else ())
    prev = tuple(np.asarray(a, F) for a in prev)
    if identity is None:
        identity = np.asarray(cam_cur, F).tobytes() == np.asarray(cam_prev, F).tobytes()
    flag = albedo[..., 3]
    pos = position(cam_cur, cam_prev, identity, flag, nd[..., 3], W, H)
    masks = dict(pos) if return_masks else None
    sb, sn, sc, sm, history = gather(pos, flag, nd[..., :3], prev, depth_tol, normal_cos, masks)
    with np.errstate(all="ignore"):
        n_raw = sn / sb
        n_h = np.fmin(n_raw, F(max_history))
        out, m_out = blend(accum, moment2, history, sc / sb[..., None], sm / sb, n_h)
    if return_masks:
        masks.update(history=history, capped=history & (n_raw > F(max_history)), uncapped=history & (n_raw < F(max_history)))
        return out, m_out, masks
    return out, m_out
