"""A numpy model of the previous-frame-normal contracts (include/agpt.h): agpt_render_features_surface_motion's prev_normal and
agpt_temporal_accumulate_surface_motion.

The temporal step needs no arithmetic of its own.  normal_depth_cur.xyz is read by nothing but step 4's facing test, and .w is not read for
a moved pixel (its te comes from prev_point), so the new call equals the call it extends fed a copy of normal_depth_cur in which the xyz
of every prev_point.w == 1 pixel is replaced by prev_normal.xyz: tests/motion_model.py or tests/temporal_clamp_model.py on that buffer.
prev_normal is assembled from prev_point.w, normal_depth and the values of agpt_kat_surface as the header's table states."""
import numpy as np

import motion_model as mm
import temporal_clamp_model as cm

F = np.float32


def substituted(normal_depth, prev_point, prev_normal):
    """normal_depth with the xyz of every pixel whose prev_point.w is 1 replaced by prev_normal.xyz (bits, NaNs included)"""
    nd = np.array(normal_depth, F, copy=True)
    moved = np.asarray(prev_point, F)[..., 3] == 1
    nd[..., :3][moved] = np.asarray(prev_normal, F)[..., :3][moved]
    return nd


def accumulate_surface_motion(cam_cur, cam_prev, accum, moment2, albedo, normal_depth, prev, prev_point, prev_normal, clamp=None, **kw):
    """agpt_temporal_accumulate_surface_motion -> (hist_accum[H, W, 4], hist_moment2[H, W]).  clamp: None, or the clamp model's
    keywords (radius, demodulate, gamma, clamped_max_history); kw: max_history, depth_tol, normal_cos, identity"""
    nd = substituted(normal_depth, prev_point, prev_normal)
    if clamp is None:
        return mm.accumulate_motion(cam_cur, cam_prev, accum, moment2, albedo, nd, prev, prev_point, **kw)
    return cm.accumulate_clamped(cam_cur, cam_prev, accum, moment2, albedo, nd, prev=prev, prev_point=prev_point, **dict(clamp, **kw))


def prev_normals(prev_point, normal_depth, followed, old_ns):
    """prev_normal[H, W, 4]: zeros on a miss (w == 0); the bits of normal_depth.xyz for w == 2 and for a moved sphere or plane; on
    `followed` -- the w == 1 pixels whose hit is a triangle -- old_ns[H, W, 3], the reconstruction on the older record; w = prev_point.w"""
    pp, nd = np.asarray(prev_point, F), np.asarray(normal_depth, F)
    out = np.zeros(pp.shape, F)
    hit = pp[..., 3] != 0
    out[..., :3] = np.where(hit[..., None], np.where(np.asarray(followed)[..., None], np.asarray(old_ns, F), nd[..., :3]), F(0))
    out[..., 3] = pp[..., 3]
    return out


# ---- the turning card of the tests ------------------------------------------------------------------------------------------------
TURN_DEGREES = 40.0      # frame 1: the card of motion_model's scene turned about its vertical axis; cos 40 = 0.766 < normal_cos = 0.9


def turn_y(degrees, centre=(0.0, 1.0, 0.0)):
    """the 4 x 4 matrix of a turn about the vertical axis through `centre`"""
    a = np.deg2rad(degrees)
    R = np.eye(4)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    t0, t1 = np.eye(4), np.eye(4)
    t0[:3, 3], t1[:3, 3] = -np.asarray(centre), np.asarray(centre)
    return (t1 @ R @ t0).astype(F)


def card_scene_with(card_verts):
    """motion_model.card_scene() with the card's vertices given"""
    import ag_pathtracer_amd as ag
    d = ag.scenes.SceneDesc("turned-card")
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.6, 0.6, 0.6))
    red = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.7, 0.2, 0.15))
    d.add_mesh(mm.FLOOR[0], None, None, mm.FLOOR[1], grey)
    assert d.add_mesh(card_verts, None, None, mm.card_mesh()[1], red) == mm.CARD_PRIM
    d.add_area_light(mm.LIGHT[0], mm.LIGHT[1], (40.0, 40.0, 40.0))
    d.set_camera(*mm.CARD_CAMERA)
    return d


def card_shares(cam, cur, prev, prev_point, prev_normal, on_card):
    """the share of card pixels that take history with agpt_temporal_accumulate_motion and with the new call, by the models"""
    old, _ = mm.accumulate_motion(cam, cam, *cur, prev, prev_point)
    new, _ = accumulate_surface_motion(cam, cam, *cur, prev, prev_point, prev_normal)
    took_old, took_new = old[..., 3] > cur[0][..., 3], new[..., 3] > cur[0][..., 3]
    return took_old[on_card].mean(), took_new[on_card].mean(), new
