"""A numpy model of the motion-vector contracts (include/agpt.h): agpt_scene_snapshot_positions' generations, k_motion's prev_point
and agpt_temporal_accumulate_motion, float32 operation by operation like tests/temporal_model.py, whose functions it uses.  Film
buffers are [H, W, ...] in Accumulator::pixels order (buffer row r holds film row y = H - 1 - r); rays and hits are flat in that
order too."""
import numpy as np

import temporal_model as tm

F = np.float32
MISS, ANALYTIC = -1, -2          # ids of a hit record that names no triangle: nothing hit, a sphere or a plane
FLT_MAX = F(3.402823466e+38)


def triangle_bases(meshes):
    """meshes: [(verts[n, 3], indices[3m, 3] rows (v, n, t) per corner)] in the order the scene's meshes were added -> the global
    id of each mesh's first triangle"""
    counts = [np.asarray(ix).reshape(-1, 3).shape[0] // 3 for _, ix in meshes]
    return [int(b) for b in np.concatenate([[0], np.cumsum(counts)[:-1]])]


def generation(meshes):
    """float32[T, 3, 3]: the three corner positions of every triangle by global triangle id -- what a snapshot holds (w lanes aside)"""
    parts = [np.asarray(v, F).reshape(-1, 3)[np.asarray(ix).reshape(-1, 3)[:, 0]].reshape(-1, 3, 3) for v, ix in meshes]
    return np.concatenate(parts).astype(F) if parts else np.zeros((0, 3, 3), F)


def feature_rays(cam, W, H):
    """(O[3], once[H * W, 3], D[H * W, 3]) in buffer order: the origin of k_feature_rays' rays, their direction as Camera::GetRay
    leaves it (what a ray query is handed: the library normalises it once more) and as traced (tm.feature_directions)"""
    c = tm.camera(cam)
    x = np.arange(W).astype(F)[None, :]
    y = (H - 1 - np.arange(H)).astype(F)[:, None]
    s = ((x + F(0.5)) / F(W))[..., None] + np.zeros((H, 1, 1), F)
    t = ((y + F(0.5)) / F(H))[..., None] + np.zeros((1, W, 1), F)
    offset = c["u"] * F(0) + c["v"] * F(0)
    pixel = (c["llc"] + s * c["horizontal"]) + t * c["vertical"]
    once = tm.normalize((pixel - c["origin"]) - offset).astype(F)
    D = tm.normalize(once).astype(F)
    assert D.tobytes() == tm.feature_directions(cam, W, H).tobytes()
    return (c["origin"] + offset).astype(F), once.reshape(-1, 3), D.reshape(-1, 3)


def hit_records(hits, prim_bases):
    """agpt_hit / oracle hit records (hit, prim, tri, t, b1, b2) -> (id, t, b1, b2): id = the global triangle id of a mesh hit,
    MISS or ANALYTIC.  prim_bases: {primitive index of a mesh: its triangle base}"""
    ids = np.full(len(hits), MISS, np.int64)
    for k, h in enumerate(hits):
        if h["hit"]:
            ids[k] = prim_bases[int(h["prim"])] + int(h["tri"]) // 3 if int(h["prim"]) in prim_bases else ANALYTIC
    return ids, hits["t"].astype(F), hits["b1"].astype(F), hits["b2"].astype(F)


def prev_points(hits, O, D, gen_old, gen_new):
    """k_motion: float32[N, 4] = (p.xyz, w) for N hit records (id, t, b1, b2) of the rays (O[3], D[N, 3])"""
    ids, t, b1, b2 = hits
    O, D = np.asarray(O, F), np.asarray(D, F)
    old = np.ascontiguousarray(gen_old, F).reshape(-1, 3, 3)
    new = np.ascontiguousarray(gen_new, F).reshape(-1, 3, 3)
    out = np.zeros((len(ids), 4), F)
    hit = ids != MISS
    with np.errstate(all="ignore"):
        now = (O + t[:, None] * D).astype(F)
        tri = ids >= 0
        g = np.where(tri, ids, 0)
        moved = tri & (old[g].view(np.uint32) != new[g].view(np.uint32)).reshape(len(ids), -1).any(-1) if len(old) else tri & False
        if len(old):
            v0, v1, v2 = old[g, 0], old[g, 1], old[g, 2]
            b0 = (F(1) - b1) - b2
            was = ((v0 * b0[:, None] + v1 * b1[:, None]) + v2 * b2[:, None]).astype(F)
        else:
            was = now
    out[:, :3] = np.where(hit[:, None], np.where(moved[:, None], was, now), F(0))
    out[:, 3] = np.where(hit, np.where(moved, F(1), F(2)), F(0))
    return out


def position(cam_cur, cam_prev, identity, flag, depth, prev_point, W, H):
    """Step 3 with the per-pixel switch: tm.position where prev_point.w != 1; where it is 1, the arithmetic on Q = m.xyz - P.origin,
    whatever `identity` says"""
    pos = tm.position(cam_cur, cam_prev, identity, flag, depth, W, H)
    m = np.asarray(prev_point, F)
    moved = m[..., 3] == 1
    with np.errstate(all="ignore"):
        mine = tm.project(cam_prev, (m[..., :3] - tm.camera(cam_prev)["origin"]).astype(F), W, H)
    return {k: np.where(moved, mine[k], pos[k]) for k in ("found", "x0", "y0", "fx", "fy", "te")}, moved


def accumulate_motion(cam_cur, cam_prev, accum, moment2, albedo, normal_depth, prev, prev_point, max_history=32.0,
                      depth_tol=tm.DEPTH_TOL, normal_cos=tm.NORMAL_COS, identity=None):
    """agpt_temporal_accumulate_motion -> (hist_accum[H, W, 4], hist_moment2[H, W]): tm.accumulate's steps 4-6 on the positions of
    `position` above.  prev as for tm.accumulate; prev_point[H, W, 4] is not read on the first frame."""
    accum, moment2, albedo, nd = (np.asarray(a, F) for a in (accum, moment2, albedo, normal_depth))
    H, W = moment2.shape
    if prev is None:
        return accum.copy(), moment2.copy()
    prev = tuple(np.asarray(a, F) for a in prev)
    if identity is None:
        identity = np.asarray(cam_cur, F).tobytes() == np.asarray(cam_prev, F).tobytes()
    flag = albedo[..., 3]
    pos, _ = position(cam_cur, cam_prev, identity, flag, nd[..., 3], prev_point, W, H)
    sb, sn, sc, sm, history = tm.gather(pos, flag, nd[..., :3], prev, depth_tol, normal_cos)
    with np.errstate(all="ignore"):
        return tm.blend(accum, moment2, history, sc / sb[..., None], sm / sb, np.fmin(sn / sb, F(max_history)))


# ---- the card scene of the tests ---------------------------------------------------------------------------------------------
CARD_W, CARD_H = 64, 48
CARD_CAMERA = ([0.0, 1.0, -4.0], [0.0, 1.0, 0.0], [0, 1, 0], CARD_W / float(CARD_H), 45.0, 0.0)
CARD_MOVE = (0.3, 0.0, -0.5)      # frame 1: 0.3 sideways and 0.5 (12.5 % of its depth of 4, against depth_tol 0.05) towards the camera


def card_mesh(offset=(0.0, 0.0, 0.0), n=6):
    """an n x n-quad card of side 1 in the plane z = 0 around (0, 1, 0), moved by `offset`: (verts, indices)"""
    g = np.linspace(-0.5, 0.5, n + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    verts = (np.stack([X, Y + 1.0, np.zeros_like(X)], -1).reshape(-1, 3) + np.asarray(offset, np.float64)).astype(F)
    tri = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, i * (n + 1) + j + 1, (i + 1) * (n + 1) + j + 1
            tri += [a, b, c, c, b, d]
    idx = np.zeros((len(tri), 3), np.int32)
    idx[:, 0] = tri
    return verts, idx


FLOOR = (np.array([[-5, 0, -5], [5, 0, -5], [-5, 0, 5], [5, 0, 5]], F), np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], np.int32))
CARD_PRIM, CARD_BASE = 1, 2       # the card is the second primitive; its triangles follow the floor's two
LIGHT = ((1.6, 2.0, 1.0), 0.3)    # the sphere light (primitive 2): in view, up and to the right behind the card


def card_scene(offset=(0.0, 0.0, 0.0)):
    """a static two-triangle floor, the card, a sphere light; the static camera looks at the card from 4 away"""
    import ag_pathtracer_amd as ag
    d = ag.scenes.SceneDesc("card")
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.6, 0.6, 0.6))
    red = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.7, 0.2, 0.15))
    d.add_mesh(FLOOR[0], None, None, FLOOR[1], grey)
    v, ix = card_mesh(offset)
    assert d.add_mesh(v, None, None, ix, red) == CARD_PRIM
    d.add_area_light(LIGHT[0], LIGHT[1], (40.0, 40.0, 40.0))
    d.set_camera(*CARD_CAMERA)
    return d


def card_meshes(offset=(0.0, 0.0, 0.0)):
    return [FLOOR, card_mesh(offset)]
