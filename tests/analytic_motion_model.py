"""A numpy model of the motion vectors of moved spheres and planes (include/agpt.h: agpt_scene_snapshot_positions' analytic records
and agpt_render_features_motion's prev_point), on top of tests/motion_model.py: a hit on sphere or plane k whose 20 record bytes differ
between the two generations becomes w = 1 and p = c_old + (p - c_new) * s per component, float32, every operation rounded on its own;
everything else is motion_model.prev_points' row."""
import numpy as np

import motion_model as mm

F = np.float32
MESH, SPHERE, PLANE = 0, 1, 2      # the model's own kinds (not the C enum)


def records(desc):
    """(float32[P, 5], kinds[P]) of a SceneDesc: per primitive index (cx, cy, cz, r, r2) as agpt_scene_add_sphere / _plane / _area_light
    store them -- r2 = r * r in float32 for a sphere, r / r2 = size / 2 per axis for a plane, zeros for a mesh"""
    rec, kinds = [], []
    for op in desc.ops:
        if op[0] == "mesh":
            rec.append(np.zeros(5, F))
            kinds.append(MESH)
        elif op[0] in ("sphere", "area_light"):
            r = F(op[2])
            rec.append(np.array([op[1][0], op[1][1], op[1][2], r, r * r], F))
            kinds.append(SPHERE)
        elif op[0] == "plane":
            rec.append(np.array([op[1][0], op[1][1], op[1][2], F(op[2][0]) / F(2), F(op[2][1]) / F(2)], F))
            kinds.append(PLANE)
    return (np.stack(rec).astype(F) if rec else np.zeros((0, 5), F)), np.array(kinds, np.int64)


def hit_records(hits, prim_bases):
    """motion_model.hit_records plus the primitive index of every hit (-1 on a miss): ((id, t, b1, b2), prim)"""
    prim = np.where(hits["hit"] != 0, hits["prim"].astype(np.int64), -1)
    return mm.hit_records(hits, prim_bases), prim


def moved(rec_old, rec_new):
    """bool[P]: the record bytes differ (-0 against +0 counts, a NaN against itself does not)"""
    a = np.ascontiguousarray(rec_old, F).view(np.uint32)
    b = np.ascontiguousarray(rec_new, F).view(np.uint32)
    return (a != b).any(-1)


def prev_points(hits, prim, O, D, gen_old, gen_new, rec_old, rec_new, kinds):
    """k_motion with analytic generations: float32[N, 4]"""
    out = mm.prev_points(hits, O, D, gen_old, gen_new)
    ids = hits[0]
    rec_old, rec_new = np.asarray(rec_old, F).reshape(-1, 5), np.asarray(rec_new, F).reshape(-1, 5)
    if len(rec_old) == 0:
        return out
    on = ids == mm.ANALYTIC
    k = np.where(on, prim, 0)
    differ = on & moved(rec_old, rec_new)[k]
    a, b = rec_old[k], rec_new[k]
    with np.errstate(all="ignore"):
        q = (a[:, 3] / b[:, 3]).astype(F)
        qz = (a[:, 4] / b[:, 4]).astype(F)
        plane = np.asarray(kinds)[k] == PLANE
        s = np.stack([q, np.where(plane, F(1), q), np.where(plane, qz, q)], -1).astype(F)
        now = out[:, :3]
        was = (a[:, :3] + ((now - b[:, :3]).astype(F) * s).astype(F)).astype(F)
        ok = np.isfinite(s).all(-1) & np.isfinite(was).all(-1)
    use = differ & ok
    out[:, :3] = np.where(use[:, None], was, out[:, :3])
    out[:, 3] = np.where(use, F(1), out[:, 3])
    return out


def prev_points64(hits, prim, O, D, rec_old, rec_new, kinds):
    """the moved rows of prev_points in float64 from the float32 inputs (rows of unmoved or non-analytic hits: NaN)"""
    ids, t = hits[0], hits[1]
    k = np.where(ids == mm.ANALYTIC, prim, 0)
    a, b = np.asarray(rec_old, np.float64)[k], np.asarray(rec_new, np.float64)[k]
    now = np.asarray(O, np.float64) + t.astype(np.float64)[:, None] * np.asarray(D, np.float64)
    plane = np.asarray(kinds)[k] == PLANE
    with np.errstate(all="ignore"):
        q = a[:, 3] / b[:, 3]
        s = np.stack([q, np.where(plane, 1.0, q), np.where(plane, a[:, 4] / b[:, 4], q)], -1)
        was = a[:, :3] + (now - b[:, :3]) * s
    return np.where((ids == mm.ANALYTIC)[:, None], was, np.nan)
