"""CPU checks of the previous-frame normals (agpt_scene_snapshot_surfaces, agpt_render_features_surface_motion,
agpt_temporal_accumulate_surface_motion, agpt_kat_surface): symbols, Python wrappers, the argument checks that need no device, the
model's substitution rule, and -- from the CPU oracle's hits alone -- the property the feature exists for: a card turned by more than
acos(normal_cos) loses all its history with agpt_temporal_accumulate_motion and keeps it with the new call."""
import ctypes as C

import numpy as np

import ag_pathtracer_amd as ag
import motion_model as mm
import surface_motion_model as sm
from denoise_features import host_features
from helpers import assert_exported, oracle_scene
from oracle import binding as ob

F = np.float32
INVALID = -1
NEW = ("agpt_scene_snapshot_surfaces", "agpt_render_features_surface_motion", "agpt_temporal_accumulate_surface_motion", "agpt_kat_surface")


def test_symbols_declared_and_exported():
    assert_exported(NEW)


def test_python_wrappers_exist():
    for cls, names in ((ag.Scene, ("snapshot_surfaces", "kat_surface")),
                       (ag.PathTracer, ("render_features_surface_motion", "render_features_surface_motion_to_host")),
                       (ag.Context, ("temporal_accumulate_surface_motion", "temporal_to_host"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    import inspect
    assert "prev_normal" in inspect.signature(ag.Context.temporal_to_host).parameters


def test_argument_failures_without_a_context_name_their_function():
    L = ag.lib()
    assert L.agpt_scene_snapshot_surfaces(None) == INVALID
    assert b"agpt_scene_snapshot_surfaces" in L.agpt_last_error()
    assert L.agpt_render_features_surface_motion(None, None, None, None, None, None) == INVALID
    assert b"agpt_render_features_surface_motion: NULL" in L.agpt_last_error()
    rp = ag.RenderParams(64, 48, 0, 0, 64, 48, 0, 0, 0, 5, 64, 0, 0, 0, 0, 0, 0, 0, 0)
    rp.spp_count = 4
    assert L.agpt_render_features_surface_motion(None, C.byref(rp), None, None, None, None) == INVALID
    assert b"agpt_render_features_surface_motion: spp" in L.agpt_last_error()
    nothing = [None] * 12
    assert L.agpt_temporal_accumulate_surface_motion(None, None, None, *nothing) == INVALID
    assert b"agpt_temporal_accumulate_surface_motion: NULL" in L.agpt_last_error()
    cam = ag.camera_desc(*mm.CARD_CAMERA)
    clamp = ag.TemporalClampParams(2, 0, 1.0, 8.0)
    for change, word in ((dict(width=0), b"film"), (dict(max_history=0.0), b"max_history"), (dict(normal_cos=2.0), b"normal_cos"), (dict(), b"NULL")):
        q = ag.TemporalParams(8, 8, cam, cam, 32.0, ag.TEMPORAL_DEPTH_TOL, ag.TEMPORAL_NORMAL_COS)
        for k, v in change.items():
            setattr(q, k, v)
        for cp in (None, C.byref(clamp)):
            assert L.agpt_temporal_accumulate_surface_motion(None, C.byref(q), cp, *nothing) == INVALID, change
            msg = L.agpt_last_error()
            assert b"agpt_temporal_accumulate_surface_motion" in msg and word in msg, (change, msg)
    ids, f = (C.c_uint32 * 1)(0), (C.c_float * 3)()
    assert L.agpt_kat_surface(None, -1, 1, ids, f, f, f, f) == INVALID
    assert b"agpt_kat_surface" in L.agpt_last_error()


def test_substitution_touches_moved_pixels_only():
    rng = np.random.RandomState(3)
    nd = rng.normal(size=(5, 7, 4)).astype(F)
    pn = rng.normal(size=(5, 7, 4)).astype(F)
    pn[0, 0, 1] = np.nan
    pp = np.zeros((5, 7, 4), F)
    pp[..., 3] = rng.choice(np.array([0, 1, 2, 3, np.nan], F), size=(5, 7))
    pp[0, 0, 3] = 1
    out = sm.substituted(nd, pp, pn)
    moved = pp[..., 3] == 1
    assert moved.any() and not moved.all()
    assert out[..., 3].tobytes() == nd[..., 3].tobytes()
    assert out[..., :3][moved].tobytes() == pn[..., :3][moved].tobytes() and out[..., :3][~moved].tobytes() == nd[..., :3][~moved].tobytes()
    assemble = sm.prev_normals(pp, nd, moved, pn[..., :3])
    assert assemble[..., 3].tobytes() == pp[..., 3].tobytes() and (assemble[pp[..., 3] == 0] == 0).all()
    assert assemble[..., :3][pp[..., 3] == 2].tobytes() == nd[..., :3][pp[..., 3] == 2].tobytes()


def turned_card_on_the_oracle(degrees):
    """the two frames of the turning card from the CPU oracle, frame 1's prev_point from the oracle's hits, and its prev_normal: the
    flat card's frame-0 normal on the card's pixels -> (cur, prev, prev_point, prev_normal, on_card)"""
    cw, ch = mm.CARD_W, mm.CARD_H
    rest = mm.card_mesh()[0]
    turned = ag.transform_arrays(sm.turn_y(degrees), rest)[0]
    f0 = host_features(mm.card_scene(), cw, ch)
    f1 = host_features(sm.card_scene_with(turned), cw, ch)
    O, once, D = mm.feature_rays(ag.camera_vectors(mm.CARD_CAMERA), cw, ch)
    rays = np.zeros(cw * ch, ob.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"] = O, once, mm.FLT_MAX
    hits, _ = oracle_scene(sm.card_scene_with(turned)).intersect(rays)
    rec = mm.hit_records(hits, {0: 0, mm.CARD_PRIM: mm.CARD_BASE})
    pp = mm.prev_points(rec, O, D, mm.generation(mm.card_meshes()), mm.generation([mm.FLOOR, (turned, mm.card_mesh()[1])])).reshape(ch, cw, 4)
    on_card = ((hits["hit"] == 1) & (hits["prim"] == mm.CARD_PRIM)).reshape(ch, cw)
    rest_card = (f0[3]["hit"] == 1) & (f0[3]["prim"] == mm.CARD_PRIM)
    n_rest = f0[1][::-1][rest_card][0, :3]                     # (host_features' hits are in film order, its buffers in buffer order)
    assert (f0[1][::-1][rest_card][:, :3] == n_rest).all() and abs(abs(n_rest[2]) - 1) < 1e-6
    pn = sm.prev_normals(pp, f1[1], on_card, np.broadcast_to(n_rest, (ch, cw, 3)))
    rng = np.random.RandomState(5)

    def sums(n):
        a = np.zeros((ch, cw, 4), F)
        a[..., :3] = rng.uniform(0, 2, (ch, cw, 3)) * n
        a[..., 3] = n
        return a, (rng.uniform(0, 6, (ch, cw)) * n).astype(F)
    return sums(4) + (f1[0], f1[1]), sums(8) + (f0[0], f0[1]), pp, pn, on_card


def test_a_turned_card_keeps_its_history_only_with_its_previous_normal():
    cur, prev, pp, pn, on_card = turned_card_on_the_oracle(sm.TURN_DEGREES)
    assert on_card.sum() >= 100 and np.array_equal(pp[..., 3] == 1, on_card)
    old, new, out = sm.card_shares(ag.camera_vectors(mm.CARD_CAMERA), cur, prev, pp, pn, on_card)
    print("card turned %g degrees: %d card pixels, history for %.3f of them with their previous normal, for %.3f without"
          % (sm.TURN_DEGREES, int(on_card.sum()), new, old))
    assert old == 0.0
    assert new >= 0.9
