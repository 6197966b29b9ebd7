"""CPU checks of the motion vectors (agpt_scene_snapshot_positions, agpt_render_features_motion, agpt_temporal_accumulate_motion):
symbols, the argument checks that need no context, and the numpy model (tests/motion_model.py) -- equal to tests/temporal_model.py
where nothing moved, and on the card scene the property the feature exists for: a mesh that moved towards the camera keeps its
history with the motion call and loses all of it without."""
import ctypes as C
import functools
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np

import ag_pathtracer_amd as ag
import motion_model as mm
import temporal_model as tm
from denoise_features import host_features
from helpers import assert_exported, oracle_scene
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agpt_build", os.path.join(ROOT, "ag-pathtracer_amd", "build.py"))
b = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(b)
F = np.float32
INVALID = -1
H, W = 29, 37
CAM_A = ([0.3, 1.4, -6.0], [0, 0, 0], [0, 1, 0], W / float(H), 42.0, 0.0)
CAM_B = ([0.5, 1.3, -5.8], [0.1, 0, 0], [0, 1, 0], W / float(H), 42.0, 0.0)


def test_symbols_declared_and_exported():
    assert_exported(("agpt_scene_snapshot_positions", "agpt_render_features_motion", "agpt_temporal_accumulate_motion"))
    assert "agpt_motion.hip" in b.SOURCES and "agpt_motion.h" in b.HEADERS


def test_argument_failures_without_a_context_name_their_function():
    L = ag.lib()
    assert L.agpt_scene_snapshot_positions(None) == INVALID
    assert b"agpt_scene_snapshot_positions" in L.agpt_last_error()
    assert L.agpt_render_features_motion(None, None, None, None, None) == INVALID
    assert b"agpt_render_features_motion: NULL" in L.agpt_last_error()
    rp = ag.RenderParams(64, 48, 0, 0, 64, 48, 0, 0, 0, 5, 64, 0, 0, 0, 0, 0, 0, 0, 0)
    assert L.agpt_render_features_motion(None, C.byref(rp), None, None, None) == INVALID
    assert b"agpt_render_features_motion: NULL" in L.agpt_last_error()
    rp.spp_count = 4
    assert L.agpt_render_features_motion(None, C.byref(rp), None, None, None) == INVALID
    assert b"agpt_render_features_motion: spp" in L.agpt_last_error()
    p = ag.TemporalParams(W, H, ag.camera_desc(*CAM_A), ag.camera_desc(*CAM_B), 32.0, ag.TEMPORAL_DEPTH_TOL, ag.TEMPORAL_NORMAL_COS)
    nothing = [None] * 11
    assert L.agpt_temporal_accumulate_motion(None, None, *nothing) == INVALID
    assert b"agpt_temporal_accumulate_motion: NULL" in L.agpt_last_error()
    for change, word in ((dict(width=0), b"film"), (dict(max_history=0.0), b"max_history"), (dict(depth_tol=-1.0), b"depth_tol"),
                         (dict(normal_cos=2.0), b"normal_cos"), (dict(), b"NULL")):
        q = ag.TemporalParams(W, H, p.cam_cur, p.cam_prev, 32.0, ag.TEMPORAL_DEPTH_TOL, ag.TEMPORAL_NORMAL_COS)
        for k, v in change.items():
            setattr(q, k, v)
        assert L.agpt_temporal_accumulate_motion(None, C.byref(q), *nothing) == INVALID, change
        msg = L.agpt_last_error()
        assert b"agpt_temporal_accumulate_motion" in msg and word in msg, (change, msg)


def test_motion_unit_compiles_without_scratch_or_lds():
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "agpt_motion.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + b.SOURCE_FLAGS.get("agpt_motion.hip", []) + \
            ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out, os.path.join(b.CSRC, "agpt_motion.hip")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"remark: Function Name: (\S+)", p.stderr)
    assert len(names) == 2 and all(any(k in n for n in names) for k in ("k_snapshot_positions", "k_motion")), names
    for what in (r"ScratchSize \[bytes/lane\]", r"VGPRs Spill", r"SGPRs Spill", r"LDS Size \[bytes/block\]"):
        assert [int(v) for v in re.findall(what + r": (\d+)", p.stderr)] == [0, 0], what
    assert "-ffp-contract=off" in flags and not b.SOURCE_FLAGS.get("agpt_motion.hip")


# ---- nothing moved: the model is temporal_model's --------------------------------------------------------------------------
def frame(seed, n, t=5.0):
    rng = np.random.RandomState(seed)
    accum = np.zeros((H, W, 4), F)
    accum[..., :3] = rng.uniform(0, 2, (H, W, 3)) * n
    accum[..., 3] = n
    m2 = (rng.uniform(0, 6, (H, W)) * n).astype(F)
    albedo = np.ones((H, W, 4), F)
    albedo[..., 3] = rng.choice([0.0, 1.0, 2.0], size=(H, W))
    nd = np.zeros((H, W, 4), F)
    nd[..., 1] = 1
    nd[..., 3] = np.where(albedo[..., 3] != 0, t * rng.uniform(0.98, 1.02, (H, W)), 0)
    return accum, m2, albedo, nd


def test_model_equals_temporal_model_where_nothing_moved():
    cur, h = frame(1, 4), frame(2, 8)
    prev = (h[0], h[1], cur[2], h[3])
    rng = np.random.RandomState(3)
    pp = rng.normal(size=(H, W, 4)).astype(F) * 4
    pp[..., 3] = rng.choice([0.0, 2.0], size=(H, W))
    for cams in ((CAM_A, CAM_A), (CAM_A, CAM_B)):
        va, vb = ag.camera_vectors(cams[0]), ag.camera_vectors(cams[1])
        want = tm.accumulate(va, vb, *cur, prev, max_history=6.0)
        got = mm.accumulate_motion(va, vb, *cur, prev, pp, max_history=6.0)
        assert (want[0][..., 3] > cur[0][..., 3]).any()
        for g, w_ in zip(got, want):
            assert np.array_equal(g.view(np.uint32), w_.view(np.uint32))
        first = mm.accumulate_motion(va, vb, *cur, None, None)
        assert first[0].tobytes() == cur[0].tobytes() and first[1].tobytes() == cur[1].tobytes()


def test_prev_points_cases():
    old = np.arange(18, dtype=F).reshape(2, 3, 3)
    new = old.copy()
    new[1, 2, 0] += 1                                    # triangle 1 moved, triangle 0 did not
    O = np.array([0, 0, -1], F)
    D = np.array([[0, 0, 1]] * 4, F)
    ids = np.array([mm.MISS, mm.ANALYTIC, 0, 1])
    t, b1, b2 = np.array([0, 2, 3, 4], F), np.array([0, 0, .25, .25], F), np.array([0, 0, .5, .5], F)
    pp = mm.prev_points((ids, t, b1, b2), O, D, old, new)
    assert pp[:, 3].tolist() == [0, 2, 2, 1]
    assert pp[0].tolist() == [0, 0, 0, 0] and pp[1, :3].tolist() == [0, 0, 1] and pp[2, :3].tolist() == [0, 0, 2]
    assert pp[3, :3].tobytes() == ((old[1, 0] * F(.25) + old[1, 1] * F(.25)) + old[1, 2] * F(.5)).tobytes()
    # -0 against +0 counts as moved; the same NaN bytes do not
    z = old.copy()
    z[0, 0, 0] = -0.0
    assert mm.prev_points((ids, t, b1, b2), O, D, z, old)[2, 3] == 1
    n = old.copy()
    n[0, 1, 1] = np.nan
    assert mm.prev_points((ids, t, b1, b2), O, D, n, n.copy())[2, 3] == 2


# ---- the card scene -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def card_frames():
    """the two frames of the card scene from the CPU oracle: per frame (albedo, normal_depth, hits in film order), and frame 1's
    prev_point from the oracle's hits on the model's feature rays"""
    cw, ch = mm.CARD_W, mm.CARD_H
    frames = []
    for offset in ((0.0, 0.0, 0.0), mm.CARD_MOVE):
        albedo, nd, _, hits = host_features(mm.card_scene(offset), cw, ch)
        frames.append((albedo, nd, hits))
    O, once, D = mm.feature_rays(ag.camera_vectors(mm.CARD_CAMERA), cw, ch)
    rays = np.zeros(cw * ch, ob.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"] = O, once, mm.FLT_MAX
    hits, _ = oracle_scene(mm.card_scene(mm.CARD_MOVE)).intersect(rays)
    # (the same hits as host_features': its rays are the oracle camera's, the model's are the same bytes)
    assert np.array_equal(hits.reshape(ch, cw)[::-1]["prim"], frames[1][2]["prim"])
    assert np.array_equal(hits.reshape(ch, cw)[::-1]["t"].view(np.uint32), frames[1][2]["t"].view(np.uint32))
    rec = mm.hit_records(hits, {0: 0, mm.CARD_PRIM: mm.CARD_BASE})
    pp = mm.prev_points(rec, O, D, mm.generation(mm.card_meshes()), mm.generation(mm.card_meshes(mm.CARD_MOVE)))
    on_card = (hits["hit"] == 1) & (hits["prim"] == mm.CARD_PRIM)
    assert ((hits["hit"] == 1) & (hits["prim"] == 2)).any() and (hits["hit"] == 0).any()      # the light and the sky are in view
    return frames, pp.reshape(ch, cw, 4), on_card.reshape(ch, cw)


def card_buffers(seed=5):
    """(cur, prev) for frame 1 of the card scene: 4 samples now, a history of 8 everywhere on frame 0"""
    (f0, f1), _, _ = card_frames()
    rng = np.random.RandomState(seed)
    shape = f0[0].shape[:2]

    def sums(n):
        a = np.zeros(shape + (4,), F)
        a[..., :3] = rng.uniform(0, 2, shape + (3,)) * n
        a[..., 3] = n
        return a, (rng.uniform(0, 6, shape) * n).astype(F)
    acc, m2 = sums(4)
    h_acc, h_m2 = sums(8)
    return (acc, m2, f1[0], f1[1]), (h_acc, h_m2, f0[0], f0[1])


def test_card_scene_keeps_its_history_only_with_motion_vectors():
    _, pp, on_card = card_frames()
    cur, prev = card_buffers()
    va = ag.camera_vectors(mm.CARD_CAMERA)
    n_card = int(on_card.sum())
    assert n_card >= 100
    # w is 1 exactly on the card, 2 on the floor and the light, 0 on the sky
    assert np.array_equal(pp[..., 3] == 1, on_card)
    assert set(np.unique(pp[..., 3][~on_card])) <= {0.0, 2.0} and (pp[..., 3] == 2).any()
    out, _ = mm.accumulate_motion(va, va, *cur, prev, pp)
    control, _ = tm.accumulate(va, va, *cur, prev)
    took = out[..., 3] > cur[0][..., 3]
    took_control = control[..., 3] > cur[0][..., 3]
    share = took[on_card].mean()
    print("card scene %dx%d: %d card pixels, history for %.3f of them with motion vectors, for %d without"
          % (mm.CARD_W, mm.CARD_H, n_card, share, int(took_control[on_card].sum())))
    assert share >= 0.9
    assert not took_control[on_card].any()
    # off the card the two agree bit for bit
    assert out[~on_card].tobytes() == control[~on_card].tobytes()
