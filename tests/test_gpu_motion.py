"""Motion vectors on the GPU (agpt_scene_snapshot_positions, agpt_render_features_motion, agpt_temporal_accumulate_motion) against
the numpy model of their contracts (tests/motion_model.py): the feature pass bit for bit on full films and tiles, every update route
between two snapshots as REFIT and as REBUILD, the snapshot rules, the temporal call where nothing moved against
agpt_temporal_accumulate, the card scene (history follows the moved card; without motion vectors it is lost), synthetic buffers that hold
every case of prev_point, the argument checks that need a context, and the three calls on a caller's non-blocking stream."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import motion_model as mm
import temporal_model as tm
from helpers import bits as u32, film_point, gpu_context, gpu_scene, unit
from morph_cases import targets as morph_targets
from skin_cases import binding

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW, CH = mm.CARD_W, mm.CARD_H
CARD_BASES = {0: 0, mm.CARD_PRIM: mm.CARD_BASE}
PT = ag.PathTracer(5)


def model_prev_point(g, cam, W, H, meshes_old, meshes_new, bases):
    """the model's prev_point[H, W, 4] for the scene as it stands: the hits come from agpt_intersect_batch on the model's feature rays"""
    O, once, D = mm.feature_rays(ag.camera_vectors(cam), W, H)
    rays = np.zeros(W * H, ag.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"] = O, once, mm.FLT_MAX
    hits, _ = g.Intersect(rays)
    rec = mm.hit_records(hits, bases)
    pp = mm.prev_points(rec, O, D, mm.generation(meshes_old), mm.generation(meshes_new))
    return pp.reshape(H, W, 4), hits.reshape(H, W)


def check_features_motion(g, cam, W, H, meshes_old, meshes_new, bases, moved_prims):
    """render_features_motion on the full film: albedo / normal_depth are render_features' bytes, prev_point is the model's, w is 1
    exactly on the pixels of the moved primitives -> (albedo, normal_depth, prev_point, hits)"""
    g.set_camera(*cam)
    albedo, nd = PT.render_features_to_host(g, W, H)
    a2, n2, pp = PT.render_features_motion_to_host(g, W, H)
    assert a2.tobytes() == albedo.tobytes() and n2.tobytes() == nd.tobytes()
    model, hits = model_prev_point(g, cam, W, H, meshes_old, meshes_new, bases)
    differ = (u32(pp) != u32(model)).any(-1)
    assert not differ.any(), np.argwhere(differ)[:8]
    on_moved = (hits["hit"] == 1) & np.isin(hits["prim"], list(moved_prims))
    assert np.array_equal(pp[..., 3] == 1, on_moved)
    assert set(np.unique(pp[..., 3])) <= {0.0, 1.0, 2.0}
    return albedo, nd, pp, hits


# ---- 1. the feature pass ----------------------------------------------------------------------------------------------------
def with_normals(mesh):
    v, ix = mesh
    ix = ix.copy()
    ix[:, 1] = ix[:, 0]
    n = np.zeros_like(v)
    n[:, 2] = -1
    return v, n, ix


def two_mesh_scene():
    """two cards with vertex normals side by side (8 and 18 triangles) before the sky, no floor: the second mesh's triangle base is 8"""
    d = ag.scenes.SceneDesc("two-cards")
    m = [d.add_material(ag.MAT_DIFFUSE_ONLY, c) for c in ((0.2, 0.6, 0.3), (0.7, 0.6, 0.2))]
    for k, (n, dx) in enumerate(((2, -0.7), (3, 0.7))):
        v, nn, ix = with_normals(mm.card_mesh((dx, 0.0, 0.0), n))
        d.add_mesh(v, nn, None, ix, m[k])
    d.add_uniform_infinite_light([.5, .5, .5])
    d.set_camera(*mm.CARD_CAMERA)
    return d


def bent(v, amount=0.25):
    """a non-rigid pose: every vertex pushed along z by a function of its x and y"""
    p = v.astype(np.float64)
    p[:, 2] += amount * np.sin(3.0 * p[:, 0] + 1.0) * np.cos(2.0 * p[:, 1])
    p[:, 0] += 0.15
    return p.astype(F)


def test_features_pass_on_the_card_scene():
    g = gpu_scene(mm.card_scene())
    try:
        g.snapshot_positions()
        g.update_mesh(mm.CARD_PRIM, mm.card_mesh(mm.CARD_MOVE)[0], None, "refit")
        g.snapshot_positions()
        _, _, pp, hits = check_features_motion(g, mm.CARD_CAMERA, CW, CH, mm.card_meshes(), mm.card_meshes(mm.CARD_MOVE), CARD_BASES,
                                               [mm.CARD_PRIM])
        assert (pp[..., 3] == 1).sum() >= 100 and (pp[..., 3] == 2).any() and (pp[..., 3] == 0).any()
        # the sphere light is an analytic primitive: w = 2
        assert (pp[..., 3][(hits["hit"] == 1) & (hits["prim"] == 2)] == 2).all() and (hits["prim"] == 2).any()
    finally:
        g.close()


def test_features_pass_on_a_tile_with_a_pitch_and_a_second_mesh_that_moved():
    desc = two_mesh_scene()
    meshes = [(op[1], op[4]) for op in desc.ops if op[0] == "mesh"]
    moved = [meshes[0], (bent(meshes[1][0]), meshes[1][1])]
    g = gpu_scene(desc)
    ctx = gpu_context()
    W, H = 37, 19
    try:
        g.snapshot_positions()
        g.update_mesh(1, moved[1][0], desc.ops[3][2], "refit")
        g.snapshot_positions()
        albedo, nd, pp, _ = check_features_motion(g, mm.CARD_CAMERA, W, H, meshes, moved, {0: 0, 1: 8}, [1])
        assert (pp[..., 3] == 1).any() and (pp[..., 3] == 2).any() and (pp[..., 3] == 0).any()
        x0, y0, w, h = 5, 3, 29, 11
        pitch, row0 = W + 3, H - y0 - h
        sentinel = np.full((h, pitch, 4), -7.0, F)
        ptrs = [ctx.alloc(sentinel.nbytes) for _ in range(3)]
        try:
            for p in ptrs:
                ctx.upload(p, sentinel)
            PT.render_features_motion(g, W, H, *ptrs, tile=(x0, y0, w, h), accum_pitch=pitch, accum_row0=row0)
            got = [ctx.download(p, (h, pitch, 4)) for p in ptrs]
        finally:
            for p in ptrs:
                ctx.free(p)
        rows = slice(H - y0 - h, H - y0)
        outside = np.ones((h, pitch), bool)
        outside[:, x0:x0 + w] = False
        for t, full in zip(got, (albedo, nd, pp)):
            assert t[:, x0:x0 + w].tobytes() == full[rows, x0:x0 + w].tobytes()
            assert (t[outside] == -7.0).all()
    finally:
        g.close()


# ---- 2. every update route between the two snapshots ---------------------------------------------------------------------------
ROUTES = ("host", "transform", "pose", "morph", "fused", "smooth")
ROUTE_PRIM, ROUTE_BASE = 1, 2


def route_scene():
    """the card scene with vertex normals on the card (the routes move normals too)"""
    d = ag.scenes.SceneDesc("card+n")
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.6, 0.6, 0.6))
    red = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.7, 0.2, 0.15))
    d.add_mesh(mm.FLOOR[0], None, None, mm.FLOOR[1], grey)
    v, n, ix = with_normals(mm.card_mesh())
    assert d.add_mesh(v, n, None, ix, red, 2) == ROUTE_PRIM
    d.add_area_light(mm.LIGHT[0], mm.LIGHT[1], (40.0, 40.0, 40.0))
    d.set_camera(*mm.CARD_CAMERA)
    return d


def turn_y(degrees, centre=(0.0, 1.0, 0.0)):
    a = np.deg2rad(degrees)
    R = np.eye(4)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    t0, t1 = np.eye(4), np.eye(4)
    t0[:3, 3], t1[:3, 3] = -np.asarray(centre), np.asarray(centre)
    return (t1 @ R @ t0).astype(F)


JOINTS = np.stack([turn_y(20), turn_y(-15, (0.2, 1.0, 0.0)), np.eye(4, dtype=F)])


def apply_route(g, route, mode, rest):
    """moves the card of route_scene() on g by `route`; -> the positions the route's host twin gives"""
    v0, n0, ix = rest
    if route in ("host", "torch"):
        v1 = bent(v0)
        if route == "host":
            g.update_mesh(ROUTE_PRIM, v1, n0, mode)
        else:
            import torch
            g.update_mesh(ROUTE_PRIM, torch.from_numpy(v1).cuda(), torch.from_numpy(n0).cuda(), mode)
        return v1
    if route == "smooth":
        v1 = bent(v0)
        g.set_mesh_normals_mode(ROUTE_PRIM, "smooth")
        g.update_mesh(ROUTE_PRIM, v1, None, mode)
        return v1
    if route == "transform":
        M = turn_y(25)
        g.transform_mesh(ROUTE_PRIM, M, mode)
        return ag.transform_arrays(M, v0, n0)[0]
    J, Wt = binding(len(v0), 4, seed=11)
    dP, dN = morph_targets(len(v0), 3, seed=12, extent=1.0), morph_targets(len(n0), 3, seed=13, extent=1.0)
    w = np.array([0.75, 0.0, -0.5], F)
    if route == "pose":
        g.set_mesh_skin(ROUTE_PRIM, J, Wt, n_joints=3)
        g.pose_mesh(ROUTE_PRIM, JOINTS, mode)
        return ag.skin_arrays(JOINTS, v0, J, Wt, n0)[0]
    g.set_mesh_morph_targets(ROUTE_PRIM, dP, dN)
    mv, mn = ag.morph_arrays(w, v0, dP, n0, dN)
    if route == "morph":
        g.morph_mesh(ROUTE_PRIM, w, None, mode)
        return mv
    assert route == "fused"
    g.set_mesh_skin(ROUTE_PRIM, J, Wt, n_joints=3)
    g.morph_mesh(ROUTE_PRIM, w, JOINTS, mode)
    return ag.skin_arrays(JOINTS, mv, J, Wt, mn)[0]


def run_route(route, mode, ctx=None):
    """snapshot, the route, snapshot, the feature pass: prev_point is the model's on the route's host-twin arrays -> (prev_point,
    whether the BVH's slot order changed)"""
    desc = route_scene()
    g = desc.instantiate(ag.Scene(ctx if ctx is not None else gpu_context()))
    try:
        rest = with_normals(mm.card_mesh())
        _, order_before = g.bvh(ROUTE_PRIM)
        g.snapshot_positions()
        v1 = apply_route(g, route, mode, rest)
        assert np.isfinite(v1).all() and v1.tobytes() != rest[0].tobytes()
        g.snapshot_positions()
        old, new = [mm.FLOOR, (rest[0], rest[2])], [mm.FLOOR, (v1, rest[2])]
        _, _, pp, _ = check_features_motion(g, mm.CARD_CAMERA, CW, CH, old, new, {0: 0, ROUTE_PRIM: ROUTE_BASE}, [ROUTE_PRIM])
        assert (pp[..., 3] == 1).sum() >= 50
        _, order_after = g.bvh(ROUTE_PRIM)
        return pp, order_before.tobytes() != order_after.tobytes()
    finally:
        g.close()


@pytest.mark.parametrize("route", ROUTES)
def test_every_update_route_as_refit_and_as_rebuild(route):
    pp_refit, reordered = run_route(route, "refit")
    assert not reordered
    pp_rebuild, reordered = run_route(route, "rebuild")
    print("%s: the rebuild %s the slot order" % (route, "changed" if reordered else "kept"))
    if route in ("host", "smooth"):
        assert reordered                      # (the bent card's tree is another one: ids, not slots, index the snapshots)
    # the two trees hold the same triangles: where they name the same one (everywhere but on a shared edge) the bytes are equal
    same = (u32(pp_refit) == u32(pp_rebuild)).all(-1)
    assert same.mean() >= 0.99, same.mean()


TORCH_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch                      # before the library touches the GPU (INTEGRATION.md section 3)
torch.zeros(1, device="cuda")
import ag_pathtracer_amd as ag
import test_gpu_motion as t
ctx = ag.Context(0)
for mode in ("refit", "rebuild"):
    pp, _ = t.run_route("torch", mode, ctx)
    print("torch %%s: %%d moved pixels" %% (mode, int((pp[..., 3] == 1).sum())))
torch.cuda.synchronize()
ctx.close()
print("torch-ok")
"""


def test_the_torch_device_tensor_route():
    """Scene.update_mesh with torch tensors on the GPU (agpt_scene_update_mesh_device) between the two snapshots, in a child process:
    torch must initialise the GPU before the library does"""
    code = TORCH_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "torch-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_a_seventy_primitive_scene():
    """the long-list trace path: one of 70 meshes moves"""
    from test_gpu_mesh_update_device import seventy_prims
    desc = seventy_prims()
    meshes = [(op[1], op[4]) for op in desc.ops if op[0] == "mesh"]
    bases = dict(enumerate(mm.triangle_bases(meshes)))
    prim = 33
    v, n, _, _ = ag.scenes.blob_mesh(5, 4, center=(-1.5, 1.2, -2.0), radius=1.2, seed=prim)   # (some ten pixels across on the film below)
    assert v.shape == meshes[prim][0].shape and bases[prim] > 0
    moved = list(meshes)
    moved[prim] = (v, meshes[prim][1])
    g = gpu_scene(desc)
    try:
        g.snapshot_positions()
        g.update_mesh(prim, v, n, "refit")
        g.snapshot_positions()
        _, _, pp, _ = check_features_motion(g, desc.camera, CW, CH, meshes, moved, bases, [prim])
        assert (pp[..., 3] == 1).any() and (pp[..., 3] == 2).any()
    finally:
        g.close()


# ---- 3. the snapshot rules -------------------------------------------------------------------------------------------------------
def test_snapshot_rules():
    g = ag.Scene(gpu_context())
    try:
        with pytest.raises(ag.AgptError):
            g.snapshot_positions()                                    # not committed
        assert b"agpt_scene_snapshot_positions" in ag.lib().agpt_last_error()
        mm.card_scene().instantiate(g)
        with pytest.raises(ag.AgptError):
            PT.render_features_motion_to_host(g, CW, CH)              # no snapshot yet
        assert b"agpt_render_features_motion" in ag.lib().agpt_last_error() and b"snapshot" in ag.lib().agpt_last_error()
        poses = [mm.card_meshes(o) for o in ((0.0, 0.0, 0.0), (0.3, 0.0, -0.5), (-0.2, 0.1, 0.2))]
        g.snapshot_positions()                                        # one snapshot: both generations are pose 0
        _, _, pp, _ = check_features_motion(g, mm.CARD_CAMERA, CW, CH, poses[0], poses[0], CARD_BASES, [])
        assert set(np.unique(pp[..., 3])) == {0.0, 2.0}
        # three snapshots, two more poses: the older generation is the second-newest pose
        g.update_mesh(mm.CARD_PRIM, poses[1][1][0], None, "refit")
        g.snapshot_positions()
        check_features_motion(g, mm.CARD_CAMERA, CW, CH, poses[0], poses[1], CARD_BASES, [mm.CARD_PRIM])
        g.update_mesh(mm.CARD_PRIM, poses[2][1][0], None, "rebuild")
        g.snapshot_positions()
        check_features_motion(g, mm.CARD_CAMERA, CW, CH, poses[1], poses[2], CARD_BASES, [mm.CARD_PRIM])
        # moved and moved back between two snapshots: nothing moved
        g.update_mesh(mm.CARD_PRIM, poses[0][1][0], None, "refit")
        g.update_mesh(mm.CARD_PRIM, poses[2][1][0], None, "refit")
        g.snapshot_positions()
        _, _, pp, _ = check_features_motion(g, mm.CARD_CAMERA, CW, CH, poses[2], poses[2], CARD_BASES, [])
        assert set(np.unique(pp[..., 3])) == {0.0, 2.0}
        # a commit drops both generations
        g.commit()
        with pytest.raises(ag.AgptError):
            PT.render_features_motion_to_host(g, CW, CH)
        g.snapshot_positions()
        assert set(np.unique(PT.render_features_motion_to_host(g, CW, CH)[2][..., 3])) == {0.0, 2.0}
    finally:
        g.close()


def test_a_scene_without_triangles():
    d = ag.scenes.SceneDesc("spheres")
    m = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.5, 0.5, 0.5))
    d.add_sphere((0.0, 1.0, 0.0), 0.7, m)
    d.add_uniform_infinite_light([.5, .5, .5])
    d.set_camera(*mm.CARD_CAMERA)
    g = gpu_scene(d)
    try:
        g.snapshot_positions()
        _, _, pp, hits = check_features_motion(g, mm.CARD_CAMERA, 5, 3, [], [], {}, [])
        assert (hits["hit"] == 1).any() and set(np.unique(pp[..., 3])) == {0.0, 2.0}
    finally:
        g.close()


# ---- 4. nothing moved: agpt_temporal_accumulate's bytes ------------------------------------------------------------------------
def test_nothing_moved_equals_temporal_accumulate_on_rendered_frames():
    import test_gpu_temporal as tt
    cur, prev, out = tt.rendered_pair()
    g = tt.c1_scene()
    g.snapshot_positions()
    g.set_camera(*tt.C1_CAM)
    albedo, nd, pp = PT.render_features_motion_to_host(g, tt.RW, tt.RH)
    assert albedo.tobytes() == cur[2].tobytes() and nd.tobytes() == cur[3].tobytes()
    assert set(np.unique(pp[..., 3])) == {0.0, 2.0}
    ctx = gpu_context()
    for cams, want in (((tt.C1_CAM, tt.C1_PAN), out), ((tt.C1_CAM, tt.C1_CAM), tt.run_gpu((tt.C1_CAM, tt.C1_CAM), cur, prev))):
        got = ctx.temporal_to_host(cams[0], cams[1], *cur, prev=prev, prev_point=pp)
        assert (want[0][..., 3] > cur[0][..., 3]).any()
        assert np.array_equal(u32(got[0]), u32(want[0])) and np.array_equal(u32(got[1]), u32(want[1]))


# ---- 5. the card scene -------------------------------------------------------------------------------------------------------------
def render_card_frame(g, k, motion):
    acc, m2, _, _ = PT.render_adaptive_to_host(g, CW, CH, 4, 4, 4, 0.0, seed_base=k + 1)
    assert (acc[..., 3] == 4).all()
    if motion:
        return (acc, m2) + PT.render_features_motion_to_host(g, CW, CH)
    return (acc, m2) + PT.render_features_to_host(g, CW, CH)


@pytest.mark.parametrize("move", ["translate", "turn"])
def test_card_scene_history_follows_the_card(move):
    """frame 0 at rest, frame 1 with the card moved 0.5 towards the camera and 0.3 sideways -- or turned 5 degrees by transform_mesh.
    The existing call finds no history for the translated card (the control); the motion call does, and equals the model bit for bit."""
    ctx = gpu_context()
    g = gpu_scene(mm.card_scene())
    try:
        g.snapshot_positions()
        f0 = render_card_frame(g, 0, False)
        prev = (f0[0], f0[1], f0[2], f0[3])                    # the first frame's history is the frame itself
        if move == "translate":
            new = mm.card_mesh(mm.CARD_MOVE)[0]
            g.update_mesh(mm.CARD_PRIM, new, None, "refit")
        else:
            M = turn_y(5.0)
            new = ag.transform_arrays(M, mm.card_mesh()[0])[0]
            g.transform_mesh(mm.CARD_PRIM, M, "refit")
        g.snapshot_positions()
        acc, m2, albedo, nd, pp = render_card_frame(g, 1, True)
        model_pp, hits = model_prev_point(g, mm.CARD_CAMERA, CW, CH, mm.card_meshes(), [mm.FLOOR, (new, mm.card_mesh()[1])], CARD_BASES)
        assert np.array_equal(u32(pp), u32(model_pp))
        on_card = (hits["hit"] == 1) & (hits["prim"] == mm.CARD_PRIM)
        assert on_card.sum() >= 100 and np.array_equal(pp[..., 3] == 1, on_card)
        cur = (acc, m2, albedo, nd)
        control = ctx.temporal_to_host(mm.CARD_CAMERA, mm.CARD_CAMERA, *cur, prev=prev)
        got = ctx.temporal_to_host(mm.CARD_CAMERA, mm.CARD_CAMERA, *cur, prev=prev, prev_point=pp)
        va = ag.camera_vectors(mm.CARD_CAMERA)
        model = mm.accumulate_motion(va, va, *cur, prev, pp, identity=True)
        took, took_control = got[0][..., 3] > 4, control[0][..., 3] > 4
        print("card %s: %d card pixels, history for %.3f of them with motion vectors, for %.3f without"
              % (move, int(on_card.sum()), took[on_card].mean(), took_control[on_card].mean()))
        assert np.array_equal(u32(got[0]), u32(model[0])) and np.array_equal(u32(got[1]), u32(model[1]))
        assert took[on_card].mean() >= 0.9
        if move == "translate":
            assert not took_control[on_card].any()
    finally:
        g.close()


# ---- 6. synthetic buffers ----------------------------------------------------------------------------------------------------------
CAM_CUR = ([0.3, 1.4, -6.0], [0.0, 0.0, 0.0], [0, 1, 0], 37 / 19.0, 42.0, 0.0)
CAM_PREV = ([0.58, 0.62, -3.62], [0.5, 0.3, 0.0], [0.05, 1, 0], 37 / 19.0, 42.0, 0.0)
MAX_HISTORY, DEPTH_TOL, NORMAL_COS = 6.0, 0.0625, 0.9


def synthetic(W, H, cam_prev, seed=20250114):
    """(cur, prev, prev_point): random buffers; prev_point's w from {0, 1, 2, 3, NaN}; its points in front of the previous camera and
    on its film (the previous buffers made coherent there so that the history is accepted), behind it, off its film, in runs of
    adjacent floats across each film edge, and with NaN and Inf coordinates"""
    rng = np.random.RandomState(seed + W)
    P = tm.camera(ag.camera_vectors(cam_prev))
    flag = rng.choice([0.0, 1.0, 2.0], size=(H, W), p=[0.2, 0.6, 0.2]).astype(F)
    geometry = flag != 0
    albedo = np.ones((H, W, 4), F)
    albedo[..., 3] = flag
    nd = np.zeros((H, W, 4), F)
    nd[..., :3] = np.where(geometry[..., None], unit(rng.normal(size=(H, W, 3))), 0)
    nd[..., 3] = np.where(geometry, rng.uniform(1.5, 9.0, (H, W)), 0)
    n_c = np.where(rng.uniform(size=(H, W)) < 0.1, 0.0, 4.0).astype(F)
    accum = np.zeros((H, W, 4), F)
    accum[..., :3] = rng.uniform(0, 2, (H, W, 3)) * n_c[..., None]
    accum[..., 3] = n_c
    m2 = (rng.uniform(0, 6, (H, W)) * n_c).astype(F)
    p_albedo = np.ones((H, W, 4), F)
    p_albedo[..., 3] = rng.choice([0.0, 1.0, 2.0], size=(H, W))
    p_nd = np.zeros((H, W, 4), F)
    p_nd[..., :3] = unit(rng.normal(size=(H, W, 3)))
    p_nd[..., 3] = rng.uniform(1.0, 9.0, (H, W))
    n_q = rng.choice([0.0, 1.5, 3.0, 8.0, 12.25], size=(H, W), p=[0.1, 0.2, 0.2, 0.25, 0.25]).astype(F)
    h_acc = np.zeros((H, W, 4), F)
    h_acc[..., :3] = rng.uniform(0, 2, (H, W, 3)) * n_q[..., None]
    h_acc[..., 3] = n_q
    h_m2 = (rng.uniform(0, 6, (H, W)) * n_q).astype(F)

    pp = np.zeros((H, W, 4), F)
    pp[..., 3] = rng.choice(np.array([0.0, 1.0, 2.0, 3.0, np.nan], F), size=(H, W), p=[0.1, 0.6, 0.1, 0.1, 0.1])
    kinds = rng.choice(["film", "behind", "off", "nonfinite"], size=(H, W), p=[0.6, 0.15, 0.15, 0.1])
    if W * H == 1:                                   # the one pixel of the smallest film moved, and to a place on the film
        pp[..., 3], kinds[...] = 1, "film"
    edge_runs = []
    for r in range(H):
        for c in range(W):
            k = kinds[r, c]
            depth = rng.uniform(1.5, 9.0)
            if k == "film":
                p = film_point(P, rng.uniform(0.02, 0.98), rng.uniform(0.02, 0.98), depth)
            elif k == "behind":
                p = P["origin"].astype(np.float64) + depth * P["w"].astype(np.float64) + rng.normal(size=3) * 0.3
            elif k == "off":
                p = film_point(P, rng.choice([-0.6, 1.7]), rng.uniform(-0.5, 1.5), depth)
            else:
                p = rng.normal(size=3)
                p[rng.randint(3)] = rng.choice([np.nan, np.inf, -np.inf])
            pp[r, c, :3] = p
    va, vb = ag.camera_vectors(CAM_CUR), ag.camera_vectors(cam_prev)

    def on_film(q):
        probe = np.empty((H, W, 4), F)
        probe[...] = (q[0], q[1], q[2], 1.0)
        return bool(mm.position(va, vb, False, flag, nd[..., 3], probe, W, H)[0]["found"][0, 0])

    # runs of 8 adjacent floats across each film edge (sx = -1, sx = W, sy = -1, sy = H), in the first pixels of the film: one
    # coordinate of a point on the edge is bisected, by the model's own arithmetic, down to the two neighbours the edge lies between
    flat = pp.reshape(-1, 4)
    at = 0
    for axis, edge in ((0, -0.5 / W), (0, (W + 0.5) / W), (1, -0.5 / H), (1, (H + 0.5) / H)):
        if at + 8 > len(flat):
            break
        base = film_point(P, edge if axis == 0 else 0.5, edge if axis == 1 else 0.5, 4.0).astype(F)
        j = int(np.argmax(np.abs(P["horizontal" if axis == 0 else "vertical"])))
        ends = [base.copy(), base.copy()]
        ends[0][j] -= F(0.05)
        ends[1][j] += F(0.05)
        assert on_film(ends[0]) != on_film(ends[1])
        lo, hi = (int(e[j:j + 1].view(np.int32)[0]) for e in ends)     # (one sign: the integers order like the floats)
        assert (lo < 0) == (hi < 0)
        inside_lo = on_film(ends[0])
        while abs(hi - lo) > 1:
            mid = (lo + hi) // 2
            q = base.copy()
            q[j:j + 1] = np.array([mid], np.int32).view(F)
            lo, hi = (mid, hi) if on_film(q) == inside_lo else (lo, mid)
        step = 1 if hi > lo else -1
        run = []
        for k in range(-3, 5):
            q = base.copy()
            q[j:j + 1] = np.array([lo + k * step], np.int32).view(F)
            flat[at] = (q[0], q[1], q[2], 1.0)
            run.append(at)
            at += 1
        edge_runs.append(run)
    pp = flat.reshape(H, W, 4)

    # the previous buffers coherent where the moved pixels land, so that their history is accepted
    pos, moved = mm.position(va, vb, False, flag, nd[..., 3], pp, W, H)
    for r, c in zip(*np.nonzero(moved & pos["found"] & (rng.uniform(size=(H, W)) < 0.8))):
        for tap in range(4):
            qx, qy = pos["x0"][r, c] + (tap & 1), pos["y0"][r, c] + (tap >> 1)
            if 0 <= qx < W and 0 <= qy < H:
                q = (H - 1 - qy, qx)
                p_albedo[q][3] = flag[r, c]
                p_nd[q][3] = pos["te"][r, c] * F(1 + rng.uniform(-0.03, 0.03))
                p_nd[q][:3] = unit(nd[r, c, :3] + rng.normal(size=3) * 0.08) if geometry[r, c] else 0
                if h_acc[q][3] == 0:
                    h_acc[q] = (3.0, 2.0, 1.0, 8.0)
    return (accum, m2, albedo, nd), (h_acc, h_m2, p_albedo, p_nd), pp, edge_runs


@pytest.mark.parametrize("film", [(1, 1), (5, 3), (37, 19)])
@pytest.mark.parametrize("cameras", ["different", "equal"])
def test_synthetic_buffers_match_the_model_bit_for_bit(film, cameras):
    W, H = film
    cam_prev = CAM_PREV if cameras == "different" else CAM_CUR
    cur, prev, pp, edge_runs = synthetic(W, H, cam_prev)
    va, vb = ag.camera_vectors(CAM_CUR), ag.camera_vectors(cam_prev)
    kw = dict(max_history=MAX_HISTORY, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    model = mm.accumulate_motion(va, vb, *cur, prev, pp, **kw)
    if (W, H) == (37, 19):
        # every case occurs in these inputs
        pos, moved = mm.position(va, vb, cameras == "equal", cur[2][..., 3], cur[3][..., 3], pp, W, H)
        took = model[0][..., 3] > cur[0][..., 3]
        assert (moved & took).any() and (moved & ~pos["found"]).any() and (moved & pos["found"] & ~took).any()
        assert (~moved & took).any() and (~moved & ~took).any()
        assert np.isnan(pp[..., 3]).any() and (pp[..., 3] == 3).any() and (~np.isfinite(pp[..., :3])[moved]).any()
        found = pos["found"].reshape(-1)
        for run in edge_runs:
            assert len(run) == 8 and found[run].any() and not found[run].all(), found[run]     # the run straddles its edge
        assert len(edge_runs) == 4
        if cameras == "equal":
            plain = tm.accumulate(va, vb, *cur, prev, **kw)
            assert plain[0].tobytes() != model[0].tobytes()                                    # (the points, not the pixels, decide)
        print("synthetic %dx%d, %s cameras: %d moved pixels, %d of them with history, %d not found"
              % (W, H, cameras, moved.sum(), (moved & took).sum(), (moved & ~pos["found"]).sum()))
    ctx = gpu_context()
    a = ctx.temporal_to_host(CAM_CUR, cam_prev, *cur, prev=prev, prev_point=pp, **kw)
    b = ctx.temporal_to_host(CAM_CUR, cam_prev, *cur, prev=prev, prev_point=pp, **kw)
    differ = (u32(a[0]) != u32(model[0])).any(-1) | (u32(a[1]) != u32(model[1]))
    print("pixels that differ from the model: %d" % differ.sum())
    assert not differ.any(), np.argwhere(differ)[:8]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # the first frame: the current values, and prev_point is not read
    first = ctx.temporal_to_host(CAM_CUR, cam_prev, *cur, prev=None, prev_point=pp)
    assert first[0].tobytes() == cur[0].tobytes() and first[1].tobytes() == cur[1].tobytes()


# ---- 7. the argument checks that need a context ------------------------------------------------------------------------------------
def test_arguments_that_need_a_context():
    ctx = gpu_context()
    W, H = 5, 3
    cur, prev, pp, _ = synthetic(W, H, CAM_PREV)
    host = list(cur) + list(prev)
    ptrs = [ctx.alloc(a.nbytes) for a in host] + [ctx.alloc(W * H * 16), ctx.alloc(W * H * 4), ctx.alloc(pp.nbytes)]
    try:
        for p, a in zip(ptrs, host):
            ctx.upload(p, a)
        ctx.upload(ptrs[10], pp)
        params = ag.TemporalParams(W, H, ag.camera_desc(*CAM_CUR), ag.camera_desc(*CAM_PREV), MAX_HISTORY, DEPTH_TOL, NORMAL_COS)
        ctx.temporal_accumulate_motion(params, *ptrs)
        good = ctx.download(ptrs[8], (H, W, 4))
        for p, a in zip(ptrs[:8] + ptrs[10:], host + [pp]):
            assert ctx.download(p, a.shape).tobytes() == a.tobytes()        # the inputs are left alone

        def refused(args, word):
            with pytest.raises(ag.AgptError):
                ctx.temporal_accumulate_motion(params, *args)
            msg = ag.lib().agpt_last_error()
            assert b"agpt_temporal_accumulate_motion" in msg and word in msg, msg
        for k in (0, 1, 2, 3, 8, 9):                       # the existing checks, in their order
            refused(ptrs[:k] + [0] + ptrs[k + 1:], b"NULL")
        for k in (4, 5, 6, 7):
            refused(ptrs[:k] + [0] + ptrs[k + 1:], b"prev")
        for k in range(8):
            refused(ptrs[:8] + [ptrs[k], ptrs[9], ptrs[10]], b"alias")
        refused(ptrs[:8] + [ptrs[8], ptrs[8], ptrs[10]], b"outputs")
        refused(ptrs[:10] + [0], b"prev_point")            # then a NULL prev_point_cur
        refused(ptrs[:8] + [ptrs[10], ptrs[9], ptrs[10]], b"prev_point")    # then an output aliasing it
        refused(ptrs[:8] + [ptrs[8], ptrs[10], ptrs[10]], b"prev_point")
        refused(ptrs[:8] + [ptrs[0], ptrs[9], 0], b"alias")                 # the existing checks come first
        refused(ptrs[:6] + [0, 0] + ptrs[8:10] + [0], b"prev buffers")
        assert ctx.download(ptrs[8], (H, W, 4)).tobytes() == good.tobytes()
    finally:
        for p in ptrs:
            ctx.free(p)
    # agpt_render_features_motion: NULL or aliased outputs
    g = gpu_scene(mm.card_scene())
    out = [ctx.alloc(CW * CH * 16) for _ in range(3)]
    try:
        g.snapshot_positions()
        for args in ((out[0], out[1], 0), (out[0], out[1], out[0]), (out[0], out[1], out[1]), (out[0], out[0], out[2]), (0, out[1], out[2])):
            with pytest.raises(ag.AgptError):
                PT.render_features_motion(g, CW, CH, *args)
            assert b"agpt_render_features_motion" in ag.lib().agpt_last_error()
        with pytest.raises(ag.AgptError):
            PT.render_features_motion(g, CW, CH, *out, tile=(0, 0, CW + 1, CH))
        PT.render_features_motion(g, CW, CH, *out)
    finally:
        for p in out:
            ctx.free(p)
        g.close()


# ---- 8. a caller's non-blocking stream ------------------------------------------------------------------------------------------
def test_the_three_calls_on_a_non_blocking_stream():
    """the six-step shape of tests/test_gpu_streams.py: the outputs hold a constant and are cleared behind the delay, the temporal
    call's inputs hold another frame's values until the caller's copies behind the delay put the real ones there"""
    from test_gpu_streams import Stage
    W, H = 37, 19
    cur, prev, pp_syn, _ = synthetic(W, H, CAM_PREV)
    wrong_cur, wrong_prev, wrong_pp, _ = synthetic(W, H, CAM_PREV, seed=77)
    with Stage() as st:
        g = st.scene(mm.card_scene())
        st.open()
        st.call("snapshot_positions (first)", g.snapshot_positions)
        g.update_mesh(mm.CARD_PRIM, mm.card_mesh(mm.CARD_MOVE)[0], None, "refit")
        st.open()
        st.call("snapshot_positions", g.snapshot_positions)
        outs = [st.output((CH, CW, 4), -7.0) for _ in range(3)]
        st.open(outs)
        st.call("render_features_motion", PT.render_features_motion, g, CW, CH, *[b.dst for b in outs])
        albedo, nd, pp = (st.read(b) for b in outs)
        model_pp, hits = model_prev_point(g, mm.CARD_CAMERA, CW, CH, mm.card_meshes(), mm.card_meshes(mm.CARD_MOVE), CARD_BASES)
        assert np.array_equal(u32(pp), u32(model_pp)) and (pp[..., 3] == 1).sum() >= 100
        ref = PT.render_features_to_host(g, CW, CH)
        assert albedo.tobytes() == ref[0].tobytes() and nd.tobytes() == ref[1].tobytes()
        # agpt_temporal_accumulate_motion
        ins = [st.buffer(real, wrong) for real, wrong in zip(list(cur) + list(prev) + [pp_syn], list(wrong_cur) + list(wrong_prev) + [wrong_pp])]
        hacc, hm2 = st.output((H, W, 4), -7.0), st.output((H, W), -7.0)
        params = ag.TemporalParams(W, H, ag.camera_desc(*CAM_CUR), ag.camera_desc(*CAM_PREV), MAX_HISTORY, DEPTH_TOL, NORMAL_COS)
        st.open(ins + [hacc, hm2])
        st.call("temporal_accumulate_motion", st.ctx.temporal_accumulate_motion, params, *([b.dst for b in ins[:8]] + [hacc.dst, hm2.dst, ins[8].dst]))
        got = st.read(hacc), st.read(hm2)
    model = mm.accumulate_motion(ag.camera_vectors(CAM_CUR), ag.camera_vectors(CAM_PREV), *cur, prev, pp_syn, max_history=MAX_HISTORY,
                                 depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    assert np.array_equal(u32(got[0]), u32(model[0])) and np.array_equal(u32(got[1]), u32(model[1]))
