"""Previous-frame normals on the GPU (agpt_scene_snapshot_surfaces, agpt_render_features_surface_motion,
agpt_temporal_accumulate_surface_motion, agpt_kat_surface): the temporal call against the merged calls on a substituted buffer bit for
bit; prev_normal against agpt_kat_surface on the older generation and against a second scene committed from the old arrays, at every
texturing level; the turning card, which keeps its history only with the new call; the snapshot rules; the argument checks; a caller's
stream, the torch route and the C++ example."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import motion_model as mm
import surface_motion_model as sm
import texture_filter_model as fm
import texture_model as txm
from helpers import bits as u32, build_cpp_example, gpu_context, gpu_scene, unit

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW, CH = mm.CARD_W, mm.CARD_H
PT = ag.PathTracer(5)
KW = dict(max_history=6.0, depth_tol=0.0625, normal_cos=0.9)


# ---- 1. the temporal call against the merged calls ------------------------------------------------------------------------------
SEEDS = {(5, 3): dict(seed=36)}      # (checked with the model alone: four moved geometry pixels of this film take history)


def synthetic_with_normals(W, H, cam_prev):
    """test_gpu_motion's synthetic buffers plus prev_normal.  The moved pixels take turns through five kinds: 0 the current normal is
    made to fail while prev_normal keeps the coherent one, 1 prev_normal random (fails) while the current one stays, 2 both near the
    coherent one, 3 a NaN in prev_normal, 4 prev_normal the current normal's bits -> (cur, prev, prev_point, prev_normal)"""
    import test_gpu_motion as gm
    cur, prev, pp, _ = gm.synthetic(W, H, cam_prev, **SEEDS.get((W, H), {}))
    rng = np.random.RandomState(99 + W)
    nd = cur[3].copy()
    pn = np.zeros((H, W, 4), F)
    pn[..., :3] = unit(rng.normal(size=(H, W, 3)))               # (pixels that did not move: never read)
    pn[..., 3] = pp[..., 3]
    # the pixels whose history the merged call accepts come first: the kinds decide something there
    va, vb = ag.camera_vectors(gm.CAM_CUR), ag.camera_vectors(cam_prev)
    took = mm.accumulate_motion(va, vb, *cur, prev, pp, **KW)[0][..., 3] > cur[0][..., 3]
    moved = pp[..., 3] == 1
    first = moved & took & (cur[2][..., 3] != 0)
    order = list(zip(*np.nonzero(first))) + list(zip(*np.nonzero(moved & ~first)))
    for k, (r, c) in enumerate(order):
        kind = k % 5
        if kind == 0:
            pn[r, c, :3] = nd[r, c, :3]
            nd[r, c, :3] = unit(-nd[r, c, :3] + rng.normal(size=3) * 0.1) if cur[2][r, c, 3] != 0 else nd[r, c, :3]
        elif kind == 2:
            pn[r, c, :3] = unit(nd[r, c, :3] + rng.normal(size=3) * 0.02) if cur[2][r, c, 3] != 0 else nd[r, c, :3]
        elif kind == 3:
            pn[r, c, rng.randint(3)] = np.nan
        elif kind == 4:
            pn[r, c, :3] = nd[r, c, :3]
    return (cur[0], cur[1], cur[2], nd), prev, pp, pn


def clamp_of(radius):
    return None if radius is None else ag.TemporalClampParams(radius, 1, 1.0, 3.0)


def clamp_model_of(radius):
    return None if radius is None else dict(radius=radius, demodulate=1, gamma=1.0, clamped_max_history=3.0)


@pytest.mark.parametrize("radius", [None, 1, 3])
@pytest.mark.parametrize("film", [(1, 1), (5, 3), (37, 19)])
@pytest.mark.parametrize("cameras", ["different", "equal"])
def test_temporal_call_equals_the_merged_calls_on_the_substituted_buffer(film, cameras, radius):
    import test_gpu_motion as gm
    W, H = film
    cam_prev = gm.CAM_PREV if cameras == "different" else gm.CAM_CUR
    cur, prev, pp, pn = synthetic_with_normals(W, H, cam_prev)
    va, vb = ag.camera_vectors(gm.CAM_CUR), ag.camera_vectors(cam_prev)
    moved = pp[..., 3] == 1
    # the census, by the model alone: which moved pixels take history with the current normal, which with the previous one
    with_cur = mm.accumulate_motion(va, vb, *cur, prev, pp, **KW)[0][..., 3] > cur[0][..., 3]
    with_prev = sm.accumulate_surface_motion(va, vb, *cur, prev, pp, pn, **KW)[0][..., 3] > cur[0][..., 3]
    print("synthetic %dx%d %s: %d moved; history with prev_normal only %d, with the current normal only %d, with both %d, NaN normals %d"
          % (W, H, cameras, moved.sum(), (moved & with_prev & ~with_cur).sum(), (moved & with_cur & ~with_prev).sum(),
             (moved & with_cur & with_prev).sum(), (moved & np.isnan(pn[..., :3]).any(-1)).sum()))
    if W * H > 1:
        assert (moved & with_prev & ~with_cur).any() and (moved & with_cur & ~with_prev).any()
        assert (moved & np.isnan(pn[..., :3]).any(-1)).any() and (moved & (u32(pn[..., :3]) == u32(cur[3][..., :3])).all(-1)).any()
    if W * H > 15:
        assert (moved & with_cur & with_prev).any()
        assert np.array_equal(with_cur[~moved], with_prev[~moved])
    ctx = gpu_context()
    clamp = clamp_of(radius)
    got = ctx.temporal_to_host(gm.CAM_CUR, cam_prev, *cur, prev=prev, prev_point=pp, prev_normal=pn, clamp=clamp, **KW)
    sub = (cur[0], cur[1], cur[2], sm.substituted(cur[3], pp, pn))
    want = ctx.temporal_to_host(gm.CAM_CUR, cam_prev, *sub, prev=prev, prev_point=pp, clamp=clamp, **KW)
    differ = (u32(got[0]) != u32(want[0])).any(-1) | (u32(got[1]) != u32(want[1]))
    assert not differ.any(), np.argwhere(differ)[:8]
    model = sm.accumulate_surface_motion(va, vb, *cur, prev, pp, pn, clamp=clamp_model_of(radius), **KW)
    assert np.array_equal(u32(got[0]), u32(model[0])) and np.array_equal(u32(got[1]), u32(model[1]))
    if W * H > 1:
        plain = ctx.temporal_to_host(gm.CAM_CUR, cam_prev, *cur, prev=prev, prev_point=pp, clamp=clamp, **KW)
        assert plain[0].tobytes() != got[0].tobytes()                      # (the previous normal decides somewhere)
    # prev_normal with the current normal's bits everywhere: the merged call on the unmodified buffers
    same = np.concatenate([cur[3][..., :3], pp[..., 3:]], -1)
    a = ctx.temporal_to_host(gm.CAM_CUR, cam_prev, *cur, prev=prev, prev_point=pp, prev_normal=same, clamp=clamp, **KW)
    b = ctx.temporal_to_host(gm.CAM_CUR, cam_prev, *cur, prev=prev, prev_point=pp, clamp=clamp, **KW)
    assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(u32(a[1]), u32(b[1]))
    # the first frame: the current values, neither prev_point nor prev_normal is read
    first = ctx.temporal_to_host(gm.CAM_CUR, cam_prev, *cur, prev=None, prev_point=pp, prev_normal=pn, clamp=clamp)
    assert first[0].tobytes() == cur[0].tobytes() and first[1].tobytes() == cur[1].tobytes()


# ---- 2. the feature pass, plain level -------------------------------------------------------------------------------------------
FW, FH = 61, 47                     # 2867 pixels: eleven blocks and a part of one
BLOB_PRIM, BLOB_AT = 3, ((-1.15, 1.0, 0.3), 0.55)


def blob(seed=4):
    v, n, _, ix = ag.scenes.blob_mesh(7, 5, center=BLOB_AT[0], radius=BLOB_AT[1], seed=seed)
    return v.astype(F), n.astype(F), ix


def card_and_blob(card_verts=None, blob_arrays=None):
    """motion_model's card scene (floor, card, sphere light) plus a blob with vertex normals beside the card"""
    d = sm.card_scene_with(mm.card_mesh()[0] if card_verts is None else card_verts)
    green = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.2, 0.6, 0.3))
    v, n, ix = blob()
    if blob_arrays is not None:
        v, n = blob_arrays
    assert d.add_mesh(v, n, None, ix, green) == BLOB_PRIM
    return d


def bent_blob():
    """a non-rigid pose of the blob: positions sheared and pushed, normals turned and left unnormalised"""
    v, n, _ = blob()
    p = v.astype(np.float64)
    p[:, 0] += 0.2 * np.sin(4.0 * p[:, 1]) + 0.1
    p[:, 2] -= 0.15 * p[:, 1]
    M = sm.turn_y(35.0, BLOB_AT[0])[:3, :3].astype(np.float64)
    return p.astype(F), (n.astype(np.float64) @ M.T * 1.3).astype(F)


def pixel_hits(g, cam, W, H, bases):
    """per pixel of the film, in buffer order: (hits, global triangle id or -1) from agpt_intersect_batch on the model's feature rays"""
    O, once, _ = mm.feature_rays(ag.camera_vectors(cam), W, H)
    rays = np.zeros(W * H, ag.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"] = O, once, mm.FLT_MAX
    hits, _ = g.Intersect(rays)
    ids = mm.hit_records(hits, bases)[0]
    return hits.reshape(H, W), np.where(ids >= 0, ids, -1).reshape(H, W)


def kat_at(g, hits, ids, mask, generation):
    """agpt_kat_surface on the pixels of `mask` -> ns[H, W, 3] (zero elsewhere), ss[H, W, 3]"""
    ns, ss = np.zeros(ids.shape + (3,), F), np.zeros(ids.shape + (3,), F)
    if mask.any():
        ns[mask], ss[mask] = g.kat_surface(ids[mask], hits["b1"][mask], hits["b2"][mask], generation)
    return ns, ss


def check_surface_features(g, cam, W, H, bases, old_scene=None):
    """render_features_surface_motion on the full film: three buffers are render_features_motion's bytes; prev_normal follows the
    header's table with agpt_kat_surface(1) as the yardstick -> the four buffers, hits, ids"""
    g.set_camera(*cam)
    a3 = PT.render_features_motion_to_host(g, W, H)
    albedo, nd, pp, pn = PT.render_features_surface_motion_to_host(g, W, H)
    for got, want in zip((albedo, nd, pp), a3):
        assert got.tobytes() == want.tobytes()
    hits, ids = pixel_hits(g, cam, W, H, bases)
    on_mesh = ids >= 0
    live, _ = kat_at(g, hits, ids, on_mesh, -1)
    assert np.array_equal(u32(live)[on_mesh], u32(nd[..., :3])[on_mesh])            # the KAT is the feature kernel's arithmetic
    followed = on_mesh & (pp[..., 3] == 1)
    old_ns, _ = kat_at(g, hits, ids, followed, 1)
    want = sm.prev_normals(pp, nd, followed, old_ns)
    differ = (u32(pn) != u32(want)).any(-1)
    assert not differ.any(), np.argwhere(differ)[:8]
    assert pn[..., 3].tobytes() == pp[..., 3].tobytes()
    miss = pp[..., 3] == 0
    assert (u32(pn)[miss] == 0).all() and np.array_equal(u32(pn[..., :3])[pp[..., 3] == 2], u32(nd[..., :3])[pp[..., 3] == 2])
    if old_scene is not None:                                                            # a second scene committed from the old arrays
        again, _ = kat_at(old_scene, hits, ids, followed, -1)
        assert np.array_equal(u32(again)[followed], u32(pn[..., :3])[followed])
    return albedo, nd, pp, pn, hits, ids


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_features_pass_follows_a_turned_card_and_a_bent_mesh_with_normals(mode):
    desc = card_and_blob()
    bases = {0: 0, mm.CARD_PRIM: mm.CARD_BASE, BLOB_PRIM: mm.CARD_BASE + 72}
    g, old = gpu_scene(desc), gpu_scene(desc)
    ctx = gpu_context()
    try:
        g.snapshot_surfaces()
        g.transform_mesh(mm.CARD_PRIM, sm.turn_y(sm.TURN_DEGREES), mode)
        g.update_mesh(BLOB_PRIM, *bent_blob(), mode)
        g.snapshot_surfaces()
        albedo, nd, pp, pn, hits, ids = check_surface_features(g, mm.CARD_CAMERA, FW, FH, bases, old)
        on_card, on_blob = (ids >= mm.CARD_BASE) & (ids < mm.CARD_BASE + 72), ids >= mm.CARD_BASE + 72
        assert (pp[..., 3][on_card] == 1).all() and (pp[..., 3][on_blob] == 1).all() and on_card.sum() >= 100 and on_blob.sum() >= 100
        assert (pp[..., 3] == 2).any() and (pp[..., 3] == 0).any()
        # the old normals are other normals: the card's is its rest normal, the blob's differ nearly everywhere
        assert (np.abs(pn[..., 2][on_card]) > 0.9999).all() and (np.abs(nd[..., 2][on_card]) < 0.8).all()
        assert (u32(pn[..., :3]) != u32(nd[..., :3])).any(-1)[on_blob].mean() > 0.95
        # newer generation = the live records
        newer, _ = kat_at(g, hits, ids, ids >= 0, 0)
        assert np.array_equal(u32(newer)[ids >= 0], u32(nd[..., :3])[ids >= 0])
        # a tile with a pitch and a row offset
        x0, y0, w, h = 7, 5, 41, 30
        pitch, row0 = FW + 3, FH - y0 - h               # (the film row that the buffer's first row holds)
        sentinel = np.full((h, pitch, 4), -7.0, F)
        ptrs = [ctx.alloc(sentinel.nbytes) for _ in range(4)]
        try:
            for p in ptrs:
                ctx.upload(p, sentinel)
            PT.render_features_surface_motion(g, FW, FH, *ptrs, tile=(x0, y0, w, h), accum_pitch=pitch, accum_row0=row0)
            got = [ctx.download(p, sentinel.shape) for p in ptrs]
        finally:
            for p in ptrs:
                ctx.free(p)
        rows = slice(FH - y0 - h, FH - y0)
        outside = np.ones(sentinel.shape[:2], bool)
        outside[:, x0:x0 + w] = False
        for t, full in zip(got, (albedo, nd, pp, pn)):
            assert t[:, x0:x0 + w].tobytes() == full[rows, x0:x0 + w].tobytes()
            assert (t[outside] == -7.0).all()
    finally:
        g.close()
        old.close()


def test_a_moved_sphere_and_a_moved_plane_among_seventy_primitives():
    import test_gpu_analytic_update as au
    desc = au.seventy()
    desc.add_plane((0.0, -2.6, 0.0), (12.0, 12.0), 0)
    g = gpu_scene(desc)
    try:
        g.snapshot_surfaces()
        g.update_sphere(2, (-3.0, 1.0, -2.0), 0.9)
        g.update_plane(70, (0.5, -2.4, 0.25), (11.0, 13.0))
        g.snapshot_surfaces()
        W, H = 61, 47
        a3 = PT.render_features_motion_to_host(g, W, H)
        albedo, nd, pp, pn = PT.render_features_surface_motion_to_host(g, W, H)
        for got, want in zip((albedo, nd, pp), a3):
            assert got.tobytes() == want.tobytes()
        hits, _ = pixel_hits(g, desc.camera, W, H, {})
        for prim in (2, 70):
            on = (hits["hit"] == 1) & (hits["prim"] == prim)
            assert on.sum() >= 20 and (pp[..., 3][on] == 1).all()
        moved = pp[..., 3] == 1
        assert np.array_equal(moved, (hits["hit"] == 1) & np.isin(hits["prim"], (2, 70)))
        hit = pp[..., 3] != 0
        assert np.array_equal(u32(pn[..., :3])[hit], u32(nd[..., :3])[hit]) and (u32(pn)[~hit] == 0).all()
        assert pn[..., 3].tobytes() == pp[..., 3].tobytes()
    finally:
        g.close()


# ---- 3. textured, sampled and normal-mapped levels --------------------------------------------------------------------------------
GRID_N, GRID_W, GRID_H = 4, 53, 41
TILT = None
LEVELS = ("textured", "sampled", "normal")
NORMAL_SCALE = 0.75
SAMPLER = (ag.FILTER_BILINEAR, ag.WRAP_MIRROR, ag.WRAP_CLAMP)
GRID_CAMERA = ([0.25, 1.5, -3.0], [0.0, 1.0, 0.0], [0, 1, 0], GRID_W / float(GRID_H), 45.0, 0.0)


def grid_mesh():
    """a 4 x 4-quad sheet on the grid of quarters around (0, 1, 0), bulged in z by eighths, with vertex normals and uvs that leave [0, 1]"""
    g = np.arange(GRID_N + 1) * 0.25 - 0.5
    X, Y = np.meshgrid(g, g, indexing="ij")
    Z = 0.125 * ((np.arange(GRID_N + 1)[:, None] + np.arange(GRID_N + 1)[None, :]) % 2)
    verts = np.stack([X, Y + 1.0, Z], -1).reshape(-1, 3).astype(F)
    normals = unit(np.stack([0.3 * X, 0.2 * Y, -np.ones_like(X)], -1).reshape(-1, 3))
    uvs = np.stack([1.6 * (X + 0.5) - 0.2, 1.3 * (Y + 0.5) + 0.1], -1).reshape(-1, 2).astype(F)
    tri = []
    n = GRID_N
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, i * (n + 1) + j + 1, (i + 1) * (n + 1) + j + 1
            tri += [a, b, c, c, b, d]
    idx = np.repeat(np.array(tri, np.int32)[:, None], 3, 1)
    return verts, normals, uvs, idx


@functools.lru_cache(None)
def tilt_image():
    rng = np.random.RandomState(31)
    theta, phi = np.radians(rng.uniform(5, 40, (8, 8))), rng.uniform(0, 2 * np.pi, (8, 8))
    n = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)
    return (0.5 * n + 0.5).astype(F)


def grid_scene(level):
    d = ag.scenes.SceneDesc("grid-" + level)
    m = d.add_material(ag.MAT_DISNEY, (0.5, 0.5, 0.5), 0.6, 0.1)
    d.add_mesh(*grid_mesh(), m, 1)
    colour = d.add_texture(np.random.RandomState(32).uniform(0.1, 0.9, (4, 4, 3)).astype(F))
    d.set_material_texture(m, colour)
    if level != "textured":
        d.set_texture_sampler(colour, *SAMPLER)
    if level == "normal":
        t = d.add_texture(tilt_image())
        d.set_texture_sampler(t, *SAMPLER)
        d.set_material_normal_texture(m, t, NORMAL_SCALE)
    d.add_uniform_infinite_light([.5, .5, .5])
    d.set_camera(*GRID_CAMERA)
    return d


@pytest.mark.parametrize("level", LEVELS)
def test_textured_levels_translated_and_turned(level):
    g = gpu_scene(grid_scene(level))
    try:
        g.snapshot_surfaces()
        T = np.eye(4, dtype=F)
        T[0, 3] = 0.25                                               # a power of two on a grid of quarters: every sum is exact
        g.transform_mesh(0, T, "refit")
        g.snapshot_surfaces()
        albedo, nd, pp, pn = PT.render_features_surface_motion_to_host(g, GRID_W, GRID_H)
        a3 = PT.render_features_motion_to_host(g, GRID_W, GRID_H)
        assert all(x.tobytes() == y.tobytes() for x, y in zip((albedo, nd, pp), a3))
        hits, ids = pixel_hits(g, GRID_CAMERA, GRID_W, GRID_H, {0: 0})
        on = ids >= 0
        assert on.sum() >= 200 and (pp[..., 3][on] == 1).all() and (pp[..., 3][~on] == 0).all()
        every = np.arange(2 * GRID_N * GRID_N)
        for b in ((0.25, 0.5), (0.0, 0.0), (0.125, 0.0625)):        # the records' bytes did not change: equal at any barycentrics
            k0 = g.kat_surface(every, np.full(every.shape, b[0], F), np.full(every.shape, b[1], F), 0)
            k1 = g.kat_surface(every, np.full(every.shape, b[0], F), np.full(every.shape, b[1], F), 1)
            assert k0[0].tobytes() == k1[0].tobytes() and k0[1].tobytes() == k1[1].tobytes()
        assert np.array_equal(u32(pn[..., :3])[on], u32(nd[..., :3])[on]) and pn[..., 3].tobytes() == pp[..., 3].tobytes()
        # turned: the older generation is the translated sheet
        g.transform_mesh(0, sm.turn_y(sm.TURN_DEGREES) @ T, "refit")
        g.snapshot_surfaces()
        albedo, nd, pp, pn = PT.render_features_surface_motion_to_host(g, GRID_W, GRID_H)
        hits, ids = pixel_hits(g, GRID_CAMERA, GRID_W, GRID_H, {0: 0})
        on = ids >= 0
        assert on.sum() >= 150 and (pp[..., 3][on] == 1).all()
        old_ns, old_ss = kat_at(g, hits, ids, on, 1)
        if level != "normal":
            want, check = old_ns, on
        else:
            mesh = grid_mesh()
            u, v = np.zeros(ids.shape, F), np.zeros(ids.shape, F)
            for r, c in zip(*np.nonzero(on)):
                t = 3 * int(ids[r, c])
                uv0, uv1, uv2 = (mesh[2][mesh[3][t + k, 2]] for k in range(3))
                u[r, c], v[r, c] = txm.interpolate_uv(uv0, uv1, uv2, hits["b1"][r, c], hits["b2"][r, c])
            texel = fm.value(tilt_image(), u, v, *SAMPLER)
            want = np.zeros_like(old_ns)
            want[on] = gpu_context().kat_normal_map(old_ns[on], old_ss[on], texel[on], NORMAL_SCALE)
            check = on & ~(fm.floor_flip_distance(tilt_image(), u, v) < 1e-5)
            assert check.sum() >= 0.99 * on.sum()
            assert (u32(want) != u32(old_ns)).any(-1)[check].mean() > 0.95          # the map moves the old normal too
        same = (u32(pn[..., :3]) == u32(want)).all(-1)
        print("%s level, turned: %d sheet pixels, %d checked, %d differ" % (level, on.sum(), check.sum(), (check & ~same).sum()))
        assert same[check].all()
        assert (u32(pn[..., :3]) != u32(nd[..., :3])).any(-1)[on].mean() > 0.95
    finally:
        g.close()


# ---- 4. the point of it ---------------------------------------------------------------------------------------------------------
def card_frame(g, k, surfaces):
    acc, m2, _, _ = PT.render_adaptive_to_host(g, CW, CH, 4, 4, 4, 0.0, seed_base=k + 1)
    assert (acc[..., 3] == 4).all()
    return (acc, m2) + (PT.render_features_surface_motion_to_host(g, CW, CH) if surfaces else PT.render_features_to_host(g, CW, CH))


def turned_card_shares(ctx, g):
    """frame 0 at rest, frame 1 with the card turned by sm.TURN_DEGREES: (the shares of card pixels with history from the old and the
    new call, the model's, card pixels)"""
    g.snapshot_surfaces()
    f0 = card_frame(g, 0, False)
    g.transform_mesh(mm.CARD_PRIM, sm.turn_y(sm.TURN_DEGREES), "refit")
    g.snapshot_surfaces()
    acc, m2, albedo, nd, pp, pn = card_frame(g, 1, True)
    hits, ids = pixel_hits(g, mm.CARD_CAMERA, CW, CH, {0: 0, mm.CARD_PRIM: mm.CARD_BASE})
    on_card = ids >= mm.CARD_BASE
    assert on_card.sum() >= 100 and np.array_equal(pp[..., 3] == 1, on_card)
    cur = (acc, m2, albedo, nd)
    old = ctx.temporal_to_host(mm.CARD_CAMERA, mm.CARD_CAMERA, *cur, prev=f0, prev_point=pp)
    new = ctx.temporal_to_host(mm.CARD_CAMERA, mm.CARD_CAMERA, *cur, prev=f0, prev_point=pp, prev_normal=pn)
    va = ag.camera_vectors(mm.CARD_CAMERA)
    m_old, m_new, model = sm.card_shares(va, cur, f0, pp, pn, on_card)
    assert np.array_equal(u32(new[0]), u32(model))
    return (old[0][..., 3] > 4)[on_card].mean(), (new[0][..., 3] > 4)[on_card].mean(), m_old, m_new, int(on_card.sum())


def test_a_turned_card_keeps_its_history_only_with_the_new_call():
    """cos 40 = 0.766 < 0.9 and the floor's taps are perpendicular: the merged call finds history for no card pixel"""
    g = gpu_scene(mm.card_scene())
    try:
        old, new, m_old, m_new, n = turned_card_shares(gpu_context(), g)
    finally:
        g.close()
    print("card turned %g degrees: %d card pixels, history for %.3f of them with agpt_temporal_accumulate_surface_motion (model %.3f), "
          "for %.3f with agpt_temporal_accumulate_motion (model %.3f)" % (sm.TURN_DEGREES, n, new, m_new, old, m_old))
    assert old == 0.0 and m_old == 0.0
    assert new == m_new
    assert new >= 0.9


# ---- 5. the snapshot rules and the argument checks ------------------------------------------------------------------------------
def last_error():
    return ag.lib().agpt_last_error()


def test_snapshot_rules():
    g = ag.Scene(gpu_context())
    try:
        with pytest.raises(ag.AgptError):
            g.snapshot_surfaces()                                       # not committed
        assert b"agpt_scene_snapshot_surfaces" in last_error()
        mm.card_scene().instantiate(g)
        with pytest.raises(ag.AgptError):
            PT.render_features_surface_motion_to_host(g, CW, CH)       # no snapshot at all
        assert b"agpt_render_features_surface_motion" in last_error() and b"agpt_scene_snapshot_positions" in last_error()
        g.snapshot_positions()
        with pytest.raises(ag.AgptError):
            PT.render_features_surface_motion_to_host(g, CW, CH)       # positions only
        assert b"agpt_scene_snapshot_surfaces comes first" in last_error()
        with pytest.raises(ag.AgptError):
            g.kat_surface([0], [0.25], [0.25], 1)
        g.kat_surface([0], [0.25], [0.25], -1)
        with pytest.raises(ag.AgptError):
            g.kat_surface([2 + 72], [0.25], [0.25], -1)                 # one past the last triangle
        g.snapshot_surfaces()
        g.transform_mesh(mm.CARD_PRIM, sm.turn_y(sm.TURN_DEGREES), "refit")
        g.snapshot_surfaces()
        _, nd, pp, pn = PT.render_features_surface_motion_to_host(g, CW, CH)
        moved = pp[..., 3] == 1
        assert moved.sum() >= 100 and (u32(pn[..., :3]) != u32(nd[..., :3])).any(-1)[moved].all()
        # snapshot_positions in between: absent again, and the next snapshot_surfaces is a first one for the records
        g.transform_mesh(mm.CARD_PRIM, sm.turn_y(10.0), "refit")
        g.snapshot_positions()
        with pytest.raises(ag.AgptError):
            PT.render_features_surface_motion_to_host(g, CW, CH)
        assert b"agpt_scene_snapshot_surfaces comes first" in last_error()
        assert (PT.render_features_motion_to_host(g, CW, CH)[2][..., 3] == 1).sum() >= 100
        g.transform_mesh(mm.CARD_PRIM, sm.turn_y(-25.0), "refit")
        g.snapshot_surfaces()
        _, nd, pp, pn = PT.render_features_surface_motion_to_host(g, CW, CH)
        moved = pp[..., 3] == 1
        assert moved.sum() >= 100 and np.array_equal(u32(pn[..., :3])[moved], u32(nd[..., :3])[moved])
        # a REBUILD keeps the generations, a commit drops them
        g.transform_mesh(mm.CARD_PRIM, sm.turn_y(sm.TURN_DEGREES), "rebuild")
        g.snapshot_surfaces()
        _, nd, pp, pn = PT.render_features_surface_motion_to_host(g, CW, CH)
        moved = pp[..., 3] == 1
        assert moved.sum() >= 100 and (u32(pn[..., :3]) != u32(nd[..., :3])).any(-1)[moved].all()
        g.commit()
        with pytest.raises(ag.AgptError):
            PT.render_features_surface_motion_to_host(g, CW, CH)
        with pytest.raises(ag.AgptError):
            g.kat_surface([0], [0.25], [0.25], 0)
        g.snapshot_surfaces()
        _, nd, pp, pn = PT.render_features_surface_motion_to_host(g, CW, CH)
        assert set(np.unique(pp[..., 3])) == {0.0, 2.0} and pn[..., 3].tobytes() == pp[..., 3].tobytes()
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
        g.snapshot_surfaces()
        g.update_sphere(0, (0.1, 1.0, 0.0), 0.6)
        g.snapshot_surfaces()
        _, nd, pp, pn = PT.render_features_surface_motion_to_host(g, 5, 3)
        assert (pp[..., 3] == 1).any() and (pp[..., 3] == 0).any()
        assert np.array_equal(u32(pn[..., :3]), u32(nd[..., :3])) and pn[..., 3].tobytes() == pp[..., 3].tobytes()
        with pytest.raises(ag.AgptError):
            g.kat_surface([0], [0.25], [0.25], 0)
    finally:
        g.close()


def test_arguments_that_need_a_context():
    import test_gpu_motion as gm
    ctx = gpu_context()
    W, H = 5, 3
    cur, prev, pp, pn = synthetic_with_normals(W, H, gm.CAM_PREV)
    host = list(cur) + list(prev)
    ptrs = [ctx.alloc(a.nbytes) for a in host] + [ctx.alloc(W * H * 16), ctx.alloc(W * H * 4), ctx.alloc(pp.nbytes), ctx.alloc(pn.nbytes)]
    try:
        for p, a in zip(ptrs, host):
            ctx.upload(p, a)
        ctx.upload(ptrs[10], pp)
        ctx.upload(ptrs[11], pn)
        params = ag.TemporalParams(W, H, ag.camera_desc(*gm.CAM_CUR), ag.camera_desc(*gm.CAM_PREV), KW["max_history"], KW["depth_tol"], KW["normal_cos"])
        for clamp in (None, ag.TemporalClampParams(2, 0, 1.0, 8.0)):
            ctx.temporal_accumulate_surface_motion(params, clamp, *ptrs)
            good = ctx.download(ptrs[8], (H, W, 4))
            for p, a in zip(ptrs[:8] + ptrs[10:], host + [pp, pn]):
                assert ctx.download(p, a.shape).tobytes() == a.tobytes()        # the inputs are left alone

            def refused(args, word, clamp=clamp):
                with pytest.raises(ag.AgptError):
                    ctx.temporal_accumulate_surface_motion(params, clamp, *args)
                msg = last_error()
                assert b"agpt_temporal_accumulate_surface_motion" in msg and word in msg, msg
            for k in (0, 1, 2, 3, 8, 9):                       # the existing checks, in their order
                refused(ptrs[:k] + [0] + ptrs[k + 1:], b"NULL")
            for k in (4, 5, 6, 7):
                refused(ptrs[:k] + [0] + ptrs[k + 1:], b"prev")
            for k in range(8):
                refused(ptrs[:8] + [ptrs[k], ptrs[9], ptrs[10], ptrs[11]], b"alias")
            refused(ptrs[:8] + [ptrs[8], ptrs[8], ptrs[10], ptrs[11]], b"outputs")
            refused(ptrs[:10] + [0, ptrs[11]], b"prev_point")
            refused(ptrs[:8] + [ptrs[10], ptrs[9], ptrs[10], ptrs[11]], b"prev_point")
            refused(ptrs[:10] + [ptrs[10], 0], b"NULL prev_normal")             # then a NULL prev_normal_cur
            refused(ptrs[:8] + [ptrs[11], ptrs[9], ptrs[10], ptrs[11]], b"aliases prev_normal")   # then an output aliasing it
            refused(ptrs[:8] + [ptrs[8], ptrs[11], ptrs[10], ptrs[11]], b"aliases prev_normal")
            refused(ptrs[:10] + [0, 0], b"prev_point")                          # the earlier check comes first
            if clamp is not None:
                refused(ptrs[:10] + [0, 0], b"radius", ag.TemporalClampParams(4, 0, 1.0, 8.0))
                refused(ptrs, b"gamma", ag.TemporalClampParams(2, 0, -1.0, 8.0))
            assert ctx.download(ptrs[8], (H, W, 4)).tobytes() == good.tobytes()
    finally:
        for p in ptrs:
            ctx.free(p)
    g = gpu_scene(mm.card_scene())
    out = [ctx.alloc(CW * CH * 16) for _ in range(4)]
    try:
        g.snapshot_surfaces()
        for args, word in (((out[0], out[1], 0, out[3]), b"prev_point"), ((out[0], out[1], out[0], out[3]), b"prev_point"),
                           ((out[0], out[0], out[2], out[3]), b"outputs"), ((0, out[1], out[2], out[3]), b"NULL"),
                           ((out[0], out[1], out[2], 0), b"NULL prev_normal"), ((out[0], out[1], out[2], out[0]), b"prev_normal_dev aliases"),
                           ((out[0], out[1], out[2], out[1]), b"prev_normal_dev aliases"), ((out[0], out[1], out[2], out[2]), b"prev_normal_dev aliases"),
                           ((out[0], out[1], 0, 0), b"prev_point")):
            with pytest.raises(ag.AgptError):
                PT.render_features_surface_motion(g, CW, CH, *args)
            assert b"agpt_render_features_surface_motion" in last_error() and word in last_error(), (word, last_error())
        with pytest.raises(ag.AgptError):
            PT.render_features_surface_motion(g, CW, CH, *out, tile=(0, 0, CW + 1, CH))
        PT.render_features_surface_motion(g, CW, CH, *out)
    finally:
        for p in out:
            ctx.free(p)
        g.close()


# ---- 6. other routes --------------------------------------------------------------------------------------------------------------
def test_the_three_calls_on_a_non_blocking_stream():
    import test_gpu_motion as gm
    from test_gpu_streams import Stage
    W, H = 37, 19
    cur, prev, pp_syn, pn_syn = synthetic_with_normals(W, H, gm.CAM_PREV)
    wrong_cur, wrong_prev, wrong_pp, _ = gm.synthetic(W, H, gm.CAM_PREV, seed=77)
    wrong_pn = np.ones_like(pn_syn)
    with Stage() as st:
        g = st.scene(mm.card_scene())
        st.open()
        st.call("snapshot_surfaces (first)", g.snapshot_surfaces)
        g.transform_mesh(mm.CARD_PRIM, sm.turn_y(sm.TURN_DEGREES), "refit")
        st.open()
        st.call("snapshot_surfaces", g.snapshot_surfaces)
        outs = [st.output((CH, CW, 4), -7.0) for _ in range(4)]
        st.open(outs)
        st.call("render_features_surface_motion", PT.render_features_surface_motion, g, CW, CH, *[b.dst for b in outs])
        albedo, nd, pp, pn = (st.read(b) for b in outs)
        ref = PT.render_features_surface_motion_to_host(g, CW, CH)
        assert all(x.tobytes() == y.tobytes() for x, y in zip((albedo, nd, pp, pn), ref))
        moved = pp[..., 3] == 1
        assert moved.sum() >= 100 and (np.abs(pn[..., 2][moved]) > 0.9999).all() and (np.abs(nd[..., 2][moved]) < 0.8).all()
        ins = [st.buffer(real, wrong) for real, wrong in zip(list(cur) + list(prev) + [pp_syn, pn_syn],
                                                             list(wrong_cur) + list(wrong_prev) + [wrong_pp, wrong_pn])]
        params = ag.TemporalParams(W, H, ag.camera_desc(*gm.CAM_CUR), ag.camera_desc(*gm.CAM_PREV), KW["max_history"], KW["depth_tol"], KW["normal_cos"])
        got = {}
        for radius in (None, 2):
            hacc, hm2 = st.output((H, W, 4), -7.0), st.output((H, W), -7.0)
            st.open(ins + [hacc, hm2])
            st.call("temporal_accumulate_surface_motion", st.ctx.temporal_accumulate_surface_motion, params, clamp_of(radius),
                    *([b.dst for b in ins[:8]] + [hacc.dst, hm2.dst, ins[8].dst, ins[9].dst]))
            got[radius] = st.read(hacc), st.read(hm2)
    va, vb = ag.camera_vectors(gm.CAM_CUR), ag.camera_vectors(gm.CAM_PREV)
    for radius in (None, 2):
        model = sm.accumulate_surface_motion(va, vb, *cur, prev, pp_syn, pn_syn, clamp=clamp_model_of(radius), **KW)
        assert np.array_equal(u32(got[radius][0]), u32(model[0])) and np.array_equal(u32(got[radius][1]), u32(model[1]))


TORCH_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch                      # before the library touches the GPU (INTEGRATION.md section 3)
torch.zeros(1, device="cuda")
import numpy as np
import ag_pathtracer_amd as ag
import motion_model as mm
import test_gpu_surface_motion as t
ctx = ag.Context(0)
for mode in ("refit", "rebuild"):
    g = t.card_and_blob().instantiate(ag.Scene(ctx))
    g.snapshot_surfaces()
    v, n = t.bent_blob()
    g.update_mesh(t.BLOB_PRIM, torch.from_numpy(v).cuda(), torch.from_numpy(n).cuda(), mode)
    g.snapshot_surfaces()
    bases = {0: 0, mm.CARD_PRIM: mm.CARD_BASE, t.BLOB_PRIM: mm.CARD_BASE + 72}
    old = t.card_and_blob().instantiate(ag.Scene(ctx))
    pp = t.check_surface_features(g, mm.CARD_CAMERA, t.FW, t.FH, bases, old)[2]
    print("torch %%s: %%d moved pixels" %% (mode, int((pp[..., 3] == 1).sum())))
    assert (pp[..., 3] == 1).sum() >= 100
    g.close()
    old.close()
torch.cuda.synchronize()
ctx.close()
print("torch-ok")
"""


def test_the_torch_device_tensor_route():
    """Scene.update_mesh with torch tensors on the GPU between the two snapshots, in a child process: torch must initialise the GPU
    before the library does"""
    code = TORCH_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "torch-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_the_cpp_example_agrees_with_python(tmp_path):
    exe = build_cpp_example(tmp_path, "turning_scene")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    fields = dict(kv.split("=") for kv in r.stdout.split() if "=" in kv)
    g = gpu_scene(mm.card_scene())
    try:
        old, new, _, _, n = turned_card_shares(gpu_context(), g)
    finally:
        g.close()
    assert int(fields["card_pixels"]) == n
    assert float(fields["share_motion"]) == pytest.approx(old, abs=5e-7) and float(fields["share_surface_motion"]) == pytest.approx(new, abs=5e-7)
