"""agpt_temporal_accumulate on the GPU against the numpy model of its contract (tests/temporal_model.py): bit for bit on synthetic
buffers that hold every case of the contract and on rendered frames, the static-camera chain against one longer render, the cap,
disocclusion, the first frame, determinism, the argument checks that need a context, and the chain into agpt_denoise."""
import numpy as np
import pytest

import ag_pathtracer_amd as ag
import denoise_model as dm
import temporal_model as tm
from helpers import gpu_context, gpu_scene, unit

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 37, 29                      # synthetic film: not a multiple of the 64 x 4 tile, more than one block
CAM_CUR = ([0.3, 1.4, -6.0], [0.0, 0.0, 0.0], [0, 1, 0], W / float(H), 42.0, 0.0)
# the previous camera stood 2.5 further along the view direction, shifted sideways and turned: near points lie behind it, points
# just in front of it project far off its film
CAM_PREV = ([0.58, 0.62, -3.62], [0.5, 0.3, 0.0], [0.05, 1, 0], W / float(H), 42.0, 0.0)
MAX_HISTORY, DEPTH_TOL, NORMAL_COS = 6.0, 0.0625, 0.9


def synthetic_inputs(seed=20240917):
    """(current buffers, previous buffers): seeded random, then made coherent where the current pixels land so that history is
    accepted for most of them, then threshold cases written last into cells of their own."""
    rng = np.random.RandomState(seed)
    va, vb = ag.camera_vectors(CAM_CUR), ag.camera_vectors(CAM_PREV)
    flag = rng.choice([0.0, 1.0, 2.0], size=(H, W), p=[0.2, 0.6, 0.2]).astype(F)
    geometry = flag != 0
    albedo = np.ones((H, W, 4), F)
    albedo[..., :3] = np.where(geometry[..., None], rng.uniform(0.05, 1, (H, W, 3)), 1.0)
    albedo[..., 3] = flag
    nd = np.zeros((H, W, 4), F)
    nd[..., :3] = np.where(geometry[..., None], unit(rng.normal(size=(H, W, 3))), 0)
    nd[..., 3] = np.where(geometry, rng.uniform(1.5, 9.0, (H, W)), 0)
    n_c = np.where(rng.uniform(size=(H, W)) < 0.06, 0.0, 4.0).astype(F)
    accum = np.zeros((H, W, 4), F)
    accum[..., :3] = rng.uniform(0, 2, (H, W, 3)) * n_c[..., None]
    accum[..., 3] = n_c
    m2 = (rng.uniform(0, 6, (H, W)) * n_c).astype(F)

    # the previous frame: random, incoherent
    p_flag = rng.choice([0.0, 1.0, 2.0], size=(H, W)).astype(F)
    p_albedo = np.ones((H, W, 4), F)
    p_albedo[..., 3] = p_flag
    p_nd = np.zeros((H, W, 4), F)
    p_nd[..., :3] = unit(rng.normal(size=(H, W, 3)))
    p_nd[..., 3] = rng.uniform(1.0, 9.0, (H, W))
    n_q = rng.choice([0.0, 1.5, 3.0, 8.0, 12.25, 20.0], size=(H, W), p=[0.1, 0.18, 0.18, 0.18, 0.18, 0.18]).astype(F)
    h_acc = np.zeros((H, W, 4), F)
    h_acc[..., :3] = rng.uniform(0, 2, (H, W, 3)) * n_q[..., None]
    h_acc[..., 3] = n_q
    h_m2 = (rng.uniform(0, 6, (H, W)) * n_q).astype(F)

    # coherent where 70 % of the current pixels land: their flag, a depth within 3 % and a normal within a few degrees
    nd_geom = nd.copy()
    pos = tm.position(va, vb, False, flag, nd[..., 3], W, H)
    rows, cols = np.nonzero(pos["found"] & (rng.uniform(size=(H, W)) < 0.7))
    for r, c in zip(rows, cols):
        for tap in range(4):
            qx, qy = pos["x0"][r, c] + (tap & 1), pos["y0"][r, c] + (tap >> 1)
            if 0 <= qx < W and 0 <= qy < H:
                q = (H - 1 - qy, qx)
                p_albedo[q][3] = flag[r, c]
                p_nd[q][3] = pos["te"][r, c] * F(1 + rng.uniform(-0.03, 0.03))
                p_nd[q][:3] = unit(nd[r, c, :3] + rng.normal(size=3) * 0.08) if geometry[r, c] else 0

    # threshold cases, each in a tap-0 cell of its own, written last: a depth exactly depth_tol * te away, one float beyond it,
    # a normal whose dot is exactly normal_cos, and one just under it
    ok = pos["found"] & geometry & (pos["x0"] >= 0) & (pos["y0"] >= 0) & (pos["fx"] < 0.9) & (pos["fy"] < 0.9) & (n_c > 0)
    taken = set()
    kinds = ("depth_on", "depth_beyond", "normal_on", "normal_under")
    count = dict.fromkeys(kinds, 0)
    for r, c in zip(*np.nonzero(ok)):
        q = (H - 1 - pos["y0"][r, c], pos["x0"][r, c])
        if q in taken or count[kinds[len(taken) % 4]] >= 12:
            continue
        kind = kinds[len(taken) % 4]
        te = pos["te"][r, c]
        zmax = F(DEPTH_TOL) * np.fmax(te, F(1e-3))
        depth, normal = te, nd[r, c, :3].copy()
        if kind.startswith("depth"):
            exact = [d for d in (F(te + zmax), F(te - zmax)) if np.abs(te - d) == zmax]
            if not exact:
                continue
            depth = exact[0] if kind == "depth_on" else np.nextafter(exact[0], F(np.inf) if exact[0] > te else F(-np.inf))
        else:
            nd[r, c, :3] = (1, 0, 0)
            normal = np.array([NORMAL_COS if kind == "normal_on" else np.nextafter(F(NORMAL_COS), F(0)), 0.43, 0], F)
        taken.add(q)
        count[kind] += 1
        p_albedo[q][3] = flag[r, c]
        p_nd[q] = (normal[0], normal[1], normal[2], depth)
        h_acc[q] = (3.0, 2.0, 1.0, 8.0)
    assert min(count.values()) >= 1, count
    assert nd[..., 3].tobytes() == nd_geom[..., 3].tobytes()      # (the positions above still hold: only normals were rewritten)
    return (va, vb), (accum, m2, albedo, nd), (h_acc, h_m2, p_albedo, p_nd)


def run_gpu(cams, cur, prev, **kw):
    return gpu_context().temporal_to_host(cams[0], cams[1], *cur, prev=prev, **kw)


def test_synthetic_buffers_match_the_model_bit_for_bit():
    (va, vb), cur, prev = synthetic_inputs()
    kw = dict(max_history=MAX_HISTORY, depth_tol=DEPTH_TOL, normal_cos=NORMAL_COS)
    model_acc, model_m2, m = tm.accumulate(va, vb, *cur, prev, return_masks=True, **kw)
    flag, n_c = cur[2][..., 3], cur[0][..., 3]
    any_tap = lambda name: np.logical_or.reduce(m[name])
    # every case of the contract occurs in these inputs
    assert m["off_film"].any() and m["behind"].any() and m["found"].any()
    for f in (0, 1, 2):
        assert (any_tap("flag_mismatch") & (flag == f)).any(), f
        assert (m["history"] & (flag == f)).any(), f
    assert any_tap("empty_tap").any()
    assert ((n_c == 0) & m["history"]).any() and ((n_c == 0) & ~m["history"]).any()
    assert m["capped"].any() and m["uncapped"].any()
    assert any_tap("depth_on").any() and any_tap("depth_out").any()
    assert any_tap("normal_on").any() and any_tap("normal_out").any()
    assert (m["found"] & ~m["history"]).any()                                  # landed on the film, every tap rejected
    used = np.stack(m["used"]).sum(0)
    assert (used == 4).any() and ((used > 0) & (used < 4)).any()
    print("synthetic %dx%d: %d pixels with history (%d capped), %d off the film, %d behind, %d found but rejected"
          % (W, H, m["history"].sum(), m["capped"].sum(), m["off_film"].sum(), m["behind"].sum(), (m["found"] & ~m["history"]).sum()))
    acc, m2 = run_gpu((CAM_CUR, CAM_PREV), cur, prev, **kw)
    differ = (acc != model_acc).any(-1) | (m2 != model_m2)
    print("pixels that differ from the model: %d" % differ.sum())
    assert acc.tobytes() == model_acc.tobytes(), np.argwhere(differ)[:8]
    assert m2.tobytes() == model_m2.tobytes(), np.argwhere(differ)[:8]


# ---- rendered frames ------------------------------------------------------------------------------------------------------
RW, RH = 48, 40
C1_CAM = ([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], RW / float(RH), 45.0, 0.0)
C1_PAN = ([-1.16, 1.21, -4.72], [0.05, 0, 0], [0, 1, 0], RW / float(RH), 45.0, 0.0)
_RENDERED = {}


def c1_scene():
    """C1 (scenes.py): the backdrop mesh, the gold sphere, the key light's emitter sphere, a uniform sky"""
    if "scene" not in _RENDERED:
        _RENDERED["scene"] = gpu_scene(ag.scenes.scene_c1())
    return _RENDERED["scene"]


def render_frame(cam, first_sample=0, spp=4, seed_base=0):
    """samples [first_sample, first_sample + spp) of every pixel into fresh buffers -> (accum, moment2, albedo, normal_depth);
    accum.w = spp"""
    g = c1_scene()
    g.set_camera(*cam)
    pt = ag.PathTracer(5)
    start = np.zeros((RH, RW, 4), F)
    start[..., 3] = first_sample          # the count selects the samples; the sums start at zero
    acc, m2, _, _ = pt.render_adaptive_to_host(g, RW, RH, first_sample + spp, first_sample + spp, spp, 0.0, accum=start, seed_base=seed_base)
    assert (acc[..., 3] == first_sample + spp).all()
    acc[..., 3] = spp
    albedo, nd = pt.render_features_to_host(g, RW, RH)
    return acc, m2, albedo, nd


def rendered_pair():
    """two frames of C1 with a small pan between them, the second accumulated onto the first"""
    if "pair" not in _RENDERED:
        prev = render_frame(C1_PAN, seed_base=1)
        cur = render_frame(C1_CAM, seed_base=2)
        hist = run_gpu((C1_PAN, C1_PAN), prev, None)                      # first frame: its history is itself
        assert hist[0].tobytes() == prev[0].tobytes() and hist[1].tobytes() == prev[1].tobytes()
        prev_buffers = (hist[0], hist[1], prev[2], prev[3])
        out = run_gpu((C1_CAM, C1_PAN), cur, prev_buffers)
        _RENDERED["pair"] = (cur, prev_buffers, out)
    return _RENDERED["pair"]


def test_rendered_frames_match_the_model_bit_for_bit():
    cur, prev, (acc, m2) = rendered_pair()
    assert len(np.unique(cur[2][..., 3])) >= 2                            # surfaces and sky in view
    model_acc, model_m2, m = tm.accumulate(ag.camera_vectors(C1_CAM), ag.camera_vectors(C1_PAN), *cur, prev, identity=False,
                                           return_masks=True)
    took = acc[..., 3] > cur[0][..., 3]
    print("C1 %dx%d pan: %d pixels took history, %d did not (%d off the film)" % (RW, RH, took.sum(), (~took).sum(), m["off_film"].sum()))
    assert took.any() and (~took).any()
    assert np.array_equal(took, m["history"])
    assert acc.tobytes() == model_acc.tobytes(), np.argwhere((acc != model_acc).any(-1))[:8]
    assert m2.tobytes() == model_m2.tobytes(), np.argwhere(m2 != model_m2)[:8]


def test_static_camera_chain_equals_one_longer_render():
    """Three 4-spp frames of samples [4k, 4k + 4) chained through the identity rule carry 12 samples: w == 12 exactly, sums within
    rtol 1e-5 of one 12-spp render -- per frame and value one divide, one multiply and one add on non-negative numbers, at most
    3 * 2^-24 relative each, about 5e-7 over three frames."""
    hist = None
    for k in range(3):
        cur = render_frame(C1_CAM, first_sample=4 * k)
        acc, m2 = run_gpu((C1_CAM, C1_CAM), cur, hist, max_history=1e30)
        hist = (acc, m2, cur[2], cur[3])
    g = c1_scene()
    g.set_camera(*C1_CAM)
    ref_acc, ref_m2, _, _ = ag.PathTracer(5).render_adaptive_to_host(g, RW, RH, 12, 12, 4, 0.0)
    assert (acc[..., 3] == 12).all() and (ref_acc[..., 3] == 12).all()
    for got, want, what in ((acc[..., :3], ref_acc[..., :3], "rgb"), (m2, ref_m2, "moment2")):
        with np.errstate(all="ignore"):
            rel = np.where(want != 0, np.abs(got.astype(np.float64) - want) / np.abs(want.astype(np.float64)), 0.0)
        print("static chain %s: max relative difference %.3g" % (what, rel.max()))
        assert (got[want == 0] == 0).all(), what
        assert np.allclose(got, want, rtol=1e-5, atol=0), (what, rel.max())


def flat_frame(seed, n, depth=5.0):
    rng = np.random.RandomState(seed)
    accum = np.zeros((H, W, 4), F)
    accum[..., :3] = rng.uniform(0, 2, (H, W, 3)) * n
    accum[..., 3] = n
    m2 = (rng.uniform(0, 6, (H, W)) * n).astype(F)
    albedo = np.ones((H, W, 4), F)
    nd = np.zeros((H, W, 4), F)
    nd[..., 2] = -1
    nd[..., 3] = depth
    return accum, m2, albedo, nd


def test_cap_and_disocclusion():
    cur = flat_frame(1, 4)
    cur[0][2, 3] = 0          # a pixel without samples of its own
    cur[1][2, 3] = 0
    h = flat_frame(2, 8)
    prev = (h[0], h[1], cur[2], cur[3])
    for cams in ((CAM_CUR, CAM_CUR), (CAM_CUR, CAM_PREV)):
        va, vb = ag.camera_vectors(cams[0]), ag.camera_vectors(cams[1])
        # the cap: a history count of 8 enters as 2
        acc, m2 = run_gpu(cams, cur, prev, max_history=2.0, depth_tol=1e9, normal_cos=-1.0)
        model = tm.accumulate(va, vb, *cur, prev, max_history=2.0, depth_tol=1e9, normal_cos=-1.0)
        assert acc.tobytes() == model[0].tobytes() and m2.tobytes() == model[1].tobytes()
        took = acc[..., 3] > cur[0][..., 3]
        assert took.any() and (acc[took][:, 3] == cur[0][took][:, 3] + 2).all()
        if cams[0] is cams[1]:
            assert took.all() and acc[2, 3, 3] == 2
        # disocclusion: depth_tol = 0 and every previous depth offset -> nothing is accepted
        far = prev[3].copy()
        far[..., 3] += 0.25
        acc, m2 = run_gpu(cams, cur, (prev[0], prev[1], prev[2], far), depth_tol=0.0)
        assert acc.tobytes() == cur[0].tobytes() and m2.tobytes() == cur[1].tobytes()


def test_first_frame_and_determinism():
    (va, vb), cur, prev = synthetic_inputs()
    acc, m2 = run_gpu((CAM_CUR, CAM_PREV), cur, None)
    assert acc.tobytes() == cur[0].tobytes() and m2.tobytes() == cur[1].tobytes()
    a = run_gpu((CAM_CUR, CAM_PREV), cur, prev, max_history=MAX_HISTORY)
    b = run_gpu((CAM_CUR, CAM_PREV), cur, prev, max_history=MAX_HISTORY)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert not np.array_equal(a[0], cur[0])


def test_arguments_that_need_a_context():
    """checks 6-8 of the header's list, and that the inputs are left alone"""
    ctx = gpu_context()
    (va, vb), cur, prev = synthetic_inputs()
    host = list(cur) + list(prev)
    ptrs = [ctx.alloc(a.nbytes) for a in host] + [ctx.alloc(W * H * 16), ctx.alloc(W * H * 4)]
    try:
        for p, a in zip(ptrs, host):
            ctx.upload(p, a)
        params = ag.TemporalParams(W, H, ag.camera_desc(*CAM_CUR), ag.camera_desc(*CAM_PREV), MAX_HISTORY, DEPTH_TOL, NORMAL_COS)
        ctx.temporal_accumulate(params, *ptrs)
        good = ctx.download(ptrs[8], (H, W, 4))
        for p, a in zip(ptrs, host):
            assert ctx.download(p, a.shape).tobytes() == a.tobytes()

        def refused(args, word):
            with pytest.raises(ag.AgptError):
                ctx.temporal_accumulate(params, *args)
            msg = ag.lib().agpt_last_error()
            assert b"agpt_temporal_accumulate" in msg and word in msg, msg
        for k in (0, 1, 2, 3, 8, 9):                       # 6: a NULL current or output pointer
            refused(ptrs[:k] + [0] + ptrs[k + 1:], b"NULL")
        for k in (4, 5, 6, 7):                             # 7: prev pointers partly NULL
            refused(ptrs[:k] + [0] + ptrs[k + 1:], b"prev")
            refused(ptrs[:4] + [ptrs[j] if j == k else 0 for j in (4, 5, 6, 7)] + ptrs[8:], b"prev")
        for k in range(8):                                 # 8: an output aliases an input, or the other output
            refused(ptrs[:8] + [ptrs[k], ptrs[9]], b"alias")
            refused(ptrs[:8] + [ptrs[8], ptrs[k]], b"alias")
        refused(ptrs[:8] + [ptrs[8], ptrs[8]], b"outputs")
        refused(ptrs[:6] + [0, 0] + [ptrs[0], ptrs[9]], b"prev")          # 7 before 8
        bad = ag.TemporalParams(W, H, ag.camera_desc(*CAM_CUR), ag.camera_desc(*CAM_PREV), 0.0, DEPTH_TOL, NORMAL_COS)
        with pytest.raises(ag.AgptError):
            ctx.temporal_accumulate(bad, *ptrs)
        assert ctx.download(ptrs[8], (H, W, 4)).tobytes() == good.tobytes()
    finally:
        for p in ptrs:
            ctx.free(p)


def test_history_passes_through_the_denoiser_unchanged():
    """agpt_denoise on the accumulated history equals the denoiser's own model on it, bit for bit -- on the rendered pair's outputs,
    and on the same pair capped at 2.5 samples of history, whose counts (6.5) are not integers"""
    cur, prev, (acc, m2) = rendered_pair()
    ctx = gpu_context()
    capped = run_gpu((C1_CAM, C1_PAN), cur, prev, max_history=2.5)
    assert (capped[0][..., 3] == 6.5).any()
    for what, (a, m) in (("history", (acc, m2)), ("history capped at 2.5", capped)):
        out = ctx.denoise_to_host(a, m, cur[2], cur[3])
        model = dm.denoise(a, m, cur[2], cur[3])
        differ = (out != model).any(-1)
        print("denoised %s: %d of %d pixels differ from the model" % (what, differ.sum(), differ.size))
        assert out.tobytes() == model.tobytes(), (what, np.argwhere(differ)[:8])
    # and it resolves as it is
    p = ctx.alloc(acc.nbytes)
    try:
        ctx.upload(p, acc)
        assert ctx.resolve_counts(p, RW * RH).shape == (RW * RH,)
    finally:
        ctx.free(p)
