"""agpt_temporal_accumulate_clamped on the GPU against the numpy model of its contract (tests/temporal_clamp_model.py): synthetic
buffers that hold every case of step 5' (tests/temporal_clamp_cases.py; the census is taken from the model's masks) bit for bit at
every radius, with and without demodulation, with equal and different cameras, with and without prev_point; gamma = +Inf against
the two existing calls on rendered frames; determinism and the first frame; the argument checks that need a context; the call on a
caller's non-blocking stream; and the card scene -- the card moves sideways, its shadow leaves a patch of floor, and on that patch
the clamped history is closer to the new lighting than the unclamped one."""
import numpy as np
import pytest

import ag_pathtracer_amd as ag
import motion_model as mm
import temporal_clamp_cases as cases
import temporal_clamp_model as cm
import temporal_model as tm
from adaptive_model import luminance
from denoise_cases import same_but_for_nan_payloads
from helpers import bits as u32, gpu_context, gpu_scene

pytestmark = pytest.mark.gpu
F = np.float32
PT = ag.PathTracer(5)
KW = dict(max_history=cases.MAX_HISTORY, depth_tol=cases.DEPTH_TOL, normal_cos=cases.NORMAL_COS)


def same(got, want):
    """the same bits, NaN payloads excepted"""
    return all(same_but_for_nan_payloads(np.ascontiguousarray(g, F), np.ascontiguousarray(w, F)) for g, w in zip(got, want))


# ---- 1. synthetic buffers against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("film", cases.FILMS)
@pytest.mark.parametrize("cameras", ["equal", "different"])
@pytest.mark.parametrize("motion", [False, True], ids=["prev_point NULL", "prev_point given"])
def test_synthetic_buffers_match_the_model_bit_for_bit(film, cameras, motion):
    W, H = film
    cur, prev, pp, cam_prev = cases.synthetic(W, H, cameras, motion)
    va, vb = ag.camera_vectors(cases.CAM_CUR), ag.camera_vectors(cam_prev)
    ctx = gpu_context()
    if motion:
        assert (pp[..., 3] == 1).any()
    for radius in (1, 2, 3):
        for demodulate in (0, 1):
            model = cm.accumulate_clamped(va, vb, *cur, prev, prev_point=pp, radius=radius, demodulate=demodulate, gamma=cases.GAMMA,
                                          clamped_max_history=cases.CLAMPED_MAX_HISTORY, return_masks=True, **KW)
            if W * H >= 30:
                count = {k: int(model[2][k].sum()) for k in cases.CENSUS_20 + cases.CENSUS_1}
                print("%dx%d %s cameras, radius %d, demodulate %d: %d pixels with history, %s" % (W, H, cameras, radius, demodulate,
                                                                                                  model[2]["history"].sum(), count))
                for k in cases.CENSUS_20:
                    assert count[k] >= 20, (k, count)
                for k in cases.CENSUS_1:
                    assert count[k] >= 1, (k, count)
            clamp = ag.TemporalClampParams(radius, demodulate, cases.GAMMA, cases.CLAMPED_MAX_HISTORY)
            got = ctx.temporal_to_host(cases.CAM_CUR, cam_prev, *cur, prev=prev, prev_point=pp, clamp=clamp, **KW)
            differ = (u32(got[0]) != u32(model[0])).any(-1) | (u32(got[1]) != u32(model[1]))
            differ &= ~(np.isnan(model[0]).any(-1) | np.isnan(model[1]))
            print("pixels that differ from the model: %d" % differ.sum())
            assert same(got, model[:2]), np.argwhere(differ)[:8]
    # two calls are bit-identical; the first frame returns the current buffers and reads nothing else
    again = ctx.temporal_to_host(cases.CAM_CUR, cam_prev, *cur, prev=prev, prev_point=pp, clamp=clamp, **KW)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    first = ctx.temporal_to_host(cases.CAM_CUR, cam_prev, *cur, prev=None, prev_point=pp, clamp=clamp, **KW)
    assert first[0].tobytes() == cur[0].tobytes() and first[1].tobytes() == cur[1].tobytes()


# ---- 2. gamma = +Inf: the two existing calls ------------------------------------------------------------------------------------------
def test_infinite_gamma_equals_the_existing_calls_on_rendered_frames():
    import test_gpu_temporal as tt
    cur, prev, out = tt.rendered_pair()
    g = tt.c1_scene()
    g.snapshot_positions()
    g.set_camera(*tt.C1_CAM)
    _, _, pp = PT.render_features_motion_to_host(g, tt.RW, tt.RH)
    ctx = gpu_context()
    assert np.isfinite(cur[0]).all() and np.isfinite(prev[0]).all()
    for cams, want in (((tt.C1_CAM, tt.C1_PAN), out), ((tt.C1_CAM, tt.C1_CAM), tt.run_gpu((tt.C1_CAM, tt.C1_CAM), cur, prev))):
        assert (want[0][..., 3] > cur[0][..., 3]).any()
        moving = ctx.temporal_to_host(cams[0], cams[1], *cur, prev=prev, prev_point=pp)
        for radius, demodulate in ((1, 0), (2, 1), (3, 1)):
            clamp = ag.TemporalClampParams(radius, demodulate, float("inf"), 1.0)
            got = ctx.temporal_to_host(cams[0], cams[1], *cur, prev=prev, clamp=clamp)
            assert np.array_equal(u32(got[0]), u32(want[0])) and np.array_equal(u32(got[1]), u32(want[1]))
            got = ctx.temporal_to_host(cams[0], cams[1], *cur, prev=prev, prev_point=pp, clamp=clamp)
            assert np.array_equal(u32(got[0]), u32(moving[0])) and np.array_equal(u32(got[1]), u32(moving[1]))
        # a finite gamma does clamp these frames
        some = ctx.temporal_to_host(cams[0], cams[1], *cur, prev=prev, clamp=ag.TemporalClampParams(2, 1, 0.5, 1.0))
        assert not np.array_equal(u32(some[0]), u32(want[0]))


# ---- 3. the argument checks that need a context, in the header's order -------------------------------------------------------------
def test_arguments_that_need_a_context():
    ctx = gpu_context()
    W, H = 5, 3
    cur, prev, pp, cam_prev = cases.synthetic(W, H, "different", True)
    host = list(cur) + list(prev)
    ptrs = [ctx.alloc(a.nbytes) for a in host] + [ctx.alloc(W * H * 16), ctx.alloc(W * H * 4), ctx.alloc(pp.nbytes)]
    nan, inf = float("nan"), float("inf")
    try:
        for p, a in zip(ptrs, host):
            ctx.upload(p, a)
        ctx.upload(ptrs[10], pp)
        params = ag.TemporalParams(W, H, ag.camera_desc(*cases.CAM_CUR), ag.camera_desc(*cam_prev), cases.MAX_HISTORY, cases.DEPTH_TOL,
                                   cases.NORMAL_COS)
        good_clamp = ag.TemporalClampParams(2, 1, 1.0, 8.0)
        ctx.temporal_accumulate_clamped(params, good_clamp, *ptrs)
        good = ctx.download(ptrs[8], (H, W, 4))
        ctx.temporal_accumulate_clamped(params, good_clamp, *(ptrs[:10] + [0]))        # prev_point may be NULL
        for p, a in zip(ptrs[:8] + ptrs[10:], host + [pp]):
            assert ctx.download(p, a.shape).tobytes() == a.tobytes()                   # the inputs are left alone

        def refused(clamp, args, word):
            with pytest.raises(ag.AgptError):
                ctx.temporal_accumulate_clamped(params, clamp, *args)
            msg = ag.lib().agpt_last_error()
            assert b"agpt_temporal_accumulate_clamped" in msg and word in msg, msg
        bad_clamp = ag.TemporalClampParams(0, 7, -1.0, 0.0)
        for k in (0, 1, 2, 3, 8, 9):                           # agpt_temporal_accumulate's checks first, whatever the clamp struct
            refused(bad_clamp, ptrs[:k] + [0] + ptrs[k + 1:], b"NULL")
        for k in (4, 5, 6, 7):
            refused(None, ptrs[:k] + [0] + ptrs[k + 1:], b"prev")
        for k in range(8):
            refused(bad_clamp, ptrs[:8] + [ptrs[k], ptrs[9], ptrs[10]], b"alias")
        refused(bad_clamp, ptrs[:8] + [ptrs[8], ptrs[8], ptrs[10]], b"outputs")
        aliased = ptrs[:8] + [ptrs[10], ptrs[9], ptrs[10]]
        refused(None, aliased, b"NULL clamp")                  # 1. a NULL clamp struct, before everything below
        for radius in (0, 4, -1):                              # 2.
            refused(ag.TemporalClampParams(radius, 7, -1.0, 0.0), aliased, b"radius")
        for demodulate in (2, -1):                             # 3.
            refused(ag.TemporalClampParams(3, demodulate, -1.0, 0.0), aliased, b"demodulate")
        for gamma in (-1.0, -1e-30, nan):                      # 4.
            refused(ag.TemporalClampParams(1, 0, gamma, 0.0), aliased, b"gamma")
        for cmh in (0.0, -1.0, inf, nan):                      # 5.
            refused(ag.TemporalClampParams(1, 1, 0.0, cmh), aliased, b"clamped_max_history")
        refused(good_clamp, aliased, b"prev_point")            # 6. an output aliasing prev_point_cur
        refused(good_clamp, ptrs[:8] + [ptrs[8], ptrs[10], ptrs[10]], b"prev_point")
        # the limits themselves are accepted
        for clamp in (ag.TemporalClampParams(1, 0, 0.0, 1e-30), ag.TemporalClampParams(3, 1, inf, 1e30)):
            ctx.temporal_accumulate_clamped(params, clamp, *ptrs)
        ctx.temporal_accumulate_clamped(params, good_clamp, *ptrs)
        assert ctx.download(ptrs[8], (H, W, 4)).tobytes() == good.tobytes()
    finally:
        for p in ptrs:
            ctx.free(p)


# ---- 4. a caller's non-blocking stream ---------------------------------------------------------------------------------------------
def test_the_call_on_a_non_blocking_stream():
    """the six-step shape of tests/test_gpu_streams.py: the outputs hold a constant and are cleared behind the delay, the inputs hold
    another frame's values until the caller's copies behind the delay put the real ones there"""
    from test_gpu_streams import Stage
    W, H = 37, 19
    cur, prev, pp, cam_prev = cases.synthetic(W, H, "different", True)
    wrong_cur, wrong_prev, wrong_pp, _ = cases.synthetic(W, H, "different", True, seed=77)
    clamp = ag.TemporalClampParams(3, 1, cases.GAMMA, cases.CLAMPED_MAX_HISTORY)
    with Stage() as st:
        ins = [st.buffer(real, wrong) for real, wrong in zip(list(cur) + list(prev) + [pp], list(wrong_cur) + list(wrong_prev) + [wrong_pp])]
        hacc, hm2 = st.output((H, W, 4), -7.0), st.output((H, W), -7.0)
        params = ag.TemporalParams(W, H, ag.camera_desc(*cases.CAM_CUR), ag.camera_desc(*cam_prev), cases.MAX_HISTORY, cases.DEPTH_TOL,
                                   cases.NORMAL_COS)
        st.open(ins + [hacc, hm2])
        st.call("temporal_accumulate_clamped", st.ctx.temporal_accumulate_clamped, params, clamp,
                *([b.dst for b in ins[:8]] + [hacc.dst, hm2.dst, ins[8].dst]))
        got = st.read(hacc), st.read(hm2)
    model = cm.accumulate_clamped(ag.camera_vectors(cases.CAM_CUR), ag.camera_vectors(cam_prev), *cur, prev, prev_point=pp, radius=3,
                                  demodulate=1, gamma=cases.GAMMA, clamped_max_history=cases.CLAMPED_MAX_HISTORY, **KW)
    assert same(got, model)


# ---- 5. the card scene ------------------------------------------------------------------------------------------------------------
CW, CH = mm.CARD_W, mm.CARD_H


def reference(g):
    acc, _ = PT.render_to_host(g, CW, CH, 256)
    return luminance((acc[..., :3] / F(256)).astype(F))


def test_card_scene_the_shadow_does_not_trail_behind_the_card():
    """frame 0 at 64 spp; the card moved sideways (REFIT) and a snapshot; frame 1 at 4 spp with the motion features.  On the floor
    pixels the shadow left -- their 256-spp reference luminance at least doubled (and rose: black stays black) -- the clamped history
    is closer to frame 1's reference than agpt_temporal_accumulate_motion's on the same buffers."""
    ctx = gpu_context()
    g = gpu_scene(mm.card_scene())
    try:
        g.set_camera(*mm.CARD_CAMERA)
        g.snapshot_positions()
        y0 = reference(g)
        acc0, m20, _, _ = PT.render_adaptive_to_host(g, CW, CH, 64, 64, 64, 0.0, seed_base=1)
        assert (acc0[..., 3] == 64).all()
        albedo0, nd0 = PT.render_features_to_host(g, CW, CH)
        prev = (acc0, m20, albedo0, nd0)                      # the first frame's history is the frame itself
        g.update_mesh(mm.CARD_PRIM, mm.card_mesh(cases.CARD_SLIDE)[0], None, "refit")
        g.snapshot_positions()
        y1 = reference(g)
        acc, m2, _, _ = PT.render_adaptive_to_host(g, CW, CH, 4, 4, 4, 0.0, seed_base=2)
        assert (acc[..., 3] == 4).all()
        albedo, nd, pp = PT.render_features_motion_to_host(g, CW, CH)
        cur = (acc, m2, albedo, nd)
        assert (pp[..., 3] == 1).sum() >= 100
        floor = cases.floor_pixels(albedo0, nd0) & cases.floor_pixels(albedo, nd)
        uncovered = cases.uncovered_pixels(floor, y0, y1)
        assert uncovered.sum() >= 30, uncovered.sum()
        clamp = ag.TemporalClampParams(cases.CARD_CLAMP["radius"], cases.CARD_CLAMP["demodulate"], cases.CARD_CLAMP["gamma"],
                                       cases.CARD_CLAMP["clamped_max_history"])
        plain = ctx.temporal_to_host(mm.CARD_CAMERA, mm.CARD_CAMERA, *cur, prev=prev, prev_point=pp)
        got = ctx.temporal_to_host(mm.CARD_CAMERA, mm.CARD_CAMERA, *cur, prev=prev, prev_point=pp, clamp=clamp)
        va = ag.camera_vectors(mm.CARD_CAMERA)
        model = cm.accumulate_clamped(va, va, *cur, prev, prev_point=pp, identity=True, **cases.CARD_CLAMP)
        assert np.array_equal(u32(got[0]), u32(model[0])) and np.array_equal(u32(got[1]), u32(model[1]))

        def error(hist):
            with np.errstate(all="ignore"):
                y = luminance((hist[..., :3] / hist[..., 3:4]).astype(F))
            return float(np.abs(y.astype(np.float64) - y1)[uncovered].mean())
        e_plain, e_clamped = error(plain[0]), error(got[0])
        print("card scene %dx%d: %d uncovered floor pixels (reference luminance %.4f -> %.4f); mean absolute luminance error there "
              "%.5f unclamped, %.5f clamped" % (CW, CH, uncovered.sum(), y0[uncovered].mean(), y1[uncovered].mean(), e_plain, e_clamped))
        assert e_clamped < e_plain
    finally:
        g.close()
