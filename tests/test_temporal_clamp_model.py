"""CPU checks of the neighbourhood clamp of temporal history (agpt_temporal_accumulate_clamped): the symbol and its struct, the
argument checks that need no context (the kernels' cross-compiled resources: test_temporal_api.py), and the numpy model (tests/temporal_clamp_model.py)
-- equal to tests/temporal_model.py and tests/motion_model.py bit for bit where nothing can be clamped (gamma = +Inf), and on the
stale-shadow frame (tests/temporal_clamp_cases.py) the property the feature exists for: the shadow that the history still holds is
pulled to what the frame says now, and the pixels around it keep their bits."""
import ctypes as C
import importlib.util
import os

import numpy as np

import ag_pathtracer_amd as ag
import motion_model as mm
import temporal_clamp_cases as cases
import temporal_clamp_model as cm
import temporal_model as tm
from helpers import assert_exported, bits as u32, struct_layout
from test_motion_model import CAM_A, CAM_B, H, W, frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agpt_build", os.path.join(ROOT, "ag-pathtracer_amd", "build.py"))
b = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(b)
F = np.float32
INVALID = -1


def test_symbol_declared_and_exported():
    assert_exported(("agpt_temporal_accumulate_clamped",))
    assert "agpt_temporal.hip" in b.SOURCES and "agpt_temporal.h" in b.HEADERS
    assert not b.SOURCE_FLAGS.get("agpt_temporal.hip")


def test_struct_layout_matches_ctypes(tmp_path):
    struct_layout(tmp_path, {"agpt_temporal_clamp_params": ag.TemporalClampParams})


def test_argument_failures_without_a_context_name_the_function_and_the_field():
    L = ag.lib()
    nothing = [None] * 11
    clamp = ag.TemporalClampParams(2, 0, 1.0, 8.0)
    assert L.agpt_temporal_accumulate_clamped(None, None, C.byref(clamp), *nothing) == INVALID
    assert b"agpt_temporal_accumulate_clamped: NULL" in L.agpt_last_error()
    desc_a, desc_b = ag.camera_desc(*CAM_A), ag.camera_desc(*CAM_B)
    nan, inf = float("nan"), float("inf")
    for change, word in ((dict(width=0), b"film"), (dict(height=-3), b"film"), (dict(max_history=0.0), b"max_history"),
                         (dict(max_history=inf), b"max_history"), (dict(depth_tol=-1.0), b"depth_tol"), (dict(depth_tol=nan), b"depth_tol"),
                         (dict(normal_cos=2.0), b"normal_cos"), (dict(normal_cos=nan), b"normal_cos"),
                         (dict(width=0, max_history=0.0), b"film"), (dict(max_history=0.0, depth_tol=-1.0), b"max_history"),
                         (dict(), b"NULL")):
        q = ag.TemporalParams(W, H, desc_a, desc_b, 32.0, ag.TEMPORAL_DEPTH_TOL, ag.TEMPORAL_NORMAL_COS)
        for k, v in change.items():
            setattr(q, k, v)
        # the clamp struct is looked at behind agpt_temporal_accumulate's checks: a NULL or a bad one changes nothing here
        for cl in (C.byref(clamp), None, C.byref(ag.TemporalClampParams(0, 7, -1.0, 0.0))):
            assert L.agpt_temporal_accumulate_clamped(None, C.byref(q), cl, *nothing) == INVALID, change
            msg = L.agpt_last_error()
            assert b"agpt_temporal_accumulate_clamped" in msg and word in msg, (change, msg)


def moved_points(seed=3):
    rng = np.random.RandomState(seed)
    pp = rng.normal(size=(H, W, 4)).astype(F) * 2
    pp[..., 2] += 1
    pp[..., 3] = rng.choice([0.0, 1.0, 2.0], size=(H, W))
    return pp


def test_infinite_gamma_is_the_unclamped_call_bit_for_bit():
    cur, h = frame(1, 4), frame(2, 8)
    prev = (h[0], h[1], cur[2], h[3])
    pp = moved_points()
    for cams in ((CAM_A, CAM_A), (CAM_A, CAM_B)):
        va, vb = ag.camera_vectors(cams[0]), ag.camera_vectors(cams[1])
        for radius in (1, 3):
            for demodulate in (0, 1):
                kw = dict(radius=radius, demodulate=demodulate, gamma=np.inf, clamped_max_history=2.0, max_history=6.0)
                want = tm.accumulate(va, vb, *cur, prev, max_history=6.0)
                got = cm.accumulate_clamped(va, vb, *cur, prev, **kw)
                assert (want[0][..., 3] > cur[0][..., 3]).any()
                assert np.array_equal(u32(got[0]), u32(want[0])) and np.array_equal(u32(got[1]), u32(want[1]))
                want = mm.accumulate_motion(va, vb, *cur, prev, pp, max_history=6.0)
                got = cm.accumulate_clamped(va, vb, *cur, prev, prev_point=pp, **kw)
                assert np.array_equal(u32(got[0]), u32(want[0])) and np.array_equal(u32(got[1]), u32(want[1]))
        # a finite gamma on the same buffers does clamp: the comparison above is not vacuous
        some = cm.accumulate_clamped(va, vb, *cur, prev, gamma=1.0, max_history=6.0, return_masks=True)[2]
        assert some["clamped"].any() and some["unclamped"].any()
        first = cm.accumulate_clamped(va, vb, *cur, None)
        assert first[0].tobytes() == cur[0].tobytes() and first[1].tobytes() == cur[1].tobytes()


def test_stale_shadow_is_pulled_to_the_current_frame():
    """The expected values: a clamped disc pixel keeps min(32, 8) = 8 history samples at lo = mu - sd ~ 1 - 0.3 / sqrt(4) = 0.85
    beside its own 4 at 1.0, (4 + 8 * 0.85) / 12 = 0.9; unclamped it keeps 32 at 0.1, (4 + 32 * 0.1) / 36 = 0.2."""
    cur, prev, disc = cases.stale_shadow()
    assert disc.sum() == 113
    va = ag.camera_vectors(cases.SHADOW_CAM)
    plain = tm.accumulate(va, va, *cur, prev)
    out, m2, masks = cm.accumulate_clamped(va, va, *cur, prev, radius=2, demodulate=0, gamma=1.0, clamped_max_history=8.0, return_masks=True)
    y_clamped, y_plain = cases.mean_luminance(out, disc), cases.mean_luminance(plain[0], disc)
    outside = masks["unclamped"][~disc].mean()
    print("stale shadow: disc mean luminance %.3f clamped, %.3f unclamped; %.4f of the pixels outside the disc unclamped"
          % (y_clamped, y_plain, outside))
    assert masks["history"].all()
    assert y_clamped >= 0.7
    assert y_plain <= 0.3
    assert outside >= 0.99
    keep = masks["unclamped"]
    assert np.array_equal(u32(out)[keep], u32(plain[0])[keep]) and np.array_equal(u32(m2)[keep], u32(plain[1])[keep])
    assert masks["clamped"][disc].all() and (out[..., 3][disc] == 4 + 8).all() and (out[..., 3][keep] == 4 + 32).all()


def test_one_pixel_film_takes_the_current_mean_exactly():
    """k = 1 and sd = 0: lo = hi = the current mean, so any finite gamma replaces the history mean by it"""
    va = ag.camera_vectors(CAM_A)
    accum = np.array([[[2.0, 4.0, 1.0, 4.0]]], F)
    albedo = np.array([[[0.5, 0.25, 1.0, 1.0]]], F)
    nd = np.array([[[0.0, 1.0, 0.0, 5.0]]], F)
    m2 = np.array([[3.0]], F)
    prev = (np.array([[[80.0, 8.0, 0.8, 16.0]]], F), np.array([[40.0]], F), albedo, nd)
    mean = accum[0, 0, :3] / F(4)
    for gamma in (0.0, 1.0, 1e30):
        for demodulate in (0, 1):
            out, mo, masks = cm.accumulate_clamped(va, va, accum, m2, albedo, nd, prev, radius=1, demodulate=demodulate, gamma=gamma,
                                                   clamped_max_history=8.0, return_masks=True)
            assert masks["k"][0, 0] == 1 and masks["sd0"][0, 0] and masks["clamped"][0, 0]
            c_new = (mean / albedo[0, 0, :3]) * albedo[0, 0, :3] if demodulate else mean
            assert out[0, 0, 3] == 12
            assert out[0, 0, :3].tobytes() == (accum[0, 0, :3] + c_new * F(8)).astype(F).tobytes()
    # +Inf: Inf * 0 is a NaN bound, which clamps nothing
    out, mo = cm.accumulate_clamped(va, va, accum, m2, albedo, nd, prev, radius=1, gamma=np.inf)
    want = tm.accumulate(va, va, accum, m2, albedo, nd, prev)
    assert out.tobytes() == want[0].tobytes() and mo.tobytes() == want[1].tobytes()


def test_card_slide_uncovers_enough_floor_for_the_gpu_test():
    """the offset of the GPU test's card scene, checked with the CPU oracle: 256-spp references of the two poses, floor pixels whose
    luminance at least doubled"""
    from adaptive_model import luminance
    from denoise_features import host_features
    from helpers import oracle_render
    cw, ch = mm.CARD_W, mm.CARD_H
    y, floor = [], []
    for offset in ((0.0, 0.0, 0.0), cases.CARD_SLIDE):
        desc = mm.card_scene(offset)
        acc, _ = oracle_render(desc, cw, ch, 256)
        y.append(luminance((acc[..., :3] / F(256)).astype(F)))
        albedo, nd, _, _ = host_features(desc, cw, ch)
        floor.append(cases.floor_pixels(albedo, nd))
    uncovered = cases.uncovered_pixels(floor[0] & floor[1], y[0], y[1])
    print("card slide %s: %d floor pixels, %d uncovered, reference luminance there %.4f -> %.4f"
          % (cases.CARD_SLIDE, (floor[0] & floor[1]).sum(), uncovered.sum(), y[0][uncovered].mean(), y[1][uncovered].mean()))
    assert (floor[0] & floor[1]).sum() >= 1000
    assert uncovered.sum() >= 30
