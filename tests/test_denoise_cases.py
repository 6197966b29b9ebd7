"""The synthetic denoiser inputs (tests/denoise_cases.py) on the CPU: every class of their census is populated on the main film, the
vectorised model (tests/denoise_model.py) equals an independent scalar reference written here from the contract's text
(include/agpt.h, "agpt_denoise"), np.fmax changes nothing on finite inputs, and NaN operands of the contract's three max() give
what the contract states.

The scalar reference is a Python loop over pixels and taps on np.float32 scalars; the taps outside the film are found by index.
Measured: all 12 shapes of the GPU test with 1, 5 and 8 passes and both demodulate values take 3.5 s together on one CPU core (at most
0.7 s a case; the reference alone on the main film with 8 passes: 0.16 s), the whole file 4.5 s.
"""
import math

import numpy as np
import pytest

import denoise_cases as dc
import denoise_model as dm
from adaptive_model import luminance

F = np.float32
MAIN_SEED = dc.shape_seed(*dc.MAIN)


# ---- coverage -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [False, True])
def test_every_census_class_occurs_on_the_main_film(demodulate):
    W, H = dc.MAIN
    census = dc.census(dc.synthetic_inputs(W, H, MAIN_SEED), dc.MAIN_ITERATIONS, demodulate)
    out = census.pop("output")
    print("census of the %dx%d film, %d passes, demodulate %d:" % (W, H, dc.MAIN_ITERATIONS, demodulate))
    for name, count in census.items():
        print("    %-50s %d" % (name, count))
    assert {"taps_outside_spacing_%d" % (1 << i) for i in range(dc.MAIN_ITERATIONS)} <= set(census)
    empty = [name for name, count in census.items() if count == 0]
    assert not empty, empty
    assert np.isfinite(out).all() and (out[..., 3] == 1).all()
    assert out.tobytes() == dm.denoise(*dc.synthetic_inputs(W, H, MAIN_SEED), dc.MAIN_ITERATIONS, demodulate).tobytes()


@pytest.mark.parametrize("W,H", [s for s in dc.SHAPES if s[0] * s[1] > 15])
def test_a_flush_of_subnormals_would_show_in_the_output(W, H):
    """the black cells: with an exp whose subnormal results are zero the model's 1-pass output changes on every film that has room
    for them, and the unflushed output there is a non-zero subnormal"""
    inputs = dc.synthetic_inputs(W, H, dc.shape_seed(W, H))
    for demodulate in (False, True):
        assert dc.census(inputs, 1, demodulate)["pixels_decided_by_subnormal_weights_at_spacing_1"] > 0
    rgb = dm.denoise(*inputs, 1, False)[..., :3]
    assert ((rgb > 0) & (rgb < dc.TINY)).any()


def test_the_inputs_are_seeded_and_have_the_stated_form():
    for W, H in dc.SHAPES:
        a = dc.synthetic_inputs(W, H, dc.shape_seed(W, H))
        b = dc.synthetic_inputs(W, H, dc.shape_seed(W, H))
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b]
        accum, moment2, albedo, nd = a
        assert accum.shape == (H, W, 4) and moment2.shape == (H, W) and albedo.shape == (H, W, 4) and nd.shape == (H, W, 4)
        assert all(x.dtype == F and np.isfinite(x).all() for x in a)
        flag = albedo[..., 3]
        assert np.isin(flag, (0, 1, 2)).all() and (albedo[flag != 1][:, :3] == 1).all()
        assert np.isin(accum[..., 3], dc.COUNTS).all()
    accum, moment2, albedo, nd = dc.synthetic_inputs(*dc.MAIN, MAIN_SEED)
    assert all((albedo[..., :3] == v).any() for v in dc.ALBEDO_CASES)
    assert all(((nd[..., 3] == v) & (albedo[..., 3] == 1)).any() for v in dc.DEPTH_CASES)
    mean = luminance(accum[..., :3])[accum[..., 3] > 0] / accum[..., 3][accum[..., 3] > 0]
    assert (mean > 10).any() and (mean < 1).any()


# ---- the scalar reference -------------------------------------------------------------------------------------------------
K = (F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16))


def fmaxf(a, b):
    """C's fmaxf: a NaN operand yields the other one"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def lum(r, g, b):
    return (F(0.212671) * r + F(0.715160) * g) + F(0.072169) * b


def expc(x):
    return F(math.exp(float(x)))


def scalar_denoise(accum, moment2, albedo, normal_depth, iterations, demodulate, sigma_z=dm.SIGMA_Z, sigma_n=dm.SIGMA_N,
                   sigma_l=dm.SIGMA_L):
    """agpt_denoise as include/agpt.h words it, one pixel and one tap at a time -> out[H, W, 4]"""
    H, W = moment2.shape
    sigma_z, sigma_n, sigma_l = F(sigma_z), F(sigma_n), F(sigma_l)
    pix = [(y, x) for y in range(H) for x in range(W)]
    acc = {p: [F(a) for a in accum[p]] for p in pix}
    flag = {p: float(albedo[p][3]) for p in pix}
    ns = {p: [F(a) for a in normal_depth[p][:3]] for p in pix}
    t = {p: F(normal_depth[p][3]) for p in pix}
    state = {}   # p -> (r, g, b, v); no entry: EXCLUDED
    floor = {}
    with np.errstate(all="ignore"):
        for p in pix:
            r, g, b, n = acc[p]
            if not n > 0:
                continue
            c = [r / n, g / n, b / n]
            v = F(0)
            if not n < 2:
                mu = lum(r, g, b) / n
                v = fmaxf(F(0), F(moment2[p]) / n - mu * mu) * n / (n - F(1)) / n
            if demodulate:
                a = [fmaxf(F(ch), F(1e-3)) for ch in albedo[p][:3]]
                floor[p] = a
                c = [c[0] / a[0], c[1] / a[1], c[2] / a[2]]
                v = v / (lum(*a) * lum(*a))
            state[p] = (c[0], c[1], c[2], v)
        for i in range(iterations):
            s = 1 << i
            new = {}
            for p, (rp, gp, bp, vp) in state.items():
                y, x = p
                Yp = lum(rp, gp, bp)
                zden = sigma_z * F(s) * fmaxf(t[p], F(1e-3))
                nden = sigma_n * sigma_n
                lden = sigma_l * np.sqrt(vp) + F(1e-6)
                sw, sc, sv = F(0), [F(0), F(0), F(0)], F(0)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        q = (y + s * dy, x + s * dx)
                        if q[0] < 0 or q[0] >= H or q[1] < 0 or q[1] >= W:
                            continue
                        if flag[q] != flag[p] or q not in state:
                            continue
                        rq, gq, bq, vq = state[q]
                        ez = en = F(0)
                        if flag[p] != 0:
                            ez = abs(t[p] - t[q]) / zden
                            d = [ns[p][0] - ns[q][0], ns[p][1] - ns[q][1], ns[p][2] - ns[q][2]]
                            en = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / nden
                        el = abs(Yp - lum(rq, gq, bq)) / lden
                        w = (K[dx + 2] * K[dy + 2]) * expc(-((ez + en) + el))
                        sw = sw + w
                        sc = [sc[0] + w * rq, sc[1] + w * gq, sc[2] + w * bq]
                        sv = sv + (w * w) * vq
                new[p] = (sc[0] / sw, sc[1] / sw, sc[2] / sw, sv / (sw * sw))
            state = new
        out = np.zeros((H, W, 4), F)
        out[..., 3] = 1
        for p, (r, g, b, _) in state.items():
            if demodulate:
                a = floor[p]
                r, g, b = r * a[0], g * a[1], b * a[2]
            out[p][:3] = (r, g, b)
    return out


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("W,H", dc.SHAPES)
def test_the_model_equals_the_scalar_reference(W, H, demodulate):
    """every shape of the GPU test -- films narrower than the shift of the wider spacings among them --, 1, 5 and 8 passes"""
    inputs = dc.synthetic_inputs(W, H, dc.shape_seed(W, H))
    for iterations in (1, 5, 8):
        model = dm.denoise(*inputs, iterations, demodulate)
        scalar = scalar_denoise(*inputs, iterations, demodulate)
        assert np.isfinite(model).all()
        assert scalar.tobytes() == model.tobytes(), (iterations, np.argwhere((scalar != model).any(-1))[:8])


def test_other_sigmas_on_a_small_film():
    inputs = dc.synthetic_inputs(5, 3, dc.shape_seed(5, 3))
    for sig in ((0.3, 1.0, 1.5), (10.0, 0.05, 40.0)):
        assert scalar_denoise(*inputs, 3, True, *sig).tobytes() == dm.denoise(*inputs, 3, True, *sig).tobytes()


# ---- max() is fmaxf -------------------------------------------------------------------------------------------------------
def test_fmax_changes_nothing_on_finite_inputs():
    accum, moment2, albedo, nd = dc.synthetic_inputs(*dc.MAIN, MAIN_SEED)
    n = accum[..., 3]
    with np.errstate(all="ignore"):
        mu = luminance(accum[..., :3]) / n
        arg = moment2 / n - mu * mu
        keep = n >= 2                                   # (elsewhere v is 0 whatever the clamp gives; n = 0 makes the argument NaN)
        assert np.isfinite(arg[keep]).all()
        assert np.maximum(F(0), arg)[keep].tobytes() == np.fmax(F(0), arg)[keep].tobytes()
    assert np.maximum(albedo[..., :3], dm.ALBEDO_FLOOR).tobytes() == np.fmax(albedo[..., :3], dm.ALBEDO_FLOOR).tobytes()
    assert np.maximum(nd[..., 3], dm.DEPTH_FLOOR).tobytes() == np.fmax(nd[..., 3], dm.DEPTH_FLOOR).tobytes()


@pytest.mark.parametrize("kind", ["albedo", "moment2", "count"])
def test_a_nan_albedo_channel_is_the_floor_and_a_nan_moment2_a_variance_of_zero(kind):
    """(and a NaN count, which is not > 0, excludes its pixel)"""
    poisoned, stated, (y, x) = dc.nan_case(kind)
    c, v = dm.prepare(*poisoned[:3], True)
    cs, vs = dm.prepare(*stated[:3], True)
    assert c.tobytes() == cs.tobytes() and v.tobytes() == vs.tobytes() and np.isfinite(c).all()
    if kind == "moment2":
        assert dm.prepare(*poisoned[:3], False)[1][y, x] == 0
    out = dm.denoise(*poisoned, 3, True)
    assert np.isfinite(out).all() and out.tobytes() == dm.denoise(*stated, 3, True).tobytes()
    small, _, _ = dc.nan_case(kind, 9, 7)
    assert scalar_denoise(*small, 3, True).tobytes() == dm.denoise(*small, 3, True).tobytes()


def test_a_nan_depth_floors_the_denominator_and_poisons_the_numerator():
    """max(t_p, 1e-3) is the floor for a NaN t_p, but ez's numerator |t_p - t_q| is NaN with it: the pixel and every pixel of its
    flag that taps it come out NaN, whatever the denominator.  So no output shows the floor -- the issue's expectation for a NaN t
    cannot be met by an output comparison, on the model or on the device.  What can be pinned is the model's denominator itself
    (run_pass hands it out with return_taps), the set of NaN pixels, and every other pixel's bytes."""
    poisoned, _, (y, x) = dc.nan_case("depth")
    c, v = dm.prepare(*poisoned[:3], True)
    for step in (1, 4):
        zden = dm.run_pass(c, v, *poisoned[2:], step, return_taps=True)[2]["zden"]
        assert zden[y, x] == F(dm.SIGMA_Z) * F(step) * dm.DEPTH_FLOOR and np.isfinite(zden).all()
    assert fmaxf(F(np.nan), dm.DEPTH_FLOOR) == dm.DEPTH_FLOOR          # (the scalar reference's)
    clean = dc.synthetic_inputs(*dc.MAIN, MAIN_SEED)
    out, ref = dm.denoise(*poisoned, 3, True), dm.denoise(*clean, 3, True)
    assert np.isnan(out[y, x, :3]).all() and (out[..., 3] == 1).all()
    yy, xx = np.mgrid[0:dc.MAIN[1], 0:dc.MAIN[0]]
    outside = np.maximum(abs(yy - y), abs(xx - x)) > 2 * ((1 << 3) - 1)
    assert outside.any() and out[outside].tobytes() == ref[outside].tobytes()
    assert not np.isnan(out[poisoned[2][..., 3] != 1]).any()          # other flags never tap it
    small, _, (sy, sx) = dc.nan_case("depth", 9, 7)
    scalar, model = scalar_denoise(*small, 3, True), dm.denoise(*small, 3, True)
    assert np.isnan(model[sy, sx, :3]).all() and dc.same_but_for_nan_payloads(scalar, model)
