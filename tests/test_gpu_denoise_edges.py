"""agpt_denoise on the synthetic films of tests/denoise_cases.py against the numpy model of its contract (tests/denoise_model.py): film
shapes from one pixel to one past the 64-pixel tile of k_denoise_pass and films narrower than the tap reach, every iteration count,
the floors of the contract hit exactly, counts that are no positive integers, flags mixed pixel by pixel, tap weights that are fp32
subnormals and black pixels whose output rests on such weights alone -- a device that flushed subnormals anywhere between the fp64
exp and the store would write 0 there, on every film of more than 15 pixels at 1 pass and on the main film at 2 --
(tests/test_denoise_cases.py asserts that the inputs hold every one of these, and checks the model against a scalar reference
written from the contract's text); then the bounds of the out buffer and the reuse of the context's scratch buffer across
film sizes, how far one pixel reaches, and non-finite inputs.

tests/test_gpu_denoise.py admits 4 differing pixels per film for a double-rounding tie between the device's and the host's fp64 exp
(about 2^-28 per call).  These films have a few thousand pixels, the inputs are fixed by their seeds, and the allowance here is zero:
the output equals the model's byte for byte (helpers.denoise_edge prints the count).  No film needed another seed.
"""
import numpy as np
import pytest

import ag_pathtracer_amd as ag
import denoise_cases as dc
import denoise_model as dm
from helpers import denoise_edge, gpu_context

pytestmark = pytest.mark.gpu
F = np.float32
_MODEL = {}


def inputs_of(W, H):
    return dc.synthetic_inputs(W, H, dc.shape_seed(W, H))


def model_of(W, H, iterations, demodulate, sigmas=dc.SIGMAS):
    key = (W, H, iterations, demodulate, sigmas)
    if key not in _MODEL:
        _MODEL[key] = dm.denoise(*inputs_of(W, H), iterations, demodulate, *sigmas)
        _MODEL[key].setflags(write=False)
    return _MODEL[key]


def reach(k):
    """how far (Chebyshev) a pixel's value travels in k passes: two taps of spacing 1, 2, .. 2^(k-1)"""
    return 2 * ((1 << k) - 1)


def chebyshev(W, H, y, x):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.maximum(abs(yy - y), abs(xx - x))


# ---- shapes and iteration counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", dc.SHAPES)
def test_every_shape_and_iteration_count_matches_the_model(W, H):
    ctx = gpu_context()
    inputs = inputs_of(W, H)
    for iterations in (range(1, 9) if (W, H) == dc.MAIN else (1, 5, 8)):
        for demodulate in (False, True):
            out = ctx.denoise_to_host(*inputs, iterations, demodulate)
            assert (out[..., 3] == 1).all()
            denoise_edge(out, model_of(W, H, iterations, demodulate), "%dx%d iterations %d demodulate %d" % (W, H, iterations, demodulate))


@pytest.mark.parametrize("sigmas", [(0.3, 1.0, 1.5), (10.0, 0.05, 40.0)])
def test_other_sigmas_on_the_main_film(sigmas):
    W, H = dc.MAIN
    for demodulate in (False, True):
        out = gpu_context().denoise_to_host(*inputs_of(W, H), dc.MAIN_ITERATIONS, demodulate, *sigmas)
        denoise_edge(out, model_of(W, H, dc.MAIN_ITERATIONS, demodulate, sigmas), "sigmas %r demodulate %d" % (sigmas, demodulate))


# ---- bounds and stale scratch ---------------------------------------------------------------------------------------------
SENTINEL = F(-7.5)
ORDER = ((129, 9), (1, 1), (65, 5), (3, 130), (129, 9))
PASSES = (4, 5)                                   # an even count starts in out, an odd one in the scratch buffer


def denoise_device(ctx, W, H, iterations, demodulate):
    """ctx.denoise on device buffers, out one film longer than W * H -> (out[:W * H] as [H, W, 4], the tail, the four inputs read back)"""
    host = [np.ascontiguousarray(a) for a in inputs_of(W, H)]
    n = W * H
    start = np.full((2 * n, 4), SENTINEL, F)
    start[:n] = np.nan
    ptrs = []
    try:
        for a in host + [start]:
            ptrs.append(ctx.alloc(a.nbytes))
            ctx.upload(ptrs[-1], a)
        ctx.denoise(ag.DenoiseParams(W, H, iterations, int(demodulate), *dc.SIGMAS), *ptrs)
        out = ctx.download(ptrs[4], (2 * n, 4))
        back = [ctx.download(p, a.shape) for p, a in zip(ptrs, host)]
    finally:
        for p in ptrs:
            ctx.free(p)
    return out[:n].reshape(H, W, 4), out[n:], [b.tobytes() == a.tobytes() for a, b in zip(host, back)]


@pytest.mark.parametrize("demodulate", [False, True])
def test_out_bounds_and_scratch_reuse_across_film_sizes(demodulate):
    """one context runs 129x9, 1x1, 65x5, 3x130, 129x9: its scratch buffer is grown by the first call and reused at smaller and
    equal sizes.  Each result equals that of the same call made first in a context of its own, and the model's."""
    first = {}
    for W, H in set(ORDER):
        for iterations in PASSES:
            fresh = ag.Context(0)
            try:
                first[W, H, iterations] = denoise_device(fresh, W, H, iterations, demodulate)[0]
            finally:
                fresh.close()
    ctx = ag.Context(0)
    try:
        for W, H in ORDER:
            for iterations in PASSES:
                out, tail, inputs_kept = denoise_device(ctx, W, H, iterations, demodulate)
                what = "%dx%d iterations %d demodulate %d after other film sizes" % (W, H, iterations, demodulate)
                assert (tail == SENTINEL).all(), what
                assert all(inputs_kept), what
                assert not np.isnan(out).any(), what
                assert out.tobytes() == first[W, H, iterations].tobytes(), what
                denoise_edge(out, model_of(W, H, iterations, demodulate), what)
    finally:
        ctx.close()


# ---- reach ----------------------------------------------------------------------------------------------------------------
def live_pixel_near_the_centre(inputs, W, H):
    """a flag-1 pixel with samples in the two middle columns"""
    accum, _, albedo, _ = inputs
    ok = (albedo[..., 3] == 1) & (accum[..., 3] >= 2)
    ok[:, :W // 2 - 1] = False
    ok[:, W // 2 + 1:] = False
    return tuple(np.argwhere(ok)[len(np.argwhere(ok)) // 2])


@pytest.mark.parametrize("k", [1, 3, 5])
def test_one_pixel_reaches_no_farther_than_the_taps(k):
    W, H = 129, 9
    ctx = gpu_context()
    inputs = inputs_of(W, H)
    y, x = live_pixel_near_the_centre(inputs, W, H)
    changed = [a.copy() for a in inputs]
    changed[0][y, x, :3] = changed[0][y, x, :3] * F(3) + F(1)
    clean = ctx.denoise_to_host(*inputs, k, True)
    out = ctx.denoise_to_host(*changed, k, True)
    denoise_edge(out, dm.denoise(*changed, k, True), "129x9 iterations %d, one pixel changed" % k)
    outside = chebyshev(W, H, y, x) > reach(k)
    differ = (out != clean).any(-1)
    print("iterations %d: %d pixels changed, all within %d of (%d, %d); %d pixels lie outside" % (k, differ.sum(), reach(k), x, y, outside.sum()))
    assert outside.any() and (differ & ~outside).any()
    assert out[outside].tobytes() == clean[outside].tobytes()


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["albedo", "moment2", "count"])
def test_a_nan_operand_of_max_yields_the_other_one(kind):
    """a NaN albedo channel is the floor, a NaN moment2 a variance of 0 (fmaxf), and a NaN count excludes its pixel: finite, and the
    model's bytes"""
    poisoned, stated, _ = dc.nan_case(kind)
    for demodulate in (False, True):
        out = gpu_context().denoise_to_host(*poisoned, 3, demodulate)
        assert np.isfinite(out).all()
        denoise_edge(out, dm.denoise(*poisoned, 3, demodulate), "NaN %s demodulate %d" % (kind, demodulate))
        assert out.tobytes() == dm.denoise(*stated, 3, demodulate).tobytes()


def check_poisoned(out, model, clean, y, x, k, what):
    """the model's set of non-finite pixels (NaN payloads are not compared), its bytes at every other pixel, and beyond the reach of
    k passes the bytes of the run without the poison"""
    W, H = dc.MAIN
    bad, bad_model = ~np.isfinite(out).all(-1), ~np.isfinite(model).all(-1)
    outside = chebyshev(W, H, y, x) > reach(k)
    print("%s: %d pixels non-finite (the model: %d), the farthest %d from (%d, %d) of a reach of %d" %
          (what, bad.sum(), bad_model.sum(), chebyshev(W, H, y, x)[bad].max() if bad.any() else -1, x, y, reach(k)))
    assert bad[y, x] and np.array_equal(bad, bad_model), (what, np.argwhere(bad != bad_model)[:8])
    assert dc.same_but_for_nan_payloads(out, model), what
    assert outside.any() and out[outside].tobytes() == clean[outside].tobytes(), what


def test_a_nan_depth_poisons_its_taps_and_no_more():
    """max(t_p, 1e-3) is the floor for a NaN t_p, but ez's numerator is NaN with it (tests/test_denoise_cases.py): the pixel and
    those of its flag that tap it are NaN, as in the model; every other pixel has the model's bytes"""
    poisoned, _, (y, x) = dc.nan_case("depth")
    ctx = gpu_context()
    clean = ctx.denoise_to_host(*inputs_of(*dc.MAIN), 3, True)
    out = ctx.denoise_to_host(*poisoned, 3, True)
    check_poisoned(out, dm.denoise(*poisoned, 3, True), clean, y, x, 3, "NaN t")


@pytest.mark.parametrize("value", [np.inf, np.nan])
def test_non_finite_radiance_spreads_as_far_as_the_taps_and_stops(value):
    W, H = dc.MAIN
    _, _, (y, x) = dc.nan_case("albedo")               # (the pixel only: a flag-1 pixel with samples)
    ctx = gpu_context()
    inputs = inputs_of(W, H)
    poisoned = [a.copy() for a in inputs]
    poisoned[0][y, x, :3] = value
    for demodulate in (False, True):
        clean = ctx.denoise_to_host(*inputs, 3, demodulate)
        denoise_edge(clean, model_of(W, H, 3, demodulate), "37x29 iterations 3 demodulate %d" % demodulate)
        out = ctx.denoise_to_host(*poisoned, 3, demodulate)
        check_poisoned(out, dm.denoise(*poisoned, 3, demodulate), clean, y, x, 3, "accum.rgb = %r demodulate %d" % (value, demodulate))
