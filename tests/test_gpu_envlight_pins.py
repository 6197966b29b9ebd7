"""The environment light's device functions against the reference's own InfiniteAreaLight, function by function.

agpt_kat_env_light runs env_Le, env_pdf_li and env_sample_li -- the functions k_shade calls -- one lane per case on the cases of
tests/envlight_cases.py; tests/golden/envlight_cases.npz holds what the reference returned for them (tests/test_envlight_pins.py says
what they reach).  Exact arithmetic: every output bit for bit, NaN matching NaN by class, with the scene tables in LDS and under
AGPT_SHADE_GLOBAL_TABLES (the known-answer kernel reads the map's record from global memory either way; agpt_li_batch does not).  Fast
arithmetic: the directions, the texels and what was sampled at all stay exact (include/agpt.h), the pdfs hold to rel 1e-4 + abs 1e-6,
the tolerance of test_gpu_shading_fast.py.  Only the fixture and the oracle are read here, never the reference.
"""
import os
import sys

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import compare_render_with_oracle, gpu_scene

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import envlight_cases as ec  # noqa: E402
from test_envlight_pins import c_library_note, fixture, weights  # noqa: E402

pytestmark = pytest.mark.gpu
KNOB = "AGPT_SHADE_GLOBAL_TABLES"


@pytest.fixture(params=["lds", "global"])
def tables(request, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    if request.param == "global":
        monkeypatch.setenv(KNOB, "1")
    return request.param


def check_exact(s, light, name):
    g = fixture()
    u, _ = ec.draws(name, weights(name))
    le, pli, wi, pdf, sle, ok = s.env_light(light, ec.directions(name), u)
    what = "%slight %d, map %s: " % (c_library_note(), light, name)
    assert np.array_equal(ok, g[name + "/ok"]), what + "ok"
    ec.assert_same(wi, g[name + "/wi"], what + "Sample_Li wi")
    ec.assert_same(pdf, g[name + "/pdf"], what + "Sample_Li pdf")
    ec.assert_same(sle, g[name + "/sle"], what + "Sample_Li radiance")
    ec.assert_same(le, g[name + "/le"], what + "Le")
    ec.assert_same(pli, g[name + "/pdf_li"], what + "Pdf_Li")


def check_fast(s, light, name):
    g = fixture()
    u, _ = ec.draws(name, weights(name))
    s.set_shading_arith("fast")
    le, pli, wi, pdf, sle, ok = s.env_light(light, ec.directions(name), u)
    what = "%sfast, light %d, map %s: " % (c_library_note(), light, name)
    assert np.array_equal(ok, g[name + "/ok"]), what + "ok"
    ec.assert_same(wi, g[name + "/wi"], what + "Sample_Li wi")
    ec.assert_same(sle, g[name + "/sle"], what + "Sample_Li radiance")
    ec.assert_same(le, g[name + "/le"], what + "Le")
    for got, want, which in ((pdf, g[name + "/pdf"], "Sample_Li pdf"), (pli, g[name + "/pdf_li"], "Pdf_Li")):
        fin = np.isfinite(want)
        excess = np.abs(got[fin] - want[fin]) / (1e-4 * np.abs(want[fin]) + 1e-6)
        print(name, which, "largest |difference| / (1e-4 |reference| + 1e-6): %.4f" % (excess.max() if excess.size else 0))
        ec.assert_same(got[~fin], want[~fin], what + which + " where the reference is not finite")
        assert np.array_equal(got == 0, want == 0), what + which      # the early returns: a pole, a texel of no weight
        assert (excess <= 1).all(), what + which


def test_the_products_table_is_the_one_the_draws_were_built_on():
    """the draws sit on the entries of a cdf built by the oracle's Distribution1D (the generator has no device): the product's host
    constructor, through agpt_kat_distribution1d, builds the same one from the same weights"""
    from helpers import gpu_context
    for name in ec.MAPS:
        func, cdf, fi = ec.map_table(name, weights(name))
        got_cdf, got_fi, _, _ = gpu_context().distribution1d(func, np.zeros(0, np.float32))
        assert got_cdf.tobytes() == cdf.tobytes() and np.float32(got_fi).tobytes() == np.float32(fi).tobytes(), name


@pytest.mark.parametrize("name", ec.MAPS)
def test_exact_light(tables, name):
    s = gpu_scene(ec.map_scene(name))
    try:
        check_exact(s, 0, name)
    finally:
        s.close()


@pytest.mark.parametrize("name", ec.MAPS)
def test_fast_light(name):
    s = gpu_scene(ec.map_scene(name))
    try:
        check_fast(s, 0, name)
    finally:
        s.close()


def test_second_map_of_a_scene(tables):
    """light 2 is the scene's second map: it must not be read through the first one's record; light 1 is no map at all"""
    s = gpu_scene(ec.li_scene("two_maps"))
    try:
        with pytest.raises(ag.AgptError):
            s.env_light(1, np.ones((1, 3), np.float32), None)
        with pytest.raises(ag.AgptError):
            s.env_light(3, np.ones((1, 3), np.float32), None)
        for light, name in enumerate(ec.TWO_MAPS):
            if name is not None:
                check_exact(s, light, name)
        check_fast(s, 2, ec.TWO_MAPS[2])
    finally:
        s.close()


@pytest.mark.parametrize("name", ec.LI_SCENES)
def test_li(tables, name):
    g = fixture()
    s = gpu_scene(ec.li_scene(name))
    try:
        assert s.shade_variant()[2] == (tables == "lds")
        L, after, st = ag.PathTracer(ec.LI_DEPTH).Li(s, g["li_%s/rays" % name], g["li_%s/states" % name])
    finally:
        s.close()
    ec.assert_same(L, g["li_%s/L" % name], c_library_note() + "Li " + name)
    assert np.array_equal(after, g["li_%s/after" % name])
    assert [st.closest_rays, st.anyhit_rays] == list(g["li_%s/calls" % name])


@pytest.mark.parametrize("name", ec.LI_SCENES)
def test_render_equals_the_oracles(name):
    compare_render_with_oracle(ec.li_scene(name), 64, 64, 2)
