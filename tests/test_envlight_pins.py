"""The environment light against the reference's own InfiniteAreaLight, function by function, on the CPU.

tests/golden/envlight_cases.npz holds what the reference's Le, Pdf_Li and Sample_Li returned for the cases of tests/envlight_cases.py
-- ten maps from 1x1 to 500x250, most of them with a texel count that is no power of two and a width unrelated to the height -- and what
PathTracer::Li returned on two scenes lit by such maps (tests/golden/make_envlight_golden.py, from oracle/_ref/libref_hotpath.so).  Here
the oracle is held to it bit for bit, NaN matching NaN by class; tests/test_gpu_envlight_pins.py does the same for the kernels.

The second half asserts, on the fixture alone, that the cases reach what they were built to reach.  One of them reads differently from
what one might expect: a draw of exactly 1.0 lands in the LAST interval of the cdf whatever its weight.  Where that interval has a width
the sample is (n - 1 + 1) / n = 1 and the texel index n -- one row past the map's last; the reference builds a direction beyond the south
pole with a negative pdf from it, and so do its peers.  Where the interval is flat (the last texel is black, or its weight is lost in the
rounding of a long cdf) the texel is n - 1, sampled with the last texel's weight: nothing if that is 0.
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import envlight_cases as ec  # noqa: E402
import make_envlight_golden as mg  # noqa: E402
from test_refpin import xorshift_steps  # noqa: E402

F = np.float32
INV2PI, TWOPI = F(0.15915494309189533576888), F(6.28318530717958647692528)


@functools.lru_cache(maxsize=None)
def fixture():
    g = mg.load()
    return {k: g[k] for k in g.files}


def weights(name):
    return fixture()["weights/%d" % ec.map_size(name)[1]]


@functools.lru_cache(maxsize=None)
def selected(name):
    """(u, of_cdf, ok, texel index) of the map's draws, from the fixture"""
    w, h = ec.map_size(name)
    g = fixture()
    u, of = ec.draws(name, weights(name))
    row, col = ec.texel_of(g[name + "/wi"], w, h)
    return u, of, g[name + "/ok"], row * w + col


def c_library_note():
    """'' if the oracle's table has the fixture's row weights on this machine, else the sentence that says whose fault a mismatch is"""
    for name in ec.MAPS:
        h = ec.map_size(name)[1]
        if ec.oracle_row_weights(h).tobytes() != weights(name).tobytes():
            return ("the C library's sinf on this machine rounds sin(theta) of a %d-row map differently from the one the fixture was "
                    "generated with: the importance tables differ, which is no fault of the oracle or the kernels -- " % h)
    return ""


# ---- the peers against the fixture ----------------------------------------------------------------------------------------------------
def test_the_maps_are_the_ones_the_fixture_was_made_for():
    g = fixture()
    for name in ec.MAPS:
        assert ec.map_sha256(name) == g["sha256/" + name].tobytes().hex(), name


def test_host_row_weights_are_the_fixtures(oracle):
    """sin(theta) per row, as the host constructors round it here (the oracle's table; the product's calls the same sinf)"""
    assert c_library_note() == ""


def test_regenerated_fixture_is_the_committed_bytes():
    from oracle import ref_binding as rb
    if not rb.has_env_light():
        pytest.skip("oracle/_ref/libref_hotpath.so with ref_env_* is built only where the reference is")
    made, g = mg.generate(), fixture()
    assert sorted(made) == sorted(g)
    for key, a in made.items():
        a = np.asarray(a)
        assert g[key].dtype == a.dtype and g[key].shape == a.shape and g[key].tobytes() == a.tobytes(), key


def check_light(call, name, who):
    """call(d, u) -> (Le, Pdf_Li, wi, pdf, sampled Le, ok) against the fixture's rows of map `name`"""
    g = fixture()
    u, _ = ec.draws(name, weights(name))
    le, pli, wi, pdf, sle, ok = call(ec.directions(name), u)
    what = "%s%s, map %s: " % (c_library_note(), who, name)
    assert np.array_equal(ok, g[name + "/ok"]), what + "ok"
    ec.assert_same(wi, g[name + "/wi"], what + "Sample_Li wi")
    ec.assert_same(pdf, g[name + "/pdf"], what + "Sample_Li pdf")
    ec.assert_same(sle, g[name + "/sle"], what + "Sample_Li radiance")
    ec.assert_same(le, g[name + "/le"], what + "Le")
    ec.assert_same(pli, g[name + "/pdf_li"], what + "Pdf_Li")


def oracle_call(o, light):
    def call(d, u):
        wi, pdf, sle, ok = o.env_sample_li(light, u)
        return o.env_le(light, d), o.env_pdf_li(light, d), wi, pdf, sle, ok
    return call


@pytest.fixture
def correctly_rounded(oracle):
    """the trig definition of the calls (the constructors before it run with the C library's)"""
    def on():
        oracle.set_trig_mode(oracle.TRIG_CORRECTLY_ROUNDED)
    yield on
    oracle.set_trig_mode(oracle.TRIG_LIBM)


@pytest.mark.parametrize("name", ec.MAPS)
def test_oracle_light(oracle, correctly_rounded, name):
    o = ec.map_scene(name).instantiate(oracle.OracleScene())
    correctly_rounded()
    check_light(oracle_call(o, 0), name, "oracle")


def test_oracle_second_map_of_a_scene(oracle, correctly_rounded):
    o = ec.li_scene("two_maps").instantiate(oracle.OracleScene())
    with pytest.raises(ValueError):
        o.env_le(1, np.ones((1, 3), F))
    correctly_rounded()
    for light, name in enumerate(ec.TWO_MAPS):
        if name is not None:
            check_light(oracle_call(o, light), name, "oracle, light %d of the two-map scene" % light)


@pytest.mark.parametrize("name", ec.LI_SCENES)
def test_oracle_li(oracle, correctly_rounded, name):
    g = fixture()
    rays, states = g["li_%s/rays" % name], g["li_%s/states" % name]
    o = ec.li_scene(name).instantiate(oracle.OracleScene())
    o.set_max_depth(ec.LI_DEPTH)
    correctly_rounded()
    n = len(rays)
    L, after, calls = np.zeros((n, 3), F), np.zeros(n, np.uint32), [0, 0]
    for i in range(n):
        L[i], after[i], st = o.li(rays[i], int(states[i]))
        calls[0] += st.closest_rays
        calls[1] += st.anyhit_rays
    ec.assert_same(L, g["li_%s/L" % name], c_library_note() + "Li " + name)
    assert np.array_equal(after, g["li_%s/after" % name])
    assert np.array_equal(xorshift_steps(states, g["li_%s/draws" % name]), after)
    assert calls == list(g["li_%s/calls" % name])


# ---- what the cases reach, on the fixture alone ------------------------------------------------------------------------------------------
def test_fixture_is_small_and_whole():
    g = fixture()
    assert os.path.getsize(os.path.join(HERE, "golden", mg.NAME)) < 512 * 1024
    for name in ec.MAPS:
        u, _ = ec.draws(name, weights(name))
        assert len(g[name + "/ok"]) == len(u) and len(g[name + "/le"]) == len(ec.directions(name)) >= ec.N_RANDOM_DIRS + 24
        assert np.isfinite(g[name + "/le"]).all() and np.isfinite(g[name + "/wi"]).all()
    for name in ec.LI_SCENES:
        assert len(g["li_%s/rays" % name]) == ec.N_LI and g["li_%s/L" % name].max() > 0 and g["li_%s/draws" % name].max() >= 10


@pytest.mark.parametrize("name, least", [("33x17", 20), ("33x17_sun", 20), ("500x250", 400)])
def test_cdf_draws_that_round_to_the_texel_before(name, least):
    """a draw equal to cdf[i] has du == 0, and fl(fl(i / n) * n) can fall below i: the reference lights from texel i - 1 then"""
    w, h = ec.map_size(name)
    u, of, ok, idx = selected(name)
    at = (of >= 0) & (ok == 1)
    before = at & (idx == of - 1)
    assert before.sum() >= least
    assert np.isin(of[before], ec.round_trip_misses(w * h)).all()
    assert (at & (idx == of)).sum() >= least      # and the others stay


@pytest.mark.parametrize("name", ec.MAPS)
def test_draw_of_one_lands_in_the_last_interval(name):
    w, h = ec.map_size(name)
    g = fixture()
    u, of, ok, idx = selected(name)
    k = int(np.flatnonzero(u == 1)[0])
    func, cdf, _ = ec.map_table(name, weights(name))
    assert ok[k] == (func[-1] != 0)
    if not ok[k]:
        assert name in ("33x17_black", "8x4_black")
    elif cdf[-2] < 1:      # texel index n: row h, column 0, past the south pole
        want = ec._spherical(np.pi * (h + .5) / h, np.pi / w)
        assert np.abs(g[name + "/wi"][k] - want).max() < 1e-6 and g[name + "/pdf"][k] < 0
    else:
        assert name == "500x250" and idx[k] == w * h - 1 and g[name + "/pdf"][k] > 0


def test_all_black_map():
    """funcInt == 0: nothing is ever sampled; Pdf_Li is 0 / 0 -- a NaN, as the reference returns it -- except where sin(theta) is 0"""
    g = fixture()
    assert not g["8x4_black/ok"].any() and not g["8x4_black/wi"].any() and not g["8x4_black/sle"].any()
    assert not g["8x4_black/le"].any()
    pli = g["8x4_black/pdf_li"]
    assert np.isnan(pli).sum() >= ec.N_RANDOM_DIRS and (np.isnan(pli) | (pli == 0)).all() and (pli == 0).any()


def test_black_rows_and_columns():
    """flat runs of the cdf: no draw samples with a black texel's weight, yet some draws that round to the texel before light from one"""
    g = fixture()
    u, of, ok, idx = selected("33x17_black")
    func = ec.map_table("33x17_black", weights("33x17_black"))[0]
    assert (func == 0).sum() == 2 * 33 + 2 * 17 - 4
    lit = ok == 1
    assert (g["33x17_black/pdf"][lit] != 0).all()
    onto_black = lit & (func[np.minimum(idx, len(func) - 1)] == 0)
    assert onto_black.any() and not g["33x17_black/sle"][onto_black].any()
    assert (g["33x17_black/pdf_li"] == 0).sum() > 100


@pytest.mark.parametrize("name", [m for m in ec.MAPS if ec.map_size(m)[0] > 1])
def test_a_pdf_direction_whose_column_clamps(name):
    """phi * INV2PI * width reaches width for phi at 2 pi: Pdf_Li clamps the column to width - 1 where Le wraps it to 0"""
    w, h = ec.map_size(name)
    d = ec.directions(name).astype(np.float64)
    phi = np.arctan2(d[:, 2], d[:, 0]).astype(F)
    phi = np.where(phi < 0, phi + TWOPI, phi).astype(F)
    x = ((phi * INV2PI).astype(F) * F(w)).astype(F).astype(np.int64)
    assert (x >= w).any()
    if fixture()[name + "/ok"].any():      # the two columns hold different weights on at least one such row
        func = ec.map_table(name, weights(name))[0].reshape(h, w)
        theta = np.arccos(np.clip(d[x >= w, 1] / np.linalg.norm(d[x >= w], axis=1), -1, 1))
        y = np.clip((theta / np.pi * h).astype(np.int64), 0, h - 1)
        assert (func[y, w - 1] != func[y, 0]).any()


@pytest.mark.parametrize("name", [m for m in ec.MAPS if ec.map_size(m)[0] * ec.map_size(m)[1] <= ec.SMALL])
def test_every_texel_is_selected_or_has_no_weight(name):
    u, of, ok, idx = selected(name)
    func = ec.map_table(name, weights(name))[0]
    assert set(np.flatnonzero(func)) <= set(idx[ok == 1])


def test_selected_texels_tell_width_from_height():
    """rows with idx / width != idx % height among the selected texels: exchanging width and height cannot go unseen"""
    for name in ec.MAPS:
        w, h = ec.map_size(name)
        if min(w, h) < 3:
            continue
        u, of, ok, idx = selected(name)
        i = np.unique(idx[(ok == 1) & (idx < w * h)])
        if len(i):
            assert len(np.unique((i // w)[i // w != i % h])) >= (4 if h > 4 else 2), name
