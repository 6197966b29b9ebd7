"""Texture samplers, CPU side: the C entry point and the argument checks that need no context, the scene descriptions, and the
numpy model of the sampled lookup (tests/texture_filter_model.py) against hand-computed cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import texture_filter_model as fm
import texture_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ERR_INVALID = -1   # AGPT_ERR_INVALID (include/agpt.h)
MODES = (fm.REPEAT, fm.CLAMP, fm.MIRROR)


def test_symbol_and_constants_are_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "agpt.h")).read()
    assert re.search(r"int agpt_scene_set_texture_sampler\(agpt_scene\*, int texture, int filter, int wrap_u, int wrap_v\);", h)
    assert re.search(r"enum \{ AGPT_FILTER_NEAREST = 0, AGPT_FILTER_BILINEAR = 1 \};", h)
    assert re.search(r"enum \{ AGPT_WRAP_REPEAT = 0, AGPT_WRAP_CLAMP = 1, AGPT_WRAP_MIRROR = 2 \};", h)
    L = ag.lib()
    assert "agpt_scene_set_texture_sampler" in ag.EXPORTS and hasattr(L, "agpt_scene_set_texture_sampler")
    assert L.agpt_scene_set_texture_sampler.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    assert (ag.FILTER_NEAREST, ag.FILTER_BILINEAR) == (fm.NEAREST, fm.BILINEAR) == (0, 1)
    assert (ag.WRAP_REPEAT, ag.WRAP_CLAMP, ag.WRAP_MIRROR) == MODES == (0, 1, 2)


def test_null_scene_is_invalid_with_a_message():
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    assert L.agpt_scene_set_texture_sampler(None, 0, 0, 0, 0) == ERR_INVALID
    assert b"agpt_scene_set_texture_sampler" in L.agpt_last_error()


@pytest.mark.gpu
def test_documented_errors_on_a_scene():
    from helpers import gpu_context
    L = ag.lib()
    L.agpt_last_error.restype = C.c_char_p
    s = ag.Scene(gpu_context())
    try:
        tex = s.add_texture(np.ones((2, 2, 3), F))
        for t in (-1, 1, 7):
            assert L.agpt_scene_set_texture_sampler(s.h, t, 0, 0, 0) == ERR_INVALID and b"texture id" in L.agpt_last_error()
        for f in (-1, 2):
            assert L.agpt_scene_set_texture_sampler(s.h, tex, f, 0, 0) == ERR_INVALID and b"filter" in L.agpt_last_error()
        for wu, wv in ((-1, 0), (3, 0), (0, -1), (0, 3)):
            assert L.agpt_scene_set_texture_sampler(s.h, tex, 1, wu, wv) == ERR_INVALID and b"wrap" in L.agpt_last_error()
        s.set_texture_sampler(tex)                                                   # the default is accepted ...
        s.set_texture_sampler(tex, ag.FILTER_NEAREST, ag.WRAP_REPEAT, ag.WRAP_REPEAT)
        for f in (ag.FILTER_NEAREST, ag.FILTER_BILINEAR):                            # ... and so is every combination
            for wu in MODES:
                for wv in MODES:
                    s.set_texture_sampler(tex, f, wu, wv)
        mat = s.add_material(ag.MAT_DISNEY, [.5, .5, .5], .5, 0.)
        s.set_material_texture(mat, tex)
        v, n, t, idx = ag.scenes.heightfield(2)
        s.add_mesh(v, n, t, idx, mat, 1)
        s.set_camera([0, 3, 3], [0, 0, 0], [0, 1, 0], 1.0)
        s.commit()
        assert L.agpt_scene_set_texture_sampler(s.h, tex, 0, 0, 0) == ERR_INVALID and b"committed" in L.agpt_last_error()
    finally:
        s.close()


def test_scene_descriptions_carry_samplers():
    d = ag.scenes.scene_textured()
    d.set_texture_sampler(0, ag.FILTER_BILINEAR, ag.WRAP_CLAMP, ag.WRAP_MIRROR)
    d.set_texture_sampler(1)
    assert [op for op in d.ops if op[0] == "texture_sampler"] == [("texture_sampler", 0, 1, 1, 2), ("texture_sampler", 1, 0, 0, 0)]

    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append((name,) + a) or 0

    r = d.instantiate(Recorder())
    assert [c for c in r.calls if c[0] == "set_texture_sampler"] == [("set_texture_sampler", 0, 1, 1, 2), ("set_texture_sampler", 1, 0, 0, 0)]


# ---- the model against hand-computed cases ---------------------------------------------------------------------------
def test_wrap_by_hand():
    x = np.arange(-4, 8)
    assert fm.wrap(x, 3, fm.REPEAT).tolist() == [2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1]
    assert fm.wrap(x, 3, fm.CLAMP).tolist() == [0, 0, 0, 0, 0, 1, 2, 2, 2, 2, 2, 2]
    assert fm.wrap(x, 3, fm.MIRROR).tolist() == [2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]     # ... | 0 1 2 | 2 1 0 | 0 1 ...
    for mode in MODES:
        assert fm.wrap(x, 1, mode).tolist() == [0] * len(x)                              # one texel: always it
    assert fm.wrap(fm.INT_MAX, 3, fm.REPEAT) == 1 and fm.wrap(fm.INT_MAX + 1, 3, fm.REPEAT) == 2     # 2147483647 = 3 * 715827882 + 1
    assert fm.wrap(fm.INT_MIN, 3, fm.CLAMP) == 0 and fm.wrap(fm.INT_MAX + 1, 3, fm.CLAMP) == 2


def image(values):
    """[H, W] -> rgb[H, W, 3] = (a, 2a, -a): three channels that go through the same operations with other numbers"""
    a = np.asarray(values, F)
    return np.stack([a, 2 * a, -a], -1).astype(F)


def rgb(a):
    return [a, 2 * a, -a]


TEX22 = image([[1, 2], [3, 5]])
TEX53 = image([[10 * y + x for x in range(3)] for y in range(5)])     # height 5, width 3


@pytest.mark.parametrize("tex,u,v,want_taps,want", [
    # 2 x 2, centre: s = t = .5 -> taps 0 | 1 on both axes in every mode, weights 1/2: top = 1 + .5 * (2 - 1) = 1.5,
    # bot = 3 + .5 * (5 - 3) = 4, c = 1.5 + .5 * (4 - 1.5) = 2.75
    (TEX22, .5, .5, {m: (0, 1, 0, 1, .5, .5) for m in MODES}, {m: 2.75 for m in MODES}),
    # 2 x 2, u = v = 0: s = t = -.5 -> x0 = -1, weights 1/2.  REPEAT: taps 1 | 0: c00 = 5, c10 = 3, c01 = 2, c11 = 1: top = 5 + .5 * (3 - 5)
    # = 4, bot = 2 + .5 * (1 - 2) = 1.5, c = 4 + .5 * (1.5 - 4) = 2.75.  CLAMP: -1 -> 0.  MIRROR: Mod(-1, 4) = 3 -> 4 - 1 - 3 = 0: texel (0, 0)
    (TEX22, 0., 0., {fm.REPEAT: (1, 0, 1, 0, .5, .5), fm.CLAMP: (0, 0, 0, 0, .5, .5), fm.MIRROR: (0, 0, 0, 0, .5, .5)},
     {fm.REPEAT: 2.75, fm.CLAMP: 1., fm.MIRROR: 1.}),
    # 2 x 2, u = .875, v = .25: s = 1.25 -> x0 = 1, fx = .25, x0 + 1 = 2 -> REPEAT 0, CLAMP 1, MIRROR Mod(2, 4) = 2 -> 1; t = 0 -> y0 = 0,
    # fy = 0.  REPEAT: top = 2 + .25 * (1 - 2) = 1.75; the others: 2
    (TEX22, .875, .25, {fm.REPEAT: (1, 0, 0, 1, .25, 0.), fm.CLAMP: (1, 1, 0, 1, .25, 0.), fm.MIRROR: (1, 1, 0, 1, .25, 0.)},
     {fm.REPEAT: 1.75, fm.CLAMP: 2., fm.MIRROR: 2.}),
    # 3 wide, 5 high, u = 1.125, v = -.25: s = 2.875 -> x0 = 2, fx = .875, x0 + 1 = 3 -> REPEAT 0, CLAMP 2, MIRROR Mod(3, 6) = 3 -> 2;
    # t = -1.75 -> y0 = -2, fy = .25, y0 + 1 = -1 -> REPEAT 3 | 4, CLAMP 0 | 0, MIRROR Mod(-2, 10) = 8 -> 1 | Mod(-1, 10) = 9 -> 0.
    # REPEAT: top = 32 + .875 * (30 - 32) = 30.25, bot = 42 + .875 * (40 - 42) = 40.25, c = 30.25 + .25 * 10 = 32.75
    # CLAMP: texel (2, 0) = 2.  MIRROR: top = 12, bot = 2, c = 12 + .25 * (2 - 12) = 9.5
    (TEX53, 1.125, -.25, {fm.REPEAT: (2, 0, 3, 4, .875, .25), fm.CLAMP: (2, 2, 0, 0, .875, .25), fm.MIRROR: (2, 2, 1, 0, .875, .25)},
     {fm.REPEAT: 32.75, fm.CLAMP: 2., fm.MIRROR: 9.5}),
    # 3 wide, 5 high, u = .5, v = .5: s = 1, t = 2: on the texel centre, both weights 0 -> texel (1, 2) = 21 in every mode
    (TEX53, .5, .5, {m: (1, 2, 2, 3, 0., 0.) for m in MODES}, {m: 21. for m in MODES}),
])
def test_bilinear_by_hand(tex, u, v, want_taps, want):
    for mode in MODES:
        got = fm.taps(tex, F(u), F(v), fm.BILINEAR, mode, mode)
        assert tuple(float(a) for a in got) == tuple(float(a) for a in want_taps[mode]), mode
        c = fm.value(tex, F(u), F(v), fm.BILINEAR, mode, mode)
        assert c.dtype == F and c.tolist() == rgb(want[mode]), mode


def test_the_two_axes_wrap_on_their_own():
    # the 3 x 5 case above with CLAMP along u and REPEAT along v: x 2 | 2, y 3 | 4 -> top = 32, bot = 42, c = 32 + .25 * 10 = 34.5
    assert fm.value(TEX53, F(1.125), F(-.25), fm.BILINEAR, fm.CLAMP, fm.REPEAT).tolist() == rgb(34.5)
    # ... and the other way round: x 2 | 0, y 0 | 0 -> 2 + .875 * (0 - 2) = .25
    assert fm.value(TEX53, F(1.125), F(-.25), fm.BILINEAR, fm.REPEAT, fm.CLAMP).tolist() == rgb(.25)


def test_nearest_by_hand():
    # u = 1.125, v = -.25 on the 3 x 5 image: floor(2.875) = 2, floor(-1.75) = -2 -> REPEAT (2, 3), CLAMP (2, 0), MIRROR (2, 1)
    for mode, texel in ((fm.REPEAT, 32.), (fm.CLAMP, 2.), (fm.MIRROR, 12.)):
        assert fm.value(TEX53, F(1.125), F(-.25), fm.NEAREST, mode, mode).tolist() == rgb(texel)
    # the default sampler is texture_model's lookup
    rng = np.random.RandomState(3)
    u, v = rng.uniform(-3, 4, 500).astype(F), rng.uniform(-3, 4, 500).astype(F)
    assert np.array_equal(fm.value(TEX53, u, v), tm.value(TEX53, u, v))
    assert np.array_equal(fm.value(TEX53, u, v, fm.NEAREST, fm.REPEAT, fm.REPEAT), tm.value(TEX53, u, v))


def test_equal_taps_return_the_tap_bitwise():
    rng = np.random.RandomState(4)
    u, v = rng.uniform(-3, 4, 2000).astype(F), rng.uniform(-3, 4, 2000).astype(F)
    c = np.array([.1, 1 / 3, 1e-8], F)
    for shape in ((1, 1), (4, 1), (3, 5)):
        const = np.broadcast_to(c, shape + (3,))
        for wu in MODES:
            for wv in MODES:
                got = fm.value(const, u, v, fm.BILINEAR, wu, wv)
                assert got.view(np.uint32).tolist() == np.broadcast_to(c, got.shape).copy().view(np.uint32).tolist()
    # a plateau: texels 2k and 2k + 1 equal -> anywhere between their centres the blend is that value
    plateau = np.repeat(rng.uniform(.05, .95, (1, 6, 3)).astype(F), 2, axis=1)      # 1 x 12
    for k in range(6):
        uu = ((2 * k + .5 + rng.uniform(.01, .99, 200)) / 12).astype(F)
        got = fm.value(plateau, uu, rng.uniform(-2, 2, 200).astype(F), fm.BILINEAR, fm.CLAMP, fm.MIRROR)
        assert (got.view(np.uint32) == plateau[0, 2 * k].view(np.uint32)).all()


def test_non_finite_and_saturating_coordinates():
    for u, v in ((float("nan"), .5), (.5, float("inf")), (float("-inf"), float("nan"))):
        for mode in MODES:
            assert fm.taps(TEX53, F(u), F(v), fm.BILINEAR, mode, mode) == (0, 0, 0, 0, 0, 0)
            assert fm.value(TEX53, F(u), F(v), fm.BILINEAR, mode, mode).tolist() == TEX53[0, 0].tolist()
    # finite u whose position is beyond the int range (1e30 * 3) or overflows to infinity (3e38 * 3): the conversion saturates at
    # INT_MAX = 3 * 715827882 + 1 -> REPEAT taps 1 | 2, weight 0; v = .5 -> t = 2, row 2
    for u in (1e30, 3e38):
        x0, x1, y0, y1, fx, fy = fm.taps(TEX53, F(u), F(.5), fm.BILINEAR, fm.REPEAT, fm.REPEAT)
        assert (int(x0), int(x1), int(y0), int(y1), float(fx), float(fy)) == (1, 2, 2, 3, 0., 0.)
        assert fm.value(TEX53, F(u), F(.5), fm.BILINEAR, fm.REPEAT, fm.REPEAT).tolist() == rgb(21.)
        assert fm.value(TEX53, F(-u), F(.5), fm.BILINEAR, fm.CLAMP, fm.CLAMP).tolist() == rgb(20.)
        assert fm.value(TEX53, F(u), F(.5), fm.BILINEAR, fm.CLAMP, fm.CLAMP).tolist() == rgb(22.)
