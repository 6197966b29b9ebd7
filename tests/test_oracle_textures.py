"""The CPU oracle's image textures, material maps, samplers and normal maps (oracle/agpt_oracle.h), no GPU.  The oracle implements the
contract of include/agpt.h on its own; here it is held to the numpy models of the same contract (tests/texture_model.py,
texture_filter_model.py, normal_map_model.py) lookup by lookup, to the equivalences the GPU tests rest on -- now as properties of the
oracle's per-hit derivation --, and the cases of test_gpu_textured_paths.py are shown to exercise what they claim."""
import itertools

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import normal_map_model as nm
import test_gpu_fuzz as t_fuzz
import test_gpu_material_maps as t_maps
import test_gpu_normal_map as t_normal
import test_gpu_texture_filter as t_filter
import test_gpu_textures as t_textures
import texture_filter_model as fm
import texture_model as tm
import textured_path_cases as tp
from helpers import bits, oracle_render, oracle_scene
from oracle import binding as ob
from texture_cases import FLAT, without_textures

F = np.float32


# ---- 1. value(u, v) against the models ---------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 4), (5, 3), (16, 16)]      # width x height


def lookup_coordinates(n):
    """coordinates for an axis of n texels: inside [0, 1], outside on both sides, positions that are integers exactly (u = (k + .5) / n
    where that product is exact), -0.0, magnitudes whose float-to-int conversion saturates -- +-3e38 is finite but its position is not,
    on an axis of more than one texel: only the rule "fx = 0 where the conversion saturated" keeps inf - inf out of the blend -- and the
    non-finite values"""
    rng = np.random.RandomState(100 + n)
    on_texel = [F(k + .5) / F(n) for k in range(-n - 1, 2 * n + 2)]
    c = np.concatenate([rng.uniform(0, 1, 24), rng.uniform(-3.5, -0.01, 12), rng.uniform(1.01, 4.5, 12), on_texel,
                        [0.0, -0.0, 1.0, 0.5, 3e9, -3e9, 1e30, -1e30, 3e38, -3e38, np.nan, np.inf, -np.inf]]).astype(F)
    return c


@pytest.mark.parametrize("size", SIZES)
def test_texture_value_is_the_models_bit_for_bit(size):
    w, h = size
    tex = np.random.RandomState(7 * w + h).uniform(0.05, 0.95, (h, w, 3)).astype(F)
    cu, cv = lookup_coordinates(w), lookup_coordinates(h)
    u, v = (a.reshape(-1) for a in np.meshgrid(cu, cv, indexing="ij"))
    with np.errstate(invalid="ignore", over="ignore"):
        s, t = tm.texel_position((h, w), u, v)
    integer = np.isfinite(s) & (s == np.floor(s)) & (np.abs(s) < 64)
    assert integer.sum() >= len(cv) * (w + 1), "positions exactly on a texel are among the inputs"
    assert np.signbit(u[u == 0]).any()
    o = ob.OracleScene()
    checked = 0
    for filter, wu, wv in itertools.product((fm.NEAREST, fm.BILINEAR), (fm.REPEAT, fm.CLAMP, fm.MIRROR), (fm.REPEAT, fm.CLAMP, fm.MIRROR)):
        ti = o.add_texture(tex)
        o.set_texture_sampler(ti, filter, wu, wv)
        got = o.texture_value(ti, u, v)
        want = fm.value(tex, u, v, filter, wu, wv)
        same = (bits(got) == bits(want)).all(-1)
        assert same.all(), (size, filter, wu, wv, u[~same][:4], v[~same][:4], got[~same][:4], want[~same][:4])
        checked += same.size
    # the nearest-texel model of the first texture feature: the default sampler.  It follows HDRTexture::value's bare (int) cast, which C
    # leaves undefined outside int's range, so it is asked only where that cast is defined
    ti = o.add_texture(tex)
    with np.errstate(invalid="ignore"):
        defined = ~(np.isfinite(u) & np.isfinite(v)) | ((np.abs(np.floor(s)) < F(2.0 ** 31)) & (np.abs(np.floor(t)) < F(2.0 ** 31)))
    assert defined.sum() > 0.8 * defined.size and (~defined).any()
    with np.errstate(invalid="ignore", over="ignore"):
        want = tm.value(tex, u[defined], v[defined])
    assert np.array_equal(bits(o.texture_value(ti, u[defined], v[defined])), bits(want))
    print("%dx%d: %d lookups equal texture_filter_model, %d equal texture_model" % (w, h, checked, defined.sum()))


def test_texture_calls_refuse_what_the_product_refuses():
    o = ob.OracleScene()
    disney, mirror = o.add_material(ob.MAT_DISNEY, [.5, .5, .5], .5, .5), o.add_material(ob.MAT_MIRROR, [.5, .5, .5])
    t = o.add_texture(np.zeros((2, 3, 3), F))
    assert t == 0 and o.add_texture(np.zeros((1, 1, 3), F)) == 1
    for bad in (lambda: o.set_material_texture(2, t), lambda: o.set_material_texture(disney, 2), lambda: o.set_texture_sampler(t, 2, 0, 0),
                lambda: o.set_texture_sampler(t, 0, 3, 0), lambda: o.set_texture_sampler(5, 0, 0, 0),
                lambda: o.set_material_param_texture(mirror, ob.PARAM_ROUGHNESS, t, 0), lambda: o.set_material_param_texture(disney, 2, t, 0),
                lambda: o.set_material_param_texture(disney, ob.PARAM_METALLIC, t, 3),
                lambda: o.set_material_normal_texture(disney, t, float("nan")), lambda: o.set_material_normal_texture(disney, 7, 1.0)):
        with pytest.raises(ValueError):
            bad()
    o.set_material_normal_texture(disney, -1, float("nan"))        # (texture = -1: the scale is ignored)
    # a material with a slot on a sphere or a plane: refused at commit, as agpt_scene_commit refuses it; restored to the constant it passes
    for add in (lambda s, m: s.add_sphere([0, 0, 0], 1.0, m), lambda s, m: s.add_plane([0, 0, 0], [1, 1], m)):
        for slot in (lambda s, m, t: s.set_material_texture(m, t), lambda s, m, t: s.set_material_param_texture(m, ob.PARAM_METALLIC, t, 2),
                     lambda s, m, t: s.set_material_normal_texture(m, t, 1.0)):
            d = ag.SceneDesc("refused")
            m = d.add_material(ag.MAT_DISNEY, [.5, .5, .5], .5, .5)
            add(d, m)
            tex = d.add_texture(np.full((2, 2, 3), .5, F))
            slot(d, m, tex)
            with pytest.raises(ValueError):
                d.instantiate(ob.OracleScene())
            slot(d, m, -1)
            d.instantiate(ob.OracleScene())


# ---- 2. the perturbation against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.25, 3.0])
def test_normal_map_is_the_model_bit_for_bit(scale):
    ns, ss, rgb = t_normal.kat_items()
    want = nm.perturb(ns, ss, rgb, scale)
    got = ob.normal_map(ns, ss, rgb, scale)
    same = (bits(got) == bits(want)).all(-1)
    untouched = (bits(want) == bits(ns)).all(-1)
    print("oracle normal map scale %g: %d of %d items bit-identical; %d of them untouched" % (scale, same.sum(), same.size, untouched.sum()))
    assert same.all(), np.nonzero(~same)[0][:8]
    assert untouched[4096:].sum() >= 8 and not untouched[4096:].all() and not untouched[:4096].any()
    # scale 0 with a texel above the surface: tx = ty = 0 and tz > 0, the no-op rule, whatever the texel's r and g
    up = rgb[:4096, 2] > .5
    assert np.array_equal(bits(ob.normal_map(ns[:4096][up], ss[:4096][up], rgb[:4096][up], 0.0)), bits(ns[:4096][up]))
    assert np.array_equal(bits(ob.normal_map(ns, ss, rgb, 0.0)), bits(nm.perturb(ns, ss, rgb, 0.0)))


# ---- 3. the oracle alone, whole renders: the equivalences the GPU tests assert ------------------------------------------------------
def assert_same_render(a, b, W=64, H=64, spp=3, depth=5, expect_lookups=True, **kw):
    """the oracle renders descriptions a (decorated) and b (plain) to the same bits and the same counts; a's lookups are counted"""
    xa, sa = oracle_render(a, W, H, spp, depth, **kw)
    census = ob.census()
    xb, sb = oracle_render(b, W, H, spp, depth, **kw)
    assert np.array_equal(bits(xa), bits(xb)), a.name
    assert sa.as_dict() == sb.as_dict()
    assert sum(ob.census().values()) == 0          # the plain scene looks nothing up
    if expect_lookups:
        assert sum(census[k] for k in ob.CENSUS_NAMES[:4]) > 0, a.name
    return census


@pytest.mark.parametrize("which", ["c1", "textured"])
def test_constant_images_equal_the_plain_scene(which):
    base = ag.scenes.scene_c1() if which == "c1" else ag.scenes.scene_textured()
    plain = without_textures(base)
    for tw, th in ((1, 1), (7, 5)):
        assert_same_render(t_textures.with_constant_textures(base, tw, th), plain)
        assert_same_render(t_maps.with_constant_maps(plain, tw, th, constant_colour_too=True), plain)
    for slot in ("colour", "maps"):
        for wrap in t_filter.WRAPS.values():
            for tw, th in ((1, 4), (5, 3)):
                census = assert_same_render(t_filter.with_constant_images(plain, slot, tw, th, wrap), plain)
                assert tw * th == 1 or census["bilinear_fractional"] > 0       # (fractional weights between equal taps: the tap exactly)


@pytest.mark.parametrize("kind", list(t_normal.KINDS))
def test_flat_normal_maps_equal_the_plain_scene(kind):
    plain = t_normal.varying_scene(kind)
    for filter in (ag.FILTER_NEAREST, ag.FILTER_BILINEAR):
        for scale in (1.0, 3.0):
            census = assert_same_render(t_normal.varying_scene(kind, (FLAT, filter, ag.WRAP_REPEAT, ag.WRAP_MIRROR, scale)), plain, spp=2)
            assert census["normal_noop"] == census["lookup_normal"] > 0 and census["normal_applied"] == 0


@pytest.mark.parametrize("seed", t_fuzz.TEXTURED_SEEDS)
def test_noop_decorations_of_the_fuzz_scenes_equal_the_plain_scene(seed):
    d, plain, W, H, spp, depth, _, _ = t_fuzz.textured_case(seed)
    assert_same_render(d, plain, W, H, spp, depth, expect_lookups=False, seed_base=seed)


@pytest.mark.parametrize("degenerate_uv", [False, True])
def test_one_texel_per_mesh_equals_one_material_per_mesh(degenerate_uv):
    assert_same_render(t_textures.palette_scene(degenerate_uv, True), t_textures.palette_scene(degenerate_uv, False))
    census = assert_same_render(t_maps.palette_scene(degenerate_uv, "all", True), t_maps.palette_scene(degenerate_uv, "all", False))
    assert census["rebuild_fewer_lobes"] > 0 and census["lookup_deep"] > 0


@pytest.mark.parametrize("slot", ["colour", "params"])
@pytest.mark.parametrize("wrap", list(t_filter.WRAPS))
def test_plateau_per_mesh_equals_material_per_mesh(slot, wrap):
    w = t_filter.WRAPS[wrap]
    census = assert_same_render(t_filter.plateau_scene(slot, w, True), t_filter.plateau_scene(slot, w, False))
    assert census["bilinear_fractional"] > 0 and census["lookup_deep"] > 0


def test_li_counts_like_render():
    """oracle_li on a textured scene: the census of one path, read after the call"""
    o = oracle_scene(tp.desc_of("varying-normal-shared"), 5)
    ray, state = o.camera_ray(0.5, 0.5)
    o.li(ray, state)
    census = ob.census()
    assert census["lookup_colour"] == census["lookup_normal"] >= 1


# ---- 4. the inputs of test_gpu_textured_paths.py see the feature ----------------------------------------------------------------
def test_case_list_reaches_all_sixteen_exact_instantiations():
    reached = {}
    for c in tp.CASES:
        assert tp.variant(c, "lds")[3] == int(any(op[0] == "env_light" for op in tp.desc_of(c.name).ops))
        assert t_fuzz.texturing_level(tp.desc_of(c.name)) == c.level, c.name
        d = tp.desc_of(c.name)
        assert d.n_prims <= 256 and d.n_materials <= 128 and d.n_lights <= 64      # (below the limits: the knob alone decides the placement)
        for tables in tp.TABLES:
            reached.setdefault(tp.variant(c, tables), c.name)
    for v in sorted(reached):
        print("instantiation (level, fast, lds, env) = %s: %s" % (v, reached[v]))
    assert set(reached) == set(itertools.product((1, 2, 3, 4), (0,), (0, 1), (0, 1)))
    for name in tp.FAST_CASES + [tp.LI_CASE, tp.ADAPTIVE_CASE]:
        assert name in tp.BY_NAME
    assert sorted(tp.BY_NAME[n].level for n in tp.FAST_CASES) == [1, 2, 3, 4]
    assert tp.BY_NAME[tp.LI_CASE].level == 4 and tp.BY_NAME[tp.ADAPTIVE_CASE].level == 4


def test_parameter_edge_image_holds_the_edges():
    img = tp.param_edge_image()
    assert {0.0, 1.0} <= set(img[..., 2].reshape(-1).tolist())
    assert {F(0.0), F(.02), F(1.0)} <= set(img[..., 1].reshape(-1)) and img[..., 1].max() > 1
    assert (tp.flat_patches_image().reshape(-1, 3) == FLAT[0, 0]).all(-1).sum() >= 20


TOTALS = {}


@pytest.mark.parametrize("name", [c.name for c in tp.CASES])
def test_case_census_and_sensitivity(name):
    """the census counters the case promises are non-zero, and each change that applies to it -- every image rolled by one texel,
    BILINEAR turned to NEAREST, the normal scale negated -- changes more than 5 % of the pixels, oracle against oracle"""
    case, d = tp.BY_NAME[name], tp.desc_of(name)
    acc, st, census = tp.oracle_reference(name)
    print("census %s: %s" % (name, " ".join("%s=%d" % kv for kv in census.items())))
    for counter in case.promises:
        assert census[counter] > 0, (name, counter)
    assert st["outliers"] == 0 and acc[..., :3].mean() > 0.01
    TOTALS[name] = census
    changes = [("rolled", tp.rolled, True), ("nearest", tp.nearest, tp.has_bilinear(d)), ("negated", tp.negated, tp.has_normal_map(d))]
    assert case.level < 3 or name.startswith("varying-normal") or changes[1][2]
    assert (case.level == 4) == changes[2][2]
    for what, change, applies in changes:
        if not applies:
            continue
        other, _ = oracle_render(change(d), tp.W, tp.H, tp.SPP, tp.DEPTH)
        share = float((bits(other[..., :3]) != bits(acc[..., :3])).any(-1).mean())
        print("sensitivity %s %s: %.1f %% of the pixels change" % (name, what, 100 * share))
        assert share > 0.05, (name, what, share)


def test_every_counter_is_reached_across_the_case_list():
    total = {k: 0 for k in ob.CENSUS_NAMES}
    for c in tp.CASES:
        census = TOTALS.get(c.name) or tp.oracle_reference(c.name)[2]
        for k, v in census.items():
            total[k] += v
    print("census over the case list:", total)
    assert all(v > 0 for v in total.values()), total
