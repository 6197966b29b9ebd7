"""Whole textured paths on the GPU against the textured CPU oracle, bit for bit: images, roughness / metallic maps, samplers and normal
maps that vary inside triangles, at every path vertex, in all sixteen exact instantiations of the four texturing levels (LDS or global
tables, with or without an environment map), through agpt_render, agpt_li_batch and agpt_render_adaptive; and the fast arithmetic within
the project's tolerance of the same oracle.  The cases are textured_path_cases.py's; test_oracle_textures.py proves on the CPU that
each of them looks up what it claims, deeper than the first hit, and that its images decide the picture."""
import numpy as np
import pytest

import ag_pathtracer_amd as ag
import textured_path_cases as tp
from helpers import bits, close_fraction, gpu_scene, oracle_render, oracle_scene
from oracle import binding as ob

F = np.float32
COUNTS = ("closest_rays", "anyhit_rays", "outliers", "shaded_vertices")


def scene_with_tables(name, tables, monkeypatch):
    """the case on the GPU with its shading tables placed as `tables` says (the knob is read when the scene is committed)"""
    monkeypatch.delenv("AGPT_SHADE_GLOBAL_TABLES", raising=False)
    if tables == "global":
        monkeypatch.setenv("AGPT_SHADE_GLOBAL_TABLES", "1")
    return gpu_scene(tp.desc_of(name))


@pytest.mark.gpu
@pytest.mark.parametrize("tables", tp.TABLES)
@pytest.mark.parametrize("name", [c.name for c in tp.CASES])
def test_textured_render_is_the_oracles(name, tables, monkeypatch):
    case = tp.BY_NAME[name]
    oacc, ost, _ = tp.oracle_reference(name)
    g = scene_with_tables(name, tables, monkeypatch)
    try:
        variant = g.shade_variant()
        acc, st = ag.PathTracer(tp.DEPTH).render_to_host(g, tp.W, tp.H, tp.SPP)
    finally:
        g.close()
    same = (bits(acc[..., :3]) == bits(oacc[..., :3])).all(-1)      # every pixel of the film: none is excluded
    print("%s %s: variant (level, fast, lds, env) = %s, %d of %d pixels bit-identical, counts %s / oracle %s" % (
        name, tables, variant, same.sum(), same.size, [int(getattr(st, k)) for k in COUNTS], [ost[k] for k in COUNTS]))
    assert variant == tp.variant(case, tables)
    assert same.size == tp.W * tp.H and same.all(), np.argwhere(~same)[:8]
    for k in COUNTS:
        assert int(getattr(st, k)) == ost[k], k


@pytest.mark.gpu
def test_li_batch_is_the_oracles():
    """agpt_li_batch on 2000 of the oracle's camera rays through a level-4 scene: radiance and RNG end states"""
    desc = tp.desc_of(tp.LI_CASE)
    o = oracle_scene(desc, tp.DEPTH)
    n = 2000
    rng = np.random.RandomState(11)
    rays, states = np.zeros(n, ag.RAY_DTYPE), np.zeros(n, np.uint32)
    for i in range(n):
        rays[i], states[i] = o.camera_ray(float(rng.uniform()), float(rng.uniform()), rng=int(rng.randint(1, 2 ** 31 - 1)))
    want, after = np.zeros((n, 3), F), np.zeros(n, np.uint32)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        for i in range(n):
            want[i], after[i], _ = o.li(rays[i], int(states[i]))
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    g = gpu_scene(desc)
    try:
        assert g.shade_variant()[0] == 4
        got, got_after, st = ag.PathTracer(tp.DEPTH).Li(g, rays, states)
    finally:
        g.close()
    print("textured Li: %d of %d values bit-identical, %d RNG end states" % ((bits(got) == bits(want)).all(-1).sum(), n, (got_after == after).sum()))
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(got_after, after)
    assert st.samples == n and (want > 0).any(-1).mean() > 0.5


@pytest.mark.gpu
def test_adaptive_render_is_the_oracles():
    """agpt_render_adaptive on a level-4 scene: every pixel holds samples [0, n) of its streams, bit-identical to the textured oracle's
    render at spp = n; with rel_error 0 the film is the uniform render at max_spp"""
    desc = tp.desc_of(tp.ADAPTIVE_CASE)
    W, H, MIN, STEP, MAX = 16, 16, 4, 4, 32
    g = gpu_scene(desc)
    try:
        assert g.shade_variant()[0] == 4
        pt = ag.PathTracer(tp.DEPTH)
        acc, m2, st, ast = pt.render_adaptive_to_host(g, W, H, MIN, MAX, STEP, 0.0, abs_floor=0.01)
        assert (acc[..., 3] == MAX).all()
        assert np.array_equal(bits(acc[..., :3]), bits(oracle_render(desc, W, H, MAX, tp.DEPTH)[0][..., :3]))
        levels = ()
        for rel in (0.1, 0.2, 0.05, 0.3, 0.03):
            acc, m2, st, ast = pt.render_adaptive_to_host(g, W, H, MIN, MAX, STEP, rel, abs_floor=0.01)
            counts = acc[..., 3].astype(np.int64)
            levels = np.unique(counts)
            if len(levels) >= 3:
                break
    finally:
        g.close()
    assert len(levels) >= 3, levels
    assert set(levels.tolist()) <= set(range(MIN, MAX + 1, STEP))
    for c in levels:
        ref = oracle_render(desc, W, H, int(c), tp.DEPTH)[0]
        sel = counts == c
        assert acc[sel][:, :3].tobytes() == ref[sel][:, :3].tobytes(), c
    assert ast.samples == int(counts.sum()) and st.samples == ast.samples


@pytest.mark.gpu
@pytest.mark.parametrize("name", tp.FAST_CASES)
def test_fast_arithmetic_stays_within_tolerance_of_the_textured_oracle(name):
    """AGPT_SHADING_FAST against the textured oracle, the project's L2 rule: at least 99 % of the pixels within
    1e-3 |oracle| + 1e-6 at 1 and 2 spp, the ray totals within 1e-3 of the exact mode's"""
    g = gpu_scene(tp.desc_of(name))
    try:
        for spp in (1, 2):
            oacc, _, _ = tp.oracle_reference(name, spp)
            g.set_shading_arith("exact")
            exact, est = ag.PathTracer(tp.DEPTH).render_to_host(g, tp.W, tp.H, spp)
            g.set_shading_arith("fast")
            assert g.shade_variant()[:2] == (tp.BY_NAME[name].level, 1)
            fast, fst = ag.PathTracer(tp.DEPTH).render_to_host(g, tp.W, tp.H, spp)
            share = close_fraction(fast[..., :3], oacc[..., :3], 1e-3)
            print("fast %s at %d spp: %.5f of the pixels within 1e-3 of the textured oracle, rays %d / exact %d" % (name, spp, share, fst.rays, est.rays))
            assert np.array_equal(bits(exact[..., :3]), bits(oacc[..., :3]))
            assert fast.tobytes() != exact.tobytes()
            assert share >= 0.99
            assert abs(fst.rays - est.rays) <= 1e-3 * est.rays
    finally:
        g.close()
