"""The fast shading arithmetic (agpt_scene_set_shading_arith(AGPT_SHADING_FAST), include/agpt.h) against the exact CPU oracle,
at the tolerance the port is judged at:
    L1  BSDF known answers (tests/golden/bsdf_kat.npz): f and pdf within rel 1e-4 (+abs 1e-6), sampled wi within abs 1e-5, the
        same specular flag and the same zero / non-zero pdf, on >= 99.9 % of the entries; nothing non-finite the fixture has finite;
    L2  1 and 2 spp with the same seeds: >= 99 % of pixels with every channel within 1e-3 |oracle| + 1e-6;
    L3  16 spp: per-channel image means within rel 1e-3 (same seeds), and RMSE(fast, seed B vs oracle, seed A) <= 1.2 x the
        oracle's own seed-to-seed RMSE.
Plus what the fast mode keeps exactly: determinism (repeats, sample-batch splits, rank shares) and ray totals, and the switch's
hygiene.  Every check runs for both modes; the exact mode passes them trivially (it is bit-identical to the oracle)."""
import os
import sys

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from ag_pathtracer_amd import tiles
from helpers import close_fraction, gpu_context, gpu_scene, oracle_render, oracle_scene, tile_rows

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as mg  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ["exact", "fast"]
SEED_A, SEED_B = 0, 0x5EED0B


def lens_mirror():
    d = ag.scenes.scene_c1()
    d.name = "lens-mirror"
    d.add_material(ag.MAT_MIRROR, [.9, .9, .9])
    d.add_sphere([2.2, 0.0, 0.5], 1.0, 2)
    d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.1)
    return d


# name -> (description, film W, H, tile (x0, y0, w, h), max depth)
SCENES = {
    "c2": (lambda: ag.scenes.scene_c2(), 1280, 720, (592, 312, 96, 96), 5),
    "c3": (lambda: ag.scenes.scene_c3(), 1920, 1080, (912, 492, 96, 96), 5),
    "c5": (lambda: ag.scenes.scene_c5(scale=0.2), 1920, 1080, (912, 492, 96, 96), 5),
    "simple": (lambda: ag.scenes.scene_simple_test(), 128, 128, (0, 0, 128, 128), 5),
    "lens_mirror": (lens_mirror, 96, 96, (0, 0, 96, 96), 3),
}
_DESC = {}


def desc_of(name):
    if name not in _DESC:
        _DESC[name] = SCENES[name][0]()
    return _DESC[name]


def oracle_tile(name, spp, seed_base):
    _, W, H, tile, depth = SCENES[name]
    acc, st = oracle_render(desc_of(name), W, H, spp, depth, tile=tile, seed_base=seed_base, threads=16)
    return tile_rows(acc, H, tile).reshape(-1, 3), st


def gpu_tile(g, name, spp, seed_base, **kw):
    _, W, H, tile, depth = SCENES[name]
    acc, st = ag.PathTracer(depth).render_to_host(g, W, H, spp, tile=tile, seed_base=seed_base, **kw)
    return tile_rows(acc, H, tile).reshape(-1, 3), st


def scene_in_mode(name, mode):
    g = gpu_scene(desc_of(name))
    g.set_shading_arith(mode)
    return g


# ---- L1 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_l1_bsdf_known_answers(mode):
    g = np.load(os.path.join(HERE, "golden", "bsdf_kat.npz"))
    s = ag.Scene(gpu_context())
    mats = mg.kat_materials(s)
    s.add_sphere([0, 0, 0], 1.0, mats[0])
    s.commit()
    s.set_shading_arith(mode)   # after commit: takes effect at the next call
    ok = {k: [] for k in ("f", "pdf", "sf", "spdf", "wi", "spec", "pdf_zero", "spdf_zero")}
    bit_same = []   # f / pdf entries bit-identical to the fixture (the exact kernels' answers)
    for m in mats:
        f, pdf = s.bsdf_eval(m, g["wo"], g["wi"])
        wi, sf, spdf, spec = s.bsdf_sample(m, g["wo"], g["u"])
        want = {"f": g["f_%d" % m], "pdf": g["pdf_%d" % m], "sf": g["sf_%d" % m], "spdf": g["spdf_%d" % m], "wi": g["swi_%d" % m]}
        got = {"f": f, "pdf": pdf, "sf": sf, "spdf": spdf, "wi": wi}
        for k in want:
            fin = np.isfinite(want[k])
            assert np.isfinite(got[k][fin]).all(), "material %d %s: non-finite where the fixture is finite" % (m, k)
        for k in ("f", "pdf", "sf", "spdf"):
            ok[k].append((np.abs(got[k] - want[k]) <= 1e-4 * np.abs(want[k]) + 1e-6).reshape(-1))
        both = (spdf != 0) & (want["spdf"] != 0)   # wi is only defined where a direction was sampled
        ok["wi"].append(np.all(np.abs(wi - want["wi"]) <= 1e-5, axis=1)[both])
        ok["spec"].append(spec == g["spec_%d" % m])
        ok["pdf_zero"].append((pdf == 0) == (want["pdf"] == 0))
        ok["spdf_zero"].append((spdf == 0) == (want["spdf"] == 0))
        bit_same.append(np.concatenate([f.reshape(-1).view(np.uint32) == want["f"].reshape(-1).view(np.uint32),
                                        pdf.view(np.uint32) == want["pdf"].view(np.uint32)]))
    s.close()
    bit_same = float(np.concatenate(bit_same).mean())
    print(mode, "f / pdf entries bit-identical to the fixture: %.4f" % bit_same)
    if mode == "exact":
        assert bit_same == 1.0
    else:   # the known-answer entry points ran the _fast kernels, not the exact ones
        assert bit_same < 1.0
    frac = {k: float(np.concatenate(v).mean()) for k, v in ok.items()}
    print(mode, frac)
    for k, v in frac.items():
        assert v >= (1.0 if mode == "exact" else 0.999), (k, frac)


def peak_directions(n=512, seed=13):
    """(wo, wi) in the shading frame with the half vector inside the narrowest lobe the materials have -- alpha at its clamp of .001 --:
    tan(theta_h) = .001 t, t in [0, 3], where sin^2(theta_h) = 1 - wh.z^2 is about 1e-6 and an ulp of wh.z is a tenth of D"""
    rng = np.random.RandomState(seed)
    wo = rng.normal(size=(n, 3))
    wo[:, 2] = np.abs(wo[:, 2]) + 0.2
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    tan, phi = 1e-3 * rng.uniform(0, 3, n), rng.uniform(0, 2 * np.pi, n)
    wh = np.stack([tan * np.cos(phi), tan * np.sin(phi), np.ones(n)], 1)
    wh /= np.linalg.norm(wh, axis=1, keepdims=True)
    wi = 2 * (wo * wh).sum(1, keepdims=True) * wh - wo
    return wo.astype(np.float32), wi.astype(np.float32)


@pytest.mark.parametrize("mode", MODES)
def test_l1_bsdf_at_the_peak_of_the_narrowest_lobe(mode):
    """L1 where the fixture's materials (roughness >= .25) do not reach: the oracle's f and pdf of smooth Disney materials at half
    vectors inside the lobe.  The half vector keeps normalize's bits in the fast units (agpt_shade_arith.h: sh_normalize_rn); through
    v_rsq_f32 the fast f and pdf were off by up to a tenth here."""
    wo, wi = peak_directions()
    d = ag.SceneDesc("peak")
    mats = [d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], rough, metal) for rough, metal in ((0.0, 1.0), (0.02, 0.0), (0.0, 0.5))]
    d.add_sphere([0, 0, 0], 1.0, mats[0])
    o, s = oracle_scene(d), gpu_scene(d)
    s.set_shading_arith(mode)
    ok = []
    try:
        for m in mats:
            f, pdf = s.bsdf_eval(m, wo, wi)
            want = [o.bsdf_eval(m, a, b) for a, b in zip(wo, wi)]
            want_f, want_pdf = np.array([w[0] for w in want], np.float32), np.array([w[1] for w in want], np.float32)
            assert (want_pdf > 100).mean() > 0.9                 # inside the lobe: its pdf is 1 / (pi alpha^2) ~ 3e5 at the centre
            ok.append(np.abs(f - want_f) <= 1e-4 * np.abs(want_f) + 1e-6)
            ok.append((np.abs(pdf - want_pdf) <= 1e-4 * np.abs(want_pdf) + 1e-6)[:, None])
            if mode == "exact":
                assert f.tobytes() == want_f.tobytes() and pdf.tobytes() == want_pdf.tobytes()
    finally:
        s.close()
    frac = float(np.concatenate([a.reshape(-1) for a in ok]).mean())
    print(mode, "f / pdf entries within rel 1e-4 of the oracle at the lobe's peak: %.5f" % frac)
    assert frac >= (1.0 if mode == "exact" else 0.999)


# ---- L2 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["c2", "c3", "c5", "simple", "lens_mirror"])
def test_l2_pixels_at_low_spp(mode, name):
    g = scene_in_mode(name, mode)
    for spp in (1, 2):
        got, st = gpu_tile(g, name, spp, SEED_A)
        want, ost = oracle_tile(name, spp, SEED_A)
        frac = close_fraction(got, want, 1e-3)
        print(name, mode, spp, "within 1e-3: %.5f  rays %d / %d" % (frac, st.rays, ost.rays))
        assert frac >= 0.99, (name, spp, frac)
    g.close()


# ---- L3 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["c2", "c3", "c5"])
def test_l3_image_statistics_at_16spp(mode, name):
    spp = 16
    g = scene_in_mode(name, mode)
    got_a, _ = gpu_tile(g, name, spp, SEED_A)
    got_b, _ = gpu_tile(g, name, spp, SEED_B)
    g.close()
    ora, _ = oracle_tile(name, spp, SEED_A)
    orb, _ = oracle_tile(name, spp, SEED_B)
    m_got, m_want = got_a.mean(0, dtype=np.float64), ora.mean(0, dtype=np.float64)
    mean_rel = np.abs(m_got - m_want) / np.maximum(np.abs(m_want), 1e-12)
    rmse = lambda a, b: float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))
    r_fast, r_oracle = rmse(got_b, ora), rmse(orb, ora)
    print(name, mode, "mean rel %s  rmse %.6g vs oracle seed-to-seed %.6g" % (mean_rel, r_fast, r_oracle))
    assert (mean_rel <= 1e-3).all(), mean_rel
    assert r_fast <= 1.2 * r_oracle, (r_fast, r_oracle)
    assert r_oracle > 0


# ---- determinism and ray totals --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_determinism_splits_and_rank_shares(mode):
    desc = ag.scenes.scene_c3(aspect=256 / 144.)
    W, H, spp = 256, 144, 4
    g = gpu_scene(desc)
    g.set_shading_arith(mode)
    pt = ag.PathTracer(5)
    full, st = pt.render_to_host(g, W, H, spp)
    again, st2 = pt.render_to_host(g, W, H, spp)
    assert again.tobytes() == full.tobytes() and st2.rays == st.rays
    split, st3 = pt.render_to_host(g, W, H, spp, samples_per_batch=1)
    assert split.tobytes() == full.tobytes() and st3.rays == st.rays
    ctx = g.ctx
    world = 3
    dst = ctx.alloc(W * H * 16)
    try:
        ctx.memset(dst, 0xFF, W * H * 16)
        for rank in range(world):
            rows = tiles.max_local_rows(H, world)
            local = ctx.alloc(rows * W * 16)
            try:
                ctx.memset(local, 0, rows * W * 16)
                pt.render(g, W, H, spp, local, accum_pitch=W, interleave=(tiles.BLOCK_ROWS, world, rank))
                ctx.deinterleave_tiles(local, W, H, tiles.BLOCK_ROWS, world, rank, dst)
            finally:
                ctx.download(local, (1,))   # synchronises the stream before the buffer is freed
                ctx.free(local)
        got = ctx.download(dst, (H, W, 4))
    finally:
        ctx.free(dst)
    assert got[..., :3].tobytes() == full[..., :3].tobytes()
    # ray totals against the exact mode on the same scene
    g.set_shading_arith("exact")
    ex, est = pt.render_to_host(g, W, H, spp)
    g.close()
    assert abs(st.rays - est.rays) <= 1e-3 * est.rays, (st.rays, est.rays)
    assert st.outliers <= max(2 * est.outliers, 1e-6 * st.samples), (st.outliers, est.outliers)
    if mode == "exact":
        assert ex.tobytes() == full.tobytes()


# ---- switch hygiene --------------------------------------------------------------------------------------------
def test_fast_differs_and_exact_is_restored():
    desc = ag.scenes.scene_c3(aspect=160 / 90.)
    W, H, spp = 160, 90, 2
    g = gpu_scene(desc)   # committed once, switched three times
    pt = ag.PathTracer(5)
    first, st1 = pt.render_to_host(g, W, H, spp)
    g.set_shading_arith("fast")
    fast, _ = pt.render_to_host(g, W, H, spp)
    g.set_shading_arith(ag.SHADING_EXACT)
    last, st3 = pt.render_to_host(g, W, H, spp)
    g.close()
    assert fast.tobytes() != first.tobytes(), "the fast mode renders the exact image: the switch is not wired"
    assert close_fraction(fast[..., :3], first[..., :3], 1e-3) >= 0.99
    assert last.tobytes() == first.tobytes() and st3.rays == st1.rays


def test_unknown_mode_is_rejected():
    g = gpu_scene(ag.scenes.scene_c1())
    with pytest.raises(ag.AgptError):
        g.set_shading_arith(2)
    assert b"agpt_scene_set_shading_arith" in g.L.agpt_last_error()
    with pytest.raises(ValueError):
        g.set_shading_arith("approximate")
    # a rejected call leaves the mode as it was
    a, _ = ag.PathTracer(5).render_to_host(g, 32, 32, 1)
    g.set_shading_arith("exact")
    b, _ = ag.PathTracer(5).render_to_host(g, 32, 32, 1)
    g.close()
    assert a.tobytes() == b.tobytes()


def test_li_batch_honours_the_mode():
    desc = ag.scenes.scene_c3(scale=0.05)
    o = oracle_scene(desc, 5)
    g = gpu_scene(desc)
    n = 2000
    rng = np.random.RandomState(11)
    rays = np.zeros(n, ag.RAY_DTYPE)
    states = np.zeros(n, np.uint32)
    for i in range(n):
        r, s = o.camera_ray(float(rng.uniform()), float(rng.uniform()), rng=int(rng.randint(1, 2 ** 31 - 1)))
        rays[i] = r
        states[i] = s
    pt = ag.PathTracer(5)
    exact, ea, est = pt.Li(g, rays, states)
    g.set_shading_arith("fast")
    fast, fa, fst = pt.Li(g, rays, states)
    g.close()
    assert fast.tobytes() != exact.tobytes()
    assert close_fraction(fast, exact, 1e-3) >= 0.99
    assert abs(fst.rays - est.rays) <= 1e-2 * est.rays and fst.samples == n
