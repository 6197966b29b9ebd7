"""Ended paths are retired where a batch is consumed: a path that ends with its last vertex' light sample still pending joins no
queue, and its sample is added where the batch is consumed (finished_radiance, agpt_shade_kernels.h): inside k_accumulate for
agpt_render, inside k_export_li for agpt_li_batch, and by one k_resolve_pending pass over the finished batch for
agpt_render_adaptive.  Everything here is compared bit for bit with the CPU oracle on the same per-(pixel, sample) streams.

Scene: C1 (backdrop + gold microfacet sphere, a far sphere light, a uniform sky, open to that sky) plus one emitter sphere, seen
by a camera that has the sphere, the emitter and the sky in view.
Paths end by a miss, by a black / zero-pdf BSDF sample, at MaxDepth and behind a hit on a light sphere; both light types are drawn.
A path ends WITH a pending sample when it ends at a vertex that sampled a light (no specular material here, so every shaded vertex
does): at MaxDepth -- the ray after the last bounce is answered, not traced -- or by a black sample.  It ends WITHOUT one when the
vertex it ends at is not shaded: a miss (that iteration's k_shade has added the previous vertex' sample first), MaxDepth 0, or a
camera ray that only meets emitters and the sky.  The precondition test counts both kinds with the oracle alone.

Sample counts 1, 3, 4, 64, 96 give sample groups G = 1, 1, 4, 64, 32 in one, three, one, one and three runs per pixel: a block of
k_accumulate owns 256 / G pixels (256, 64, 4, 8), which on these films is a partly filled block (13x7 = 91 pixels, 16x16 at G = 1) or
several blocks (16x16 at G = 4, 32, 64).  16x16 takes the 8x8-block pixel order, 13x7 the row-major one."""
import os

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import helpers
from ag_pathtracer_amd import tiles
from helpers import gpu_scene, oracle_scene
from oracle import binding as ob

FILMS = [(16, 16), (13, 7)]
SPPS = [1, 3, 4, 64, 96]
DEPTHS = [0, 1, 5]


def retire_scene():
    d = ag.scenes.scene_c1()
    d.name = "retire"
    d.add_area_light([1.6, -0.2, 0.4], 0.7, ag.scenes.KEY_LIGHT * np.float32(3))
    # turned to the right and opened up: the gold sphere, the emitter, the floor and -- past the backdrop's edge -- the sky are in view
    d.set_camera([-1.46, 1.16, -4.64], [3, 0.3, 0.5], [0, 1, 0], 1.0, 60.0, 0.0)
    return d


_ORACLE = {}


def oracle_render(W, H, spp, depth, spp_begin=0):
    """helpers.oracle_render of the retire scene, once per argument set: (read-only accumulator, (closest, any-hit, outliers))"""
    key = (W, H, spp, depth, spp_begin)
    if key not in _ORACLE:
        acc, st = helpers.oracle_render(retire_scene(), W, H, spp, depth, spp_begin=spp_begin)
        acc.setflags(write=False)
        _ORACLE[key] = (acc, (int(st.closest_rays), int(st.anyhit_rays), int(st.outliers)))
    return _ORACLE[key]


def film_paths(o, W, H, sample=0, seed_base=0):
    """The camera rays of MyApp::Tick's loop (myapp.cpp:165-167) for one sample of every pixel, with the stream state Li starts from."""
    rays = np.zeros(W * H, ag.RAY_DTYPE)
    states = np.zeros(W * H, np.uint32)
    for y in range(H):
        for x in range(W):
            f, u = ob.rng_floats(ob.sample_seed(y * W + x, W * H, sample, seed_base), 2)
            s = (np.float32(x) + f[0]) / np.float32(W)
            t = (np.float32(y) + f[1]) / np.float32(H)
            rays[y * W + x], states[y * W + x] = o.camera_ray(float(s), float(t), rng=int(u[1]))
    return rays, states


# ---- precondition, oracle alone ------------------------------------------------------------------------------------------
def test_scene_ends_paths_with_and_without_a_pending_sample():
    """16x16, 1 spp, MaxDepth 5 and 1: paths that end at a shaded vertex (shaded_vertices == MaxDepth: with a pending sample), paths
    whose camera ray is never shaded (without), camera rays that miss and camera rays whose first hit is the emitter sphere -- all
    counted non-zero.  (oracle_li's Ray constructor normalises the direction once more, so these are the film's paths up to an ulp
    of their first direction: the same population, which is what the counts are about.)"""
    W, H = 16, 16
    for depth in (5, 1):
        o = oracle_scene(retire_scene(), depth)
        rays, states = film_paths(o, W, H)
        hits, _ = o.intersect(rays)
        ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
        try:
            res = [o.li(rays[i], int(states[i])) for i in range(W * H)]
        finally:
            ob.set_trig_mode(ob.TRIG_LIBM)
        shaded = np.array([int(st.shaded_vertices) for _, _, st in res])
        with_pending = int((shaded == depth).sum())
        without = int((shaded == 0).sum())
        early = int(((shaded > 0) & (shaded < depth)).sum())   # ended before MaxDepth: a miss or a black sample
        misses = int((hits["hit"] == 0).sum())
        emitter = int(((hits["hit"] != 0) & (hits["prim"] == emitter_prim(o))).sum())
        print("depth %d: %d paths end with a pending sample, %d without, %d early, %d camera misses, %d emitter hits"
              % (depth, with_pending, without, early, misses, emitter))
        assert with_pending > 0 and without > 0 and misses > 0 and emitter > 0
        if depth == 5:
            assert early > 0


def emitter_prim(o):
    """List index of the emitter sphere in view: the primitive a ray aimed at its centre from the camera hits."""
    r = np.zeros(1, ag.RAY_DTYPE)
    eye = np.float32([-1.46, 1.16, -4.64])
    r["o"] = eye
    r["d"] = np.float32([1.6, -0.2, 0.4]) - eye
    r["tmax"] = np.float32(3.402823466e+38)
    h, _ = o.intersect(r)
    assert h["hit"][0] != 0 and h["tri"][0] < 0
    return int(h["prim"][0])


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    """The scene on the shared context, and on a context created with AGPT_MIS_CLOSEST=1 (read at agpt_init): MIS queries traced as
    closest hits, whose pending sample needs the chosen light (fac4) and the hit (mis_hit)."""
    g = gpu_scene(retire_scene())
    old = os.environ.get("AGPT_MIS_CLOSEST")
    os.environ["AGPT_MIS_CLOSEST"] = "1"
    try:
        ctx = ag.Context(0)
    finally:
        if old is None:
            del os.environ["AGPT_MIS_CLOSEST"]
        else:
            os.environ["AGPT_MIS_CLOSEST"] = old
    gm = retire_scene().instantiate(ag.Scene(ctx))
    yield g, gm
    gm.close()
    ctx.close()
    g.close()


def same_bits(a, b):
    """rgb of two float32 accumulators (test_dist1d.same_bits is another function: whole arrays, flattened, the first converted)"""
    return np.array_equal(np.asarray(a)[..., :3].view(np.uint32), np.asarray(b)[..., :3].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("W,H", FILMS)
def test_render_matches_oracle(scenes, W, H, spp, depth):
    """Accumulator, closest_rays, anyhit_rays and the outlier count against the oracle, in four runs.  answered_rays has no
    counterpart in the oracle (it makes every Scene::Intersect call), so it is compared between the GPU runs only: equal in the
    default and the counting run, zero with trace_all_rays."""
    g, gm = scenes
    oacc, ocounts = oracle_render(W, H, spp, depth)
    pt = ag.PathTracer(depth)
    acc, st = pt.render_to_host(g, W, H, spp)
    full, fst = pt.render_to_host(g, W, H, spp, trace_all_rays=True)
    mis, mst = pt.render_to_host(gm, W, H, spp)
    own, cst = pt.render_to_host(g, W, H, spp, counters=2)
    for name, a, s in (("default", acc, st), ("trace_all_rays", full, fst), ("mis_closest", mis, mst), ("counting", own, cst)):
        assert same_bits(a, oacc), name
        assert (s.closest_rays, s.anyhit_rays, s.outliers) == ocounts, (name, s.closest_rays, s.anyhit_rays, s.outliers, ocounts)
    # rays that are counted, not traced: none with trace_all_rays; the same in every run that answers them; some whenever a path can
    # reach its last bounce
    assert fst.answered_rays == 0
    assert st.answered_rays == cst.answered_rays
    if depth > 0:
        assert 0 < st.answered_rays < st.closest_rays
    else:
        assert st.answered_rays == 0


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", FILMS)
def test_batch_splits_agree(scenes, W, H):
    """One batch == batches of 1 == batches of 3 samples (7 spp: 3 + 3 + 1)."""
    g, _ = scenes
    pt = ag.PathTracer(5)
    oacc, ocounts = oracle_render(W, H, 7, 5)
    one, st = pt.render_to_host(g, W, H, 7)
    assert same_bits(one, oacc)
    for spb in (1, 3):
        split, sst = pt.render_to_host(g, W, H, 7, samples_per_batch=spb)
        assert split.tobytes() == one.tobytes(), spb
        assert (sst.closest_rays, sst.anyhit_rays, sst.answered_rays, sst.outliers) == \
            (st.closest_rays, st.anyhit_rays, st.answered_rays, st.outliers), spb


@pytest.mark.gpu
def test_interleaved_rank_shares_equal_the_whole_film(scenes):
    g, _ = scenes
    W, H, spp = 16, 16, 4
    pt = ag.PathTracer(5)
    full, st = pt.render_to_host(g, W, H, spp)
    assert same_bits(full, oracle_render(W, H, spp, 5)[0])
    ctx = g.ctx
    ptr = ctx.alloc(W * H * 16)
    bufs, rays = [], 0
    try:
        for r in range(2):
            ctx.memset(ptr, 0, W * H * 16)
            rays += pt.render(g, W, H, spp, ptr, interleave=(8, 2, r)).rays
            bufs.append(ctx.download(ptr, (H, W, 4))[:tiles.max_local_rows(H, 2)].copy())
    finally:
        ctx.free(ptr)
    assert tiles.deinterleave(bufs, W, H, 2).tobytes() == full.tobytes()
    assert rays == st.rays


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [5, 1])
def test_li_batch_257_rays(scenes, depth):
    """One ray more than a block: radiance, the streams' end states and the ray total equal the oracle's."""
    g, gm = scenes
    o = oracle_scene(retire_scene(), depth)
    rays, states = film_paths(o, 16, 16)
    rays = np.concatenate([rays, rays[100:101]])
    states = np.concatenate([states, states[7:8]])
    n = len(rays)
    assert n == 257
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        res = [o.li(rays[i], int(states[i])) for i in range(n)]
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    want = np.stack([L for L, _, _ in res])
    after = np.array([s for _, s, _ in res], np.uint32)
    total = sum(st.rays for _, _, st in res)
    for scene in (g, gm):
        got, got_after, st = ag.PathTracer(depth).Li(scene, rays, states)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got_after, after)
        assert st.rays == total


@pytest.mark.gpu
def test_adaptive_pixels_match_oracle(scenes):
    """agpt_render_adaptive on the 16x16 film: every pixel holds samples [0, n) of its streams and is bit-identical to the oracle's
    render at spp = n; with rel_error 0 every pixel runs to max_spp and the film is the uniform render."""
    g, _ = scenes
    W, H, MIN, STEP, MAX = 16, 16, 4, 4, 32
    pt = ag.PathTracer(5)
    acc, m2, st, ast = pt.render_adaptive_to_host(g, W, H, MIN, MAX, STEP, 0.0, abs_floor=0.01)
    assert (acc[..., 3] == MAX).all()
    assert same_bits(acc, oracle_render(W, H, MAX, 5)[0])
    levels = ()
    for rel in (0.1, 0.2, 0.05, 0.3, 0.03):
        acc, m2, st, ast = pt.render_adaptive_to_host(g, W, H, MIN, MAX, STEP, rel, abs_floor=0.01)
        counts = acc[..., 3].astype(np.int64)
        levels = np.unique(counts)
        if len(levels) >= 3:
            break
    assert len(levels) >= 3, levels
    assert set(levels.tolist()) <= set(range(MIN, MAX + 1, STEP))
    for c in levels:
        ref = oracle_render(W, H, int(c), 5)[0]
        sel = counts == c
        assert acc[sel][:, :3].tobytes() == np.asarray(ref)[sel][:, :3].tobytes(), c
    assert ast.samples == int(counts.sum()) and st.samples == ast.samples
    # the second moment of a pixel at its count: sum of Y^2 over its samples, in sample order
    per_sample = np.stack([np.asarray(oracle_render(W, H, 1, 5, spp_begin=s)[0])[..., :3] for s in range(MAX)])
    Y = (np.float32(0.212671) * per_sample[..., 0] + np.float32(0.715160) * per_sample[..., 1]) + np.float32(0.072169) * per_sample[..., 2]
    want = np.zeros((H, W), np.float32)
    for s in range(MAX):
        want = np.where(s < counts, want + Y[s] * Y[s], want).astype(np.float32)
    assert np.all(np.abs(m2 - want) <= 1e-5 * np.abs(want) + 1e-30)


@pytest.mark.gpu
def test_emitter_gauntlet_image_and_iterations():
    """The emitter gauntlet of test_gpu_render.py (paths that cross up to three emitters: re-casts beyond the planned iterations):
    image and ray total are the oracle's and the wavefront loop runs the 8 iterations it ran with the resolve queue -- the
    termination test on the ext, mis and shadow counters neither stops before an ended path's last rays are traced nor runs on."""
    from test_gpu_render import emitter_gauntlet
    d = emitter_gauntlet()
    g = gpu_scene(d)
    a, sa = ag.PathTracer(5).render_to_host(g, 160, 120, 8)
    g.close()
    o = oracle_scene(d, 5)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        oacc, ost = o.render(160, 120, 8, rng_mode=ob.RNG_PER_SAMPLE, threads=8)
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    assert same_bits(a, oacc)
    assert sa.rays == ost.rays
    print("iterations", sa.iterations)
    assert sa.iterations == 8
