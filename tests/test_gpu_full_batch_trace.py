"""The full-batch trace kernels: the 14 instantiations k_trace_fast<MODE, ., LIST, COUNT = false, SPILL, PEEK = false, COH> that a batch
of agpt_ctx::small_batch_paths (48 Mi) paths or more selects -- MODE 0 / 1 / 2 x LIST x SPILL, and COH x SPILL.  Every other GPU
file runs batches far below that and therefore the PEEK forms.  Here a second context, created with AGPT_SMALL_BATCH_PATHS=0, calls
no batch small: ray queries, the edges of the work distribution (full_batch_cases.py; preconditions: test_full_batch_cases.py) and
renders go through the !PEEK forms and must give the oracle's bits and, byte for byte, what the shared default context gives.  One
test renders a batch of exactly 48 Mi paths on a default context, where the threshold itself selects them.

Without the peek a wave that finds its segment drained walks on through all eight segments with one failing atomic each, the empty
trailing ones of a short queue included (agpt_trace_kernels.h, pump_issue); that walk is what the ray counts of the edge test are about.
Everything is bit-exact; there is no tolerance in this file."""
import os
import time

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import full_batch_cases as fb
import ray_edge_cases as rc
from helpers import bits, gpu_context, gpu_scene, oracle_render, oracle_scene, random_rays, tile_rows
from test_gpu_coherent_trace import DEPTH, check, small_c3, through_two_emitters
from test_gpu_intersect import big_leaf_case, check_closest, deep_mesh_case, scene_75_primitives

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def full_ctx():
    """A context for which no batch is small (AGPT_SMALL_BATCH_PATHS is read at agpt_init): every non-counting production trace
    launch on it is a PEEK = false instantiation."""
    old = os.environ.get("AGPT_SMALL_BATCH_PATHS")
    os.environ["AGPT_SMALL_BATCH_PATHS"] = "0"
    try:
        ctx = ag.Context(0)
    finally:
        if old is None:
            del os.environ["AGPT_SMALL_BATCH_PATHS"]
        else:
            os.environ["AGPT_SMALL_BATCH_PATHS"] = old
    yield ctx
    ctx.close()


def on(ctx, desc):
    return desc.instantiate(ag.Scene(ctx))


# ---- ray queries: MODE 0 and 1 ---------------------------------------------------------------------------------------------------
def query(full_ctx, desc, rays):
    """check_closest on the full-batch context -- production and instrumented kernels against the oracle, closest and any-hit --
    and the production kernels' records of that context against the shared default context's, byte for byte.  The oracle's hits."""
    hits = check_closest(desc, rays, ctx=full_ctx)
    f, g = on(full_ctx, desc), gpu_scene(desc)
    try:
        assert f.Intersect(rays)[0].tobytes() == g.Intersect(rays)[0].tobytes()
        assert f.IntersectP(rays)[0].tobytes() == g.IntersectP(rays)[0].tobytes()
    finally:
        f.close()
        g.close()
    return hits


@pytest.mark.parametrize("cls,scn", [(c, s) for c in rc.CLASSES for s in ("grid1", "grid_long")])
def test_ray_edge_classes(full_ctx, cls, scn):
    """The numeric edges of the traversal arithmetic through the short-list kernel (grid1) and k_trace_fast<LIST> (grid_long)."""
    desc, rays = rc.case(cls, scn)
    assert query(full_ctx, desc, rays) > 0


def test_deep_bvh_spills(full_ctx):
    """SPILL: a BVH deeper than the stack entries kept in LDS."""
    assert query(full_ctx, *deep_mesh_case()) > 0


def test_75_primitives(full_ctx):
    d = scene_75_primitives()
    assert query(full_ctx, d, random_rays(d, 30000, seed=16)) > 4000


def test_big_leaves(full_ctx):
    assert query(full_ctx, *big_leaf_case()) > 300


# ---- the edges of the work distribution ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_scenes(full_ctx):
    """per scene of full_batch_cases: (rays, oracle closest, oracle any-hit, [(context name, scene, rays in HBM, scrub rays in HBM,
    hit records in HBM)]) on the full-batch and on the shared default context"""
    out, held = {}, []
    for scn in fb.SCENES:
        desc, rays, closest, any_ = fb.edge_count_rays(scn)
        scrub = fb.scrub_rays(desc, fb.N_MAX)
        per_ctx = []
        for name, ctx in (("full-batch", full_ctx), ("default", gpu_context())):
            g = on(ctx, desc)
            rp, sp, hp = ctx.alloc(rays.nbytes), ctx.alloc(scrub.nbytes), ctx.alloc(fb.N_MAX * ag.HIT_DTYPE.itemsize)
            ctx.upload(rp, rays)
            ctx.upload(sp, scrub)
            per_ctx.append((name, g, rp, sp, hp))
            held.append((ctx, g, (rp, sp, hp)))
        out[scn] = (rays, closest, any_, per_ctx)
    yield out
    for ctx, g, ptrs in held:
        for p in ptrs:
            ctx.free(p)
        g.close()


@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any-hit"])
@pytest.mark.parametrize("scn", list(fb.SCENES))
@pytest.mark.parametrize("n", fb.COUNTS)
def test_work_distribution_edges(edge_scenes, n, scn, any_hit):
    """The first n edge-count rays through agpt_intersect_device: one to eight non-empty segments, full and partial last chunks.
    The N_MAX scrub rays traced first leave a miss in every slot of the context's pool, so a ray the kernel skipped shows as a miss
    where the oracle hits (at least half of every prefix does); without them the correct record of an earlier call would stand in."""
    rays, closest, any_, per_ctx = edge_scenes[scn]
    want = (any_ if any_hit else closest)[:n]
    for name, g, rp, sp, hp in per_ctx:
        ctx = g.ctx
        g.intersect_device(sp, fb.N_MAX, hp, any_hit=any_hit)
        assert not ctx.download(hp, (fb.N_MAX,), ag.HIT_DTYPE)["hit"].any(), name
        ctx.memset(hp, 0xFF, fb.N_MAX * ag.HIT_DTYPE.itemsize)
        g.intersect_device(rp, n, hp, any_hit=any_hit)
        got = ctx.download(hp, (fb.N_MAX,), ag.HIT_DTYPE)
        assert (got[n:].view(np.uint8) == 0xFF).all(), name          # nothing written past the n records
        got = got[:n]
        skipped = np.nonzero((got["hit"] == 0) & (want["hit"] == 1))[0]
        assert np.array_equal(got["hit"], want["hit"]), (name, n, "first differing rays", skipped[:8], len(skipped))
        if not any_hit:
            assert np.array_equal(got["prim"], want["prim"]) and np.array_equal(got["tri"], want["tri"]), (name, n)
            m = want["hit"] == 1
            for f in ("t", "b1", "b2"):
                assert np.array_equal(bits(got[f][m]), bits(want[f][m])), (name, n, f)


# ---- renders: MODE 0 with re-cast, MODE 2, MODE 1, COH ---------------------------------------------------------------------------
def deep_emitter():
    from test_gpu_render import deep_mesh_with_emitter
    return deep_mesh_with_emitter()[0]


def lit_1500():
    from test_gpu_long_lists import lit_1500_primitives
    return lit_1500_primitives()


# name: (scene, W, H, spp, samples per batch)
RENDERS = {
    "small_c3": (small_c3, 32, 16, 64, 0),                                                       # COH, then MODE 0 / 1 / 2
    "thin_lens": (lambda: ag.scenes.scene_simple_test(aperture=0.1), 32, 16, 64, 0),            # COH bundles that diverge
    "two_emitters": (lambda: through_two_emitters()[0], 32, 16, 64, 0),                          # COH with re-casts
    "c1_row_major": (ag.scenes.scene_c1, 80, 60, 5, 2),                                          # G < 64, three batches
    "deep_emitter": (deep_emitter, 64, 48, 2, 0),                                                # SPILL + re-cast
    "deep_emitter_coherent": (deep_emitter, 16, 16, 64, 0),                                      # COH x SPILL
    "long_list_1500": (lit_1500, 48, 36, 2, 0),                                                  # LIST
    "deep_long_list": (fb.deep_long_list, *fb.DEEP_LONG_FILM, 2, 0),                                           # LIST x SPILL
}


@pytest.mark.parametrize("name", list(RENDERS))
def test_render(monkeypatch, full_ctx, name):
    """test_gpu_coherent_trace.check on the full-batch context -- the film as is and with AGPT_NO_COHERENT=1 byte-equal, the oracle's
    bits, ray total and outliers -- and the same render on the shared default context, byte-equal with equal ray counts."""
    make, W, H, spp, spb = RENDERS[name]
    desc = make()
    a, sa = check(monkeypatch, desc, W, H, spp, spb=spb, ctx=full_ctx)
    g = gpu_scene(desc)
    b, sb = ag.PathTracer(DEPTH).render_to_host(g, W, H, spp, samples_per_batch=spb)
    g.close()
    assert a.tobytes() == b.tobytes()
    assert (sa.rays, sa.closest_rays, sa.anyhit_rays, sa.answered_rays, sa.outliers) == (sb.rays, sb.closest_rays, sb.anyhit_rays, sb.answered_rays, sb.outliers)
    assert sa.anyhit_rays > 0 and sa.closest_rays > W * H * spp      # shadow rays and rays beyond the camera's were traced


def test_li_batch_equal_on_both_contexts(full_ctx):
    """agpt_li_batch on the rays of test_gpu_li.py's comparison on C1 (which holds the default context to the oracle): radiance,
    stream states and ray counts of the full-batch context are the default context's."""
    from test_gpu_li import camera_rays
    desc = ag.scenes.scene_c1()
    rays, states = camera_rays(oracle_scene(desc, 5), 3000, seed=7)
    f, g = on(full_ctx, desc), gpu_scene(desc)
    try:
        a, a_after, sa = ag.PathTracer(5).Li(f, rays, states)
        b, b_after, sb = ag.PathTracer(5).Li(g, rays, states)
    finally:
        f.close()
        g.close()
    assert a.tobytes() == b.tobytes() and a_after.tobytes() == b_after.tobytes()
    assert (sa.rays, sa.closest_rays, sa.anyhit_rays) == (sb.rays, sb.closest_rays, sb.anyhit_rays) and sa.rays > 3000 and np.any(a > 0)


# ---- the real threshold ----------------------------------------------------------------------------------------------------------
def test_batch_of_exactly_48_mi_paths():
    """1024 x 768 at 64 spp in one batch is 48 << 20 paths, the first size that is not small: on a context with no knob set the
    threshold itself selects the !PEEK instantiations (and, the sample group being 64, the coherent launch).  The same film in two
    batches of 32 samples -- small batches, sample groups of 32, no coherent launch -- must be byte-equal with the same ray counts,
    and a 32 x 16 tile of it the oracle's, bit for bit.  (The pool of a context never shrinks and this one holds some 12 GB: the
    context is this test's own and is closed at its end.)"""
    W, H, spp = 1024, 768, 64
    assert W * H * spp == 48 << 20
    assert "AGPT_SMALL_BATCH_PATHS" not in os.environ
    tile = (496, 376, 32, 16)
    desc = ag.scenes.scene_c1()
    oacc, _ = oracle_render(desc, W, H, spp, DEPTH, tile=tile)
    ctx = ag.Context(0)
    g = on(ctx, desc)
    try:
        pt = ag.PathTracer(DEPTH)
        t0 = time.perf_counter()
        one, s1 = pt.render_to_host(g, W, H, spp)
        t1 = time.perf_counter()
        two, s2 = pt.render_to_host(g, W, H, spp, samples_per_batch=32)
        t2 = time.perf_counter()
    finally:
        g.close()
        ctx.close()
    print("one batch of 48 Mi paths: %.2f s, two batches of 24 Mi: %.2f s, %d rays" % (t1 - t0, t2 - t1, s1.rays))
    assert one.tobytes() == two.tobytes()
    assert (s1.rays, s1.closest_rays, s1.anyhit_rays, s1.answered_rays, s1.outliers) == (s2.rays, s2.closest_rays, s2.anyhit_rays, s2.answered_rays, s2.outliers)
    got, want = tile_rows(one, H, tile), tile_rows(oacc, H, tile)
    assert np.array_equal(bits(got), bits(want))
    assert want.mean() > 0.01 and len(np.unique(bits(want))) > 1000     # the tile shows the scene, not a flat backdrop
