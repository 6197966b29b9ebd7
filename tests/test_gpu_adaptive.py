"""agpt_render_adaptive on the GPU against the CPU oracle and the numpy model of the contract (tests/adaptive_model.py).

Every pixel of an adaptive render holds samples [0, n) of its agpt_render streams, added in sample order, so it must be
bit-identical to the oracle's render of that pixel at spp = n; the counts must be the model's (up to decisions within rel 1e-4
of the threshold), and the result must not depend on how the work is split."""
import ctypes as C

import numpy as np
import pytest

import adaptive_model as am
import ag_pathtracer_amd as ag
import helpers
from helpers import deinterleave_np, gpu_context, gpu_scene, scene_c1

pytestmark = pytest.mark.gpu

W, H = 64, 48
MIN, STEP, MAX = 4, 4, 32
FLOOR = 0.01


def scene_lens_mirror():
    d = ag.scenes.scene_c1()
    d.add_material(ag.MAT_MIRROR, [.9, .9, .9])
    d.add_sphere([2.2, 0.0, 0.5], 1.0, 2)
    d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.1)
    return d


def scene_env():
    return ag.scenes.scene_simple_test(hdr=ag.scenes.synthetic_hdr())


def scene_700():
    from test_gpu_long_lists import _many_prims
    d = _many_prims(698, 22)
    d.add_area_light([0.0, 8.0, 0.0], 0.8, [70, 65, 60])
    d.add_plane([0, -6.5, 0], [10, 10], 0)
    d.add_uniform_infinite_light([.25, .3, .35])
    d.set_camera([0, 3, -16], [0, 0, 0], [0, 1, 0], 1.5, 50.0, 0.0)
    assert d.n_prims == 700
    return d


SCENES = {"c1": scene_c1, "lens_mirror": scene_lens_mirror, "env": scene_env, "prims700": scene_700}
_CACHE = {}


def oracle_render(desc, spp, spp_begin=0):
    """helpers.oracle_render at this file's film size: the accumulator alone"""
    return helpers.oracle_render(desc, W, H, spp, spp_begin=spp_begin)[0]


def setup(name):
    """(desc, GPU scene, per-sample oracle radiance [MAX, H, W, 3], rel_error that spreads the model's counts, model result)"""
    if name not in _CACHE:
        desc = SCENES[name]()
        samples = np.stack([oracle_render(desc, 1, spp_begin=s)[..., :3] for s in range(MAX)])
        for rel in (0.1, 0.2, 0.05, 0.3, 0.03):
            model = am.run(samples, MIN, MAX, STEP, rel, FLOOR)
            if len(np.unique(model["counts"])) >= 3:
                break
        _CACHE[name] = (desc, gpu_scene(desc), samples, rel, model)
    return _CACHE[name]


def adaptive(g, rel, **kw):
    kw.setdefault("abs_floor", FLOOR)
    return ag.PathTracer(5).render_adaptive_to_host(g, W, H, kw.pop("min_spp", MIN), kw.pop("max_spp", MAX), kw.pop("step_spp", STEP),
                                                    rel, **kw)


@pytest.mark.parametrize("name", list(SCENES))
def test_rel_error_zero_equals_uniform_render(name):
    desc, g, _, _, _ = setup(name)
    acc, m2, st, ast = adaptive(g, 0.0)
    assert (acc[..., 3] == MAX).all()
    ref, _ = ag.PathTracer(5).render_to_host(g, W, H, MAX)
    assert acc[..., :3].tobytes() == ref[..., :3].tobytes()
    assert ast.samples == W * H * MAX and st.samples == ast.samples
    assert ast.pixels_stopped == 0


@pytest.mark.parametrize("name", list(SCENES))
def test_pixels_match_oracle_and_model(name):
    desc, g, samples, rel, model = setup(name)
    acc, m2, st, ast = adaptive(g, rel)
    counts = acc[..., 3].astype(np.int64)
    levels = np.unique(counts)
    assert len(levels) >= 3, levels
    assert set(levels.tolist()) <= set(range(MIN, MAX + 1, STEP))
    # (2) every pixel bit-identical to the oracle at its own count
    for c in levels:
        ref = oracle_render(desc, int(c))
        sel = counts == c
        assert acc[sel][:, :3].tobytes() == ref[sel][:, :3].tobytes(), (name, c)
    # (3) counts as the model's, except decisions within rel 1e-4 of the threshold
    near = model["near"]
    assert near.mean() < 0.005, near.mean()
    same = counts == model["counts"]
    assert (same | near).all(), np.argwhere(~(same | near))[:8]
    assert same.mean() > 0.99
    mm = model["moment2"][same]
    assert np.all(np.abs(m2[same] - mm) <= 1e-5 * np.abs(mm) + 1e-30), name
    assert acc[same][:, :3].tobytes() == model["accum"][same].tobytes()
    # (8) sample totals
    assert ast.samples == int(counts.sum()) and st.samples == ast.samples
    assert ast.rounds >= 2 and ast.active_last > 0
    assert ast.pixels_stopped == int(((counts >= MIN) & (counts < MAX)).sum())


@pytest.mark.parametrize("name", ["c1", "prims700"])
def test_result_does_not_depend_on_the_split(name):
    desc, g, _, rel, _ = setup(name)
    acc, m2, _, _ = adaptive(g, rel)
    # samples_per_batch = 1: chunks of whole pixels, several batches per round
    a1, m1, _, _ = adaptive(g, rel, samples_per_batch=1)
    assert a1.tobytes() == acc.tobytes() and m1.tobytes() == m2.tobytes()
    # a tile of the film, written in place in a full-size buffer
    x0, y0, w, h = 16, 8, 32, 24
    at, mt, _, _ = adaptive(g, rel, tile=(x0, y0, w, h))
    rows = slice(H - y0 - h, H - y0)
    assert at[rows, x0:x0 + w].tobytes() == acc[rows, x0:x0 + w].tobytes()
    assert mt[rows, x0:x0 + w].tobytes() == m2[rows, x0:x0 + w].tobytes()
    outside = np.ones((H, W), bool)
    outside[rows, x0:x0 + w] = False
    assert not at[outside].any() and not mt[outside].any()
    # 2- and 3-rank interleaved shares
    ctx = gpu_context()
    block = 8
    for world in (2, 3):
        full_a = np.zeros_like(acc)
        full_m = np.zeros_like(m2)
        for rank in range(world):
            nrows = sum(min(block, H - y) for k, y in enumerate(range(0, H, block)) if k % world == rank)
            pa, pm = ctx.alloc(W * nrows * 16), ctx.alloc(W * nrows * 4)
            try:
                ctx.memset(pa, 0, W * nrows * 16)
                ctx.memset(pm, 0, W * nrows * 4)
                ag.PathTracer(5).render_adaptive(g, W, H, pa, pm, MIN, MAX, STEP, rel, FLOOR, interleave=(block, world, rank))
                ca = ctx.download(pa, (nrows, W, 4))
                cm = ctx.download(pm, (nrows, W))
                if world == 2 and rank == 1:
                    # the library's own de-interleave carries the counts in w unchanged
                    pf = ctx.alloc(W * H * 16)
                    try:
                        ctx.upload(pf, full_a)
                        ctx.deinterleave_tiles(pa, W, H, block, world, rank, pf)
                        dev_full = ctx.download(pf, (H, W, 4))
                    finally:
                        ctx.free(pf)
            finally:
                ctx.free(pa)
                ctx.free(pm)
            deinterleave_np(ca, H, block, world, rank, full_a)
            deinterleave_np(cm, H, block, world, rank, full_m)
        assert full_a.tobytes() == acc.tobytes(), world
        assert full_m.tobytes() == m2.tobytes(), world
        if world == 2:
            assert dev_full.tobytes() == acc.tobytes()
    # two calls (max 16, then max 32) continue the frame exactly
    a16, m16, _, s16 = adaptive(g, rel, max_spp=16)
    assert a16[..., 3].max() <= 16
    a32, m32, st, s32 = adaptive(g, rel, accum=a16, moment2=m16)
    assert a32.tobytes() == acc.tobytes() and m32.tobytes() == m2.tobytes()
    assert s32.samples == int((a32[..., 3] - a16[..., 3]).sum()) and st.samples == s32.samples
    assert s16.samples + s32.samples == int(acc[..., 3].sum())
    # a call that finds nothing to do adds nothing
    a_, m_, st_, s_ = adaptive(g, rel, accum=acc, moment2=m2)
    assert a_.tobytes() == acc.tobytes() and m_.tobytes() == m2.tobytes() and s_.samples == 0 and s_.rounds == 0


def test_resolve_counts_equals_resolve_per_count_group():
    desc, g, _, rel, _ = setup("c1")
    acc, _, _, _ = adaptive(g, rel)
    acc[0, :5] = 0.0   # five pixels without samples
    ctx = gpu_context()
    p = ctx.alloc(acc.nbytes)
    try:
        ctx.upload(p, acc)
        got = ctx.resolve_counts(p, W * H)
        counts = acc[..., 3].reshape(-1)
        assert (got[counts == 0] == 0).all()
        for c in np.unique(counts[counts > 0]):
            ref = ctx.resolve(p, W * H, int(c))
            sel = counts == c
            assert np.array_equal(got[sel], ref[sel]), c
    finally:
        ctx.free(p)


def test_fast_shading_is_deterministic():
    desc = scene_c1()
    g = gpu_scene(desc)
    try:
        g.set_shading_arith("fast")
        a, m, _, _ = adaptive(g, 0.1)
        b, n, _, _ = adaptive(g, 0.1)
        c, o, _, _ = adaptive(g, 0.1, samples_per_batch=1)
        assert a.tobytes() == b.tobytes() == c.tobytes()
        assert m.tobytes() == n.tobytes() == o.tobytes()
        assert len(np.unique(a[..., 3])) >= 2
    finally:
        g.close()


def test_bad_arguments_are_invalid_and_leave_buffers_untouched():
    desc, g, _, rel, _ = setup("c1")
    ctx = gpu_context()
    rng = np.random.RandomState(7)
    acc0 = rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
    acc0[..., 3] = 8.0
    m0 = rng.uniform(0, 1, (H, W)).astype(np.float32)
    off_grid = acc0.copy()
    off_grid[17, 33, 3] = 6.0
    pa, pm = ctx.alloc(acc0.nbytes), ctx.alloc(m0.nbytes)
    pt = ag.PathTracer(5)
    try:
        cases = [
            (acc0, dict(spp_count=4), (MIN, MAX, STEP)),
            (acc0, dict(spp_begin=4), (MIN, MAX, STEP)),
            (acc0, {}, (16, 8, 4)),            # min > max
            (acc0, {}, (6, 32, 4)),            # min not a multiple of step
            (acc0, {}, (4, 30, 4)),            # max not a multiple of step
            (acc0, {}, (0, 32, 4)),            # min < 2
            (acc0, {}, (4, 32, 0)),            # step < 1
            (acc0, dict(moment2_null=True), (MIN, MAX, STEP)),
            (off_grid, {}, (MIN, MAX, STEP)),  # an incoming count off the step grid
        ]
        for acc_in, kw, (mn, mx, st) in cases:
            ctx.upload(pa, acc_in)
            ctx.upload(pm, m0)
            null_m2 = kw.pop("moment2_null", False)
            with pytest.raises(ag.AgptError):
                pt.render_adaptive(g, W, H, pa, 0 if null_m2 else pm, mn, mx, st, rel, FLOOR, **kw)
            assert b"agpt_render_adaptive" in ag.lib().agpt_last_error()
            assert ctx.download(pa, (H, W, 4)).tobytes() == acc_in.tobytes(), (kw, mn, mx, st)
            assert ctx.download(pm, (H, W)).tobytes() == m0.tobytes(), (kw, mn, mx, st)
        rp, ap = ag.RenderParams(W, H, 0, 0, W, H, 0, 0, 0, 5, W, 0, 0, 0, 0, 0, 0, 0, 0), ag.AdaptiveParams(MIN, MAX, STEP, rel, FLOOR)
        assert ag.lib().agpt_render_adaptive(g.h, C.byref(rp), C.byref(ap), C.c_void_p(pa), None, None, None) == -1
    finally:
        ctx.free(pa)
        ctx.free(pm)
