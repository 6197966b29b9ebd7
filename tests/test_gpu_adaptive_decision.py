"""agpt_render_adaptive's decision and active list on crafted film states (tests/adaptive_cases.py), above one select / compact block.

The call takes the film's state as input, so each test uploads a state whose outcome the contract of include/agpt.h fixes -- which
pixels take samples, and what they hold afterwards -- and compares the buffers it reads back with the CPU oracle and the fp32 model
(tests/adaptive_model.py).  A pixel was active in a single-round call exactly when its count grew.  Three films of three blocks each:
row-major with a last block of 258 pixels, 8x8-tiled, and a tile inside a larger film's buffer (accum_pitch > w, accum_row0 > 0).
Nothing here allows a decision to go either way: the stop test is plain fp32 with IEEE divide and square root, and the model is too."""
import re

import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_model as am
import ag_pathtracer_amd as ag
import helpers
from helpers import deinterleave_np, gpu_context, gpu_scene, scene_c1

pytestmark = pytest.mark.gpu

F = np.float32
FILMS = ac.films()
N0, STEP, MAX, REL, FLOOR = ac.N0, ac.STEP, ac.MAX, ac.REL, ac.FLOOR
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def scene():
    return cached("scene", lambda: gpu_scene(scene_c1()))


def samples(name):
    """per-sample oracle radiance [MAX, H, W, 3] of a film's tile: computed once, never written"""
    f = FILMS[name]
    return cached(("samples", name), lambda: helpers.oracle_samples(scene_c1(), f.W, f.H, MAX, tile=f.tile))


def oracle_at(name, n):
    """helpers.oracle_render of a film's tile at n samples: the accumulator [H, W, 4]"""
    f = FILMS[name]
    return cached(("oracle", name, n), lambda: helpers.oracle_render(scene_c1(), f.W, f.H, n, tile=f.tile)[0])


def call(film, acc, m2, min_spp, max_spp, step, rel, floor=FLOOR, **kw):
    """one agpt_render_adaptive on uploaded buffers of the film's shape -> (accum, moment2, stats, adaptive stats)"""
    ctx = gpu_context()
    acc = np.ascontiguousarray(acc, F)
    m2 = np.ascontiguousarray(m2, F)
    assert acc.shape == film.shape + (4,) and m2.shape == film.shape
    pa, pm = ctx.alloc(acc.nbytes), ctx.alloc(m2.nbytes)
    try:
        ctx.upload(pa, acc)
        ctx.upload(pm, m2)
        kw.update(film.render_kw())
        try:
            st, ast = ag.PathTracer(5).render_adaptive(scene(), film.W, film.H, pa, pm, min_spp, max_spp, step, rel, floor, **kw)
        except ag.AgptError as e:
            e.buffers = (ctx.download(pa, acc.shape), ctx.download(pm, m2.shape))
            raise
        return ctx.download(pa, acc.shape), ctx.download(pm, m2.shape), st, ast
    finally:
        ctx.free(pa)
        ctx.free(pm)


def close_m2(got, model):
    """the moment2 tolerance of test_gpu_adaptive.py"""
    return np.abs(got - model) <= 1e-5 * np.abs(model) + 1e-30


def check_single_round(name, c, out, n_after, min_spp):
    """the film after one call on the crafted state c: active pixels hold the oracle's n_after samples, every other element of both
    buffers is byte-identical, and the statistics count the pattern"""
    f = FILMS[name]
    acc, m2, st, ast = out
    act = (c["cls"] == ac.ACTIVE) | (c["cls"] == ac.FRESH)
    size = int(act.sum())
    keep = np.ones(f.shape, bool)
    keep[f.brow[act], f.bcol[act]] = False
    assert acc[keep].tobytes() == c["accum"][keep].tobytes()
    assert m2[keep].tobytes() == c["moment2"][keep].tobytes()
    a, m = f.gather(acc)[act], f.gather(m2)[act]
    assert (a[:, 3] == n_after).all(), np.nonzero(act)[0][a[:, 3] != n_after][:8]
    ref = f.from_film(oracle_at(name, n_after))[act]
    bad = (a[:, :3].view(np.uint32) != ref[:, :3].view(np.uint32)).any(-1)
    assert not bad.any(), (int(bad.sum()), np.nonzero(act)[0][bad][:8])
    assert a[:, :3].tobytes() == c["exp_rgb"][act].tobytes()
    assert close_m2(m, c["exp_moment2"][act]).all()
    assert ast.rounds == (1 if size else 0)
    assert ast.active_last == size
    assert ast.samples == size * n_after - int(f.gather(c["accum"])[act, 3].sum()) and st.samples == ast.samples
    n = f.gather(acc)[:, 3]
    assert ast.pixels_stopped == int((c["cls"] == ac.STOPPED).sum()) == int(((n >= min_spp) & (n < n_after)).sum())


# ---- the active list ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILMS))
@pytest.mark.parametrize("pattern", ac.PATTERNS)
def test_active_list_patterns(name, pattern):
    f = FILMS[name]
    act = ac.pattern(f, pattern)
    c = ac.craft(f, act, samples(name), N0, STEP, MAX, seed=11)
    out = call(f, c["accum"], c["moment2"], N0, MAX, STEP, REL)
    check_single_round(name, c, out, MAX, N0)
    if pattern == "none":
        assert out[0].tobytes() == c["accum"].tobytes() and out[1].tobytes() == c["moment2"].tobytes()
        assert out[3].rounds == 0 and out[3].samples == 0 and out[3].active_last == 0


@pytest.mark.parametrize("name", list(FILMS))
@pytest.mark.parametrize("pattern", ["all", "first", "last", "last_block", "empty_middle", "one_per_wave", "pass_1", "random_50"])
def test_active_list_of_fresh_pixels(name, pattern):
    """active = not yet sampled (w = 0 < min_spp), every other pixel at max_spp; min = step = max, so one listed round of STEP ends
    the call (the full-tile warm-up is not taken: the counts differ -- except for `all`, which is the warm-up)"""
    f = FILMS[name]
    act = ac.pattern(f, pattern)
    c = ac.craft(f, act, samples(name), 0, STEP, STEP, fresh=True, seed=12)
    for rel in (REL, float("inf")):      # active whatever rel_error is
        out = call(f, c["accum"], c["moment2"], STEP, STEP, STEP, rel)
        check_single_round(name, c, out, STEP, STEP)


# ---- the warm-up choice ---------------------------------------------------------------------------------------------------------------
W_STEP, W_MIN = 2, 6     # min_spp = max_spp = 6 in steps of 2: a film at 0, 2 or 4 everywhere is below min_spp


def uniform_state(name, n):
    """the film with every tile pixel at n true samples (the model's sums of the oracle's radiance)"""
    f = FILMS[name]
    S, M = ac.sums(f.from_samples(samples(name)), n)
    acc, m2 = np.zeros(f.shape + (4,), F), np.zeros(f.shape, F)
    f.scatter(acc, np.concatenate([S, np.full((f.NP, 1), n, F)], -1))
    f.scatter(m2, M)
    return acc, m2


def set_pixel(name, acc, m2, p, n):
    f = FILMS[name]
    S, M = ac.sums(f.from_samples(samples(name))[:, p:p + 1], n)
    acc[f.brow[p], f.bcol[p]] = [S[0, 0], S[0, 1], S[0, 2], n]
    m2[f.brow[p], f.bcol[p]] = M[0]


def check_against_oracle_at_own_count(name, acc, m2, model_m2=None):
    f = FILMS[name]
    a = f.gather(acc)
    counts = a[:, 3].astype(np.int64)
    assert (counts == a[:, 3]).all()
    for cnt in np.unique(counts):
        sel = counts == cnt
        ref = f.from_film(oracle_at(name, int(cnt)))[sel] if cnt else np.zeros((int(sel.sum()), 4), F)
        assert a[sel][:, :3].tobytes() == ref[:, :3].tobytes(), (name, cnt)
    if model_m2 is not None:
        assert close_m2(f.gather(m2), model_m2).all()
    return counts


@pytest.mark.parametrize("n", [0, W_STEP])
def test_uniform_film_below_min_takes_one_full_tile_round(n):
    name = "row_major"
    f = FILMS[name]
    acc0, m0 = uniform_state(name, n)
    acc, m2, st, ast = call(f, acc0, m0, W_MIN, W_MIN, W_STEP, REL)
    _, M = ac.sums(f.from_samples(samples(name)), W_MIN)
    counts = check_against_oracle_at_own_count(name, acc, m2, M)
    assert (counts == W_MIN).all()
    assert ast.rounds == 1 and ast.active_last == f.NP
    assert ast.samples == f.NP * (W_MIN - n) and st.samples == ast.samples and ast.pixels_stopped == 0


def odd_pixel(f, block):
    return f.NP - 3 if block == f.n_blocks - 1 else block * ac.BLOCK_PIXELS + 777


@pytest.mark.parametrize("block", [2, 1, 0])
@pytest.mark.parametrize("base,odd", [(2, 4), (4, 2), (2, 0), (0, 6)])
def test_one_pixel_at_another_count_rules_out_the_full_tile_round(base, odd, block):
    """a film below min_spp except for one pixel (of the last, the middle or the first block) at another valid count: rounds over
    the listed pixels, as the model runs them; no pixel ends above what its own rounds give.  The host tells the two kinds of round
    apart by the minimum and the maximum count, which the blocks combine with atomics: a minimum taken from whichever block wrote
    last is wrong for at least two of the three placements of a lower pixel, and shows as a full-tile round the model does not run
    ((2, 0): two rounds where the model needs three)."""
    name = "row_major"
    f = FILMS[name]
    p = odd_pixel(f, block)
    acc0, m0 = uniform_state(name, base)
    set_pixel(name, acc0, m0, p, odd)
    acc, m2, st, ast = call(f, acc0, m0, W_MIN, W_MIN, W_STEP, REL)
    model = am.run(f.from_samples(samples(name)), W_MIN, W_MIN, W_STEP, REL, FLOOR, counts=f.gather(acc0)[:, 3],
                   accum=f.gather(acc0), moment2=f.gather(m0))
    counts = check_against_oracle_at_own_count(name, acc, m2, model["moment2"])
    assert np.array_equal(counts, model["counts"]) and (counts == W_MIN).all()
    assert ast.rounds == model["rounds"]
    assert ast.samples == int((counts - f.gather(acc0)[:, 3]).sum()) and st.samples == ast.samples
    assert ast.active_last == (1 if odd < base else f.NP - 1)


@pytest.mark.parametrize("block", [2, 0])
@pytest.mark.parametrize("value", ac.invalid_counts(W_STEP).tolist())
def test_invalid_count_in_a_uniform_film_is_refused(value, block):
    name = "row_major"
    f = FILMS[name]
    acc0, m0 = uniform_state(name, W_STEP)
    acc0[f.brow[odd_pixel(f, block)], f.bcol[odd_pixel(f, block)], 3] = value
    with pytest.raises(ag.AgptError) as e:
        call(f, acc0, m0, W_MIN, W_MIN, W_STEP, REL)
    assert re.search(rb"agpt_render_adaptive: 1 tile pixels", ag.lib().agpt_last_error())
    assert e.value.buffers[0].tobytes() == acc0.tobytes() and e.value.buffers[1].tobytes() == m0.tobytes()


# ---- invalid counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["row_major", "tiled", "tile"])
@pytest.mark.parametrize("per_block", [(6, 6, 6), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 3, 5)])
def test_invalid_counts_are_counted_over_the_blocks_and_refused(name, per_block):
    f = FILMS[name]
    c = ac.craft(f, ac.pattern(f, "random_50"), samples(name), N0, STEP, MAX, seed=13)
    acc0, m0 = c["accum"], c["moment2"]
    p, vals = ac.invalid_placements(f, STEP, per_block)
    assert len(p) == sum(per_block)
    acc0[f.brow[p], f.bcol[p], 3] = vals
    with pytest.raises(ag.AgptError) as e:
        call(f, acc0, m0, N0, MAX, STEP, REL)
    msg = ag.lib().agpt_last_error()
    found = re.search(rb"agpt_render_adaptive: (\d+) tile pixels", msg)
    assert found and int(found.group(1)) == len(p), msg
    assert e.value.buffers[0].tobytes() == acc0.tobytes() and e.value.buffers[1].tobytes() == m0.tobytes()


# ---- the decision arithmetic ----------------------------------------------------------------------------------------------------------
D_REL = 0.05
# n -> (min_spp, step_spp); max_spp = n + step: every pixel is tested once and the call is one round
DECISIONS = {2: (2, 2), 3: (3, 1), 4: (4, 4), 64: (4, 4), 1 << 23: (4, 4), (1 << 24) - 1: (2, 1)}


def run_decision(n, rel, floor, film_rel=None):
    """upload the crafted decision film at count n, run one call, and compare every pixel with the model: -> the adaptive stats"""
    name = "row_major"
    f = FILMS[name]
    mn, step = DECISIONS[n]
    S, M, kind = ac.decision_film(f.NP, n, D_REL if film_rel is None else film_rel, floor)
    acc0, m0 = np.zeros(f.shape + (4,), F), np.zeros(f.shape, F)
    f.scatter(acc0, np.concatenate([S, np.full((f.NP, 1), n, F)], -1))
    f.scatter(m0, M)
    acc, m2, st, ast = call(f, acc0, m0, mn, n + step, step, rel, floor)
    a = f.gather(acc)
    grew = a[:, 3] != F(n)
    expect = ac.model_active(S, M, n, rel, floor) if rel > 0 else np.ones(f.NP, bool)
    wrong = np.nonzero(grew != expect)[0]
    print("n = %d rel %g floor %g: %d of %d active under the model, %d decisions differ; kinds of those %s"
          % (n, rel, floor, expect.sum(), f.NP, len(wrong), np.bincount(kind[wrong], minlength=4).tolist()))
    assert len(wrong) == 0, [(int(p), S[p].tolist(), float(M[p]), int(kind[p])) for p in wrong[:6]]
    assert (a[grew, 3] == F(n + step)).all()
    # the pixels that grew hold S + the oracle's radiance of samples [n, n + step), added in fp32 in order; the others are untouched
    smp = cached(("decision samples", n), lambda: helpers.oracle_samples(scene_c1(), f.W, f.H, step, first=n))
    rgb = S.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(step):
            rgb = rgb + am.reject(f.from_film(smp[k]))[0]
    assert a[grew, :3].tobytes() == rgb[grew].tobytes()
    assert a[~grew].tobytes() == f.gather(acc0)[~grew].tobytes()
    assert f.gather(m2)[~grew].tobytes() == M[~grew].tobytes()
    assert ast.rounds == (1 if expect.any() else 0) and ast.active_last == int(expect.sum())
    assert ast.samples == int(expect.sum()) * step and st.samples == ast.samples
    assert ast.pixels_stopped == int((~expect).sum())
    return ast


@pytest.mark.parametrize("floor", [0.01, 0.0])
@pytest.mark.parametrize("n", list(DECISIONS))
def test_decision_is_the_models_for_every_pixel(n, floor):
    ast = run_decision(n, D_REL, floor)
    assert 2048 <= ast.active_last <= FILMS["row_major"].NP - 2048    # both members of every threshold pair decided


@pytest.mark.parametrize("rel,floor", [(float("inf"), 0.0), (float("inf"), 0.01), (0.0, 0.01), (-1.0, 0.01), (1e-30, 0.0), (1e30, 0.01)])
def test_decision_at_extreme_rel_error(rel, floor):
    """rel_error = +inf makes the right-hand side inf, or inf * 0 = NaN where mu = abs_floor = 0 (no stop); rel_error <= 0 switches
    the test off"""
    NP = FILMS["row_major"].NP
    ast = run_decision(4, rel, floor, film_rel=D_REL)
    if rel <= 0:
        assert ast.active_last == NP
    elif rel == float("inf"):
        assert (ast.active_last == 0) == (floor > 0)


# ---- sample groups and odd S ----------------------------------------------------------------------------------------------------------
GW, GH = 16, 16


@pytest.mark.parametrize("mn,step,mx", [(2, 1, 6), (3, 3, 9), (6, 6, 18), (64, 64, 128), (192, 192, 384)])
def test_sample_groups_and_odd_batches(mn, step, mx):
    """batches of S = 1, 2, 3, 6, 64 and 192 samples per pixel: sample_group(S) = 1, 2, 1, 2, 64, 64 (every adaptive test elsewhere
    runs S = 4).  A fresh frame; every pixel bit-identical to the oracle at its own count."""
    desc = scene_c1()
    smp = cached(("group samples", mx), lambda: helpers.oracle_samples(desc, GW, GH, mx))
    for rel in (0.1, 0.2, 0.05, 0.3, 0.03, 0.5, 0.02):
        model = am.run(smp, mn, mx, step, rel, FLOOR)
        if len(np.unique(model["counts"])) >= 2:
            break
    assert len(np.unique(model["counts"])) >= 2
    acc, m2, st, ast = ag.PathTracer(5).render_adaptive_to_host(scene(), GW, GH, mn, mx, step, rel, abs_floor=FLOOR)
    counts = acc[..., 3].astype(np.int64)
    levels = np.unique(counts)
    assert len(levels) >= 2 and set(levels.tolist()) <= set(range(mn, mx + 1, step)), levels
    for cnt in levels:
        ref = helpers.oracle_render(desc, GW, GH, int(cnt))[0]
        sel = counts == cnt
        assert acc[sel][:, :3].tobytes() == ref[sel][:, :3].tobytes(), (step, cnt)
    # where the model took the same decisions, its sums and second moment are the film's
    same = counts == model["counts"]
    assert acc[same][:, :3].tobytes() == model["accum"][same].tobytes()
    assert close_m2(m2[same], model["moment2"][same]).all()
    assert ast.samples == int(counts.sum()) and st.samples == ast.samples


# ---- one pixel's samples in several batches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", [0.0, 0.1])
@pytest.mark.parametrize("tile", [(5, 7, 1, 1), (9, 11, 3, 1)])
def test_tile_smaller_than_a_step_splits_a_pixels_samples(tile, rel):
    """samples_per_batch = 1 caps a batch at the tile's pixel count: with 1 or 3 pixels and 4 samples a round, one pixel's samples
    go into several batches (4 of 1; 3 + 1)"""
    W, H = 32, 24
    f = ac.Film(W, H, tile=tile)
    desc = scene_c1()
    rng = np.random.RandomState(21)
    acc0, m0 = ac.random_finite(rng, f.shape + (4,)).copy(), ac.random_finite(rng, f.shape).copy()
    f.scatter(acc0, np.zeros((f.NP, 4), F))
    f.scatter(m0, np.zeros(f.NP, F))
    acc, m2, st, ast = call(f, acc0, m0, 4, 8, 4, rel, samples_per_batch=1)
    out = ~f.tile_mask()
    assert acc[out].tobytes() == acc0[out].tobytes() and m2[out].tobytes() == m0[out].tobytes()
    a = f.gather(acc)
    counts = a[:, 3].astype(np.int64)
    assert set(counts.tolist()) <= {4, 8} and (rel > 0 or (counts == 8).all())
    smp = helpers.oracle_samples(desc, W, H, 8, tile=tile)
    for cnt in np.unique(counts):
        ref = f.from_film(helpers.oracle_render(desc, W, H, int(cnt), tile=tile)[0])
        sel = counts == cnt
        assert a[sel][:, :3].tobytes() == ref[sel][:, :3].tobytes(), cnt
        assert close_m2(f.gather(m2)[sel], ac.sums(f.from_samples(smp), int(cnt))[1][sel]).all()
    assert ast.samples == int(counts.sum()) and st.samples == ast.samples


# ---- a rank's interleaved share above one block -----------------------------------------------------------------------------------------
def test_interleaved_shares_above_one_block_equal_the_whole_film():
    """130 x 70 in row blocks of 8 over two ranks: shares of 38 and 32 rows, 4940 and 4160 pixels -- two select / compact blocks each,
    row-major (130 is no multiple of 8), the first share's rows no multiple of 8"""
    W, H, block, world = 130, 70, 8, 2
    g, ctx = scene(), gpu_context()
    acc, m2, _, _ = ag.PathTracer(5).render_adaptive_to_host(g, W, H, 4, 16, 4, 0.1, abs_floor=FLOOR)
    assert len(np.unique(acc[..., 3])) >= 2
    full_a, full_m = np.zeros_like(acc), np.zeros_like(m2)
    for rank in range(world):
        nrows = sum(min(block, H - y) for k, y in enumerate(range(0, H, block)) if k % world == rank)
        assert W * nrows > ac.BLOCK_PIXELS and (rank or nrows % 8)
        pa, pm = ctx.alloc(W * nrows * 16), ctx.alloc(W * nrows * 4)
        try:
            ctx.memset(pa, 0, W * nrows * 16)
            ctx.memset(pm, 0, W * nrows * 4)
            ag.PathTracer(5).render_adaptive(g, W, H, pa, pm, 4, 16, 4, 0.1, FLOOR, interleave=(block, world, rank))
            ca, cm = ctx.download(pa, (nrows, W, 4)), ctx.download(pm, (nrows, W))
        finally:
            ctx.free(pa)
            ctx.free(pm)
        deinterleave_np(ca, H, block, world, rank, full_a)
        deinterleave_np(cm, H, block, world, rank, full_m)
    assert full_a.tobytes() == acc.tobytes() and full_m.tobytes() == m2.tobytes()
