"""The generators of tests/adaptive_cases.py do what tests/test_gpu_adaptive_decision.py relies on: the threshold pairs are adjacent
floats between which the model flips, the patterns have the size and block placement they are named for, the local pixel order
inverts, and the forcing rules stop or activate every pixel of the films used under the model.  No GPU."""
import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_model as am
import helpers

F = np.float32
FILMS = ac.films()
COUNTS = [2, 3, 4, 64, 1 << 23, (1 << 24) - 1]


def test_films_have_the_block_structure_the_tests_are_about():
    a, b, c = FILMS["row_major"], FILMS["tiled"], FILMS["tile"]
    assert (a.NP, a.n_blocks, a.tiled) == (8450, 3, False) and a.NP - 2 * ac.BLOCK_PIXELS == ac.BLOCK + 2
    assert (b.NP, b.n_blocks, b.tiled) == (9216, 3, True) and b.NP - 2 * ac.BLOCK_PIXELS == 4 * ac.BLOCK
    assert (c.n_blocks, c.tiled) == (3, False) and c.pitch > c.x0 + c.w > c.w and c.row0 > 0
    # the tile's buffer leaves elements no tile pixel owns on every side
    m = c.tile_mask()
    assert not m[0].any() and not m[-1].any() and not m[:, 0].any() and not m[:, -1].any() and m.sum() == c.NP


@pytest.mark.parametrize("w,rows", [(128, 72), (8, 8), (16, 24), (130, 65), (100, 85), (7, 8), (8, 7), (1, 1), (3, 1)])
def test_local_order_inverts(w, rows):
    row, col = ac.pixel_rc(w, rows)
    idx = ac.local_index(w, rows)
    assert np.array_equal(idx[row, col], np.arange(w * rows))
    assert sorted(idx.reshape(-1).tolist()) == list(range(w * rows))
    if ac.is_tiled(w, rows):
        # a wave of 64 consecutive p is one 8 x 8 patch; the patches run row-major over the region
        assert (row[:64].max(), col[:64].max()) == (7, 7) and (row[63], col[63]) == (7, 7)
        if w > 8:
            assert (row[64], col[64]) == (0, 8)
    else:
        assert np.array_equal(row * w + col, np.arange(w * rows))


def test_film_maps_p_to_its_buffer_element():
    for f in FILMS.values():
        # an image that holds its own film coordinates, in the oracle's layout (row 0 = top)
        yy, xx = np.meshgrid(np.arange(f.H), np.arange(f.W), indexing="ij")
        img = np.stack([xx, f.H - 1 - yy], -1)
        got = f.from_film(img)
        assert np.array_equal(got[:, 0], f.x) and np.array_equal(got[:, 1], f.y)
        assert f.x.min() == f.x0 and f.x.max() == f.x0 + f.w - 1 and f.y.min() == f.y0 and f.y.max() == f.y0 + f.h - 1
        # pixel_of's accum_index = ((H - 1 - y) - accum_row0) * pitch + x
        flat = np.arange(f.buf_rows * f.pitch).reshape(f.shape)
        assert np.array_equal(f.gather(flat), ((f.H - 1 - f.y) - f.row0) * f.pitch + f.x)
        assert len(np.unique(f.gather(flat))) == f.NP


@pytest.mark.parametrize("film", list(FILMS))
@pytest.mark.parametrize("name", ac.PATTERNS)
def test_patterns_have_their_size_and_placement(film, name):
    f = FILMS[film]
    a = ac.pattern(f, name)
    assert a.dtype == bool and a.shape == (f.NP,)
    size = ac.pattern_size(f, name)
    per_block = np.bincount(f.block_of()[a], minlength=f.n_blocks)
    if size is not None:
        assert int(a.sum()) == size, (name, a.sum(), size)
    if name == "first":
        assert a[0] and per_block.tolist() == [1, 0, 0]
    if name == "last":
        assert a[-1] and per_block.tolist() == [0, 0, 1]
    if name == "last_block":
        assert per_block.tolist() == [0, 0, f.NP - 2 * ac.BLOCK_PIXELS]
    if name == "empty_middle":
        assert per_block.tolist() == [ac.BLOCK_PIXELS, 0, f.NP - 2 * ac.BLOCK_PIXELS]
    if name == "one_per_wave":
        per_wave = np.bincount(np.arange(f.NP)[a] // ac.WAVE, minlength=-(-f.NP // ac.WAVE))
        assert per_wave[:f.NP // ac.WAVE].tolist() == [1] * (f.NP // ac.WAVE) and per_wave.max() == 1
        assert len(np.unique(np.arange(f.NP)[a] % ac.WAVE)) == ac.WAVE
    if name.startswith("pass_") or name == "every_third_pass":
        pas = np.arange(f.NP) // ac.BLOCK
        if name == "every_third_pass":
            assert np.array_equal(a, pas % 3 == 0) and (per_block > 0).all()
        else:
            j = int(name.split("_")[1])
            assert np.array_equal(a, pas - f.block_of() * ac.PER_THREAD == j)
            tail = f.NP - 2 * ac.BLOCK_PIXELS
            assert per_block.tolist() == [ac.BLOCK, ac.BLOCK, max(0, min(ac.BLOCK, tail - j * ac.BLOCK))]
        # whole passes: every wave of a chosen pass is full, every other wave is empty
        assert set(np.unique(a.reshape(-1)[:f.NP // ac.WAVE * ac.WAVE].reshape(-1, ac.WAVE).sum(1)).tolist()) == {0, ac.WAVE}
    if name == "checkerboard":
        img = np.zeros((f.h, f.w), bool)
        img[f.row, f.col] = a
        assert not (img[:, 1:] & img[:, :-1]).any() and not (img[1:] & img[:-1]).any() and img[0, 0]
        assert (per_block > 0).all()
    if name.startswith("random_"):
        pct = int(name.split("_")[1]) / 100.0
        assert abs(a.mean() - pct) < 0.02 and 0 < a.sum() < f.NP
        assert (per_block > 0).all() and (per_block < np.bincount(f.block_of())).all()


@pytest.mark.parametrize("n", COUNTS)
def test_threshold_pairs_are_adjacent_and_the_model_flips(n):
    rng = np.random.RandomState(n % 9973)
    S = ac.log_uniform(rng, -4, 3, (4096, 3)) * F(n)
    rel, floor = 0.05, 0.01
    lo, hi, ok = ac.threshold_pairs(S, n, rel, floor)
    assert ok.all()
    assert np.array_equal(lo.view(np.uint32) + 1, hi.view(np.uint32))
    assert not ac.model_active(S, lo, n, rel, floor).any() and ac.model_active(S, hi, n, rel, floor).all()
    lhs, rhs = am.test_value(S, lo, n, rel, floor)
    exact = int((lhs == rhs).sum())
    print("n = %d: %d of %d stopping members sit at lhs == rhs" % (n, exact, len(S)))
    assert exact >= 16     # the <= of the test is exercised at equality, not only strictly below


@pytest.mark.parametrize("floor", [0.01, 0.0])
@pytest.mark.parametrize("n", COUNTS)
def test_decision_film_holds_every_kind_in_every_block(n, floor):
    NP = FILMS["row_major"].NP
    rel = 0.05
    S, M, kind = ac.decision_film(NP, n, rel, floor)
    assert S.shape == (NP, 3) and M.shape == (NP,) and S.dtype == F and M.dtype == F
    blk = np.arange(NP) // ac.BLOCK_PIXELS
    act = ac.model_active(S, M, n, rel, floor)
    assert not act[kind == 1].any() and act[kind == 2].all()
    assert (kind == 1).sum() == (kind == 2).sum() >= 2048
    for b in range(3):
        assert ((kind == 1) & (blk == b)).any() and ((kind == 2) & (blk == b)).any() and ((kind == 0) & (blk == b)).any()
    # both outcomes among the random and among the special pixels; NaN and inf moments are there
    assert act[kind == 0].any() and not act[kind == 0].all()
    assert act[kind == 3].any() and not act[kind == 3].all()
    assert np.isnan(M).sum() >= 6 and np.isposinf(M).sum() >= 9
    assert not act[np.isnan(M)].any()                                   # a NaN moment2: variance 0
    assert act[np.isposinf(M) & (np.abs(S) < 1e29).all(-1)].all()       # +inf: never stops at a finite right-hand side
    if floor > 0:
        with np.errstate(all="ignore"):
            mu = am.luminance(S) / F(n)
        assert (mu == np.nextafter(F(floor), F(0))).any() or (mu < F(floor)).any()
        near = np.abs(mu.astype(np.float64) - floor) < 1e-6 * floor
        assert (mu[near] < F(floor)).any() and (mu[near] > F(floor)).any()
    else:
        zero = (S == 0).all(-1)
        assert zero.sum() >= 15 and not act[zero & (M == 0)].any()


def test_rel_error_infinite_zero_and_negative():
    NP = FILMS["row_major"].NP
    S, M, _ = ac.decision_film(NP, 4, 0.05, 0.0)
    with np.errstate(all="ignore"):
        mu = am.luminance(S) / F(4)
    a0 = ac.model_active(S, M, 4, np.inf, 0.0)
    # inf * 0 is a NaN: no stop; inf * mu stops whatever the variance
    assert a0[~(mu > 0)].all() and not a0[mu > 0].any() and a0.any() and not a0.all()
    assert not ac.model_active(S, M, 4, np.inf, 0.01).any()
    assert ac.model_active(S, M, 4, 0.0, 0.01).all() and ac.model_active(S, M, 4, -1.0, 0.01).all()


def test_invalid_counts_are_invalid_and_placed_in_their_blocks():
    f = FILMS["row_major"]
    v = ac.invalid_counts(ac.STEP)
    ok = (v >= 0) & (v <= 2.0 ** 24) & (v == np.floor(v))
    assert ok.tolist() == [False, False, False, False, False, True] and v[-1] % ac.STEP != 0
    p, vals = ac.invalid_placements(f, ac.STEP, (6, 6, 6))
    assert len(p) == 18 == len(np.unique(p)) and np.bincount(p // ac.BLOCK_PIXELS).tolist() == [6, 6, 6]
    assert {0, ac.BLOCK_PIXELS - 1, ac.BLOCK_PIXELS, 2 * ac.BLOCK_PIXELS, f.NP - 1} <= set(p.tolist())
    for b in range(3):
        assert np.isnan(vals[p // ac.BLOCK_PIXELS == b]).sum() == 1
    p, vals = ac.invalid_placements(f, ac.STEP, (0, 0, 5))
    assert len(p) == 5 and (p >= 2 * ac.BLOCK_PIXELS).all()


_SAMPLES = {}


def samples(name):
    if name not in _SAMPLES:
        f = FILMS[name]
        _SAMPLES[name] = helpers.oracle_samples(helpers.scene_c1(), f.W, f.H, ac.MAX, tile=f.tile)
    return _SAMPLES[name]


@pytest.mark.parametrize("film", list(FILMS))
def test_forcing_rules_hold_for_every_pixel(film):
    f = FILMS[film]
    smp = samples(film)
    S0, M0 = ac.sums(f.from_samples(smp), ac.N0)
    assert (M0 > 0).mean() > 0.9
    # STOPPED: a true N0-sample sum with moment2 = 0 stops at any rel_error > 0; ACTIVE: M + max(1, M) does not, at REL
    for rel in (ac.REL, 1e-30, 10.0):
        assert not ac.model_active(S0, np.zeros_like(M0), ac.N0, rel, ac.FLOOR).any()
        assert not ac.model_active(S0, np.zeros_like(M0), ac.N0, rel, 0.0).any()
    assert ac.model_active(S0, ac.force_active(M0), ac.N0, ac.REL, ac.FLOOR).all()
    # the sums are the oracle's own at that count
    ref = helpers.oracle_render(helpers.scene_c1(), f.W, f.H, ac.N0, tile=f.tile)[0]
    assert f.from_film(ref)[:, :3].tobytes() == S0.tobytes()
    # craft: classes, counts, and a next round that moment2 registers
    act = ac.pattern(f, "random_50")
    c = ac.craft(f, act, smp, ac.N0, ac.STEP, ac.MAX, seed=3)
    a, m = f.gather(c["accum"]), f.gather(c["moment2"])
    cls = c["cls"]
    assert np.array_equal(cls == ac.ACTIVE, act) and set(np.unique(cls).tolist()) == {ac.DONE, ac.STOPPED, ac.ACTIVE}
    assert (a[cls == ac.DONE, 3] == ac.MAX).all() and (a[cls != ac.DONE, 3] == ac.N0).all()
    assert np.isfinite(c["accum"]).all() and np.isfinite(c["moment2"]).all()
    n = a[:, 3].astype(np.int64)
    model_act, _ = am.decide(a[:, :3], m, n, ac.N0, ac.MAX, ac.REL, ac.FLOOR)
    assert np.array_equal(model_act, act)
    Y2 = sum(am.luminance(am.reject(f.from_film(smp[k]))[0]).astype(np.float64) ** 2 for k in range(ac.N0, ac.MAX))
    grew = c["exp_moment2"] > m
    assert (grew | (Y2 < 2.0 ** -22 * m))[act].all() and grew[act].mean() > 0.9
    assert np.array_equal(c["n_after"], np.where(act, ac.MAX, n))
    # FRESH: active whatever rel_error is
    c = ac.craft(f, act, smp, 0, ac.STEP, ac.STEP, fresh=True, seed=4)
    a, m = f.gather(c["accum"]), f.gather(c["moment2"])
    for rel in (ac.REL, 1e30, np.inf):
        model_act, _ = am.decide(a[:, :3], m, a[:, 3].astype(np.int64), ac.STEP, ac.STEP, rel, ac.FLOOR)
        assert np.array_equal(model_act, act)
