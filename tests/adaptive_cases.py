"""Crafted film states for agpt_render_adaptive's decision (k_adaptive_select) and active list (k_adaptive_compact): pure numpy.

The call takes the film's state as input -- accum with the count in w, and moment2 --, so a test uploads any state and reads the
decision back: a pixel was active in the first round exactly when its count grew.  This module builds such states and what the
contract of include/agpt.h expects of them, from per-sample radiance the caller supplies (the CPU oracle's) and the fp32 model of
tests/adaptive_model.py.  Nothing here looks at what the kernels compute.

Layout.  The select / compact passes walk the tile in the local pixel order p of pixel_of (agpt_wavefront.h): 8x8 blocks when the
region's width and rows are multiples of 8, row-major otherwise.  A select / compact block covers BLOCK_PIXELS consecutive p, in
PER_THREAD passes of BLOCK pixels, each pass BLOCK / WAVE waves.  A Film maps p to its element of the accumulator buffer."""
import numpy as np

import adaptive_model as am

F = np.float32
WAVE = 64
BLOCK = 256                        # AGPT_BLOCK
PER_THREAD = 16                    # AGPT_ADAPT_PER_THREAD
BLOCK_PIXELS = BLOCK * PER_THREAD  # AGPT_ADAPT_BLOCK_PIXELS

DONE, STOPPED, ACTIVE, FRESH = 0, 1, 2, 3


# ---- the local pixel order ------------------------------------------------------------------------------------------------------
def is_tiled(w, rows):
    return w % 8 == 0 and rows % 8 == 0


def pixel_rc(w, rows):
    """(row, col) of every local pixel p = 0 .. w * rows - 1 of a region w wide and rows high: pixel_of's two layouts"""
    p = np.arange(w * rows, dtype=np.int64)
    if is_tiled(w, rows):
        blk, inner, per_row = p >> 6, p & 63, w >> 3
        brow = blk // per_row
        return brow * 8 + (inner >> 3), (blk - brow * per_row) * 8 + (inner & 7)
    return p // w, p % w


def local_index(w, rows):
    """[rows, w] -> p: the inverse of pixel_rc, written out on its own (not by scattering pixel_rc)"""
    row, col = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    if is_tiled(w, rows):
        return ((row >> 3) * (w >> 3) + (col >> 3)) * 64 + (row & 7) * 8 + (col & 7)
    return row * w + col


class Film:
    """A tile (x0, y0, w, h) of a W x H film in an accumulator buffer of buf_rows x pitch elements whose first row is the film's row
    row0 from the top (accum_pitch, accum_row0 of agpt_render_params).  The default is the whole film in a buffer of its own size."""

    def __init__(self, W, H, tile=None, pitch=None, row0=0, buf_rows=None):
        self.W, self.H = W, H
        self.tile = (0, 0, W, H) if tile is None else tuple(tile)
        self.x0, self.y0, self.w, self.h = self.tile
        self.pitch = W if pitch is None else pitch
        self.row0 = row0
        self.buf_rows = H - row0 if buf_rows is None else buf_rows
        self.NP = self.w * self.h
        self.n_blocks = -(-self.NP // BLOCK_PIXELS)
        self.tiled = is_tiled(self.w, self.h)
        self.row, self.col = pixel_rc(self.w, self.h)
        # film pixel (x, y) with y up, the film's row from the top, and the buffer element of every p
        self.x = self.x0 + self.col
        self.y = self.y0 + self.row
        self.top = H - 1 - self.y
        self.brow = self.top - row0
        self.bcol = self.x
        assert self.pitch >= self.x0 + self.w and self.brow.min() >= 0 and self.brow.max() < self.buf_rows

    @property
    def shape(self):
        return (self.buf_rows, self.pitch)

    def render_kw(self):
        """the keyword arguments of PathTracer.render_adaptive that place this tile"""
        return dict(tile=self.tile, accum_pitch=self.pitch, accum_row0=self.row0)

    def from_film(self, a):
        """a[H, W, ...] (the oracle's layout, row 0 = top) -> its values at the tile's pixels, [NP, ...] in p order"""
        return a[self.top, self.x]

    def from_samples(self, a):
        """a[n, H, W, ...] (per-sample radiance in the oracle's layout) -> [n, NP, ...]"""
        return a[:, self.top, self.x]

    def gather(self, buf):
        """buf[buf_rows, pitch, ...] -> [NP, ...] in p order"""
        return buf[self.brow, self.bcol]

    def scatter(self, buf, values, sel=None):
        if sel is None:
            buf[self.brow, self.bcol] = values
        else:
            buf[self.brow[sel], self.bcol[sel]] = values

    def tile_mask(self):
        m = np.zeros(self.shape, bool)
        m[self.brow, self.bcol] = True
        return m

    def block_of(self):
        return np.arange(self.NP) // BLOCK_PIXELS


# ---- activity patterns over p ---------------------------------------------------------------------------------------------------
PATTERNS = ("all", "none", "first", "last", "last_block", "empty_middle", "one_per_wave", "pass_0", "pass_1", "pass_15",
            "every_third_pass", "checkerboard", "random_1", "random_50", "random_99")


def pattern(film, name):
    """bool[NP]: the pixels the pattern makes active"""
    NP = film.NP
    p = np.arange(NP)
    blk, pas, wav = p // BLOCK_PIXELS, p // BLOCK, p // WAVE
    last = film.n_blocks - 1
    if name == "all":
        return np.ones(NP, bool)
    if name == "none":
        return np.zeros(NP, bool)
    if name == "first":
        return p == 0
    if name == "last":
        return p == NP - 1
    if name == "last_block":
        return blk == last
    if name == "empty_middle":
        assert film.n_blocks >= 3
        return blk != 1
    if name == "one_per_wave":
        return p % WAVE == (wav * 37 + 5) % WAVE      # the lane moves from wave to wave; 37 is odd: every lane takes a turn
    if name.startswith("pass_"):                      # pass j of every block only: bit j of the mask words
        return pas % PER_THREAD == int(name.split("_")[1])
    if name == "every_third_pass":
        return pas % 3 == 0
    if name == "checkerboard":
        return (film.row + film.col) % 2 == 0
    if name.startswith("random_"):
        pct = int(name.split("_")[1])
        rng = np.random.RandomState(1000 + pct)
        a = rng.uniform(size=NP) < pct / 100.0
        # neither degenerate nor blind to the ends: the first pixel follows the majority, the last one the minority
        a[0], a[-1] = pct >= 50, pct < 50
        return a
    raise KeyError(name)


def pattern_size(film, name):
    """the size the pattern is meant to have, counted another way than pattern() builds it (None: random, checked by its density)"""
    NP, nb = film.NP, film.n_blocks
    tail = NP - (nb - 1) * BLOCK_PIXELS
    n_pass, n_wave = -(-NP // BLOCK), -(-NP // WAVE)

    def passes(k):   # pixels of pass k
        return max(0, min(BLOCK, NP - k * BLOCK))

    if name == "all":
        return NP
    if name == "none":
        return 0
    if name in ("first", "last"):
        return 1
    if name == "last_block":
        return tail
    if name == "empty_middle":
        return NP - BLOCK_PIXELS
    if name == "one_per_wave":
        return sum(1 for k in range(n_wave) if k * WAVE + (k * 37 + 5) % WAVE < NP)
    if name.startswith("pass_"):
        return sum(passes(b * PER_THREAD + int(name.split("_")[1])) for b in range(nb))
    if name == "every_third_pass":
        return sum(passes(k) for k in range(0, n_pass, 3))
    if name == "checkerboard":
        return sum((film.w + (r + 1) % 2) // 2 for r in range(film.h))
    return None


def random_finite(rng, shape):
    """uniformly random fp32 bit patterns without inf / NaN"""
    b = rng.randint(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    b[(b & np.uint32(0x7F800000)) == np.uint32(0x7F800000)] &= np.uint32(0xFF7FFFFF)
    return b.view(F)


def sums(samples, n):
    """(S[..., 3], M[...]) after samples [0, n) of every pixel under the model: fp32, in sample order, the NaN / inf reject applied"""
    shape = samples.shape[1:-1]
    S, M = np.zeros(shape + (3,), F), np.zeros(shape, F)
    for k in range(n):
        clr, _ = am.reject(samples[k])
        S = S + clr
        Y = am.luminance(clr)
        M = M + Y * Y
    return S, M


def force_active(M):
    """the moment2 that keeps a pixel with second moment M active at a small rel_error: M + max(1, M) in fp32.  The variance is
    then at least about max(1, M) / n, and one more Y * Y is not absorbed (the ulp of the result is at most that of 2 M)."""
    M = np.asarray(M, F)
    return M + np.maximum(F(1), M)


def craft(film, active, samples, n0, step, max_spp, fresh=False, seed=0):
    """The buffers to upload for one single-round call with min_spp <= n0, max_spp = n0 + step (fresh: min = step = max, n0 = 0), and
    what the contract expects after it.  active: bool[NP].  samples[>= n0 + step, H, W, 3]: per-sample radiance of the film.
    Inactive tile pixels are DONE or STOPPED at random; buffer elements outside the tile hold random finite bytes.
    -> dict(accum, moment2 (to upload), cls[NP], exp_moment2[NP] (the model's, for the active pixels), n_after[NP])"""
    rng = np.random.RandomState(seed)
    NP = film.NP
    assert max_spp == n0 + step and (n0 == 0) == bool(fresh)
    acc = random_finite(rng, film.shape + (4,)).copy()
    m2 = random_finite(rng, film.shape).copy()
    cls = np.where(rng.uniform(size=NP) < 0.5, DONE, STOPPED)
    if fresh:
        cls[:] = DONE     # with min = max no count lies in [min, max): nothing can be STOPPED
    cls[active] = FRESH if fresh else ACTIVE
    S0, M0 = sums(film.from_samples(samples), n0)
    a = film.gather(acc)
    m = film.gather(m2)
    a[cls == DONE, 3] = max_spp
    for c in (STOPPED, ACTIVE, FRESH):
        sel = cls == c
        a[sel, :3] = S0[sel]
        a[sel, 3] = n0
    m[cls == STOPPED] = 0
    m[cls == ACTIVE] = force_active(M0[cls == ACTIVE])
    m[cls == FRESH] = 0
    film.scatter(acc, a)
    film.scatter(m2, m)
    # the model's next round for the active pixels
    S1, M1 = S0.copy(), m.copy()
    for k in range(n0, n0 + step):
        clr, _ = am.reject(film.from_film(samples[k]))
        S1 = S1 + clr
        Y = am.luminance(clr)
        M1 = M1 + Y * Y
    n_after = np.where(active, n0 + step, a[:, 3]).astype(np.int64)
    return dict(accum=acc, moment2=m2, cls=cls, exp_rgb=S1, exp_moment2=M1, n_after=n_after)


# ---- the stop test at its threshold -----------------------------------------------------------------------------------------------
def model_active(S, M, n, rel_error, abs_floor):
    """the model's decision for tested pixels (min_spp <= n < max_spp): active = not stop"""
    n = np.broadcast_to(np.asarray(n, np.int64), np.shape(M))
    act, _ = am.decide(np.asarray(S, F), np.asarray(M, F), n, 2, 1 << 30, rel_error, abs_floor)
    return act


def bits_to_f(b):
    return np.asarray(b, np.uint32).view(F)


def threshold_pairs(S, n, rel_error, abs_floor):
    """For every S[k] (rgb), bisect the fp32 bit pattern of moment2 in [+0, +inf] under the model: -> (M_stop, M_active), adjacent
    floats, the lower one stopping and the upper one active.  ok[k] is False where the model does not flip between +0 and +inf
    (a non-finite or NaN right-hand side) -- those S have no threshold."""
    S = np.asarray(S, F)
    lo = np.zeros(len(S), np.uint32)
    hi = np.full(len(S), 0x7F800000, np.uint32)
    ok = ~model_active(S, bits_to_f(lo), n, rel_error, abs_floor) & model_active(S, bits_to_f(hi), n, rel_error, abs_floor)
    while True:
        open_ = hi - lo > 1
        if not open_.any():
            break
        mid = lo + (hi - lo) // 2
        act = model_active(S, bits_to_f(mid), n, rel_error, abs_floor)
        hi = np.where(open_ & act, mid, hi)
        lo = np.where(open_ & ~act, mid, lo)
    return bits_to_f(lo), bits_to_f(hi), ok


def log_uniform(rng, lo_exp, hi_exp, shape):
    return (10.0 ** rng.uniform(lo_exp, hi_exp, size=shape)).astype(F)


def floor_sums(n, abs_floor):
    """grey sums S whose mean luminance mu lies just below, at (where fp32 has such a sum) and just above abs_floor, under the model"""
    if not abs_floor > 0:
        return np.zeros((0, 3), F)
    g0 = F(abs_floor) * F(n)
    cand = (g0.view(np.uint32).astype(np.int64) + np.arange(-64, 65)).astype(np.uint32).view(F)
    S = np.stack([cand] * 3, -1)
    with np.errstate(all="ignore"):
        mu = am.luminance(S) / F(n)
    below, above, at = np.nonzero(mu < F(abs_floor))[0], np.nonzero(mu > F(abs_floor))[0], np.nonzero(mu == F(abs_floor))[0]
    assert len(below) and len(above)
    pick = [below[-1], below[-2], above[0], above[1]] + list(at[:2])
    return S[pick]


def decision_film(NP, n, rel_error, abs_floor, seed=0, n_pairs=2048):
    """(S[NP, 3], M[NP], kind[NP]) for one decision call at count n: threshold pairs (kind 1: stopping member, 2: active member),
    special values (kind 3) and random log-uniform (S, M) (kind 0), shuffled over the tile so that every block holds some of each."""
    rng = np.random.RandomState((seed + 7919 * n) % (1 << 32))
    S_list, M_list, K_list = [], [], []

    def add(S, M, kind):
        S = np.asarray(S, F).reshape(-1, 3)
        M = np.asarray(M, F).reshape(-1)
        assert len(S) == len(M)
        S_list.append(S); M_list.append(M); K_list.append(np.full(len(M), kind, np.int8))

    # threshold pairs on random sums (a few with a negative channel, a few dark ones below the floor), and on the floor's neighbours
    Sp = log_uniform(rng, -4, 3, (n_pairs, 3)) * F(n)
    Sp[::17, rng.randint(3)] *= F(-1)
    Sp[5::23] *= F(1e-4)
    Sp = np.concatenate([Sp, floor_sums(n, abs_floor)])
    lo, hi, ok = threshold_pairs(Sp, n, rel_error, abs_floor)
    add(Sp[ok], lo[ok], 1)
    add(Sp[ok], hi[ok], 2)
    # special values
    big = np.array([[3.0, 2.0, 1.0]], F) * F(n)
    inf, nan, tiny = F(np.inf), F(np.nan), np.array(1, np.uint32).view(F)
    for S, M in [
        (big, F(1e-3)),                 # the clamp: moment2 / n < mu * mu, variance 0
        (big, F(0)),
        (big, F(-5.0)),                 # (a negative moment2 is garbage, but the clamp covers it)
        (big, inf), (big, nan), (big, -inf),
        (np.zeros((1, 3), F), F(0)),    # mu = 0: with abs_floor = 0 the test is 0 <= 0
        (np.zeros((1, 3), F), tiny),    # the smallest positive moment2
        (np.zeros((1, 3), F), F(1e-30)),
        (np.zeros((1, 3), F), inf), (np.zeros((1, 3), F), nan),
        (np.full((1, 3), -0.0, F), F(0)),
        (-big, F(1.0)),                 # mu < 0: the floor decides
        (np.full((1, 3), 1e30, F), F(1e20)),   # mu * mu overflows: -inf under the clamp
        (np.full((1, 3), 1e30, F), inf),       # inf - inf: a NaN under the clamp
        (np.full((1, 3), 3e38, F), F(1.0)),    # the luminance sum itself near FLT_MAX
    ]:
        for _ in range(3):              # three copies: the shuffle spreads them over the blocks
            add(S, M, 3)
    for S_ in floor_sums(n, abs_floor):
        add(S_[None], F(0), 3)
        add(S_[None], inf, 3)
    have = sum(len(m) for m in M_list)
    assert have < NP, (have, NP)
    rest = NP - have
    add(log_uniform(rng, -6, 3, (rest, 3)) * F(n), log_uniform(rng, -12, 8, rest) * F(n), 0)
    S, M, K = np.concatenate(S_list), np.concatenate(M_list), np.concatenate(K_list)
    perm = rng.permutation(NP)
    return S[perm], M[perm], K[perm]


# ---- counts the call must refuse --------------------------------------------------------------------------------------------------
def invalid_counts(step):
    """counts that are not an integer multiple of step_spp in [0, 2^24]; the last is an integer off the step grid (step >= 2)"""
    assert step >= 2
    return np.array([-1.0, 0.5, 2.0 ** 24 + 2.0, np.nan, np.inf, 3 * step + 1], F)


def invalid_placements(film, step, per_block):
    """(p, value) of the planted pixels: per_block[b] invalid counts in block b (first / middle / last ...), cycling through
    invalid_counts, at the block's first pixel, its last one and in between"""
    vals = invalid_counts(step)
    ps, vs, k = [], [], 0
    for b, cnt in enumerate(per_block):
        lo, hi = b * BLOCK_PIXELS, min(film.NP, (b + 1) * BLOCK_PIXELS)
        for p in np.unique(np.linspace(lo, hi - 1, cnt).astype(np.int64)) if cnt else []:
            ps.append(int(p)); vs.append(vals[k % len(vals)]); k += 1
    return np.array(ps, np.int64), np.array(vs, F)


# ---- the films and the parameters of the single-round calls the GPU tests make ----------------------------------------------------
def films():
    """name -> Film.  row_major: three blocks, the last one of 258 pixels (pass 0 and two pixels of pass 1).  tiled: 8x8 order, three
    blocks, the last one of four passes.  tile: a row-major tile inside a larger film, in a buffer with accum_pitch > w that starts
    at the film's fourth row."""
    return {"row_major": Film(130, 65), "tiled": Film(128, 72),
            "tile": Film(120, 100, tile=(12, 9, 100, 85), pitch=128, row0=4, buf_rows=90)}


N0, STEP, MAX = 4, 4, 8      # ACTIVE and STOPPED pixels hold N0 samples; min_spp = N0, max_spp = N0 + STEP: one round
REL, FLOOR = 1e-3, 0.01
