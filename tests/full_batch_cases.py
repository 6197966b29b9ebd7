"""Shared data of tests/test_gpu_full_batch_trace.py (no GPU needed to build it; preconditions: tests/test_full_batch_cases.py).

A production trace launch is k_trace_fast<MODE, DEPTH, LIST, COUNT, SPILL, PEEK, COH>.  PEEK is chosen by the size of the batch: below
agpt_ctx::small_batch_paths (48 Mi paths unless AGPT_SMALL_BATCH_PATHS says otherwise) a wave that finds its queue segment drained
looks at all the frontiers at once, at and above it the wave walks the segments one failing atomic each.  A context created with
AGPT_SMALL_BATCH_PATHS=0 runs the second form on batches of any size, which is what the GPU file does.

The queue of n rays is cut into AGPT_FRONTIERS = 8 segments of seg_len(n) rays, a multiple of 64, and handed out in chunks of 64 from
each segment's frontier (agpt_trace_kernels.h, pump_issue).  What can go wrong there depends on n alone: how many segments hold rays at all,
and whether the last chunk of the last of them is a full one.  COUNTS has every combination (test_full_batch_cases.py checks that)."""
import numpy as np

import ag_pathtracer_amd as ag
import ray_edge_cases as rc
from helpers import scene_bounds

F = np.float32
FRONTIERS = 8      # agpt_wavefront.h: AGPT_FRONTIERS
CHUNK = 64         # rays a wave reserves with one atomic


# ---- the segment arithmetic of k_trace_fast, restated ----------------------------------------------------------------------------
def seg_len(n):
    """rays per segment: an eighth of the queue, rounded up to whole chunks"""
    return ((n + FRONTIERS - 1) // FRONTIERS + CHUNK - 1) & ~(CHUNK - 1)


def segments(n):
    """how many of the eight segments hold at least one of the n rays"""
    return min(FRONTIERS, (n + seg_len(n) - 1) // seg_len(n))


def last_chunk(n):
    """rays in the last chunk of the last non-empty segment (every chunk before it is full)"""
    tail = n - (segments(n) - 1) * seg_len(n)
    return tail % CHUNK or CHUNK


def category(n):
    """one: a single non-empty segment; some: 2 .. 7 of them; partial: all eight, the last chunk short; full: eight full segments"""
    k = segments(n)
    if k == 1:
        return "one"
    if k < FRONTIERS:
        return "some"
    return "full" if n == FRONTIERS * seg_len(n) else "partial"


# ray counts: around one chunk, around eight chunks (the first size with eight segments), around eight segments of eight chunks, one
# large power of two and one large count that is no multiple of 64; 128 adds two full segments with six empty ones behind them, 449
# seven full segments and a single ray in the eighth
COUNTS = [1, 63, 64, 65, 128, 449, 511, 512, 513, 4095, 4096, 4097, 32768, 100000]
N_MAX = max(COUNTS)

SCENES = {"grid1": lambda: rc.grid(1), "grid_long": rc.grid_long}


# ---- rays ---------------------------------------------------------------------------------------------------------------------------
def scrub_rays(desc, n):
    """n rays that miss everything: each starts beyond the upper corner of the scene's bounds on every axis and points further away
    from it on every axis."""
    rng = np.random.RandomState(97)
    lo, hi = scene_bounds(desc)
    ext = hi - lo
    rays = np.zeros(n, ag.RAY_DTYPE)
    rays["o"] = (hi + 1.0 + ext * rng.uniform(0.5, 2.0, (n, 3))).astype(F)
    rays["d"] = rng.uniform(0.1, 1.0, (n, 3)).astype(F)
    rays["tmax"] = rc.FLT_MAX
    return rays


DEEP_LONG_FILM = (32, 24)


def deep_long_list():
    """test_gpu_render.deep_mesh_with_emitter() -- a mesh whose BVH is deeper than the stack entries k_trace_fast keeps in LDS, an emitter
    sphere in front of it, a sphere light and a sky -- plus small tetrahedra between the camera and the mesh to 70 primitives: the
    one scene here that needs LIST and SPILL together, in all three modes."""
    from test_gpu_intersect import deep_mesh
    from test_gpu_render import DEEP_UNIT, deep_mesh_with_emitter
    d, _, depth = deep_mesh_with_emitter()
    assert depth > 23
    d.name = "deep-long-list"
    _, _, scale, x = deep_mesh(DEEP_UNIT)
    s = float(scale[-1])
    rng = np.random.RandomState(64)
    while d.n_prims < 70:
        c = [float(x) * 0.6 + s * rng.uniform(-0.8, 0.8), s * 0.3 + s * rng.uniform(-0.6, 0.6), s * rng.uniform(0.2, 1.2)]
        v, idx = rc._tetra(c, s * 0.05)
        d.add_mesh(v, None, None, idx, 0, 1)
    return d


_CACHE = {}


def edge_count_rays(scn):
    """(scene, rays, oracle closest-hit records, oracle any-hit records) for SCENES[scn]: N_MAX rays of ray_edge_cases.aimed -- hits
    on triangles, vertices and spheres, a quarter with a short tmax, three in ten aimed above the scene -- ordered so that every
    prefix holds at least as many hits as misses: the oracle's hits and misses alternate, starting with a hit, until the misses run
    out.  A test takes the first n rays and the first n records.  Built once per process; the arrays are read-only."""
    if scn not in _CACHE:
        desc = SCENES[scn]()
        rays = rc.aimed(desc, N_MAX, seed=41)
        o = rc.oracle_scene(desc)
        hit = o.intersect(rays)[0]["hit"] == 1
        h, m = np.nonzero(hit)[0], np.nonzero(~hit)[0]
        assert len(h) >= len(m)
        order = np.empty(N_MAX, np.int64)
        order[0:2 * len(m):2] = h[:len(m)]
        order[1:2 * len(m):2] = m
        order[2 * len(m):] = h[len(m):]
        rays = rays[order]
        closest, any_ = o.intersect(rays)[0], o.intersect(rays, any_hit=True)[0]
        for a in (rays, closest, any_):
            a.setflags(write=False)
        _CACHE[scn] = (desc, rays, closest, any_)
    return _CACHE[scn]
