"""Preconditions of tests/test_gpu_full_batch_trace.py, on the CPU with the oracle alone: the ray counts of full_batch_cases.py reach
every shape of the work queue, the scrub rays miss everything, and every prefix of the edge-count rays hits often enough that a ray
the kernel skipped cannot hide among the misses.  Each test prints its figures (pytest -s shows them)."""
import numpy as np
import pytest

import full_batch_cases as fb
import ray_edge_cases as rc

REQUIRED = [1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 32768, 100000]


def test_segment_arithmetic_against_a_walk_over_the_queue():
    """seg_len, segments and last_chunk against the chunks a walk over the eight segments hands out, as pump_issue does: segment k is
    [k * seg_len, min((k + 1) * seg_len, n)), empty when it begins at or past n, and is taken 64 rays at a time."""
    for n in sorted(set(fb.COUNTS) | set(range(1, 1200)) | {32767, 32769, 99999, 100001}):
        L = fb.seg_len(n)
        assert L % fb.CHUNK == 0 and fb.FRONTIERS * L >= n and (L == fb.CHUNK or fb.FRONTIERS * (L - fb.CHUNK) < n)
        chunks, live = [], 0
        for k in range(fb.FRONTIERS):
            begin, end = k * L, min((k + 1) * L, n)
            if begin < end:
                live += 1
                chunks += [min(fb.CHUNK, end - b) for b in range(begin, end, fb.CHUNK)]
        assert sum(chunks) == n
        assert live == fb.segments(n), n
        assert chunks[-1] == fb.last_chunk(n), n
        assert all(c == fb.CHUNK for c in chunks[:-1]), n


def test_counts_cover_every_shape_of_the_queue():
    assert set(REQUIRED) <= set(fb.COUNTS)
    assert fb.COUNTS == sorted(set(fb.COUNTS)) and fb.N_MAX == fb.COUNTS[-1]
    by = {}
    for n in fb.COUNTS:
        by.setdefault(fb.category(n), []).append(n)
        print("n = %6d: seg_len %5d, %d non-empty segments, last chunk %2d -> %s" % (n, fb.seg_len(n), fb.segments(n), fb.last_chunk(n), fb.category(n)))
    assert set(by) == {"one", "some", "partial", "full"}, by
    # a single ray, a single chunk one short, full and -- two segments -- one over
    assert {1, 63, 64} <= set(by["one"]) and 65 in by["some"]
    # partial last chunks of 1 and of 63 rays, and one that is neither, behind eight segments
    assert {1, 63} <= {fb.last_chunk(n) for n in by["partial"]} and any(1 < fb.last_chunk(n) < 63 for n in by["partial"])
    # a short last chunk also where trailing segments are empty
    assert any(fb.last_chunk(n) < fb.CHUNK for n in by["some"]) and any(fb.last_chunk(n) == fb.CHUNK for n in by["some"])
    # eight full segments of one chunk and of many
    assert any(fb.seg_len(n) == fb.CHUNK for n in by["full"]) and any(fb.seg_len(n) > fb.CHUNK for n in by["full"])


@pytest.mark.parametrize("scn", list(fb.SCENES))
def test_scrub_rays_miss_everything(scn):
    desc = fb.SCENES[scn]()
    rays = fb.scrub_rays(desc, fb.N_MAX)
    assert len(rays) == fb.N_MAX and np.isfinite(rays["o"]).all() and np.isfinite(rays["d"]).all()
    o = rc.oracle_scene(desc)
    assert not o.intersect(rays)[0]["hit"].any()
    assert not o.intersect(rays, any_hit=True)[0]["hit"].any()


@pytest.mark.parametrize("scn", list(fb.SCENES))
def test_every_prefix_of_the_edge_count_rays_hits(scn):
    """At least half of the first n rays hit, closest and any-hit, for every n of COUNTS; beyond a single ray every prefix also holds a
    miss, and the any-hit answers are those of the closest-hit query (the scenes have no cut-outs)."""
    desc, rays, closest, any_ = fb.edge_count_rays(scn)
    assert len(rays) == len(closest) == len(any_) == fb.N_MAX
    assert desc.n_prims > 64 if scn == "grid_long" else desc.n_prims <= 64
    o = rc.oracle_scene(desc)
    assert o.intersect(rays)[0].tobytes() == closest.tobytes()            # the records belong to the rays in this order
    assert np.array_equal(any_["hit"], closest["hit"])
    assert not np.isnan(closest["t"][closest["hit"] == 1]).any()
    for n in fb.COUNTS:
        hits = int(closest["hit"][:n].sum())
        print("%s, first %6d rays: %6d hits, %6d misses" % (scn, n, hits, n - hits))
        assert 2 * hits >= n, (scn, n, hits)
        assert n == 1 or hits < n, (scn, n)
    # the records are not all alike: triangles of more than one primitive, spheres, and rays cut short by tmax
    m = closest["hit"] == 1
    assert len(np.unique(closest["prim"][m])) >= 3 and (closest["tri"][m] < 0).any() and (closest["tri"][m] >= 0).any()
    assert (rays["tmax"] < rc.FLT_MAX).sum() >= 0.1 * fb.N_MAX


def test_deep_long_list_shows_its_tetrahedra_and_its_deep_mesh():
    """The LIST x SPILL scene: more than 64 primitives, a BVH deeper than the 23 entries of the LDS stack, and a film on which the
    camera sees the deep mesh, some of the added tetrahedra and the emitter sphere."""
    import ag_pathtracer_amd as ag
    import temporal_model as tm
    from test_gpu_intersect import deep_mesh
    from test_gpu_render import DEEP_UNIT
    d = fb.deep_long_list()
    v, idx, _, _ = deep_mesh(DEEP_UNIT)
    assert d.n_prims == 70 and ag.bvh_build(v, idx, 1)[2] > 23
    W, H = fb.DEEP_LONG_FILM
    cam = ag.camera_vectors(d.camera)
    rays = np.zeros(W * H, ag.RAY_DTYPE)
    rays["o"] = tm.camera(cam)["origin"]
    rays["d"] = tm.feature_directions(cam, W, H).reshape(-1, 3)
    rays["tmax"] = rc.FLT_MAX
    hits = rc.oracle_scene(d).intersect(rays)[0]
    m = hits["hit"] == 1
    prims = hits["prim"][m]
    first_tetra = 3      # the list: the deep mesh, the light's sphere, the emitter sphere, then the tetrahedra
    assert [op[0] for op in d.ops if op[0] in ("mesh", "sphere", "area_light", "plane")][:4] == ["mesh", "area_light", "area_light", "mesh"]
    print("deep-long-list %dx%d: %d pixel centres on the deep mesh, %d on %d tetrahedra, %d on spheres, %d misses"
          % (W, H, (prims == 0).sum(), (prims >= first_tetra).sum(), len(np.unique(prims[prims >= first_tetra])), (hits["tri"][m] < 0).sum(), (~m).sum()))
    assert (prims == 0).sum() >= 20 and (prims >= first_tetra).sum() >= 20 and len(np.unique(prims[prims >= first_tetra])) >= 5
    assert (hits["tri"][m] < 0).sum() >= 3
