"""GPU parity at the numeric edges of the traversal arithmetic: the ray classes of ray_edge_cases.py (preconditions:
test_ray_edges.py) through agpt_intersect_batch / agpt_intersect_device, closest and any-hit, production and counters kernels,
against the oracle, bit for bit (test_gpu_intersect.check_closest)."""
import numpy as np
import pytest

import ag_pathtracer_amd as ag
import ray_edge_cases as rc
from helpers import gpu_scene, oracle_scene
from test_gpu_intersect import check_closest
from test_ray_edges import scaled_relation_holds

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cls,scn", rc.CASE_IDS)
def test_class_against_oracle(cls, scn):
    """Every class on grid (leaves of 1 and of up to 4 triangles; the short-list kernel with its root-box prefilter) and on
    grid_long (k_candidates + k_trace_fast<LIST>)."""
    desc, rays = rc.case(cls, scn)
    assert check_closest(desc, rays) > 0


@pytest.mark.parametrize("scn", ["grid1", "grid_long"])
def test_classes_through_the_device_entry_point(scn):
    """agpt_intersect_device on all classes at once: the host entry point's records, closest and any-hit, and the oracle's."""
    rays = np.concatenate([rc.case(cls, scn)[1] for cls in rc.CLASSES])
    desc = rc.case("threshold", scn)[0]
    g = gpu_scene(desc)
    ctx = g.ctx
    host_hits, _ = g.Intersect(rays)
    host_occ, _ = g.IntersectP(rays)
    rp = ctx.alloc(rays.nbytes)
    hp = ctx.alloc(len(rays) * ag.HIT_DTYPE.itemsize)
    ctx.upload(rp, rays)
    g.intersect_device(rp, len(rays), hp)
    dev_hits = ctx.download(hp, (len(rays),), ag.HIT_DTYPE)
    g.intersect_device(rp, len(rays), hp, any_hit=True)
    dev_occ = ctx.download(hp, (len(rays),), ag.HIT_DTYPE)
    g.intersect_device(rp, len(rays), hp, counters=True)
    dev_cnt = ctx.download(hp, (len(rays),), ag.HIT_DTYPE)
    ctx.free(rp)
    ctx.free(hp)
    g.close()
    o = oracle_scene(desc)
    oh, _ = o.intersect(rays)
    op_, _ = o.intersect(rays, any_hit=True)
    assert dev_hits.tobytes() == host_hits.tobytes() and dev_cnt.tobytes() == host_hits.tobytes()
    assert np.array_equal(dev_occ["hit"], host_occ["hit"]) and np.array_equal(dev_occ["hit"], op_["hit"])
    m = oh["hit"] == 1
    assert np.array_equal(dev_hits["hit"], oh["hit"]) and dev_hits[m].tobytes() == oh[m].tobytes()


@pytest.mark.parametrize("cls", rc.FAR16_CLASSES)
def test_far16_top_level_walk_drops_no_candidate(cls):
    """Boxes beyond the fp16 range (infinite packed planes), below its smallest normal and ordinary ones in one top-level tree: a
    candidate the fp16 walk dropped would be a hit of the oracle's that the GPU misses."""
    desc, rays = rc.case(cls, "far16")
    assert check_closest(desc, rays) > 0


@pytest.mark.parametrize("scale_d", [False, True])
@pytest.mark.parametrize("k", rc.SCALED_K)
def test_scaled(k, scale_d):
    """Oracle parity at every k; at k = +-20 also the GPU's own records against its records at k = 0 (same bits, t * 2^k), under
    the condition test_ray_edges.test_scaled_oracle_records establishes for the oracle."""
    desc, rays = rc.scaled(k, scale_d)
    assert check_closest(desc, rays) > 0
    if abs(k) == 20:
        g = gpu_scene(desc)
        hk, _ = g.Intersect(rays)
        g.close()
        d0, r0 = rc.scaled(0, scale_d)
        g = gpu_scene(d0)
        h0, _ = g.Intersect(r0)
        g.close()
        assert scaled_relation_holds(h0, hk, k)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["tiny-floor", "far-origin-y", "spike"])
def test_domain_edge(which):
    """The two measured limits of the Markstein divide's domain, |a| <= 2^-107 and an overflowing quotient, on rays the oracle
    still hits."""
    name, desc, rays = rc.domain_edge()[which]
    assert check_closest(desc, rays) > 0


def test_refit_moves_a_mesh_out_of_the_divide_s_domain_and_back():
    """The condition on the scene's boxes follows a committed mesh through agpt_scene_update_mesh (host arrays) and
    agpt_scene_update_mesh_device: the height field is committed with ordinary coordinates, refitted to the spike of domain_edge
    (one vertex at y = 2^90) and back.  The refitted tree keeps the topology built for the ordinary mesh, so only what no topology
    changes is compared with the oracle's scene of the spike: the hit flag, closest and any-hit, and the bits of t on hits.
    (Oracle scenes of the spike with leaves of 1 and of 4 triangles agree on all of it for these rays: checked below.)"""
    _, spike, rays = rc.domain_edge()[2]
    v_spike = spike.ops[1][1]
    v0, idx = rc.grid_heightfield()
    plain = ag.SceneDesc("height-field")
    plain.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
    plain.add_mesh(v0, None, None, idx, 0, 1)
    oh, _ = oracle_scene(spike).intersect(rays)
    op_, _ = oracle_scene(spike).intersect(rays, any_hit=True)
    other = ag.SceneDesc("spike-leaf4")
    other.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
    other.add_mesh(v_spike, None, None, idx, 0, 4)
    oh4, _ = oracle_scene(other).intersect(rays)
    m = oh["hit"] == 1
    assert np.array_equal(oh4["hit"], oh["hit"]) and oh4["t"][m].tobytes() == oh["t"][m].tobytes() and m.sum() > 500
    g = gpu_scene(plain)
    before, _ = g.Intersect(rays)

    def check_spike():
        for counters in (False, True):
            gh, _ = g.Intersect(rays, counters=counters)
            gp, _ = g.IntersectP(rays, counters=counters)
            assert np.array_equal(gh["hit"], oh["hit"]) and gh["t"][m].tobytes() == oh["t"][m].tobytes()
            assert np.array_equal(gp["hit"], op_["hit"])

    g.update_mesh(0, v_spike, None, "refit")
    check_spike()
    g.update_mesh(0, v0, None, "refit")
    assert g.Intersect(rays)[0].tobytes() == before.tobytes()
    ctx = g.ctx
    vp = ctx.alloc(v_spike.nbytes)
    ctx.upload(vp, v_spike)
    g.update_mesh_device(0, vp, len(v_spike), mode="refit")
    check_spike()
    ctx.upload(vp, v0)
    g.update_mesh_device(0, vp, len(v0), mode="refit")
    assert g.Intersect(rays)[0].tobytes() == before.tobytes()
    ctx.free(vp)
    g.close()
