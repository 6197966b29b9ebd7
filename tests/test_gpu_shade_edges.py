"""GPU parity on the rarely-taken branches of surface and light sampling: the cases of shade_edge_cases.py (preconditions:
test_shade_edges.py) through agpt_li_batch against the oracle's oracle_li in correctly rounded trig -- radiance bit for bit (NaN
matching NaN by class, as test_refpin.py compares), the stream state after the path, the ray and sample totals -- at depth 1 and
depth 5; their first hits through agpt_intersect_batch; the same after the mesh's records were rebuilt on the GPU (refit,
transform); one class inside a 70-primitive scene; and the FAST arithmetic at the tolerance the port is judged at."""
import numpy as np
import pytest

import ag_pathtracer_amd as ag
import shade_edge_cases as sc
from helpers import bits, close_fraction, gpu_scene, oracle_scene

pytestmark = pytest.mark.gpu
NAMES = sc.case_names()
MESH_NAMES = [n for n in NAMES if sc.cases()[n].meshes and not n.endswith("/long")]


def same(got, want):
    """bit-identical float arrays, NaN matching NaN by class"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def check_li(g, rays, states, depth, ref, what):
    want, after, total, _ = ref
    got, got_after, st = ag.PathTracer(depth).Li(g, rays, states)
    ok = same(got, want).all(1)
    assert ok.all(), "%s depth %d: %d of %d rays differ, first %s" % (what, depth, (~ok).sum(), len(ok), np.nonzero(~ok)[0][:8])
    assert np.array_equal(got_after, after), (what, depth)
    assert st.rays == total and st.samples == len(rays), (what, depth, st.rays, total)
    return got


@pytest.mark.parametrize("depth", sc.DEPTHS)
@pytest.mark.parametrize("name", NAMES)
def test_li_matches_oracle(name, depth):
    """every case (flat_uv/long: the candidates path and k_trace_fast<LIST> feed the same shading) in the exact arithmetic"""
    c = sc.cases()[name]
    g = gpu_scene(c.desc)
    try:
        check_li(g, c.rays, c.states, depth, sc.reference(name, depth), name)
    finally:
        g.close()


@pytest.mark.parametrize("name", NAMES)
def test_first_hits_match_oracle(name):
    """agpt_intersect_batch on the same rays: the hit records of the pole, zero-area and every other ray"""
    c = sc.cases()[name]
    g = gpu_scene(c.desc)
    gh, _ = g.Intersect(c.rays)
    g.close()
    oh, _ = oracle_scene(c.desc).intersect(c.rays)
    assert np.array_equal(gh["hit"], oh["hit"]) and oh["hit"].sum() >= 0.5 * len(oh)
    m = oh["hit"] == 1
    for field in ("t", "prim", "tri", "b1", "b2"):
        assert gh[field][m].tobytes() == oh[field][m].tobytes(), (name, field)


@pytest.mark.parametrize("name", MESH_NAMES)
def test_records_rebuilt_on_the_gpu(name):
    """k_update_tris and triangle_frame's degenerate branches on the device: after update_mesh(..., "refit") with the arrays the
    mesh was committed with, Li is what it was; after transform_mesh by a translation, Li is the oracle's on a fresh scene of that
    pose with the ray origins moved along."""
    c = sc.cases()[name]
    meshes = [op for op in c.desc.ops if op[0] == "mesh"]
    g = gpu_scene(c.desc)
    try:
        for prim in c.meshes:
            g.update_mesh(prim, meshes[prim][1], meshes[prim][2], "refit")
        check_li(g, c.rays, c.states, 5, sc.reference(name, 5), name + " refitted")
        for prim in c.meshes:
            g.transform_mesh(prim, sc.SHIFT, "refit")
        desc, rays = sc.moved(c)
        ref = sc.oracle_li(desc, rays, c.states, 5)
        got = check_li(g, rays, c.states, 5, ref, name + " moved")
        assert (got != 0).any(1).mean() >= 0.25
    finally:
        g.close()


def test_fast_arithmetic_on_every_class():
    """FAST against the exact GPU result (bit-identical to the oracle, test_li_matches_oracle) at depth 5: nothing non-finite where
    exact is finite, and, pooled over all cases, at least 99 % of the rays with every channel within 1e-3 |exact| + 1e-6 (L2 of
    test_gpu_shading_fast.py).  The share of each class is printed, not asserted."""
    exact, fast, cls = [], [], []
    for name in NAMES:
        c = sc.cases()[name]
        g = gpu_scene(c.desc)
        try:
            e, _, _ = ag.PathTracer(5).Li(g, c.rays, c.states)
            g.set_shading_arith("fast")
            assert g.shade_variant()[1] == 1
            f, _, _ = ag.PathTracer(5).Li(g, c.rays, c.states)
        finally:
            g.close()
        fin = np.isfinite(e)
        assert np.isfinite(f[fin]).all(), name
        exact.append(e)
        fast.append(f)
        cls += [c.cls] * len(e)
    exact, fast, cls = np.concatenate(exact), np.concatenate(fast), np.array(cls)
    fin = np.isfinite(exact).all(1)
    for k in sorted(set(cls)):
        m = fin & (cls == k)
        print("FAST %-20s %5d rays, %5d with other bits than exact, share within tolerance %.4f" %
              (k, m.sum(), (bits(fast[m]) != bits(exact[m])).any(1).sum(), close_fraction(fast[m], exact[m], 1e-3)))
    pooled = close_fraction(fast[fin], exact[fin], 1e-3)
    print("FAST pooled: %d rays, share within tolerance %.4f" % (fin.sum(), pooled))
    assert pooled >= 0.99
