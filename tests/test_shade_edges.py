"""Preconditions of tests/test_gpu_shade_edges.py, on the CPU: every case of shade_edge_cases.py enters the branch it is named after
often enough (oracle_li_tally counts the entries), the oracle's Li is finite there and mostly non-black -- so the GPU comparison
cannot pass on empty classes or on black images -- and the camera rays tests/test_gpu_li.py already runs enter none of these
branches.  Each test prints its counts (pytest -s shows them)."""
import numpy as np
import pytest

import ag_pathtracer_amd as ag
import shade_edge_cases as sc
from helpers import oracle_scene
from oracle import binding as ob
from ray_edge_cases import normalize32

F = np.float32


def _show(name, tally):
    return "%s: %s" % (name, ", ".join("%s %d" % (k, tally[i]) for k, i in sc.TALLY.items() if tally[i]))


@pytest.mark.parametrize("name", sc.case_names())
def test_case_enters_its_branch(name):
    """At depth 5: the named counters reach their minimum (100 path vertices; 30 for sphere_poles and env_axes, which have fewer
    rays, and for one side of a threshold), Li is finite on at least 99 % of the rays and non-black on at least 25 %."""
    c = sc.cases()[name]
    assert np.isfinite(c.rays["o"]).all() and np.isfinite(normalize32(c.rays["d"])).all() and (c.states != 0).all()
    want, after, total, tally = sc.reference(name, 5)
    finite = np.isfinite(want).all(1).mean()
    lit = (np.nan_to_num(want) != 0).any(1).mean()
    print("%s; %d rays, %.1f %% finite, %.1f %% non-black" % (_show(name, tally), len(c.rays), 100 * finite, 100 * lit))
    for counter, least in c.need.items():
        assert tally[sc.TALLY[counter]] >= least, (counter, int(tally[sc.TALLY[counter]]))
    assert tally[sc.TALLY["inside_pdf_inf"]] == 0      # (not reached by any class: the module docstring says so)
    assert finite >= 0.99 and lit >= 0.25


def test_depth_1_ends_every_path_after_one_vertex():
    """what distinguishes the two depths the GPU test runs: at depth 1 no ray has more than one shaded vertex, at depth 5 some do"""
    for name in ("zero_normals", "sphere_poles/disney"):
        n = len(sc.cases()[name].rays)
        assert sc.reference(name, 1)[3][sc.TALLY["shaded"]] <= n < sc.reference(name, 5)[3][sc.TALLY["shaded"]]


def test_inside_light_straddles_the_sphere_test():
    """The first hit points of inside_light's rim rays lie within 4 ulps of |p - c|^2 == r^2, at least 30 on each side of the
    reference's sqrlen(p - c) <= r2, and its other rays end inside the light on the floor or on the light's own surface."""
    c = sc.cases()["inside_light"]
    oh, p = sc.hit_points(c.desc, c.rays)
    sq = sc.sqrlen32(p - sc.LIGHT_C)
    r2 = sc.LIGHT_R * sc.LIGHT_R
    floor = (oh["hit"] == 1) & (oh["prim"] == 0)
    near = floor & (np.abs(sq.astype(np.float64) - float(r2)) <= 4 * 2.0 ** -23)
    inside, outside, exact = int((near & (sq <= r2)).sum()), int((near & (sq > r2)).sum()), int((near & (sq == r2)).sum())
    shell = int(((oh["hit"] == 1) & (oh["prim"] == 1)).sum())
    deep = int((floor & (sq < F(0.9))).sum())
    print("inside_light: %d hit points within 4 ulps inside (%d exactly on), %d outside; %d well inside; %d on the light" %
          (inside, exact, outside, deep, shell))
    assert inside >= 30 and outside >= 30 and exact >= 1
    assert deep >= 500 and shell >= 200


def test_cone_threshold_has_both_sides_next_to_the_threshold():
    """sinThetaMax2 of the first hit points, restated in fp32: at least 100 on each side of 0.00068523f, 30 of them within 1e-3
    (relative) of it"""
    c = sc.cases()["cone_threshold"]
    oh, p = sc.hit_points(c.desc, c.rays)
    assert (oh["hit"] == 1).all() and (oh["prim"] == 0).all()
    centre = np.array([0, sc.CONE_LIGHT_Y, 0], F)
    dc = np.sqrt(sc.sqrlen32(p - centre))
    s = F(1.0) * (F(1.0) / dc)
    s2 = s * s
    lim = F(0.00068523)
    close = np.abs(s2 / lim - 1) < 1e-3
    print("cone_threshold: %d small, %d wide; within 1e-3 of the threshold %d and %d" %
          ((s2 < lim).sum(), (s2 >= lim).sum(), (close & (s2 < lim)).sum(), (close & (s2 >= lim)).sum()))
    assert (s2 < lim).sum() >= 100 and (s2 >= lim).sum() >= 100
    assert (close & (s2 < lim)).sum() >= 30 and (close & (s2 >= lim)).sum() >= 30


def test_uv_threshold_meshes_lie_on_either_side_of_1e_8():
    """the reference's (double)fabsf(determinant) < 1e-8 on the two meshes' texture coordinates, restated; adjacent fp32 values;
    at least 30 first hits on each"""
    below, above = sc.uv_threshold_values()
    assert np.nextafter(below, F(1)) == above
    for s, degenerate in ((below, True), (above, False)):
        det = s * s - F(0) * F(0)        # duv02 = (-s, -s), duv12 = (0, -s)
        assert (float(np.abs(det)) < 1e-8) == degenerate
    for name in ("flat_uv/uv_threshold", "flat_uv/uv_threshold/env"):
        c = sc.cases()[name]
        oh, _ = sc.hit_points(c.desc, c.rays)
        on = [int(((oh["hit"] == 1) & (oh["prim"] == k)).sum()) for k in (0, 1)]
        tally = sc.reference(name, 5)[3]
        print("%s: first hits on the degenerate mesh %d, on the other %d; degenerate_frame %d" % (name, on[0], on[1], tally[sc.TALLY["degenerate_frame"]]))
        assert min(on) >= 30
        # the frames of the second mesh are not degenerate: the counter stays below the passed triangle tests
        assert tally[sc.TALLY["degenerate_frame"]] < tally[sc.TALLY["shaded"]]


def test_zero_area_rays_pass_every_test_before_the_rejection():
    """the tiny triangle's rejected hits: the oracle reports the floor behind it, 2^-10 further"""
    c = sc.cases()["flat_uv/zero_area"]
    down = c.rays[:300]
    oh, _ = sc.hit_points(c.desc, down)
    assert (oh["hit"] == 1).all() and (oh["tri"] != 6).all() and np.array_equal(oh["t"], down["o"][:, 1])


def test_env_axes_reach_the_map_s_edges():
    """InfiniteAreaLight::Le along the axes, restated: phi = atan2(+-0, +-1) and theta = acos(+-1) occur with every sign, and the
    nearest-texel lookup wraps to the last column (phi == 0) and to the last row (theta == 0)"""
    c = sc.cases()["env_axes/disney"]
    d = normalize32(c.rays["d"])[:240]
    assert np.array_equal(d.view(np.uint32), c.rays["d"][:240].view(np.uint32))      # signed zeros survive the normalisation
    w = d[:, [0, 2, 1]]
    phi = np.arctan2(w[:, 1].astype(np.float64), w[:, 0].astype(np.float64)).astype(F)
    theta = np.arccos(np.clip(w[:, 2], -1, 1).astype(np.float64)).astype(F)
    neg_zero = (phi == 0) & np.signbit(phi)
    col = np.floor(np.where(phi < 0, phi + F(2 * np.pi), phi) * F(0.5 / np.pi) * F(16) - F(0.5))
    row = np.floor(theta * F(1 / np.pi) * F(8) - F(0.5))
    print("env_axes: phi +0 %d, -0 %d, +-pi %d; theta 0 %d, pi %d; wrapped columns %d, rows %d" %
          (((phi == 0) & ~neg_zero).sum(), neg_zero.sum(), (np.abs(phi) > 3.14).sum(), (theta == 0).sum(), (theta > 3.14).sum(),
           (col < 0).sum(), (row < 0).sum()))
    assert ((phi == 0) & ~neg_zero).sum() >= 30 and neg_zero.sum() >= 30
    assert (phi > 3.14).sum() >= 10 and (phi < -3.14).sum() >= 10
    assert (theta == 0).sum() >= 30 and (theta > 3.14).sum() >= 30
    assert (col < 0).sum() >= 30 and (row < 0).sum() >= 30
    # the rays down onto the floor bounce: Sample_Li and Pdf_Li of the map run on at least 100 vertices
    assert sc.reference("env_axes/disney", 5)[3][sc.TALLY["shaded"]] >= 100


def test_camera_rays_of_test_gpu_li_enter_none_of_these_branches():
    """Why this suite exists: test_gpu_li.py's own inputs on C1 (3000 camera rays, seed 7, depth 5) enter the small- and the
    wide-cone branch and none of the others.  If this fails because a counter is no longer zero, the classes may have become
    redundant."""
    from test_gpu_li import camera_rays
    o = oracle_scene(ag.scenes.scene_c1(), 5)
    rays, states = camera_rays(o, 3000, seed=7)
    tally = np.zeros(len(ob.TALLY_NAMES), np.int64)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        for i in range(len(rays)):
            tally += o.li(rays[i], int(states[i]), tally=True)[3]
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    print(_show("C1 camera rays", tally))
    for counter in ("inside_sample", "inside_pdf", "ns_zero", "ts_zero", "degenerate_frame", "zero_area_reject", "sphere_pole",
                    "light_sample_rejected", "inside_pdf_inf"):
        assert tally[sc.TALLY[counter]] == 0, counter
    assert tally[sc.TALLY["small_cone"]] >= 100 and tally[sc.TALLY["wide_cone"]] >= 100


def test_tally_changes_no_output():
    """oracle_li and oracle_li_tally: the same radiance, stream and stats on a case with bounces"""
    c = sc.cases()["sphere_poles/disney"]
    o = oracle_scene(c.desc, 5)
    for i in range(len(c.rays)):
        a, b = o.li(c.rays[i], int(c.states[i])), o.li(c.rays[i], int(c.states[i]), tally=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].as_dict() == b[2].as_dict()
        assert b[3][sc.TALLY["shaded"]] == b[2].as_dict()["shaded_vertices"]
