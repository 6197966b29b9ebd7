"""The walk set of update_walk_cases.py meets the conditions that make it worth running (no GPU): counted from the action lists with
the predicted bookkeeping (Flags), and -- the last one -- from the model's scenes through the CPU oracle.  `-s` prints the census."""
import numpy as np
import pytest

import device_update_cases as dc
import update_walk_cases as uw
from helpers import bits
from oracle import binding as ob


def cells(covered, tag):
    return sorted((c for c in covered if c[0] == tag), key=repr)


@pytest.fixture(scope="module")
def zoo_cells():
    return uw.census(uw.walks(), False)


def test_the_walk_set_has_the_stated_size():
    ws = uw.walks()
    zoo, long_ = [w for w in ws if not w.layout.long], [w for w in ws if w.layout.long]
    print("walks: %d on the zoo of %s actions, %d on the 70-primitive scene of %s" % (len(zoo), [len(w.actions) for w in zoo], len(long_), [len(w.actions) for w in long_]))
    assert len(zoo) == uw.N_ZOO_WALKS <= 16 and all(len(w.actions) <= 48 for w in zoo)
    assert len(long_) == uw.N_LONG_WALKS == 2 and all(len(w.actions) <= 24 for w in long_)
    assert [w.seed for w in ws] == uw.SEEDS
    # a walk is reproduced by its seed: a second generation gives the same lists
    uw.walks.cache_clear()
    assert [w.actions for w in uw.walks()] == [w.actions for w in ws]


def test_condition_1_every_ordered_pair_of_front_ends(zoo_cells):
    """both in REFIT on one mesh (neither took the fallback), with no mirror reader anywhere and no other action on that mesh between"""
    pairs = cells(zoo_cells, "pair")
    print("pairs covered %d/81" % len(pairs))
    assert {c[1:] for c in pairs} == {(a, b) for a in uw.FRONT_ENDS for b in uw.FRONT_ENDS}


def test_condition_2_every_front_end_after_a_rebuild_a_fallback_and_a_builder_switch(zoo_cells):
    for what in ("rebuild", "fallback", "builder"):
        got = {c[1] for c in cells(zoo_cells, "after_" + what)}
        print("directly after a %s: %d/9 front ends" % (what, len(got)))
        assert got == set(uw.FRONT_ENDS), what
    assert {c[1] for c in cells(zoo_cells, "rebuild_mode")} == set(uw.FRONT_ENDS)


def test_condition_3_every_mirror_reader_in_every_state(zoo_cells):
    got = {c[1:] for c in cells(zoo_cells, "reader")}
    print("readers x states:")
    for r in uw.READERS:
        print("  %-14s %s" % (r, " ".join("%s:%s" % (s, "yes" if (r, s) in got else "NO") for s in uw.STATES)))
    assert got == {(r, s) for r in uw.READERS for s in uw.STATES}


def test_condition_4_every_front_end_in_smooth_mode_and_first_after_each_switch(zoo_cells):
    assert {c[1] for c in cells(zoo_cells, "smooth")} == set(uw.FRONT_ENDS)
    assert {c[1:] for c in cells(zoo_cells, "first_after_mode")} == {(d, k) for d in ("to_smooth", "to_given") for k in uw.FRONT_ENDS}
    print("smooth mode: 9/9 front ends; first call after a switch: 18/18")


def test_condition_5_snapshots_with_a_rebuild_a_fallback_and_a_device_only_update_between(zoo_cells):
    assert {c[1:] for c in cells(zoo_cells, "snap")} == {(s, b) for s in uw.SNAPSHOTS for b in uw.BETWEEN}
    assert len(cells(zoo_cells, "alternate")) == 2
    print("snapshots: 2 calls x (rebuild, fallback, device-only) between their generations; both alternations")


def test_condition_6_every_refusal_twice_and_once_on_stale_state(zoo_cells):
    assert {c[1:] for c in cells(zoo_cells, "refusal")} == {(w, n) for w in uw.REFUSALS for n in (1, 2)}
    assert {c[1] for c in cells(zoo_cells, "refusal_stale")} == set(uw.REFUSALS)
    counts = {w: sum(a["kind"] == "refuse" and a["what"] == w for x in uw.walks() for a in x.actions) for w in uw.REFUSALS}
    print("refusals:", counts, "-- each at least once on stale state")


def test_the_routes_and_variants_beside_the_conditions(zoo_cells):
    """both palette routes of every call that takes joints, the three forms of the sphere batch, the analytic calls, a binding and
    targets replaced under a live cache; on the 70-primitive scene every front end in REFIT and the readers behind a device-only REFIT"""
    assert uw.zoo_universe() <= zoo_cells, sorted(uw.zoo_universe() - zoo_cells, key=repr)
    long_cells = uw.census(uw.walks(), True)
    assert uw.long_universe() <= long_cells, sorted(uw.long_universe() - long_cells, key=repr)
    kinds = {}
    for w in uw.walks():
        for a in w.actions:
            kinds[a["kind"]] = kinds.get(a["kind"], 0) + 1
    print("actions by kind:", dict(sorted(kinds.items())))


def hits_of(model, rays, swapped=False):
    d = model.desc()
    if swapped:   # the same scene with the leaf sizes 1 and 4 exchanged: other trees
        d.ops = [op[:6] + (5 - op[6] if op[6] in (1, 4) else op[6],) if op[0] == "mesh" else op for op in d.ops]
    return d.instantiate(ob.OracleScene()).intersect(rays)[0]


def tie_rays(model, rays, hits):
    """the rays whose closest hit ties between two triangles at equal t, found by the oracle itself: the same scene with the leaf sizes 1
    and 4 exchanged (other trees, another visiting order) reports the same t from another triangle -> (ties, rays whose hit flag or t
    changes with the tree)"""
    other = hits_of(model, rays, swapped=True)
    same_t = (other["hit"] == hits["hit"]) & ((hits["hit"] == 0) | (bits(other["t"]) == bits(hits["t"])))
    return same_t & (hits["hit"] == 1) & ((other["prim"] != hits["prim"]) | (other["tri"] != hits["tri"])), ~same_t


@pytest.mark.parametrize("seed", uw.SEEDS)
def test_condition_7_every_step_shows_in_a_hit_record(seed):
    """the model's scene after every action that moves geometry (a front end, update_sphere, update_plane, a sphere batch) differs from the
    scene one step earlier in at least one closest-hit record of the fixed ray set (CPU oracle).  Every other action -- refusals and
    readers, and also the setters, set_radiance and the snapshots, none of which can move a hit record -- leaves all of them alone.
    After every moving step the rays whose hit ties between two triangles are at most 1 %; they are found by a second oracle scene
    with other trees (tie_rays), not by counting equal-t pairs."""
    w = uw.walk(seed)
    rays = dc.rays_for(w.layout.desc)
    model = uw.Model(w.layout)
    last = hits_of(model, rays)
    assert last["hit"].sum() > len(rays) // 4
    most, tree = 0, 0
    for i, a in enumerate(w.actions):
        model.apply(a, model.inputs(a))
        now = hits_of(model, rays)
        if a["kind"] in uw.CHANGES_GEOMETRY:
            assert now.tobytes() != last.tobytes(), "%r step %d (%s) does not show" % (w, i, uw.describe(a))
            ties, by_tree = tie_rays(model, rays, now)
            assert ties.mean() <= 0.01, "%r step %d (%s): %d rays tie" % (w, i, uw.describe(a), int(ties.sum()))
            most, tree = max(most, int(ties.sum())), max(tree, int(by_tree.sum()))
        else:
            assert now.tobytes() == last.tobytes(), "%r step %d (%s) moved something" % (w, i, uw.describe(a))
        last = now
    print("%r: %d actions, %d of %d rays hit at the end; at any step at most %d ties (%.2f %%) and %d rays whose t depends on the tree"
          % (w, len(w.actions), int(last["hit"].sum()), len(rays), most, 100.0 * most / len(rays), tree))
