"""tests/analytic_motion_model.py against tests/motion_model.py and against a float64 evaluation, on synthetic hit records: unmoved
analytic records change nothing, a translation or a scale lands where float64 says, the non-finite fallback, the byte comparison."""
import numpy as np

import analytic_motion_model as am
import motion_model as mm

F = np.float32
EPS = 2.0 ** -24


def synthetic(n=400, seed=3):
    """hit records over 2 triangles and 4 primitives (mesh, sphere, plane, sphere): a third misses, a third analytic, a third triangles"""
    rng = np.random.RandomState(seed)
    ids = rng.choice([mm.MISS, mm.ANALYTIC, 0, 1], size=n, p=[0.3, 0.4, 0.15, 0.15]).astype(np.int64)
    prim = np.where(ids == mm.ANALYTIC, rng.choice([1, 2, 3], size=n), np.where(ids >= 0, 0, -1))
    t = rng.uniform(0.5, 9.0, n).astype(F)
    b1 = rng.uniform(0, 0.5, n).astype(F)
    b2 = rng.uniform(0, 0.5, n).astype(F)
    O = np.array([0.25, 1.0, -4.0], F)
    D = rng.normal(size=(n, 3))
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(F)
    gen = rng.uniform(-2, 2, (2, 3, 3)).astype(F)
    return (ids, t, b1, b2), prim, O, D, gen


KINDS = np.array([am.MESH, am.SPHERE, am.PLANE, am.SPHERE])
REC = np.array([[0, 0, 0, 0, 0], [0.5, 1.0, 0.25, 0.75, 0.5625], [0.0, -0.5, 1.0, 4.0, 2.5], [-1.5, 2.0, 3.0, 0.3, F(0.3) * F(0.3)]], F)


def test_unmoved_records_give_the_mesh_models_bytes():
    hits, prim, O, D, gen = synthetic()
    gen_new = gen + F(0.125)
    want = mm.prev_points(hits, O, D, gen, gen_new)
    got = am.prev_points(hits, prim, O, D, gen, gen_new, REC, REC.copy(), KINDS)
    assert got.tobytes() == want.tobytes()
    assert (got[hits[0] == mm.ANALYTIC, 3] == 2).all() and (got[:, 3] == 1).any()   # (the moved triangles only)
    # no analytic generations at all (a scene of meshes only)
    assert am.prev_points(hits, prim, O, D, gen, gen_new, np.zeros((0, 5), F), np.zeros((0, 5), F), KINDS).tobytes() == want.tobytes()
    # a NaN against itself is not a move
    nan = REC.copy()
    nan[1, 0] = np.nan
    assert am.prev_points(hits, prim, O, D, gen, gen_new, nan, nan.copy(), KINDS).tobytes() == want.tobytes()


def moved_records():
    new = REC.copy()
    new[1, :3] += np.array([0.3, -0.2, 0.5], F)          # a sphere translated
    new[3, 3] = F(0.45)                                  # a sphere scaled
    new[3, 4] = F(0.45) * F(0.45)
    new[2] = np.array([0.25, -0.5, 0.5, 3.0, 3.5], F)    # a plane moved and resized
    return new


def test_translation_and_scale_agree_with_float64():
    hits, prim, O, D, gen = synthetic()
    new = moved_records()
    got = am.prev_points(hits, prim, O, D, gen, gen, REC, new, KINDS)
    on = hits[0] == mm.ANALYTIC
    assert (got[on, 3] == 1).all() and (got[~on & (hits[0] != mm.MISS), 3] == 2).all() and (got[hits[0] == mm.MISS] == 0).all()
    want = am.prev_points64(hits, prim, O, D, REC, new, KINDS)
    # Five roundings: O + t * D (two, at magnitude |O| + |t D|), the difference with c_new (one, same magnitude + |c_new|), the product
    # with s (one, after s's own: the magnitude above times |s|, twice) and the sum with c_old.  Each is half an ulp of its result.
    k = np.where(on, prim, 0)
    with np.errstate(all="ignore"):   # (the mesh's record is zeros)
        smax = np.fmax(1.0, np.fmax(REC[k, 3] / new[k, 3], np.where(KINDS[k] == am.PLANE, REC[k, 4] / new[k, 4], 0)))
    mag = (np.abs(O)[None] + np.abs(hits[1][:, None] * D) + np.abs(new[k, :3])) * smax[:, None]
    bound = EPS * (4 * mag + np.abs(REC[k, :3]) + np.abs(want))
    err = np.abs(got[:, :3].astype(np.float64) - want)
    print("max error / bound: %.3f" % np.nanmax(err[on] / bound[on]))
    assert (err[on] <= bound[on]).all()
    # the sphere translated: the point keeps its offset from the centre; the plane keeps y (s.y = 1)
    s1 = on & (prim == 1)
    now = mm.prev_points(hits, O, D, gen, gen)[:, :3]
    assert np.allclose(got[s1, :3] - REC[1, :3], now[s1] - new[1, :3], atol=1e-5) and s1.any()
    p2 = on & (prim == 2)
    assert (got[p2, 1] == (REC[2, 1] + (now[p2, 1] - new[2, 1]) * F(1)).astype(F)).all() and p2.any()


def test_fallback_rows_keep_w_2():
    hits, prim, O, D, gen = synthetic()
    still = mm.prev_points(hits, O, D, gen, gen)
    on = hits[0] == mm.ANALYTIC
    # q = r_old / r_new overflows
    old, new = REC.copy(), REC.copy()
    old[1, 3], new[1, 3] = F(1e30), F(1e-30)
    got = am.prev_points(hits, prim, O, D, gen, gen, old, new, KINDS)
    assert got.tobytes() == still.tobytes() and (on & (prim == 1)).any()
    # q is finite, the point is not
    old, new = REC.copy(), REC.copy()
    old[3, 3], new[3, 3] = F(1e38), F(1.0)
    got = am.prev_points(hits, prim, O, D, gen, gen, old, new, KINDS)
    far = np.abs(am.prev_points64(hits, prim, O, D, old, new, KINDS)).max(-1)
    over, under = on & (prim == 3) & (far > 3.5e38), on & (prim == 3) & (far < 3.3e38)
    assert over.any() and under.any()
    assert got[over].tobytes() == still[over].tobytes() and (got[under, 3] == 1).all()
    assert got[prim != 3].tobytes() == still[prim != 3].tobytes()
    # the plane's second half-size alone
    old, new = REC.copy(), REC.copy()
    new[2, 4] = F(0)
    got = am.prev_points(hits, prim, O, D, gen, gen, old, new, KINDS)
    assert got.tobytes() == still.tobytes() and (on & (prim == 2)).any()
    # the other primitives' rows of the same call are not touched by one primitive's fallback
    new = moved_records()
    new[1, 3] = F(0)
    got = am.prev_points(hits, prim, O, D, gen, gen, REC, new, KINDS)
    assert (got[on & (prim == 1), 3] == 2).all() and (got[on & (prim != 1), 3] == 1).all()


def test_negative_zero_against_zero_counts_as_moved():
    hits, prim, O, D, gen = synthetic()
    old, new = REC.copy(), REC.copy()
    old[2, 0], new[2, 0] = F(-0.0), F(0.0)
    assert am.moved(old, new).tolist() == [False, False, True, False]
    got = am.prev_points(hits, prim, O, D, gen, gen, old, new, KINDS)
    on = (hits[0] == mm.ANALYTIC) & (prim == 2)
    assert (got[on, 3] == 1).all() and on.any()
    assert (got[(hits[0] == mm.ANALYTIC) & (prim != 2), 3] == 2).all()
    # harmless: the point is where it is now, to the rounding of one subtraction and one addition
    now = mm.prev_points(hits, O, D, gen, gen)[:, :3]
    assert np.allclose(got[on, :3], now[on], rtol=0, atol=1e-5)


def test_records_of_a_description():
    import ag_pathtracer_amd as ag
    d = ag.scenes.SceneDesc("r")
    m = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.5, 0.5, 0.5))
    d.add_mesh(mm.FLOOR[0], None, None, mm.FLOOR[1], m)
    d.add_sphere((1, 2, 3), 0.3, m)
    d.add_plane((0, -1, 0), (7, 3), m)
    d.add_area_light((4, 5, 6), 0.7, (1, 1, 1))
    rec, kinds = am.records(d)
    assert kinds.tolist() == [am.MESH, am.SPHERE, am.PLANE, am.SPHERE]
    assert rec.tobytes() == np.array([[0, 0, 0, 0, 0], [1, 2, 3, F(0.3), F(0.3) * F(0.3)], [0, -1, 0, 3.5, 1.5],
                                      [4, 5, 6, F(0.7), F(0.7) * F(0.7)]], F).tobytes()
