"""agpt_morph_active, the host twin of k_morph_active (the active list agpt_scene_morph_mesh forms from a frame's weights), against the
rule of morph_model.py.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_input_cases as dic
import morph_model
from morph_cases import targets

F = np.float32
SIZES = (1, 2, 63, 64, 65, 300, 4096)


def check(weights):
    t, w = ag.morph_active(weights)
    want_t, want_w = dic.model_active(weights)
    assert t.dtype == np.int32 and w.dtype == F
    assert (t == want_t).all() and (dic.bits(w) == dic.bits(want_w)).all()
    return t, w


@pytest.mark.parametrize("T", SIZES)
def test_patterns_match_the_model(T):
    p = dic.weight_patterns(T)
    assert len(check(p["all-zero"])[0]) == 0
    assert np.signbit(p["minus-zero"]).all() and len(check(p["minus-zero"])[0]) == 0       # -0.0 is a zero weight
    t, w = check(p["mixed"])
    if T >= 63:
        assert (w < 0).any() and (w > 1).any() and 0 < len(t) < T
    assert (check(p["last-only"])[0] == [T - 1]).all()
    assert (p["all-active"] != 0).all() and len(check(p["all-active"])[0]) == T
    assert (check(p["every-other"])[0] == np.arange(0, T, 2)).all()


def test_the_list_blends_like_the_weights():
    """walking the pairs in order is morph_model.blend: the list drops exactly what the model skips"""
    T, n = 9, 17
    weights = dic.weight_patterns(T, seed=4)["mixed"]
    weights[3] = 1.5
    rest = np.random.RandomState(1).normal(size=(n, 3)).astype(F)
    deltas = targets(n, T, 5, extent=2.0)
    t, w = ag.morph_active(weights)
    acc = rest.copy()
    for k in range(len(t)):
        acc = (acc + (w[k] * deltas[t[k]]).astype(F)).astype(F)
    assert (dic.bits(acc) == dic.bits(morph_model.blend(rest, deltas, weights))).all()


def test_refusals_write_nothing():
    L = ag.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    good = dic.weight_patterns(8)["mixed"].copy()
    t_out, w_out, n_out = np.full(8, 7, np.int32), np.full(8, 7, F), C.c_int(99)

    def call(w=good, n=8, null=None):
        a = [w.ctypes.data_as(fp), n, t_out.ctypes.data_as(ip), w_out.ctypes.data_as(fp), C.byref(n_out)]
        if null is not None:
            a[null] = None
        return L.agpt_morph_active(*a)

    def refused(what, **kw):
        assert call(**kw) == -1
        err = L.agpt_last_error()
        assert err.startswith(b"agpt_morph_active: ") and what in err, err
        assert (t_out == 7).all() and (w_out == 7).all() and n_out.value == 99

    for k in (0, 2, 3, 4):
        refused(b"NULL", null=k)
    refused(b"n_targets is 0, outside 1 .. 4096", n=0)
    refused(b"n_targets is 4097, outside 1 .. 4096", w=np.zeros(4097, F), n=4097)
    bad = good.copy()
    bad[6], bad[2] = np.nan, -np.inf
    refused(b"non-finite weight (target 2)", w=bad)
    assert call() == 0
    want_t, want_w = dic.model_active(good)
    assert n_out.value == len(want_t) and (t_out[:len(want_t)] == want_t).all() and (dic.bits(w_out[:len(want_t)]) == dic.bits(want_w)).all()
