"""agpt_skin_palette, the host twin of k_pack_palette (what agpt_scene_pose_mesh forms from a frame's joint matrices), against the numpy
model of skin_model.py, bit for bit.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_input_cases as dic
import skin_model

F = np.float32


def same_bits(got, want):
    assert got.shape == want.shape
    assert not np.isnan(want).any()          # (NaN sign bits differ between machines: such palettes are kept out of byte comparisons)
    assert (dic.bits(got) == dic.bits(want)).all(), np.argwhere(dic.bits(got) != dic.bits(want))[:5]


@pytest.mark.parametrize("with_normals", [True, False], ids=["stride21", "stride13"])
@pytest.mark.parametrize("kind", dic.REGULAR)
def test_one_class_matches_the_model(kind, with_normals):
    mats = np.stack([dic.joint_of(kind, np.random.RandomState(s)) for s in range(5)])
    palette, singular = ag.skin_palette(mats, with_normals)
    assert palette.shape == (5, 21 if with_normals else 13) and singular == -1
    same_bits(palette, dic.model_palette(mats, with_normals))
    assert np.isfinite(palette).all()


@pytest.mark.parametrize("with_normals", [True, False], ids=["stride21", "stride13"])
def test_scattered_classes_match_the_model(with_normals):
    mats, names = dic.joints(70, seed=3)
    assert set(names) == set(dic.REGULAR)
    palette, singular = ag.skin_palette(mats.reshape(-1, 16), with_normals)     # (n, 16) is taken as well
    assert singular == -1
    same_bits(palette, dic.model_palette(mats, with_normals))
    if not with_normals:
        assert (dic.bits(palette[:, 12]) == 0).all()                             # the pad


def test_negative_determinant_is_a_mirror():
    m = dic.joint_of("mirror", np.random.RandomState(1))
    assert np.linalg.det(m.astype(np.float64)) < 0
    palette, _ = ag.skin_palette(m[None])
    n = palette[0, 12:].reshape(3, 3).astype(np.float64)
    assert np.allclose(n, np.linalg.inv(m[:3, :3].astype(np.float64)).T, rtol=1e-5, atol=1e-6)


def test_subnormal_determinant_is_not_flushed():
    m = dic.joint_of(dic.SUBNORMAL_DET, None)
    det = dic.model_det(m)
    assert det == F(2.0 ** -127) and 0 < det < np.finfo(F).tiny                  # a subnormal
    want = skin_model.inverse_transpose(m)
    assert np.isfinite(want).all() and (np.diag(want) == [2.0 ** 42, 2.0 ** 42, 2.0 ** 43]).all()
    palette, singular = ag.skin_palette(m[None])
    assert singular == -1
    same_bits(palette[0, 12:].reshape(3, 3), want)


@pytest.mark.parametrize("with_normals", [True, False], ids=["stride21", "stride13"])
def test_underflowing_determinant_is_singular_and_gives_the_identity(with_normals):
    mats, _ = dic.joints(9, seed=5)
    mats[4] = mats[7] = dic.joint_of(dic.ZERO_DET, None)
    assert dic.model_det(mats[4]) == 0
    palette, singular = ag.skin_palette(mats, with_normals)
    assert singular == 4                                                         # the first of them, reported and not refused
    same_bits(palette, dic.model_palette(mats, with_normals))
    if with_normals:
        same_bits(palette[4, 12:].reshape(3, 3), np.eye(3, dtype=F))
        same_bits(palette[7, 12:].reshape(3, 3), np.eye(3, dtype=F))


def test_singular_out_may_be_null():
    L = ag.lib()
    m = np.ascontiguousarray(dic.joints(3, seed=1)[0])
    out = np.zeros((3, 21), F)
    fp = C.POINTER(C.c_float)
    assert L.agpt_skin_palette(m.ctypes.data_as(fp), 3, 1, out.ctypes.data_as(fp), None) == 0
    same_bits(out, dic.model_palette(m, True))


def test_refusals_write_nothing():
    L = ag.lib()
    fp = C.POINTER(C.c_float)
    good = np.ascontiguousarray(dic.joints(12, seed=2)[0])
    out = np.full((12, 21), 7, F)
    singular = C.c_int(99)

    def call(m=good, n=12, joints=True, palette=True):
        return L.agpt_skin_palette(m.ctypes.data_as(fp) if joints else None, n, 1, out.ctypes.data_as(fp) if palette else None, C.byref(singular))

    def refused(what, **kw):
        assert call(**kw) == -1
        err = L.agpt_last_error()
        assert err.startswith(b"agpt_skin_palette: ") and what in err, err
        assert (out == 7).all() and singular.value == 99

    refused(b"NULL", joints=False)
    refused(b"NULL", palette=False)
    refused(b"n_joints is 0, outside 1 .. 65536", n=0)
    refused(b"n_joints is 65537, outside 1 .. 65536", n=65537)
    bad = good.copy()
    bad[9, 1, 2] = np.inf
    bad[5, 3] = [0, 0, 0, 2]            # a non-finite entry is looked for in every joint before any last row
    refused(b"joint 9 has a non-finite entry", m=bad)
    bad[9, 1, 2] = 0
    bad[10, 3, 0] = F(1e-30)
    refused(b"the last row of joint 5 is not (0, 0, 0, 1)", m=bad)
    nan_row = good.copy()
    nan_row[2, 3, 3] = np.nan          # the last row is an entry like any other
    refused(b"joint 2 has a non-finite entry", m=nan_row)
    assert call() == 0 and singular.value == -1
    same_bits(out, dic.model_palette(good, True))
    with pytest.raises(ValueError, match="joint matrices have shape"):
        ag.skin_palette(np.zeros((3, 3, 3), F))
