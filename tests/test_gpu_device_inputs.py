"""Joint matrices and morph weights given in device memory: agpt_scene_pose_mesh_device and agpt_scene_morph_mesh_device against the
host calls on the same numbers (scene A takes the host call, scene B the device call; device_update_cases.snapshot must be
bit-identical), and the two kernels in front of them -- k_pack_palette, k_morph_active -- against their host twins through the
known-answer calls (test_skin_palette.py and test_morph_active.py pin the twins to the numpy models)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_input_cases as dic
import device_update_cases as dc
import skin_model
from device_update_cases import BIG, big_scene, joints_of, morph_targets, pair, palette, seventy_prims, skin_of
from helpers import gpu_context
from morph_cases import targets, weights
from skin_cases import binding, single_slot

pytestmark = pytest.mark.gpu
F = np.float32
EYE = np.eye(4, dtype=F)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("refit", "host"), ("rebuild", "host"), ("rebuild", "device")]
WEIGHT_SETS = ([0, 2], [0, 1, 2])


class Uploads:
    """caller's arrays in device memory of the context (agpt_device_alloc is 256-byte aligned); on leaving they are overwritten and
    freed: the library may not still be reading them"""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def __call__(self, a, offset=0):
        a = np.ascontiguousarray(a, F)
        p = self.ctx.alloc(a.nbytes + 64)
        self.held.append((p, a.nbytes + 64))
        self.ctx.upload(p + offset, a)
        return p + offset

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p, n in self.held:
            self.ctx.memset(p, 0xFF, n)
            self.ctx.free(p)


def pose_dev(g, up, prim, mats, mode="refit"):
    m = np.asarray(mats, F).reshape(-1, 16)
    g.pose_mesh_device(prim, up(m), len(m), mode)


def morph_dev(g, up, prim, w, mats=None, mode="refit"):
    m = None if mats is None else np.asarray(mats, F).reshape(-1, 16)
    g.morph_mesh_device(prim, up(w), len(w), None if m is None else up(m), 0 if m is None else len(m), mode)


# ---- the kernels against their host twins ------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_normals", [True, False], ids=["stride21", "stride13"])
@pytest.mark.parametrize("n_joints", [1, 2, 63, 64, 65, 255, 256, 257, 487, 488, 4096])
def test_palette_kernel_equals_the_host_twin(n_joints, with_normals):
    """every class of test_skin_palette.py scattered over the joints, the subnormal determinant among them (a device that flushes it to
    zero reports the joint singular and writes the identity)"""
    mats, names = dic.joints(n_joints, seed=n_joints)
    assert n_joints < 4 or dic.SUBNORMAL_DET in names
    want, singular = ag.skin_palette(mats, with_normals)
    got, status = gpu_context().kat_skin_palette(mats, with_normals)
    assert singular == -1 and (status == dic.NONE).all(), status
    assert not np.isnan(want).any() and (dic.bits(got) == dic.bits(want)).all()


def test_palette_kernel_on_singular_joints():
    mats, _ = dic.joints(300, seed=11)
    for j in (299, 130, 131, 64):
        mats[j] = dic.joint_of(dic.ZERO_DET, None)
    for with_normals in (True, False):
        want, singular = ag.skin_palette(mats, with_normals)
        got, status = gpu_context().kat_skin_palette(mats, with_normals)
        assert singular == 64 and list(status) == [dic.NONE, dic.NONE, 64]
        assert (dic.bits(got) == dic.bits(want)).all()


@pytest.mark.parametrize("T", [1, 63, 64, 65, 255, 256, 257, 4096])
def test_active_kernel_equals_the_host_twin(T):
    for name, w in dic.weight_patterns(T).items():
        want_t, want_w = ag.morph_active(w)
        t, a, status = gpu_context().kat_morph_active(w)
        assert list(status) == [len(want_t), dic.NONE], name
        assert (t == want_t).all() and (dic.bits(a) == dic.bits(want_w)).all(), name


@pytest.mark.parametrize("word", [0, 1, 2], ids=["non-finite", "last-row", "singular"])
def test_the_lowest_offending_joint_wins(word):
    """two offenders of one kind in different waves (and blocks), the higher one first in memory order of nothing: the word is a minimum"""
    for lo, hi in ((70, 200), (3, 64), (129, 130)):
        mats, _ = dic.joints(300, seed=word)
        for j in (hi, lo):
            if word == 0:
                mats[j, 1, 2] = np.inf if j == lo else np.nan
            elif word == 1:
                mats[j, 3, j % 4] += F(0.5)
            else:
                mats[j] = dic.joint_of(dic.ZERO_DET, None)
        _, status = gpu_context().kat_skin_palette(mats)
        want = [dic.NONE] * 3
        want[word] = lo
        assert list(status) == want


def test_each_kind_has_a_word_of_its_own():
    mats, _ = dic.joints(100, seed=5)
    mats[5, 3, 3] = 2                              # a bad last row
    mats[9, 0, 0] = np.nan                         # a non-finite entry
    mats[3] = dic.joint_of(dic.ZERO_DET, None)     # singular
    mats[7, 3, 0] = F(1e-30)
    mats[70, 3, 1] = -np.inf                       # non-finite, in the last row: both words see it
    _, status = gpu_context().kat_skin_palette(mats)
    assert list(status) == [9, 5, 3]


def test_the_lowest_non_finite_weight_wins():
    for lo, hi in ((130, 290), (0, 4095), (255, 256), (63, 64)):
        w = dic.weight_patterns(4096)["mixed"].copy()
        w[hi], w[lo] = np.nan, np.inf
        _, _, status = gpu_context().kat_morph_active(w)
        assert status[1] == lo


# ---- scene parity: the device call against the host call ---------------------------------------------------------------------

@pytest.mark.parametrize("mode,builder", MODES)
def test_pose_device_equals_pose(mode, builder):
    """all eight meshes of the zoo, two frames in a row (the second finds rest pose, binding and palette buffer on the device)"""
    desc, a, b = pair(builder)
    start = dc.snapshot(b, desc, dc.PRIMS)
    for g in (a, b):
        for prim in dc.PRIMS:
            skin_of(g, prim)
    for frame in (0, 1):
        with Uploads(b.ctx) as up:
            for prim in dc.PRIMS:
                a.pose_mesh(prim, palette(prim, frame), mode)
                pose_dev(b, up, prim, palette(prim, frame), mode)
        sa, sb = dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS)
        dc.assert_same(sa, sb)
        assert sb["render"] != start["render"]
        start = sb
    a.close()
    b.close()


@pytest.mark.parametrize("fused", [False, True], ids=["morph", "fused"])
@pytest.mark.parametrize("mode,builder", MODES)
def test_morph_device_equals_morph(mode, builder, fused):
    desc, a, b = pair(builder)
    start = dc.snapshot(b, desc, dc.PRIMS)
    for g in (a, b):
        for prim in dc.PRIMS:
            morph_targets(g, prim)
            if fused:
                skin_of(g, prim)
    for frame, act in enumerate(WEIGHT_SETS):
        with Uploads(b.ctx) as up:
            for prim in dc.PRIMS:
                w = weights(3, prim + frame, act)
                mats = palette(prim, frame) if fused else None
                a.morph_mesh(prim, w, mats, mode)
                morph_dev(b, up, prim, w, mats, mode)
        sa, sb = dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS)
        dc.assert_same(sa, sb)
        assert sb["render"] != start["render"]
        start = sb
    a.close()
    b.close()


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_smooth_normals_mode(mode):
    """the palette carries M only (stride 13): a pose, then a fused morph, on the meshes with normals and on one without"""
    desc, a, b = pair()
    prims = (1, 3, dc.GRID1_N, dc.GRID4_N, dc.GRID4)
    for g in (a, b):
        for prim in prims:
            skin_of(g, prim)
            morph_targets(g, prim)
            if dc.zoo_arrays(prim)[1] is not None:
                g.set_mesh_normals_mode(prim, "smooth")
    with Uploads(b.ctx) as up:
        for prim in prims:
            a.pose_mesh(prim, palette(prim, 0), mode)
            pose_dev(b, up, prim, palette(prim, 0), mode)
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        for prim in prims:
            w = weights(3, prim, [0, 1, 2])
            a.morph_mesh(prim, w, palette(prim, 1), mode)
            morph_dev(b, up, prim, w, palette(prim, 1), mode)
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_the_global_palette_route(monkeypatch):
    """AGPT_SKIN_GLOBAL_PALETTE for the device calls of scene B, the staged palette for the host calls of scene A"""
    desc, a, b = pair()
    for g in (a, b):
        for prim in dc.PRIMS:
            skin_of(g, prim)
            morph_targets(g, prim)
    with Uploads(b.ctx) as up:
        for prim in dc.PRIMS:
            w = weights(3, prim, [0, 2])
            if prim % 2 == 0:
                a.morph_mesh(prim, w, palette(prim, 1))
            else:
                a.pose_mesh(prim, palette(prim, 1))
            monkeypatch.setenv("AGPT_SKIN_GLOBAL_PALETTE", "1")
            if prim % 2 == 0:
                morph_dev(b, up, prim, w, palette(prim, 1))
            else:
                pose_dev(b, up, prim, palette(prim, 1))
            monkeypatch.delenv("AGPT_SKIN_GLOBAL_PALETTE")
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


@pytest.mark.parametrize("fused", [False, True], ids=["pose", "fused"])
@pytest.mark.parametrize("n_joints", [487, 488])
def test_palettes_on_either_side_of_the_lds_cap(n_joints, fused):
    """487 joints of 84 B are the last that are staged, 488 are read from global memory: n_joints * stride * 4 decides, whoever wrote
    the palette; the joints between the three used ones carry every class of matrix"""
    desc, a, b = pair()
    prim = dc.GRID4_N
    used = np.array([0, n_joints // 2, n_joints - 1], np.int32)
    J, W = binding(len(dc.zoo_arrays(prim)[0]), 4, seed=prim)
    mats, _ = dic.joints(n_joints, seed=n_joints)
    mats[used] = palette(prim, 1)
    w = weights(3, 5, [0, 2])
    with Uploads(b.ctx) as up:
        for g in (a, b):
            g.set_mesh_skin(prim, used[J], W, n_joints=n_joints)
            morph_targets(g, prim)
        if fused:
            a.morph_mesh(prim, w, mats)
            morph_dev(b, up, prim, w, mats)
        else:
            a.pose_mesh(prim, mats)
            pose_dev(b, up, prim, mats)
    dc.assert_same(dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim]))
    a.close()
    b.close()


@pytest.mark.parametrize("fused", [False, True], ids=["morph", "fused"])
def test_a_capped_grid(fused, monkeypatch):
    """AGPT_MORPH_MAX_BLOCKS=1 for the device calls alone: the bytes of the uncapped host calls"""
    desc, a, b = pair(desc=big_scene())
    prims = (dc.GRID4_N, BIG)
    w = weights(3, 3, [0, 1, 2])
    for g in (a, b):
        for prim in prims:
            morph_targets(g, prim)
            if fused:
                skin_of(g, prim)
    with Uploads(b.ctx) as up:
        for prim in prims:
            mats = joints_of(prim, 0) if fused else None
            a.morph_mesh(prim, w, mats)
            monkeypatch.setenv("AGPT_MORPH_MAX_BLOCKS", "1")
            morph_dev(b, up, prim, w, mats)
            monkeypatch.delenv("AGPT_MORPH_MAX_BLOCKS")
    dc.assert_same(dc.snapshot(a, desc, prims), dc.snapshot(b, desc, prims))
    a.close()
    b.close()


def test_a_device_pose_after_a_rebuild_uploads_the_binding_again():
    desc, a, b = pair()
    for prim in (dc.GRID4_N, 4):
        for g in (a, b):
            skin_of(g, prim)
        for frame, mode in ((0, "refit"), (1, "rebuild"), (0, "refit"), (1, "refit")):   # the REBUILD destroys the device cache
            with Uploads(b.ctx) as up:
                a.pose_mesh(prim, palette(prim, frame), mode)
                pose_dev(b, up, prim, palette(prim, frame), mode)
            dc.assert_same(dc.snapshot(a, desc, [prim]), dc.snapshot(b, desc, [prim]))
    a.close()
    b.close()


def test_posed_positions_that_overflow_take_the_fallback():
    """finite matrices, positions at +Inf (the grids of test_gpu_pose_mesh's case, for its reason): the status words are clean, the
    finiteness flag of the refit is not"""
    desc, a, b = pair()
    T = EYE.copy()
    T[0, 3] = 3e38
    mats = np.stack([EYE, T, T])
    with Uploads(b.ctx) as up:
        for prim in (dc.GRID4_N, dc.GRID1):
            v, n = dc.zoo_arrays(prim)
            J, W = single_slot(len(v), 2, 0, (0,), 1.0)
            J[10:20], W[10:20] = (1, 2), (1, 1)        # x + 3e38 twice: +Inf, never NaN
            mv, _ = skin_model.skin_arrays(mats, v, J, W, n)
            assert np.isposinf(mv[10:20, 0]).all() and not np.isnan(mv).any() and np.isinf(mv).sum() == 10
            for g in (a, b):
                g.set_mesh_skin(prim, J, W)
            a.pose_mesh(prim, mats)
            pose_dev(b, up, prim, mats)
    dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


def test_a_seventy_primitive_scene_and_a_stale_mirror():
    desc, a, b = pair(desc=seventy_prims())
    prim = 7
    v, n = desc.ops[3 + prim][1:3]
    J, W = binding(len(v), 4, seed=70)
    dP, dN = targets(len(v), 3, 70, extent=3.0), targets(len(n), 3, 71, extent=5.0)
    mats = np.stack([EYE] * 3)
    mats[0, :3, 3] = [4.5, 3.0, -8.0]
    mats[1, :3, 3] = [4.0, 3.5, -8.0]
    mats[2, :3, 3] = [4.5, 2.5, -7.0]
    w = weights(3, 7, [0, 2])
    for g in (a, b):
        g.set_mesh_skin(prim, J, W)
        g.set_mesh_morph_targets(prim, dP, dN)
    before = dc.snapshot(b, desc, [prim])
    with Uploads(b.ctx) as up:
        a.morph_mesh(prim, w, mats)
        morph_dev(b, up, prim, w, mats)
    sb = dc.snapshot(b, desc, [prim])
    dc.assert_same(dc.snapshot(a, desc, [prim]), sb)
    assert sb["render"] != before["render"]
    # a REBUILD of another mesh re-flattens every mesh from the mirror: the deformed arrays must be in it
    u = desc.ops[3 + 20][1] * F(1.25)
    for g in (a, b):
        g.update_mesh(20, u, desc.ops[3 + 20][2], "rebuild")
    dc.assert_same(dc.snapshot(a, desc, [prim, 20]), dc.snapshot(b, desc, [prim, 20]))
    a.close()
    b.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def refusal(fn, call):
    """the text of the refusal behind the function's name"""
    with pytest.raises(ag.AgptError) as e:
        call()
    msg, marker = str(e.value), fn + ": "
    assert marker in msg, msg
    return msg.split(marker, 1)[1]


def test_pose_refusals_are_the_host_calls_and_change_nothing():
    desc, a, b = pair()
    prim, n_joints = dc.GRID1_N, 100
    used = np.array([0, 50, 99], np.int32)
    J, W = binding(len(dc.zoo_arrays(prim)[0]), 4, seed=prim)
    good, _ = dic.joints(n_joints, seed=1)
    good[used] = palette(prim, 0)
    with Uploads(b.ctx) as up:
        assert "has no skin" in refusal("agpt_scene_pose_mesh_device", lambda: pose_dev(b, up, prim, good))
        for g in (a, b):
            g.set_mesh_skin(prim, used[J], W, n_joints=n_joints)
        a.pose_mesh(prim, good)
        pose_dev(b, up, prim, good)
        before = dc.snapshot(b, desc, dc.PRIMS)
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), before)

        def both(mats, expect, mode="refit"):
            host = refusal("agpt_scene_pose_mesh", lambda: a.pose_mesh(prim, mats, mode))
            dev = refusal("agpt_scene_pose_mesh_device", lambda: pose_dev(b, up, prim, mats, mode))
            assert host == dev and expect in dev, (host, dev)
            dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), before)

        m = good.copy()
        m[5, 3, 3], m[9, 1, 1] = 2, np.nan
        both(m, "joint 9 has a non-finite entry")                 # a non-finite entry in any joint before any last row
        m = good.copy()
        m[3], m[7, 3, 2] = dic.joint_of(dic.ZERO_DET, None), F(1e-30)
        both(m, "the last row of joint 7 is not (0, 0, 0, 1)")    # a last row before a determinant
        m = good.copy()
        m[80, 0, 3], m[66, 2, 2] = np.inf, -np.inf                # two of a kind, in different waves
        both(m, "joint 66 has a non-finite entry")
        m = good.copy()
        m[90, 3, 3], m[12, 3, 0] = 0, 1
        both(m, "the last row of joint 12")
        m = good.copy()
        m[97] = m[20] = dic.joint_of(dic.ZERO_DET, None)
        for mode in ("refit", "rebuild"):
            both(m, "joint 20 is singular (its determinant is exactly 0)", mode)
        both(good[:99], "n_joints is 99, the skin was set with 100")
        text = refusal("agpt_scene_pose_mesh_device", lambda: b.pose_mesh_device(prim, None, n_joints))
        assert a.L.agpt_scene_pose_mesh(a.h, prim, None, n_joints, 0) == -1
        assert text == a.L.agpt_last_error().decode().split("agpt_scene_pose_mesh: ", 1)[1]
        text = refusal("agpt_scene_pose_mesh_device", lambda: b.pose_mesh_device(prim, up(good, offset=4), n_joints))
        assert "not 16-byte aligned" in text
        with pytest.raises(ValueError, match="unknown mode"):
            b.pose_mesh_device(prim, up(good), n_joints, "refresh")
        dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), before)
        pose_dev(b, up, prim, good)                               # and the call still works
        dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), before)
    a.close()
    b.close()


def test_morph_refusals_are_the_host_calls_and_change_nothing():
    desc, a, b = pair()
    prim, T = dc.GRID4_N, 300
    act = [0, 150, 299]
    good_w = weights(T, prim, act)
    good_m = palette(prim, 0)
    with Uploads(b.ctx) as up:
        assert "has no morph targets" in refusal("agpt_scene_morph_mesh_device", lambda: morph_dev(b, up, prim, good_w))
        for g in (a, b):
            morph_targets(g, prim, T)
        a.morph_mesh(prim, good_w)
        morph_dev(b, up, prim, good_w)
        before = dc.snapshot(b, desc, dc.PRIMS)
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), before)

        def both(w, mats, expect):
            host = refusal("agpt_scene_morph_mesh", lambda: a.morph_mesh(prim, w, mats))
            dev = refusal("agpt_scene_morph_mesh_device", lambda: morph_dev(b, up, prim, w, mats))
            assert host == dev and expect in dev, (host, dev)
            dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), before)

        nan = good_w.copy()
        nan[280], nan[70] = np.nan, -np.inf                       # two, in different waves
        both(nan, None, "non-finite weight (target 70)")
        both(nan, good_m, "non-finite weight (target 70)")        # the weights before the skin ...
        both(good_w, good_m, "has no skin")                       # ... which comes before the matrices
        both(good_w[:299], None, "n_targets is 299, the targets were set with 300")
        for g in (a, b):
            skin_of(g, prim)
        both(nan, good_m[:2], "non-finite weight (target 70)")    # the weights before the count of the joints
        both(good_w, good_m[:2], "n_joints is 2, the skin was set with 3")
        bad = good_m.copy()
        bad[0, 3, 3], bad[1, 2, 2] = 2, np.nan
        both(nan, bad, "non-finite weight (target 70)")           # the weights before the joints
        both(good_w, bad, "joint 1 has a non-finite entry")
        bad[1, 2, 2] = 1
        both(good_w, bad, "the last row of joint 0")
        bad = good_m.copy()
        bad[2] = dic.joint_of(dic.ZERO_DET, None)
        both(good_w, bad, "joint 2 is singular")
        assert "NULL weights" in refusal("agpt_scene_morph_mesh_device", lambda: b.morph_mesh_device(prim, None, T))
        text = refusal("agpt_scene_morph_mesh_device", lambda: b.morph_mesh_device(prim, up(good_w), T, up(good_m, offset=8), 3))
        assert "not 16-byte aligned" in text
        dc.assert_same(dc.snapshot(b, desc, dc.PRIMS), before)
        a.morph_mesh(prim, good_w, good_m)
        morph_dev(b, up, prim, good_w, good_m)                    # and the calls still work; weights need 4-byte alignment only
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        b.morph_mesh_device(prim, up(good_w, offset=4), T)
        a.morph_mesh(prim, good_w)
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
    a.close()
    b.close()


# ---- Python: torch tensors ---------------------------------------------------------------------------------------------------

TORCH_CHILD = r"""
import contextlib
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch                      # before the library touches the GPU (INTEGRATION.md section 3)
import numpy as np
torch.zeros(1, device="cuda")
import ag_pathtracer_amd as ag
import device_update_cases as dc
from morph_cases import weights

ag.lib()
with open("/proc/self/maps") as f:
    runtimes = sorted({ln.split(None, 5)[5].strip() for ln in f if "libamdhip64" in ln and len(ln.split(None, 5)) == 6})
assert len(runtimes) == 1, "torch and libagpt_hip.so are bound to different HIP runtime copies: a torch stream is no handle for the library"

waits = [0]
stream_synchronize = torch.cuda.Stream.synchronize
def counted(self):
    waits[0] += 1
    return stream_synchronize(self)
torch.cuda.Stream.synchronize = counted

desc = dc.zoo_scene()
prims = (dc.GRID1_N, dc.GRID4, dc.PRIMS[0])
for own_stream in (False, True):
    # own_stream: the context runs on a stream of torch's pool (non-blocking) and the tensors are produced on it, with no wait in between
    s = torch.cuda.Stream() if own_stream else None
    ctx = ag.Context(0, stream=s.cuda_stream if own_stream else None)
    assert (ctx.stream != 0) == own_stream
    with (torch.cuda.stream(s) if own_stream else contextlib.nullcontext()):
        a, b = desc.instantiate(ag.Scene(ctx)), desc.instantiate(ag.Scene(ctx))
        for g in (a, b):
            for prim in prims:
                dc.skin_of(g, prim)
                dc.morph_targets(g, prim)
        waits[0] = 0
        for prim in prims:
            m = dc.palette(prim, 1)
            a.pose_mesh(prim, m)
            tm = torch.from_numpy(m).cuda() * 1.0          # produced on torch's current stream
            b.pose_mesh(prim, tm)
            tm.fill_(float("nan"))
        assert waits[0] == (0 if own_stream else 3), waits
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        for k, prim in enumerate(prims):
            m, w = dc.palette(prim, 0), weights(3, prim, [0, 2])
            a.morph_mesh(prim, w, m)
            tw = torch.from_numpy(w).cuda() * 1.0
            tm = torch.from_numpy(m.reshape(3, 16)).cuda() * 1.0                # (the other accepted shape)
            # both on the device; then one of the two on the host: uploaded by the wrapper
            b.morph_mesh(prim, *((tw, tm), (tw, m), (w, tm))[k])
            tw.fill_(float("nan"))
            tm.fill_(float("nan"))
        dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        a.morph_mesh(prims[0], weights(3, 9, [1]))
        b.morph_mesh(prims[0], torch.from_numpy(weights(3, 9, [1])).cuda())       # no matrices
        dc.assert_same(dc.snapshot(a, desc, [prims[0]]), dc.snapshot(b, desc, [prims[0]]))
        # a CPU tensor or an ndarray still takes the host call: its refusal carries the host call's name
        m = dc.palette(prims[0], 1)
        a.pose_mesh(prims[0], m)
        b.pose_mesh(prims[0], torch.from_numpy(m))
        dc.assert_same(dc.snapshot(a, desc, [prims[0]]), dc.snapshot(b, desc, [prims[0]]))
        for x in (m[:2], torch.from_numpy(m[:2])):
            try:
                b.pose_mesh(prims[0], x)
            except ag.AgptError as e:
                assert "agpt_scene_pose_mesh:" in str(e)
            else:
                raise AssertionError("accepted two joints")
        try:
            b.pose_mesh(prims[0], torch.from_numpy(m[:2]).cuda())
        except ag.AgptError as e:
            assert "agpt_scene_pose_mesh_device:" in str(e)
        else:
            raise AssertionError("accepted two joints")
        before = dc.snapshot(b, desc, [prims[0]])
        tm, tw = torch.from_numpy(m).cuda(), torch.from_numpy(weights(3, 1, [0])).cuda()
        bad_m = [tm.double(), tm.half(), tm.reshape(-1), tm.reshape(4, 12), tm.transpose(1, 2), torch.empty(tm.shape, device="meta")]
        bad_w = [tw.double(), tw.reshape(3, 1), torch.cat([tw, tw])[::2], torch.empty(tw.shape, device="meta")]
        for call, what in [(lambda x: b.pose_mesh(prims[0], x), bad_m), (lambda x: b.morph_mesh(prims[0], tw, x), bad_m),
                           (lambda x: b.morph_mesh(prims[0], x, tm), bad_w), (lambda x: b.morph_mesh(prims[0], x), bad_w)]:
            for x in what:
                try:
                    call(x)
                except ValueError as e:
                    assert "pose_mesh" in str(e) or "morph_mesh" in str(e)
                else:
                    raise AssertionError("accepted %%s %%s %%s" %% (x.dtype, tuple(x.shape), x.device))
        dc.assert_same(dc.snapshot(b, desc, [prims[0]]), before)
        torch.cuda.current_stream().synchronize()
        a.close(); b.close(); ctx.close()
print("torch-ok")
"""


def test_torch_device_tensors_equal_ndarrays():
    """Scene.pose_mesh and Scene.morph_mesh with torch tensors on the GPU against the ndarray calls -- once with the context on a
    torch.cuda.Stream() that also produces the tensors, which needs no wait --; a CPU tensor and an ndarray take the host call; a wrong
    device, dtype, shape or layout raises ValueError.  In a child process: torch must initialise the GPU before the library does."""
    code = TORCH_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "torch-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
