"""CPU checks of the temporal reprojection (agpt_camera_vectors, agpt_temporal_accumulate): symbols and struct layout, every
argument check in the header's order (those before the context is looked at, with a NULL context), the new unit's cross-compiled
resources, agpt_camera_vectors against the oracle's camera, and self-checks of the numpy model (tests/temporal_model.py)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np

import ag_pathtracer_amd as ag
import temporal_model as tm
from helpers import assert_exported, struct_layout
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agpt_build", os.path.join(ROOT, "ag-pathtracer_amd", "build.py"))
b = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(b)
F = np.float32
INVALID = -1
CAM_A = ([0.3, 1.4, -6.0], [0, 0, 0], [0, 1, 0], 37 / 29., 42.0, 0.0)
CAM_B = ([0.5, 1.3, -5.8], [0.1, 0, 0], [0, 1, 0], 37 / 29., 42.0, 0.0)


def test_symbols_declared_and_exported():
    assert_exported(("agpt_camera_vectors", "agpt_temporal_accumulate"))
    header = open(os.path.join(ROOT, "include", "agpt.h")).read()
    assert "agpt_temporal.hip" in b.SOURCES
    assert "agpt_temporal.h" in b.HEADERS
    for macro, value, model in (("AGPT_TEMPORAL_DEPTH_TOL", ag.TEMPORAL_DEPTH_TOL, tm.DEPTH_TOL),
                                ("AGPT_TEMPORAL_NORMAL_COS", ag.TEMPORAL_NORMAL_COS, tm.NORMAL_COS),
                                ("AGPT_TEMPORAL_MIN_WEIGHT", ag.TEMPORAL_MIN_WEIGHT, tm.MIN_WEIGHT)):
        assert float(re.search(r"#define %s ([0-9.e-]+)f" % macro, header).group(1)) == value == model


def test_struct_layout_matches_ctypes(tmp_path):
    struct_layout(tmp_path, {"agpt_temporal_params": ag.TemporalParams})


def params(**kw):
    f = dict(width=37, height=29, cam_cur=ag.camera_desc(*CAM_A), cam_prev=ag.camera_desc(*CAM_B), max_history=32.0,
             depth_tol=ag.TEMPORAL_DEPTH_TOL, normal_cos=ag.TEMPORAL_NORMAL_COS)
    f.update(kw)
    return ag.TemporalParams(**f)


def call(L, ctx, p, ptrs):
    return L.agpt_temporal_accumulate(ctx, C.byref(p) if p is not None else None, *[C.c_void_p(v) if v else None for v in ptrs])


def test_invalid_arguments_in_the_stated_order():
    """Checks 1-5 come before the context is looked at: a NULL context and NULL buffers reach them.  Each case breaks one rule and
    every later one too (NULL context, NULL buffers), so the message names the FIRST that applies."""
    L = ag.lib()
    nothing = [0] * 10
    nan, inf = float("nan"), float("inf")
    assert call(L, None, None, nothing) == INVALID                                         # 1
    assert b"agpt_temporal_accumulate: NULL" in L.agpt_last_error()
    cases = [(dict(width=0), b"film"), (dict(height=-3), b"film"), (dict(width=1 << 16, height=1 << 16), b"film"),          # 2
             (dict(max_history=0.0), b"max_history"), (dict(max_history=-1.0), b"max_history"), (dict(max_history=inf), b"max_history"),
             (dict(max_history=nan), b"max_history"),                                                                         # 3
             (dict(depth_tol=-0.01), b"depth_tol"), (dict(depth_tol=inf), b"depth_tol"), (dict(depth_tol=nan), b"depth_tol"),  # 4
             (dict(normal_cos=1.5), b"normal_cos"), (dict(normal_cos=-1.01), b"normal_cos"), (dict(normal_cos=nan), b"normal_cos")]  # 5
    for change, word in cases:
        assert call(L, None, params(**change), nothing) == INVALID, change
        msg = L.agpt_last_error()
        assert b"agpt_temporal_accumulate" in msg and word in msg, (change, msg)
    # the order among 2-5: an earlier broken rule wins over a later one
    for change, word in ((dict(width=0, max_history=0.0, depth_tol=-1.0, normal_cos=2.0), b"film"),
                         (dict(max_history=0.0, depth_tol=-1.0, normal_cos=2.0), b"max_history"),
                         (dict(depth_tol=-1.0, normal_cos=2.0), b"depth_tol")):
        assert call(L, None, params(**change), nothing) == INVALID
        assert word in L.agpt_last_error(), (change, L.agpt_last_error())
    # the limits themselves are accepted: the call then stops at the NULL context (6)
    for change in (dict(depth_tol=0.0), dict(normal_cos=1.0), dict(normal_cos=-1.0), dict(max_history=1e-30), dict()):
        assert call(L, None, params(**change), nothing) == INVALID
        assert b"agpt_temporal_accumulate: NULL" in L.agpt_last_error(), change
    # 6 before 7 and 8: a NULL context with partly-NULL prev pointers and aliased buffers is still "NULL argument" (the
    # addresses are never dereferenced)
    fake = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0, 0, 0, 0x1000, 0x1000]
    assert call(L, None, params(), fake) == INVALID
    assert b"agpt_temporal_accumulate: NULL" in L.agpt_last_error()


def test_camera_vectors_argument_checks_and_layout():
    L = ag.lib()
    out = np.zeros(22, F)
    assert L.agpt_camera_vectors(None, out.ctypes.data_as(C.POINTER(C.c_float))) == INVALID
    assert b"agpt_camera_vectors" in L.agpt_last_error()
    assert L.agpt_camera_vectors(C.byref(ag.camera_desc(*CAM_A)), None) == INVALID
    v = ag.camera_vectors(CAM_A)
    assert v.dtype == F and v.shape == (22,)
    c = tm.camera(v)
    assert c["origin"].tobytes() == np.asarray(CAM_A[0], F).tobytes()
    for a in ("u", "v", "w"):
        assert abs(float(np.linalg.norm(c[a].astype(np.float64))) - 1) < 1e-6
    assert abs(float(np.dot(c["u"].astype(np.float64), c["w"]))) < 1e-6
    assert v[21] == 0
    assert ag.camera_vectors(CAM_A[:5] + (0.25,))[21] == F(0.125)       # lens_radius = aperture / 2
    assert ag.camera_vectors(ag.camera_desc(*CAM_A)).tobytes() == v.tobytes()


def test_camera_vectors_match_the_oracle_camera():
    """normalize(llc + s*hor + t*ver - origin) from the 22 floats equals the direction of the oracle's camera_ray for an aperture-0
    camera, bit for bit after the library's second normalisation (k_feature_rays normalises what Ray's ctor normalised)."""
    n = 0
    for cam in (CAM_A, CAM_B, ([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.0),
                ([3.0, -2.0, 7.5], [0.2, 0.4, -1.0], [0.1, 1, 0.05], 16 / 9., 63.5, 0.0)):
        c = tm.camera(ag.camera_vectors(cam))
        o = ob.OracleScene()
        o.set_camera(*cam)
        zero = c["u"] * F(0) + c["v"] * F(0)
        for s in np.linspace(0, 1, 9, dtype=F):
            for t in np.linspace(0, 1, 7, dtype=F):
                ray, _ = o.camera_ray(float(s), float(t))
                assert np.asarray(ray["o"], F).tobytes() == (c["origin"] + zero).tobytes()
                pixel = (c["llc"] + s * c["horizontal"]) + t * c["vertical"]
                once = tm.normalize(((pixel - c["origin"]) - zero).astype(F))
                assert once.astype(F).tobytes() == np.asarray(ray["d"], F).tobytes(), (cam, s, t)
                assert tm.normalize(once).tobytes() == tm.normalize(np.asarray(ray["d"], F)).tobytes()
                n += 1
    assert n == 4 * 63


def test_feature_directions_are_the_pixel_centre_rays_of_the_oracle():
    W, H = 37, 29
    o = ob.OracleScene()
    o.set_camera(*CAM_A)
    D = tm.feature_directions(ag.camera_vectors(CAM_A), W, H)
    assert D.shape == (H, W, 3) and D.dtype == F
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (17, 11), (5, 23)):
        s, t = (F(x) + F(0.5)) / F(W), (F(y) + F(0.5)) / F(H)
        ray, _ = o.camera_ray(float(s), float(t))
        assert D[H - 1 - y, x].tobytes() == tm.normalize(np.asarray(ray["d"], F)).tobytes(), (x, y)


PLAIN_KERNELS = ("k_temporal", "k_temporal_motion", "k_temporal_surface")
CLAMP_KERNELS = ("k_temporal_clamp", "k_temporal_clamp_surface")
LDS_BYTES = (64 + 2 * 3) * (4 + 2 * 3) * 16      # AGPT_TC_LDS_BYTES: the 64 x 4 tile plus a halo of 3, one float4 a pixel


def test_temporal_unit_compiles_to_its_five_kernels_with_the_stated_resources():
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "agpt_temporal.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + b.SOURCE_FLAGS.get("agpt_temporal.hip", []) + \
            ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out, os.path.join(b.CSRC, "agpt_temporal.hip")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
    # the remarks of one kernel follow its "Function Name" remark; the name is the first component of the mangled one
    usage = {}
    for part in p.stderr.split("remark: Function Name: ")[1:]:
        mangled = part.split()[0]
        n = re.match(r"_Z(\d+)", mangled)
        name = mangled[n.end():n.end() + int(n.group(1))]
        assert name not in usage, name
        usage[name] = {what: int(re.search(re.escape(what) + r": (\d+)", part).group(1))
                       for what in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")}
    assert sorted(usage) == sorted(PLAIN_KERNELS + CLAMP_KERNELS), sorted(usage)
    for name, u in usage.items():
        for what in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
            assert u[what] == 0, (name, what, u[what])
        assert u["LDS Size [bytes/block]"] == (LDS_BYTES if name in CLAMP_KERNELS else 0), (name, u)
    assert LDS_BYTES == 11200
    assert re.search(r"#define AGPT_TC_LDS_BYTES \(AGPT_TC_TILE_W \* AGPT_TC_TILE_H \* 16\)", open(os.path.join(b.CSRC, "agpt_temporal.h")).read())
    assert "-ffp-contract=off" in flags and not b.SOURCE_FLAGS.get("agpt_temporal.hip")
    # what DESIGN.md section 5.5.3 states
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("5.5.3"):]
    assert "%d B" % LDS_BYTES in section
    assert "%d waves per SIMD" % usage["k_temporal_clamp"]["Occupancy [waves/SIMD]"] in section


# ---- the model on hand-made buffers ------------------------------------------------------------------------------------
H, W = 29, 37


def frame(seed, t=5.0):
    rng = np.random.RandomState(seed)
    accum = np.zeros((H, W, 4), F)
    accum[..., :3] = rng.uniform(0, 8, (H, W, 3))
    accum[..., 3] = 4
    m2 = rng.uniform(0, 30, (H, W)).astype(F)
    albedo = np.ones((H, W, 4), F)
    nd = np.zeros((H, W, 4), F)
    nd[..., 1] = 1
    nd[..., 3] = t
    return accum, m2, albedo, nd


def test_model_first_frame_returns_the_current_buffers():
    accum, m2, albedo, nd = frame(1)
    va = ag.camera_vectors(CAM_A)
    out, mo = tm.accumulate(va, va, accum, m2, albedo, nd, None)
    assert out.tobytes() == accum.tobytes() and mo.tobytes() == m2.tobytes()


def test_model_identical_camera_bytes_take_the_identity_path():
    accum, m2, albedo, nd = frame(1)
    h_acc, h_m2, _, _ = frame(2)
    h_acc[..., 3] = 8
    va = ag.camera_vectors(CAM_A)
    out, mo, masks = tm.accumulate(va, va.copy(), accum, m2, albedo, nd, (h_acc, h_m2, albedo, nd), max_history=1e9, return_masks=True)
    # every pixel reads its own history pixel with weight 1: no position arithmetic, nothing off the film
    assert masks["found"].all() and not masks["fx"].any() and not masks["fy"].any()
    assert masks["used"][0].all() and not any(m.any() for m in masks["used"][1:])
    assert masks["te"].tobytes() == nd[..., 3].tobytes()
    assert (out[..., 3] == 12).all()
    assert out[..., :3].tobytes() == (accum[..., :3] + (h_acc[..., :3] / F(8)) * F(8)).tobytes()
    assert mo.tobytes() == (m2 + (h_m2 / F(8)) * F(8)).tobytes()
    # the reprojection arithmetic of the same camera pair lands within a rounding of the pixel centre instead: not the same path
    _, _, general = tm.accumulate(va, va.copy(), accum, m2, albedo, nd, (h_acc, h_m2, albedo, nd), identity=False, return_masks=True)
    assert general["fx"].any() or general["fy"].any()


def test_model_inconsistent_depth_everywhere_returns_the_current_buffers():
    accum, m2, albedo, nd = frame(1)
    h_acc, h_m2, _, _ = frame(2)
    p_nd = nd.copy()
    p_nd[..., 3] *= 2                      # every surface was twice as far away: nothing passes the 5 % test
    for cams in ((CAM_A, CAM_A), (CAM_A, CAM_B)):
        va, vb = ag.camera_vectors(cams[0]), ag.camera_vectors(cams[1])
        out, mo, masks = tm.accumulate(va, vb, accum, m2, albedo, nd, (h_acc, h_m2, albedo, p_nd), return_masks=True)
        assert out.tobytes() == accum.tobytes() and mo.tobytes() == m2.tobytes()
        assert not masks["history"].any() and any(m.any() for m in masks["depth_out"])


def test_model_cap_and_empty_current_pixels():
    accum, m2, albedo, nd = frame(1)
    accum[3, 4] = 0
    m2[3, 4] = 0
    h_acc, h_m2, _, _ = frame(2)
    h_acc[..., 3] = 8
    va = ag.camera_vectors(CAM_A)
    out, mo = tm.accumulate(va, va, accum, m2, albedo, nd, (h_acc, h_m2, albedo, nd), max_history=2.0)
    assert (out[..., 3] == accum[..., 3] + 2).all()
    # a pixel without samples of its own takes the history alone
    assert out[3, 4, 3] == 2 and out[3, 4, :3].tobytes() == ((h_acc[3, 4, :3] / F(8)) * F(2)).tobytes()
