"""CPU checks of the feature buffers and the denoiser (agpt_render_features, agpt_denoise): symbols and struct layout, argument
checks that need no GPU, the new unit's cross-compiled resources, the numpy model of the contract (tests/denoise_model.py) on
hand-made buffers, and the model on an oracle render of C1 -- the input the GPU quality test uses."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import numpy as np

import adaptive_model as am
import ag_pathtracer_amd as ag
import denoise_model as dm
from denoise_features import host_features
from helpers import assert_exported, oracle_scene, struct_layout
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("agpt_build", os.path.join(ROOT, "ag-pathtracer_amd", "build.py"))
b = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(b)
F = np.float32
INVALID = -1


def test_symbols_declared_and_exported():
    assert_exported(("agpt_render_features", "agpt_denoise"))
    header = open(os.path.join(ROOT, "include", "agpt.h")).read()
    assert "agpt_denoise.hip" in b.SOURCES
    assert "agpt_denoise.h" in b.HEADERS
    # the defaults the binding and the model carry are the header's
    for macro, value in (("AGPT_DENOISE_SIGMA_Z", ag.DENOISE_SIGMA_Z), ("AGPT_DENOISE_SIGMA_N", ag.DENOISE_SIGMA_N),
                         ("AGPT_DENOISE_SIGMA_L", ag.DENOISE_SIGMA_L)):
        assert float(re.search(r"#define %s ([0-9.]+)f" % macro, header).group(1)) == value
    assert (dm.SIGMA_Z, dm.SIGMA_N, dm.SIGMA_L) == (ag.DENOISE_SIGMA_Z, ag.DENOISE_SIGMA_N, ag.DENOISE_SIGMA_L)


def test_struct_layout_matches_ctypes(tmp_path):
    struct_layout(tmp_path, {"agpt_denoise_params": ag.DenoiseParams})


def test_invalid_arguments_without_a_gpu():
    L = ag.lib()
    good = dict(width=64, height=32, iterations=5, demodulate=1, sigma_z=1.0, sigma_n=0.25, sigma_l=4.0)
    # NULL everything
    assert L.agpt_denoise(None, None, None, None, None, None, None) == INVALID
    assert b"agpt_denoise" in L.agpt_last_error()
    # valid parameters, NULL context and buffers
    assert L.agpt_denoise(None, C.byref(ag.DenoiseParams(**good)), None, None, None, None, None) == INVALID
    assert b"agpt_denoise: NULL" in L.agpt_last_error()
    for change, word in ((dict(iterations=0), b"iterations"), (dict(iterations=9), b"iterations"), (dict(sigma_z=0.0), b"sigma"),
                         (dict(sigma_n=-1.0), b"sigma"), (dict(sigma_l=0.0), b"sigma"), (dict(sigma_l=float("nan")), b"sigma"),
                         (dict(width=0), b"film"), (dict(demodulate=2), b"demodulate")):
        p = ag.DenoiseParams(**dict(good, **change))
        assert L.agpt_denoise(None, C.byref(p), None, None, None, None, None) == INVALID, change
        msg = L.agpt_last_error()
        assert b"agpt_denoise" in msg and word in msg, (change, msg)

    def rp(**kw):
        f = dict(width=64, height=32, x0=0, y0=0, w=64, h=32, spp_begin=0, spp_count=0, seed_base=0, max_depth=5, accum_pitch=64)
        f.update(kw)
        return ag.RenderParams(**f)
    assert L.agpt_render_features(None, None, None, None) == INVALID
    assert b"agpt_render_features" in L.agpt_last_error()
    assert L.agpt_render_features(None, C.byref(rp()), None, None) == INVALID
    assert b"agpt_render_features: NULL" in L.agpt_last_error()
    for change, word in ((dict(spp_count=4), b"spp_count"), (dict(spp_begin=1), b"spp_begin"),
                         (dict(interleave_block=8, interleave_world=2, interleave_rank=1), b"interleave"),
                         (dict(interleave_world=2), b"interleave")):
        assert L.agpt_render_features(None, C.byref(rp(**change)), None, None) == INVALID, change
        msg = L.agpt_last_error()
        assert b"agpt_render_features" in msg and word in msg, (change, msg)


def test_denoise_unit_compiles_without_scratch():
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "agpt_denoise.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + b.SOURCE_FLAGS.get("agpt_denoise.hip", []) + \
            ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", out, os.path.join(b.CSRC, "agpt_denoise.hip")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"remark: Function Name: (\S+)", p.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    assert len(names) == len(scratch) and len(names) >= 4
    for k in ("k_feature_rays", "k_features", "k_denoise_prepare", "k_denoise_pass"):
        assert any(k in n for n in names), (k, names)
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))


# ---- the model on hand-made buffers ------------------------------------------------------------------------------------
H, W = 24, 40


def flat_features(h=H, w=W, t=5.0, color=(0.5, 0.5, 0.5)):
    albedo = np.zeros((h, w, 4), F)
    albedo[..., :3] = color
    albedo[..., 3] = 1
    nd = np.zeros((h, w, 4), F)
    nd[..., 1] = 1
    nd[..., 3] = t
    return albedo, nd


def buffers(mean, n, var_of_mean=0.0):
    """accum / moment2 of pixels with `n` samples whose mean radiance is `mean`[H, W, 3] and whose estimate of the variance of
    the mean luminance is about var_of_mean"""
    mean = np.asarray(mean, np.float64)
    n = np.broadcast_to(np.asarray(n, np.float64), mean.shape[:2])
    accum = np.zeros(mean.shape[:2] + (4,), F)
    accum[..., :3] = mean * n[..., None]
    accum[..., 3] = n
    mu = am.luminance(mean.astype(F)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m2 = n * (np.asarray(var_of_mean, np.float64) * (n - 1) + mu * mu)   # inverts v = (m2/n - mu^2) * n/(n-1) / n
    return accum, np.nan_to_num(m2).astype(F)


def test_model_constant_image_stays_constant():
    albedo, nd = flat_features()
    mean = np.broadcast_to(np.array([0.7, 0.3, 0.2]), (H, W, 3))
    for var in (0.0, 1e-3):
        for demod in (False, True):
            accum, m2 = buffers(mean, 16, var)
            out = dm.denoise(accum, m2, albedo, nd, 5, demod)
            assert np.allclose(out[..., :3], mean, rtol=1e-6, atol=0), (var, demod)
            assert (out[..., 3] == 1).all()


def test_model_edges_stop_the_filter():
    mean = np.zeros((H, W, 3))
    mean[:, W // 2:] = [0.9, 0.5, 0.1]
    accum, m2 = buffers(mean, 8, 0.0)
    # (a) a flag step, (b) a depth step, (c) a normal step along the colour edge; radiance alone separates them too (v = 0)
    for kind in ("flag", "depth", "normal", "radiance"):
        albedo, nd = flat_features(color=(1, 1, 1))
        if kind == "flag":
            albedo[:, W // 2:, 3] = 2
        elif kind == "depth":
            nd[:, W // 2:, 3] = 50.0
        elif kind == "normal":
            nd[:, W // 2:, :3] = (1, 0, 0)
        out = dm.denoise(accum, m2, albedo, nd, 5, False)
        assert (out[:, :W // 2, :3] == 0).all(), kind
        assert np.allclose(out[:, W // 2:, :3], mean[:, W // 2:], rtol=1e-6, atol=0), kind
    # the cross-edge weights are exactly zero
    albedo, nd = flat_features()
    nd[:, W // 2:, 3] = 50.0
    c, v = dm.prepare(accum, m2, albedo, False)
    _, _, w = dm.run_pass(c, v, albedo, nd, 1, return_weights=True)
    w = w.reshape(5, 5, H, W)
    assert (w[:, 3:, :, W // 2 - 1] == 0).all() and (w[:, :2, :, W // 2] == 0).all()
    assert (w[2, 2] == F(0.375) * F(0.375)).all()   # the centre tap has w = h


def test_model_pixels_without_samples_are_excluded():
    albedo, nd = flat_features()
    mean = np.broadcast_to(np.array([0.4, 0.5, 0.6]), (H, W, 3))
    n = np.full((H, W), 8.0)
    n[5, 7] = 0
    n[10:14, 20:23] = 0
    accum, m2 = buffers(mean, n, 1e-4)
    accum[5, 7, :3] = 1e6       # whatever the sums of such a pixel hold does not leak
    out = dm.denoise(accum, m2, albedo, nd, 4, True)
    empty = n == 0
    assert (out[empty][:, :3] == 0).all() and (out[..., 3] == 1).all()
    assert np.allclose(out[~empty][:, :3], mean[~empty], rtol=1e-6, atol=0)
    # one sample: kept, with v = 0
    n[:] = 1
    accum, m2 = buffers(mean, n, 0.0)
    c, v = dm.prepare(accum, m2, albedo, False)
    assert (v == 0).all()


def test_model_demodulation_round_trips_a_textured_albedo():
    rng = np.random.RandomState(5)
    albedo, nd = flat_features()
    albedo[..., :3] = rng.uniform(0.05, 1.0, (H, W, 3))     # a texture: every pixel its own colour
    irradiance = np.array([1.5, 1.2, 0.9])
    mean = albedo[..., :3].astype(np.float64) * irradiance
    accum, m2 = buffers(mean, 16, 1e-4)
    out = dm.denoise(accum, m2, albedo, nd, 5, True)
    assert np.allclose(out[..., :3], mean, rtol=2e-6, atol=0)
    # without demodulation the same filter blurs the texture
    plain = dm.denoise(accum, m2, albedo, nd, 5, False)
    assert np.abs(plain[..., :3] - mean).max() > 0.05


def test_model_variance_propagation_follows_the_b3_weights():
    # With every weight at w = h (sigma_l large enough that expc(-el) rounds to 1) a pass is the separable B3 filter, whose
    # weights sum to 1 per axis: i.i.d. noise of variance v comes out with v * sum(h^2) / sum(h)^2 = v * (sum k^2 / (sum k)^2)^2.
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    per_axis = (k ** 2).sum() / k.sum() ** 2
    assert abs(per_axis - 70.0 / 256.0) < 1e-15
    factor = per_axis ** 2
    h, w = 96, 96
    rng = np.random.RandomState(11)
    albedo, nd = flat_features(h, w)
    sigma2 = 0.01
    c = np.zeros((h, w, 3), F)
    c[...] = (0.5 + rng.normal(0, np.sqrt(sigma2), (h, w)))[..., None]     # grey: Y = c
    v = np.full((h, w), sigma2, F)
    c1, v1 = dm.run_pass(c, v, albedo, nd, 1, sigma_l=1e12)
    inner = (slice(2, -2), slice(2, -2))
    assert np.allclose(v1[inner], sigma2 * factor, rtol=1e-5)
    measured = c1[inner][..., 0].astype(np.float64).var()
    assert abs(measured / (sigma2 * factor) - 1) < 0.15, measured / (sigma2 * factor)
    # second pass (spacing 2): the taps of a pixel are independent again, the factor applies once more
    c2, v2 = dm.run_pass(c1, v1, albedo, nd, 2, sigma_l=1e12)
    inner = (slice(6, -6), slice(6, -6))
    assert np.allclose(v2[inner], sigma2 * factor * factor, rtol=1e-5)


# ---- the model on the oracle ---------------------------------------------------------------------------------------------
OW, OH = 96, 54
SPP, REF_SPP, REF_SEED = 16, 512, 0x5EED0001


def oracle_samples(desc, W, H, spp, seed_base=0, spp_begin=0):
    o = oracle_scene(desc, 5)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        acc, _ = o.render(W, H, spp, spp_begin=spp_begin, seed_base=seed_base, rng_mode=ob.RNG_PER_SAMPLE, threads=8)
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    return acc


def test_model_denoises_an_oracle_render_of_c1():
    desc = ag.scenes.scene_c1()
    cam = desc.camera
    desc.set_camera(cam[0], cam[1], cam[2], OW / float(OH), cam[4], cam[5])
    samples = np.stack([oracle_samples(desc, OW, OH, 1, spp_begin=s)[..., :3] for s in range(SPP)])
    r = am.run(samples, SPP, SPP, SPP, 0.0)
    accum = np.zeros((OH, OW, 4), F)
    accum[..., :3] = r["accum"]
    accum[..., 3] = r["counts"]
    assert accum[..., :3].tobytes() == oracle_samples(desc, OW, OH, SPP)[..., :3].tobytes()
    ref = oracle_samples(desc, OW, OH, REF_SPP, seed_base=REF_SEED)[..., :3] / F(REF_SPP)
    albedo, nd, _, hits = host_features(desc, OW, OH)
    assert len(np.unique(albedo[..., 3])) >= 2 and hits["hit"].any()
    raw = dm.display_rmse(accum[..., :3] / F(SPP), ref)
    for demod in (True, False):
        out = dm.denoise(accum, r["moment2"], albedo, nd, 5, demod)
        den = dm.display_rmse(out[..., :3], ref)
        print("C1 %dx%d %d spp: display RMSE raw %.5f, denoised %.5f (demodulate %d)" % (OW, OH, SPP, raw, den, demod))
        assert den < raw, (den, raw, demod)
