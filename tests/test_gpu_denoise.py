"""agpt_render_features and agpt_denoise on the GPU: the feature buffers against the CPU oracle (tests/denoise_features.py), the
filter against the numpy model of the contract (tests/denoise_model.py) on real render buffers, determinism, and the quality claim
(denoised display-range RMSE below the raw one against a 1024-spp reference).

Denoise against the model is expected bit-identical.  The one admitted source of difference is a double-rounding tie between the
device's and glibc's fp64 exp in expc(x) = (float)exp((double)x): about 2^-28 per call, well under one pixel per test film.  So at
most 4 pixels of a film may differ, each within rel 2^-18 (abs 1e-7) per channel -- one weight 1 fp32 ulp off, propagated through
five passes including the v -> el feedback."""
import copy

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import denoise_model as dm
from denoise_features import host_features, primitive_table
from helpers import compare_with_model, gpu_context, gpu_scene, scene_c1

pytestmark = pytest.mark.gpu
F = np.float32


def scene_c3_small():
    return ag.scenes.scene_c3(scale=0.05, aspect=160 / 90.)


def scene_mixed():
    """a plane, a mirror sphere, an emitter sphere, a diffuse-only sphere, a mesh with normals and one without, sky above;
    a lens (aperture 0.1) that the features must ignore"""
    d = ag.SceneDesc("features-mixed")
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, [0.55, 0.5, 0.45])
    mirror = d.add_material(ag.MAT_MIRROR, [0.9, 0.85, 0.8])
    red = d.add_material(ag.MAT_DISNEY, [0.8, 0.1, 0.123456789], 0.4, 0.0)
    blue = d.add_material(ag.MAT_DISNEY, [0.05, 0.2, 0.7], 0.7, 1.0)
    d.add_plane([0, -1, 0], [12, 12], grey)
    d.add_sphere([-1.6, 0.0, 0.3], 1.0, mirror)
    d.add_area_light([1.2, 1.8, 1.0], 0.5, [30, 28, 25])
    d.add_sphere([2.6, -0.4, -0.6], 0.6, grey)
    v, n, uv, idx = ag.scenes.blob_mesh(20, 14, center=(0.6, -0.2, -0.8), radius=0.7, seed=3)
    d.add_mesh(v, n, uv, idx, red, 1)
    v, n, uv, idx = ag.scenes.blob_mesh(12, 9, center=(-0.4, -0.5, -1.8), radius=0.45, seed=4)
    d.add_mesh(v, None, None, idx, blue, 1)
    d.add_uniform_infinite_light([.3, .35, .4])
    d.set_camera([0.3, 1.4, -6.0], [0, 0, 0], [0, 1, 0], 64 / 48., 42.0, 0.1)
    return d


SCENES = {"c1": (scene_c1, 64, 48), "c3_small": (scene_c3_small, 160, 90), "mixed": (scene_mixed, 64, 48)}
_CACHE = {}


def setup(name):
    """(desc, W, H, GPU scene, host albedo, host normal_depth, either-sign mask)"""
    if name not in _CACHE:
        make, W, H = SCENES[name]
        desc = make()
        _CACHE[name] = (desc, W, H, gpu_scene(desc)) + host_features(desc, W, H)
    return _CACHE[name][:7]


def sphere_pixels(name):
    """[H, W] in buffer order: pixels whose first hit is a sphere (emitter spheres included)"""
    desc, hits = _CACHE[name][0], _CACHE[name][7]
    prims, _ = primitive_table(desc)
    is_sphere = np.array([op[0] in ("sphere", "area_light") for op, _ in prims] + [False])   # (prim -1 = miss -> False)
    return is_sphere[hits["prim"]][::-1]


def normal_error(nd, exp_nd, either):
    """per pixel: max abs component difference of the shading normal (up to the sign for meshes without normals)"""
    err = np.abs(nd[..., :3].astype(np.float64) - exp_nd[..., :3]).max(-1)
    err_neg = np.abs(nd[..., :3].astype(np.float64) + exp_nd[..., :3]).max(-1)
    return np.where(either, np.minimum(err, err_neg), err)


def check_features(albedo, nd, exp_albedo, exp_nd, either, spheres):
    # flag and hit / miss, the material colour bit for bit, t bit for bit
    assert albedo.tobytes() == exp_albedo.tobytes()
    assert nd[..., 3].tobytes() == exp_nd[..., 3].tobytes()
    miss = exp_albedo[..., 3] == 0
    assert not nd[miss].any()
    # the shading normal of meshes and planes within abs 1e-5 of the expected one (spheres: test_features_sphere_normals)
    err = np.where(spheres, 0.0, normal_error(nd, exp_nd, either))
    print("shading normal of meshes and planes: max abs error %.3g" % err.max())
    assert err.max() <= 1e-5, (err.max(), np.argwhere(err > 1e-5)[:8])


@pytest.mark.parametrize("name", list(SCENES))
def test_features_match_the_oracle(name):
    desc, W, H, g, exp_albedo, exp_nd, either = setup(name)
    albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
    if name == "mixed":   # every flag, and both kinds of mesh, are in view
        assert set(np.unique(albedo[..., 3]).tolist()) == {0.0, 1.0, 2.0}
        assert either.any() and (~either & (exp_albedo[..., 3] == 1)).any()
    check_features(albedo, nd, exp_albedo, exp_nd, either, sphere_pixels(name))
    # no RNG: another seed_base gives the same bytes
    a2, n2 = ag.PathTracer(5).render_features_to_host(g, W, H, seed_base=0xDEADBEEF)
    assert a2.tobytes() == albedo.tobytes() and n2.tobytes() == nd.tobytes()


@pytest.mark.parametrize("name", ["c1", "mixed"])
def test_features_sphere_normals(name):
    """Spheres: ns within abs 1e-5 of (p - c) / r, p = o + t d with the oracle's t.

    The second figure printed is how far those hit points lie off the sphere, | |p - c| / r - 1 | (up to 4.86e-06 on C1, 2.22e-05
    on the mixed scene).  Sphere::Intersect's normalize(cross(dpdv, dpdu)) amplifies that distance by r^2 / (r^2 - z^2) near the poles
    of the sphere's z axis, where C1's camera looks: written into the buffer it missed this bound (6.14e-05 on C1, 1.78e-04 on the
    mixed scene), which is why k_features writes (p - c) / r itself for spheres."""
    desc, W, H, g, exp_albedo, exp_nd, either = setup(name)
    albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
    spheres = sphere_pixels(name)
    assert spheres.any()
    err = normal_error(nd, exp_nd, either)[spheres]
    off = np.abs(np.linalg.norm(exp_nd[..., :3].astype(np.float64), axis=-1) - 1.0)[spheres]
    print("%s: sphere shading normal max abs error %.3g over %d pixels; hit points off the sphere by up to %.3g (relative to r)"
          % (name, err.max(), spheres.sum(), off.max()))
    assert err.max() <= 1e-5, err.max()


def test_features_ignore_the_aperture():
    desc, W, H, g, exp_albedo, exp_nd, either = setup("mixed")
    assert desc.camera[5] == 0.1
    albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
    pin = copy.copy(desc)
    pin.camera = tuple(desc.camera[:5]) + (0.0,)
    gp = gpu_scene(pin)
    try:
        a0, n0 = ag.PathTracer(5).render_features_to_host(gp, W, H)
    finally:
        gp.close()
    assert a0.tobytes() == albedo.tobytes() and n0.tobytes() == nd.tobytes()


def test_features_tile_pitch_and_row0():
    desc, W, H, g, exp_albedo, exp_nd, either = setup("mixed")
    ctx = gpu_context()
    full_a, full_n = ag.PathTracer(5).render_features_to_host(g, W, H)
    x0, y0, w, h = 13, 9, 37, 22
    pitch = W + 5
    row0 = H - y0 - h            # the buffer's row 0 holds film row (H-1) - (y0+h-1)
    sentinel = np.full((h, pitch, 4), -7.0, F)
    pa, pn = ctx.alloc(sentinel.nbytes), ctx.alloc(sentinel.nbytes)
    try:
        ctx.upload(pa, sentinel)
        ctx.upload(pn, sentinel)
        ag.PathTracer(5).render_features(g, W, H, pa, pn, tile=(x0, y0, w, h), accum_pitch=pitch, accum_row0=row0)
        ta, tn = ctx.download(pa, (h, pitch, 4)), ctx.download(pn, (h, pitch, 4))
    finally:
        ctx.free(pa)
        ctx.free(pn)
    rows = slice(H - y0 - h, H - y0)
    assert ta[:, x0:x0 + w].tobytes() == full_a[rows, x0:x0 + w].tobytes()
    assert tn[:, x0:x0 + w].tobytes() == full_n[rows, x0:x0 + w].tobytes()
    outside = np.ones((h, pitch), bool)
    outside[:, x0:x0 + w] = False
    assert (ta[outside] == -7.0).all() and (tn[outside] == -7.0).all()


def test_features_bad_arguments():
    desc, W, H, g, _, _, _ = setup("c1")
    ctx = gpu_context()
    pa, pn = ctx.alloc(W * H * 16), ctx.alloc(W * H * 16)
    pt = ag.PathTracer(5)
    try:
        for kw in (dict(spp_count=1), dict(spp_begin=2), dict(interleave=(8, 2, 0)), dict(tile=(0, 0, W + 1, H)), dict(accum_pitch=W - 1)):
            with pytest.raises(ag.AgptError):
                pt.render_features(g, W, H, pa, pn, **kw)
            assert b"agpt_render_features" in ag.lib().agpt_last_error()
        with pytest.raises(ag.AgptError):
            pt.render_features(g, W, H, pa, 0)
        with pytest.raises(ag.AgptError):
            pt.render_features(g, W, H, pa, pa)
    finally:
        ctx.free(pa)
        ctx.free(pn)


# ---- the filter against the model -----------------------------------------------------------------------------------------
def render_inputs(name, kind):
    """accum / moment2 of a real render: uniform 8 or 16 spp, or an adaptive run with spread counts"""
    desc, W, H, g, _, _, _ = setup(name)
    pt = ag.PathTracer(5)
    if kind == "adaptive":
        for rel in (0.1, 0.2, 0.05, 0.3):
            acc, m2, _, _ = pt.render_adaptive_to_host(g, W, H, 4, 32, 4, rel, abs_floor=0.01)
            if len(np.unique(acc[..., 3])) >= 3:
                break
        assert len(np.unique(acc[..., 3])) >= 3
    else:
        acc, m2, _, _ = pt.render_adaptive_to_host(g, W, H, kind, kind, kind, 0.0)
        assert (acc[..., 3] == kind).all()
    return acc, m2


@pytest.mark.parametrize("name", ["c1", "c3_small"])
@pytest.mark.parametrize("kind", [8, 16, "adaptive"])
def test_denoise_matches_the_model(name, kind):
    desc, W, H, g, _, _, _ = setup(name)
    ctx = gpu_context()
    acc, m2 = render_inputs(name, kind)
    albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
    for iterations in (1, 5):
        for demod in (False, True):
            out = ctx.denoise_to_host(acc, m2, albedo, nd, iterations, demod)
            assert (out[..., 3] == 1).all()
            model = dm.denoise(acc, m2, albedo, nd, iterations, demod)
            compare_with_model(out, model, "%s %s iterations %d demodulate %d" % (name, kind, iterations, demod))


def test_denoise_excluded_pixels_and_other_sigmas():
    desc, W, H, g, _, _, _ = setup("c1")
    ctx = gpu_context()
    acc, m2 = render_inputs("c1", 8)
    acc = acc.copy()
    acc[5:9, 10:13] = 0.0          # pixels without samples
    acc[20, 31] = (3.0, 2.0, 1.0, 1.0)   # one sample: kept, v = 0
    albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
    for sig in ((1.0, 0.25, 4.0), (0.3, 1.0, 1.5), (10.0, 0.05, 40.0)):
        out = ctx.denoise_to_host(acc, m2, albedo, nd, 3, True, *sig)
        assert not out[5:9, 10:13, :3].any() and (out[..., 3] == 1).all()
        compare_with_model(out, dm.denoise(acc, m2, albedo, nd, 3, True, *sig), "sigmas %r" % (sig,))
    for iterations in (2, 8):
        out = ctx.denoise_to_host(acc, m2, albedo, nd, iterations, False)
        compare_with_model(out, dm.denoise(acc, m2, albedo, nd, iterations, False), "iterations %d" % iterations)


def test_denoise_is_deterministic_and_leaves_its_inputs():
    desc, W, H, g, _, _, _ = setup("c3_small")
    ctx = gpu_context()
    acc, m2 = render_inputs("c3_small", 16)
    albedo, nd = ag.PathTracer(5).render_features_to_host(g, W, H)
    host = [acc, m2, albedo, nd]
    ptrs = [ctx.alloc(a.nbytes) for a in host] + [ctx.alloc(W * H * 16), ctx.alloc(W * H * 16)]
    try:
        for p, a in zip(ptrs, host):
            ctx.upload(p, a)
        params = ag.DenoiseParams(W, H, 5, 1, ag.DENOISE_SIGMA_Z, ag.DENOISE_SIGMA_N, ag.DENOISE_SIGMA_L)
        ctx.denoise(params, *ptrs[:4], ptrs[4])
        ctx.denoise(params, *ptrs[:4], ptrs[5])
        o1, o2 = ctx.download(ptrs[4], (H, W, 4)), ctx.download(ptrs[5], (H, W, 4))
        assert o1.tobytes() == o2.tobytes()
        assert (o1[..., 3] == 1).all() and np.isfinite(o1).all()
        for p, a in zip(ptrs, host):
            assert ctx.download(p, a.shape).tobytes() == a.tobytes()
        # both resolves display the result
        assert np.array_equal(ctx.resolve_counts(ptrs[4], W * H), ctx.resolve(ptrs[4], W * H, 1))
        # aliasing and bad parameters are refused
        for bad in (ptrs[0], ptrs[1], ptrs[2], ptrs[3]):
            with pytest.raises(ag.AgptError):
                ctx.denoise(params, *ptrs[:4], bad)
        for change in (dict(iterations=0), dict(iterations=9), dict(sigma_n=0.0), dict(width=0)):
            p = ag.DenoiseParams(W, H, 5, 1, 1.0, 0.25, 4.0)
            for k, v in change.items():
                setattr(p, k, v)
            with pytest.raises(ag.AgptError):
                ctx.denoise(p, *ptrs[:4], ptrs[4])
            assert b"agpt_denoise" in ag.lib().agpt_last_error()
        assert ctx.download(ptrs[4], (H, W, 4)).tobytes() == o1.tobytes()
    finally:
        for p in ptrs:
            ctx.free(p)


# ---- quality --------------------------------------------------------------------------------------------------------------
REF_SPP, REF_SEED = 1024, 0x5EED0001


@pytest.mark.parametrize("name,W,H", [("c1", 256, 256), ("c3", 1920, 1080)])
def test_denoised_is_closer_to_the_reference_than_raw(name, W, H):
    desc = ag.scenes.scene_c1() if name == "c1" else ag.scenes.scene_c3(aspect=W / float(H))
    g = gpu_scene(desc)
    try:
        pt = ag.PathTracer(5)
        ref, _ = pt.render_to_host(g, W, H, REF_SPP, seed_base=REF_SEED)
        ref = ref[..., :3] / F(REF_SPP)
        acc, m2, _, _ = pt.render_adaptive_to_host(g, W, H, 16, 16, 16, 0.0)
        albedo, nd = pt.render_features_to_host(g, W, H)
        out = g.ctx.denoise_to_host(acc, m2, albedo, nd)
    finally:
        g.close()
    raw = dm.display_rmse(acc[..., :3] / F(16), ref)
    den = dm.display_rmse(out[..., :3], ref)
    print("%s %dx%d 16 spp: display RMSE raw %.5f, denoised %.5f" % (name, W, H, raw, den))
    assert den < raw, (den, raw)
