"""The coherent closest-hit launch (k_trace_fast<COH>): iteration 0 of an agpt_render batch whose sample group is 64 gives every wave
one pixel's 64 camera rays, and a step at which all voting lanes stand at the same BVH node or leaf fetches that record once, through
scalar loads.  The arithmetic is the per-lane arithmetic of every other instantiation on the same fp32 operands, so nothing may change:
each case renders once as is and once with AGPT_NO_COHERENT=1 (the ordinary instantiation) and requires the two accumulators byte for
byte equal, the ray totals equal, and the image bit-identical to the CPU oracle's with the oracle's ray total, as test_gpu_render.py
compares.  Films are 32x16 at 64 spp (32,768 paths; 512 waves of the coherent launch): batches this small run the PEEK instantiations.  The
full-size (!PEEK) ones, which a batch of 48 Mi paths selects, run the same cases through check() on a context created with
AGPT_SMALL_BATCH_PATHS=0 in test_gpu_full_batch_trace.py."""
import functools

import numpy as np
import pytest

import ag_pathtracer_amd as ag
from helpers import bits, gpu_scene, oracle_render, oracle_scene

pytestmark = pytest.mark.gpu

DEPTH = 5


def check(monkeypatch, desc, W, H, spp, spb=0, ctx=None):
    """ctx: the context the scene is instantiated on (default: the shared one).  Returns the film and its stats."""
    oacc, ost = oracle_render(desc, W, H, spp, DEPTH)
    g = gpu_scene(desc) if ctx is None else desc.instantiate(ag.Scene(ctx))
    pt = ag.PathTracer(DEPTH)
    a, sa = pt.render_to_host(g, W, H, spp, samples_per_batch=spb)
    monkeypatch.setenv("AGPT_NO_COHERENT", "1")
    b, sb = pt.render_to_host(g, W, H, spp, samples_per_batch=spb)
    monkeypatch.delenv("AGPT_NO_COHERENT")
    g.close()
    print(desc.name, dict(closest=(sa.closest_rays, sb.closest_rays), anyhit=(sa.anyhit_rays, sb.anyhit_rays),
                          answered=(sa.answered_rays, sb.answered_rays), rays=(sa.rays, ost.rays),
                          bit_exact=float(np.all(bits(a[..., :3]) == bits(oacc[..., :3]), axis=-1).mean())))
    assert a.tobytes() == b.tobytes()
    assert (sa.closest_rays, sa.anyhit_rays, sa.answered_rays) == (sb.closest_rays, sb.anyhit_rays, sb.answered_rays)
    assert np.array_equal(bits(a[..., :3]), bits(oacc[..., :3]))
    assert sa.rays == ost.rays
    assert sa.outliers == ost.outliers
    return a, sa


@functools.lru_cache(maxsize=None)
def small_c3():
    return ag.scenes.scene_c3(scale=0.02)


def test_many_small_meshes(monkeypatch):
    """C3's atrium at 1/50 of its triangles: the prefilter masks differ between the lanes of a bundle, so root pairs, uniform and mixed
    steps and leaves with several triangles all occur."""
    check(monkeypatch, small_c3(), 32, 16, 64)


def test_thin_lens_bundles_diverge(monkeypatch):
    """A thin lens gives every lane its own origin, and the light is the environment: a bundle leaves the scalar path early, and lanes
    that meet again at a node take it once more."""
    check(monkeypatch, ag.scenes.scene_simple_test(aperture=0.1), 32, 16, 64)


def through_two_emitters():
    """A camera that looks at the backdrop mesh through two emitter spheres (area lights: no material) on its axis, 1.5 and 2.6 in
    front of it, with angular radii of 9.6 and 10 degrees in a 45-degree frustum: the pixels at the film's centre cross both (two
    re-casts each, the first with Le added: the rays carry d.w = 2), those on a silhouette split their bundle."""
    from ag_pathtracer_amd.binding import create_backdrop
    d = ag.SceneDesc("through-two-emitters")
    floor = d.add_material(ag.MAT_DISNEY, [.6, .62, .45], 1.0, 0.0)
    v, n, t, idx = create_backdrop([0, -1, 20], [40, 20, 40], 7.5, 32)
    d.add_mesh(v, n, t, idx, floor, 1)
    eye = np.float64([-1.46, 1.16, -4.64])
    axis = -eye / np.linalg.norm(eye)
    prims = [d.add_area_light(list(eye + 1.5 * axis), 0.25, [4., 3., 2.]), d.add_area_light(list(eye + 2.6 * axis), 0.45, [1., 2., 3.])]
    d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera(list(eye), [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    return d, prims


def test_recast_through_emitters_inside_the_kernel(monkeypatch):
    """CUR_RECAST in the coherent kernel: parked lanes wait while the rest of their bundle traverses, then re-cast."""
    import temporal_model as tm
    W, H, sub = 32, 16, 4
    d, prims = through_two_emitters()
    # 4 x 4 rays through each pixel (CPU oracle): how many of them have the nearer emitter as closest hit
    cam = ag.camera_vectors(d.camera)
    rays = np.zeros(W * H * sub * sub, ag.RAY_DTYPE)
    rays["o"] = tm.camera(cam)["origin"]
    rays["d"] = tm.feature_directions(cam, W * sub, H * sub).reshape(-1, 3)
    rays["tmax"] = 3.402823466e+38
    hits, _ = oracle_scene(d).intersect(rays, any_hit=False)
    on = ((hits["hit"] == 1) & (hits["prim"] == prims[0]) & (hits["tri"] < 0)).reshape(H, sub, W, sub).sum((1, 3))
    print("pixels inside the nearer emitter's outline: %d, on it: %d" % ((on == sub * sub).sum(), ((on > 0) & (on < sub * sub)).sum()))
    assert (on == sub * sub).sum() >= 8 and ((on > 0) & (on < sub * sub)).sum() >= 8
    check(monkeypatch, d, W, H, 64)


def test_spilling_instantiation(monkeypatch):
    """A BVH deeper than the 23 stack entries kept in LDS (the SPILL instantiation), with an emitter sphere in front of it."""
    from test_gpu_render import deep_mesh_with_emitter
    d, prim, bvh_depth = deep_mesh_with_emitter()
    assert bvh_depth > 23
    check(monkeypatch, d, 16, 16, 64)


def test_sample_group_of_32_is_not_selected(monkeypatch):
    """96 spp: the sample group is 32, a wave would hold two pixels' rays -- the launch is not selected and the knob changes nothing."""
    check(monkeypatch, small_c3(), 32, 16, 96)


def test_two_batches_each_with_a_coherent_first_launch(monkeypatch):
    check(monkeypatch, small_c3(), 32, 16, 128, spb=64)
