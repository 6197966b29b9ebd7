"""Every entry point on a caller's stream created with hipStreamNonBlocking.  On the null stream a memset, copy, kernel or event that
the library put on stream 0 or on a side stream without a wait is ordered with everything else by the legacy null-stream rules and
cannot be seen; on a non-blocking stream it is a race.  Every case therefore has one deterministic shape, on a fresh context of its
own whose stream is such a stream S:

  1. the buffers the call reads hold finite WRONG values (other rays, another pose, a finished frame), the ones it writes a
     recognisable constant -- float payloads only, never indices, counts or sizes: a library that read them computes a wrong answer,
     not a wrong address;
  2. a delay is enqueued on S that the host does not wait for (hip_runtime.Delay: a chain of large device-to-device copies);
  3. behind it, on S, the caller's own device-to-device copies put the real inputs in place and clear the outputs;
  4. the library call is made -- while hipStreamQuery(S) still says hipErrorNotReady, and with the delay (measured once per session
     with two events) at least 4x the host time since step 2 began: only a few enqueues of tens of microseconds lie in between;
  5. where the call only enqueues, snapshot copies of its outputs are enqueued on S;
  6. S is synchronised and the results compared with the CPU oracle, the numpy models or the host twins, as the rest of the suite does.

A library operation that reads on any other stream than S sees the wrong values, one that writes before the caller's clear has its
write wiped, and one that leaves work unordered after S misses the snapshot.  Nothing here lets two streams use a context at once."""
import contextlib
import functools
import time

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import adaptive_model as am
import denoise_model as dm
import device_update_cases as dc
import hip_runtime
import ray_edge_cases as rec
import temporal_model as tm
from ag_pathtracer_amd import tiles
from denoise_features import host_features, primitive_table
from device_update_cases import about, palette, seventy_prims
from helpers import bits, compare_with_model, gpu_context, oracle_render, oracle_render_on, oracle_scene, random_rays, scene_c1
from skin_cases import binding
from test_gpu_coherent_trace import small_c3
from test_gpu_denoise import check_features
from test_gpu_intersect import deep_mesh_scene
from transform_cases import MATRICES

pytestmark = pytest.mark.gpu
F = np.float32
DEPTH = 5
_SESSION = {}


def session_delay():
    """the delay every case enqueues, sized and timed once (on a non-blocking stream of its own; its scratch comes from the shared
    null-stream context and lives as long as the process)"""
    if "delay" not in _SESSION:
        hip = hip_runtime.runtime()
        s = hip.stream_create()
        try:
            d = hip_runtime.Delay(gpu_context(), s)
        finally:
            hip.stream_destroy(s)
        print("delay: %d copies of %d MiB take %.1f ms on the GPU and %.3f ms of host time to enqueue (runtime: %s)"
              % (d.copies, d.NBYTES >> 20, d.ms, d.enqueue_ms, hip.path))
        _SESSION["delay"] = d
    return _SESSION["delay"]


class Buffer:
    """dst: what the library is given; real / poison: device copies of the values staged behind the delay (None: nothing is staged)
    and of the wrong values put there first"""

    def __init__(self, stage, real, poison):
        poison = np.ascontiguousarray(poison)
        self.shape, self.dtype, self.nbytes = poison.shape, poison.dtype, poison.nbytes
        self.dst = stage.alloc(self.nbytes)
        self.poison = stage.alloc(self.nbytes)
        stage.ctx.upload(self.poison, poison)
        self.real = None
        if real is not None:
            real = np.ascontiguousarray(real)
            assert real.nbytes == self.nbytes and real.dtype == self.dtype
            self.real = stage.alloc(self.nbytes)
            stage.ctx.upload(self.real, real)


class Stage:
    """a fresh context on a non-blocking stream of its own, its scenes and buffers, and the steps of the pattern"""

    def __init__(self):
        self.hip = hip_runtime.runtime()
        self.delay = session_delay()
        self.stream = self.hip.stream_create()
        self.ptrs, self.scenes, self.closers, self.ctx = [], [], [], None
        self.t0 = None

    def __enter__(self):
        try:
            self.ctx = ag.Context(0, stream=self.stream)
        except BaseException:
            self.hip.stream_destroy(self.stream)
            raise
        return self

    def __exit__(self, *exc):
        try:
            self.hip.stream_synchronize(self.stream)
            for c in self.closers:
                c.close()
            for g in self.scenes:
                g.close()
            for p in self.ptrs:
                self.ctx.free(p)
            self.ctx.close()
        finally:
            self.hip.stream_destroy(self.stream)
        return False

    def alloc(self, nbytes):
        self.ptrs.append(self.ctx.alloc(nbytes))
        return self.ptrs[-1]

    def scene(self, desc):
        g = ag.Scene(self.ctx)
        self.scenes.append(g)
        return desc.instantiate(g)

    def buffer(self, real, poison):
        return Buffer(self, real, poison)

    def output(self, shape, value, clear=True, dtype=F):
        """a buffer the call writes: `value` everywhere first, zeroed behind the delay if `clear`"""
        return Buffer(self, np.zeros(shape, dtype) if clear else None, np.full(shape, value, dtype))

    def open(self, bufs=(), sync_poison=True):
        """steps 1 - 3 for `bufs`.  sync_poison=False: the wrong values too are only enqueued on S, ahead of the delay (a chain of
        calls that the caller never synchronises)"""
        hip, s = self.hip, self.stream
        for b in bufs:
            hip.copy_async(b.dst, b.poison, b.nbytes, s)
        if sync_poison:
            hip.stream_synchronize(s)
        self.t0 = time.perf_counter()
        self.delay.enqueue(s)
        for b in bufs:
            if b.real is not None:
                hip.copy_async(b.dst, b.real, b.nbytes, s)

    def call(self, what, fn, *args, **kw):
        """step 4: fn(*args, **kw) with the hazard window open"""
        state = self.hip.stream_query(self.stream)
        host_ms = 1e3 * (time.perf_counter() - self.t0)
        out = fn(*args, **kw)
        print("%s: delay %.1f ms, host enqueue %.3f ms (x%.0f), stream before the call: %s"
              % (what, self.delay.ms, host_ms, self.delay.ms / host_ms, "NotReady" if state == hip_runtime.hipErrorNotReady else "done"))
        assert state == hip_runtime.hipErrorNotReady, what
        assert self.delay.ms >= 4 * host_ms, (what, self.delay.ms, host_ms)
        return out

    def snapshot(self, b):
        """step 5: a copy of b as S sees it now -> the pointer; read it after sync()"""
        p = self.alloc(b.nbytes)
        self.hip.copy_async(p, b.dst, b.nbytes, self.stream)
        return p

    def sync(self):
        self.hip.stream_synchronize(self.stream)

    def read(self, b, ptr=None):
        return self.ctx.download(b.dst if ptr is None else ptr, b.shape, b.dtype)


# ---- ray queries ----------------------------------------------------------------------------------------------------------
RAY_SCENES = {"c1": scene_c1, "grid_long": rec.grid_long, "deep": deep_mesh_scene}
N_RAYS = 4000


@functools.lru_cache(maxsize=None)
def ray_case(name):
    desc = RAY_SCENES[name]()
    rays, other = random_rays(desc, N_RAYS, seed=31), random_rays(desc, N_RAYS, seed=32)
    o = oracle_scene(desc)
    return desc, rays, other, o.intersect(rays, any_hit=False), o.intersect(rays, any_hit=True)[0]


def poisoned_hits(n):
    return np.full(n * (ag.HIT_DTYPE.itemsize // 4), 0x5A5A5A5A, np.uint32).view(ag.HIT_DTYPE)


def assert_closest(gh, oh):
    """field by field, as test_gpu_intersect.py compares"""
    assert np.array_equal(gh["hit"], oh["hit"])
    assert np.array_equal(gh["prim"], oh["prim"])
    assert np.array_equal(gh["tri"], oh["tri"])
    m = oh["hit"] == 1
    assert m.any()
    for f in ("t", "b1", "b2"):
        assert np.array_equal(bits(gh[f][m]), bits(oh[f][m])), f


@pytest.mark.parametrize("mode", ["closest", "any", "counters"])
@pytest.mark.parametrize("name", list(RAY_SCENES))
def test_ray_queries(name, mode):
    """agpt_intersect_device with the rays staged and the hit buffer cleared behind the delay: C1, 70 primitives (k_candidates, the
    LIST kernel and the candidate scratch), a tree deeper than the LDS stack (the spill scratch is allocated inside the launch);
    closest hit, any hit and the reference-order kernel with its counters.  Then agpt_intersect_batch behind another delay."""
    desc, rays, other, (oh, ost), op = ray_case(name)
    any_hit = mode == "any"
    with Stage() as st:
        g = st.scene(desc)
        b_rays = st.buffer(rays, other)
        b_hits = st.buffer(np.zeros(N_RAYS, ag.HIT_DTYPE), poisoned_hits(N_RAYS))
        st.open([b_rays, b_hits])
        stats = st.call("intersect_device %s %s" % (name, mode), g.intersect_device, b_rays.dst, N_RAYS, b_hits.dst, any_hit=any_hit,
                        counters=mode == "counters")
        gh = st.read(b_hits)
        if any_hit:
            assert np.array_equal(gh["hit"], op["hit"])
        else:
            assert_closest(gh, oh)
        if mode == "counters":
            assert stats.interior_visits == ost.interior_visits and stats.tri_tests == ost.tri_tests
        st.open()
        batch, _ = st.call("intersect_batch %s %s" % (name, mode), g.IntersectP if any_hit else g.Intersect, rays, counters=mode == "counters")
        if any_hit:
            assert np.array_equal(batch["hit"], gh["hit"])
        else:
            assert batch.tobytes() == gh.tobytes()


# ---- render -------------------------------------------------------------------------------------------------------------------
# name: (scene, W, H, spp, AGPT_MULTI_STREAM).  small_c3 at 64 spp: iteration 0 is the coherent launch
RENDERS = {"c1": (scene_c1, 64, 48, 4, None), "small_c3": (small_c3, 32, 16, 64, None), "seventy": (seventy_prims, 32, 24, 2, None),
           "deep": (deep_mesh_scene, 16, 16, 2, None), "c1_side_streams": (scene_c1, 64, 48, 4, "2")}


@functools.lru_cache(maxsize=None)
def oracle_film(make, W, H, spp):
    desc = make()
    return (desc,) + tuple(oracle_render(desc, W, H, spp, DEPTH))


def assert_film(got, oacc, what):
    same = np.all(bits(got[..., :3]) == bits(oacc[..., :3]), axis=-1)
    assert same.all(), (what, float(same.mean()), np.argwhere(~same)[:8])


def assert_totals(stats, ost):
    assert (stats.rays, stats.closest_rays, stats.anyhit_rays) == (ost.rays, ost.closest_rays, ost.anyhit_rays)


@pytest.mark.parametrize("name", list(RENDERS))
def test_render(name, monkeypatch):
    """agpt_render into an accumulator that holds 1e30 and is zeroed on S behind the delay: without stats (the call returns with its
    accumulate pass queued; the film is read through a snapshot on S) and with them"""
    make, W, H, spp, multi = RENDERS[name]
    desc, oacc, ost = oracle_film(make, W, H, spp)
    session_delay()                                # (the shared null-stream context is not created under the knob)
    if multi:
        monkeypatch.setenv("AGPT_MULTI_STREAM", multi)
    pt = ag.PathTracer(DEPTH)
    with Stage() as st:
        g = st.scene(desc)
        accum = st.output((H, W, 4), 1e30)
        st.open([accum])
        st.call("render %s, no stats" % name, pt.render, g, W, H, spp, accum.dst, want_stats=False)
        snap = st.snapshot(accum)
        st.sync()
        assert_film(st.read(accum, snap), oacc, "no stats")
        st.open([accum])
        stats = st.call("render %s, stats" % name, pt.render, g, W, H, spp, accum.dst)
        assert_film(st.read(accum), oacc, "stats")
        assert_totals(stats, ost)


@pytest.mark.parametrize("want_stats", [False, True])
def test_progressive_render_grows_the_pool_between_two_calls(want_stats):
    """samples [0, 2) at one sample per batch, then [2, 4) at the default batch: the second call needs a larger pool than the first,
    whose accumulate pass is still queued, and the caller synchronises nothing in between"""
    W, H = 64, 48
    desc = scene_c1()
    o = oracle_scene(desc, DEPTH)
    oacc, ost1 = oracle_render_on(o, W, H, 2)
    oacc, ost2 = oracle_render_on(o, W, H, 2, spp_begin=2, accum=oacc)
    pt = ag.PathTracer(DEPTH)
    with Stage() as st:
        g = st.scene(desc)
        accum = st.output((H, W, 4), 1e30)
        st.open([accum])
        s1 = st.call("progressive render, first call, stats %d" % want_stats, pt.render, g, W, H, 2, accum.dst, samples_per_batch=1,
                     want_stats=want_stats)
        s2 = pt.render(g, W, H, 2, accum.dst, spp_begin=2, want_stats=want_stats)
        snap = st.snapshot(accum)
        st.sync()
        assert_film(st.read(accum, snap), oacc, "stats %d" % want_stats)
        if want_stats:
            assert_totals(s1, ost1)
            assert_totals(s2, ost2)


# ---- the frame loop -------------------------------------------------------------------------------------------------------
FW, FH, FSPP = 48, 32, 4
FRAME_CAMS = [([-1.16, 1.21, -4.72], [0.05, 0, 0], [0, 1, 0], FW / float(FH), 45.0, 0.0),
              ([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], FW / float(FH), 45.0, 0.0)]


def c1_with_camera(cam):
    d = scene_c1()
    d.set_camera(*cam)
    return d


def test_frame_loop_is_never_synchronised_by_the_caller():
    """Two frames of C1 with a moved camera: agpt_render_adaptive (fresh buffers zeroed on S behind the delay) -> agpt_render_features
    -> agpt_temporal_accumulate -> agpt_denoise -> agpt_resolve_counts, every call behind a delay of its own, its outputs holding a
    constant until then; between the calls the caller only enqueues.  Each buffer is checked as the suite checks that call: the
    accumulator bit for bit against the oracle and moment2 against adaptive_model (test_gpu_adaptive.py), the features as
    test_gpu_denoise.check_features, the history bit for bit against temporal_model on the buffers it was given (test_gpu_temporal.py),
    the denoised frame by helpers.compare_with_model, the resolved words against a null-stream context's."""
    pt = ag.PathTracer(DEPTH)
    n = FW * FH
    finished = np.full((FH, FW, 4), 7.0, F)
    finished[..., 3] = FSPP                       # (a pixel at max_spp: a library that read it would add nothing)
    frames = []
    with Stage() as st:
        g = st.scene(scene_c1())
        prev = None
        for k, cam in enumerate(FRAME_CAMS):
            g.set_camera(*cam)
            acc = st.buffer(np.zeros((FH, FW, 4), F), finished)
            m2 = st.buffer(np.zeros((FH, FW), F), np.full((FH, FW), 3.0, F))
            alb, nd, hacc, den = (st.output((FH, FW, 4), -7.0, clear=False) for _ in range(4))
            hm2 = st.output((FH, FW), -7.0, clear=False)
            st.open([acc, m2], sync_poison=k == 0)
            st.call("frame %d render_adaptive" % k, pt.render_adaptive, g, FW, FH, acc.dst, m2.dst, FSPP, FSPP, FSPP, 0.0, seed_base=k + 1)
            st.open([alb, nd], sync_poison=False)
            st.call("frame %d render_features" % k, pt.render_features, g, FW, FH, alb.dst, nd.dst)
            cam_prev = FRAME_CAMS[k - 1] if k else cam
            params = ag.TemporalParams(FW, FH, ag.camera_desc(*cam), ag.camera_desc(*cam_prev), 32.0, ag.TEMPORAL_DEPTH_TOL, ag.TEMPORAL_NORMAL_COS)
            st.open([hacc, hm2], sync_poison=False)
            st.call("frame %d temporal_accumulate" % k, st.ctx.temporal_accumulate, params, acc.dst, m2.dst, alb.dst, nd.dst,
                    *([b.dst for b in prev] if prev else [0, 0, 0, 0]), hacc.dst, hm2.dst)
            st.open([den], sync_poison=False)
            st.call("frame %d denoise" % k, st.ctx.denoise, ag.DenoiseParams(FW, FH, 5, 1, ag.DENOISE_SIGMA_Z, ag.DENOISE_SIGMA_N, ag.DENOISE_SIGMA_L),
                    hacc.dst, hm2.dst, alb.dst, nd.dst, den.dst)
            st.open(sync_poison=False)
            words = st.call("frame %d resolve_counts" % k, st.ctx.resolve_counts, den.dst, n)
            frames.append(((acc, m2, alb, nd, hacc, hm2, den), words))
            prev = (hacc, hm2, alb, nd)
        st.sync()
        frames = [([st.read(b) for b in bufs], words) for bufs, words in frames]
    null = gpu_context()
    before = None
    for k, ((acc, m2, alb, nd, hacc, hm2, den), words) in enumerate(frames):
        cam = FRAME_CAMS[k]
        desc = c1_with_camera(cam)
        # agpt_render_adaptive at min = max = 4 samples: the oracle's film, and the model's second moment
        samples = np.stack([oracle_render(desc, FW, FH, 1, DEPTH, spp_begin=s, seed_base=k + 1)[0][..., :3] for s in range(FSPP)])
        assert_film(acc, oracle_render(desc, FW, FH, FSPP, DEPTH, seed_base=k + 1)[0], "frame %d accumulator" % k)
        assert (acc[..., 3] == FSPP).all()
        mm = am.run(samples, FSPP, FSPP, FSPP, 0.0, 0.0)["moment2"]
        assert np.all(np.abs(m2 - mm) <= 1e-5 * np.abs(mm) + 1e-30), k
        # agpt_render_features
        exp_albedo, exp_nd, either, hits = host_features(desc, FW, FH)
        prims, _ = primitive_table(desc)
        is_sphere = np.array([op[0] in ("sphere", "area_light") for op, _ in prims] + [False])
        check_features(alb, nd, exp_albedo, exp_nd, either, is_sphere[hits["prim"]][::-1])
        # agpt_temporal_accumulate on exactly these buffers
        cam_prev = FRAME_CAMS[k - 1] if k else cam
        model = tm.accumulate(ag.camera_vectors(cam), ag.camera_vectors(cam_prev), acc, m2, alb, nd, before, identity=k == 0)
        assert hacc.tobytes() == model[0].tobytes(), (k, np.argwhere((hacc != model[0]).any(-1))[:8])
        assert hm2.tobytes() == model[1].tobytes(), (k, np.argwhere(hm2 != model[1])[:8])
        if k:
            assert (hacc[..., 3] > acc[..., 3]).any()          # (history was taken)
        compare_with_model(den, dm.denoise(hacc, hm2, alb, nd), "frame %d denoised" % k)
        p = null.alloc(den.nbytes)
        try:
            null.upload(p, den)
            assert words.tobytes() == null.resolve_counts(p, n).tobytes(), k
        finally:
            null.free(p)
        before = (hacc, hm2, alb, nd)


# ---- moving geometry --------------------------------------------------------------------------------------------------------
MOVED = (dc.GRID1_N, dc.GRID4, dc.PRIMS[0])      # normals and 1 primitive per leaf, none and 4, one triangle


def posed_zoo(arrays):
    """device_update_cases.zoo_scene() with the meshes {prim: (verts, normals)} replaced: what the oracle builds afresh"""
    d = dc.zoo_scene()
    meshes = [i for i, op in enumerate(d.ops) if op[0] == "mesh"]
    for prim, (v, n) in arrays.items():
        op = d.ops[meshes[prim]]
        d.ops[meshes[prim]] = ("mesh", np.ascontiguousarray(v, F), None if n is None else np.ascontiguousarray(n, F)) + tuple(op[3:])
    return d


def assert_rays_through_updated_scene(st, g, arrays, rebuilt):
    """a ray batch on S through the updated scene against the oracle built from the same arrays: a rebuilt tree is the oracle's, so
    every field is; a refitted one differs from it, and test_gpu_mesh_update.py's rule holds -- hit flag and the bits of t equal on all
    rays but at most 2"""
    desc = posed_zoo(arrays)
    rays = dc.rays_for(dc.zoo_scene())
    o = oracle_scene(desc)
    oh, _ = o.intersect(rays)
    op, _ = o.intersect(rays, any_hit=True)
    st.open()
    gh, _ = st.call("rays through the updated scene", g.Intersect, rays)
    gp, _ = g.IntersectP(rays)
    if rebuilt:
        assert_closest(gh, oh)
        assert np.array_equal(gp["hit"], op["hit"])
    else:
        differ = (gh["hit"] != oh["hit"]) | ((oh["hit"] == 1) & (bits(gh["t"]) != bits(oh["t"])))
        assert int(differ.sum()) <= 2 and int((gp["hit"] != op["hit"]).sum()) <= 2, (int(differ.sum()), int((gp["hit"] != op["hit"]).sum()))


@contextlib.contextmanager
def twin_scene(desc):
    """the same scene on the shared null-stream context: the host-array call's side of a comparison"""
    a = desc.instantiate(ag.Scene(gpu_context()))
    try:
        yield a
    finally:
        a.close()


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_update_mesh_device_takes_arrays_produced_on_the_stream(mode):
    """agpt_scene_update_mesh_device with the arrays "produced on the context's stream": they hold another pose until the caller's
    copies behind the delay put the real one there.  Twice per mesh (the second update finds the mesh's cache)."""
    desc = dc.zoo_scene()
    with Stage() as st, twin_scene(desc) as a:
        b = st.scene(desc)
        arrays = {}
        for pose, wrong in ((1, 2), (2, 1)):
            for prim in MOVED:
                v, n = dc.zoo_arrays(prim, pose)
                w, wn = dc.zoo_arrays(prim, wrong)
                a.update_mesh(prim, v, n, mode)
                bv = st.buffer(v, w)
                bn = None if n is None else st.buffer(n, wn)
                st.open([bv] + ([bn] if bn else []))
                st.call("update_mesh_device %s prim %d pose %d" % (mode, prim, pose), b.update_mesh_device, prim, bv.dst, len(v),
                        bn.dst if bn else None, 0 if n is None else len(n), mode)
                arrays[prim] = (v, n)
            dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        assert_rays_through_updated_scene(st, b, arrays, mode == "rebuild")


def test_transform_mesh_first_and_second_call():
    """agpt_scene_transform_mesh: the first call of a mesh uploads its rest pose, the second finds it on the device"""
    desc = dc.zoo_scene()
    with Stage() as st, twin_scene(desc) as a:
        b = st.scene(desc)
        arrays = {}
        for name in ("rotation+translation", "scale+shear"):
            for prim in MOVED:
                M = about(prim, MATRICES[name])
                arrays[prim] = ag.transform_arrays(M, *dc.zoo_arrays(prim))
                a.update_mesh(prim, *arrays[prim], "refit")
                st.open()
                st.call("transform_mesh prim %d %s" % (prim, name), b.transform_mesh, prim, M, "refit")
            dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        assert_rays_through_updated_scene(st, b, arrays, False)


def test_pose_mesh_first_and_second_call():
    """agpt_scene_pose_mesh (K = 4, the palette staged in LDS): the first call of a mesh uploads its rest pose and binding"""
    desc = dc.zoo_scene()
    with Stage() as st, twin_scene(desc) as a:
        b = st.scene(desc)
        skins = {}
        for prim in MOVED:
            skins[prim] = binding(len(dc.zoo_arrays(prim)[0]), 4, seed=prim)
            b.set_mesh_skin(prim, *skins[prim], n_joints=3)
        arrays = {}
        for pose in (0, 1):
            for prim in MOVED:
                mats = palette(prim, pose)
                rest = dc.zoo_arrays(prim)
                arrays[prim] = ag.skin_arrays(mats, rest[0], *skins[prim], rest[1])
                a.update_mesh(prim, *arrays[prim], "refit")
                st.open()
                st.call("pose_mesh prim %d pose %d" % (prim, pose), b.pose_mesh, prim, mats, "refit")
            dc.assert_same(dc.snapshot(a, desc, dc.PRIMS), dc.snapshot(b, desc, dc.PRIMS))
        assert_rays_through_updated_scene(st, b, arrays, False)


# ---- tiles ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["deinterleave", "gather"])
def test_tiles_only_enqueue(entry):
    """agpt_deinterleave_tiles / agpt_gather_tiles at world = 1, 50 rows in blocks of 8 (the last block is partial): the compact buffer
    is staged and the full one cleared behind the delay, the result is read through a snapshot on S"""
    W, H, block = 40, 50, 8
    rng = np.random.RandomState(5)
    compact = rng.uniform(0, 4, (H, W, 4)).astype(F)
    expected = tiles.deinterleave([compact], W, H, 1, block)
    assert expected.tobytes() != compact.tobytes()
    with Stage() as st:
        b_in = st.buffer(compact, rng.uniform(0, 4, (H, W, 4)).astype(F))
        b_out = st.output((H, W, 4), -7.0)
        if entry == "gather":
            comm = ag.Comm(st.ctx, 1, 0)
            st.closers.append(comm)
        st.open([b_in, b_out])
        if entry == "deinterleave":
            st.call("deinterleave_tiles", st.ctx.deinterleave_tiles, b_in.dst, W, H, block, 1, 0, b_out.dst)
        else:
            st.call("gather_tiles", comm.gather_tiles, b_in.dst, W, H, block, b_out.dst)
        snap = st.snapshot(b_out)
        st.sync()
        assert st.read(b_out, snap).tobytes() == expected.tobytes()


# ---- known-answer entry points ------------------------------------------------------------------------------------------------
def test_known_answer_calls_equal_a_null_stream_context():
    """agpt_kat_bsdf_eval / _sample, agpt_kat_rng and agpt_kat_distribution1d stage their host arrays through DevBuf::in / out: behind
    the delay on S they return the bytes they return on the null stream"""
    rng = np.random.RandomState(9)
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    wo, wi = unit(rng.normal(size=(777, 3))), unit(rng.normal(size=(777, 3)))
    u = rng.uniform(size=(777, 2)).astype(F)
    func = rng.uniform(0, 3, 301).astype(F)
    uu = rng.uniform(size=500).astype(F)
    desc = scene_c1()
    flat = lambda r: b"".join(np.ascontiguousarray(x).tobytes() for x in (r if isinstance(r, tuple) else (r,)))
    with Stage() as st, twin_scene(desc) as a:
        b = st.scene(desc)
        null = gpu_context()
        for what, on_s, on_null in (("bsdf_eval", lambda: b.bsdf_eval(1, wo, wi), lambda: a.bsdf_eval(1, wo, wi)),
                                    ("bsdf_sample", lambda: b.bsdf_sample(1, wo, u), lambda: a.bsdf_sample(1, wo, u)),
                                    ("rng", lambda: st.ctx.rng_floats(12345, 640 * 480, 3, 7, 64), lambda: null.rng_floats(12345, 640 * 480, 3, 7, 64)),
                                    ("distribution1d", lambda: st.ctx.distribution1d(func, uu), lambda: null.distribution1d(func, uu))):
            st.open()
            got = st.call("kat %s" % what, on_s)
            assert flat(got) == flat(on_null()), what


def test_other_host_array_calls_equal_a_null_stream_context():
    """the remaining entry points that take or return host arrays -- agpt_li_batch (the wavefront loop between asynchronous copies of
    pageable memory), agpt_dbg_li_batch, agpt_kat_normal_map, agpt_bvh_build_device and agpt_resolve (its accumulator staged behind
    the delay) -- byte for byte against a null-stream context"""
    rng = np.random.RandomState(13)
    desc = scene_c1()
    rays = random_rays(desc, 2000, seed=33)
    states = (rng.randint(1, 2 ** 31 - 1, len(rays)).astype(np.uint32) | 1).astype(np.uint32)
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    ns, ss, rgb = unit(rng.normal(size=(300, 3))), unit(rng.normal(size=(300, 3))), rng.uniform(size=(300, 3)).astype(F)
    gv, _, gidx = dc.bumpy_grid(False)
    W, H, spp = 40, 30, 4
    film, other = (rng.uniform(0, 8, (H, W, 4)).astype(F) for _ in range(2))
    pt = ag.PathTracer(DEPTH)
    flat = lambda r: b"".join(np.ascontiguousarray(x).tobytes() for x in r)
    li = lambda g: (lambda out, after, s: (out, after, np.uint64(s.rays)))(*pt.Li(g, rays, states))
    null = gpu_context()
    with Stage() as st, twin_scene(desc) as a:
        b = st.scene(desc)
        for what, on_s, on_null in (("li_batch", lambda: li(b), lambda: li(a)),
                                    ("dbg_li_batch", lambda: (pt.DbgLi(b, rays),), lambda: (pt.DbgLi(a, rays),)),
                                    ("kat_normal_map", lambda: (st.ctx.kat_normal_map(ns, ss, rgb, 0.7),), lambda: (null.kat_normal_map(ns, ss, rgb, 0.7),)),
                                    ("bvh_build_device", lambda: ag.bvh_build_device(st.ctx, gv, gidx, 4), lambda: ag.bvh_build_device(null, gv, gidx, 4))):
            st.open()
            got = st.call(what, on_s)
            assert flat(got) == flat(on_null()), what
        accum = st.buffer(film, other)
        st.open([accum])
        words = st.call("resolve", st.ctx.resolve, accum.dst, W * H, spp)
        p = null.alloc(film.nbytes)
        try:
            null.upload(p, film)
            assert words.tobytes() == null.resolve(p, W * H, spp).tobytes()
        finally:
            null.free(p)


# ---- agpt_set_stream and work in flight -------------------------------------------------------------------------------------
def test_set_stream_synchronises_the_stream_it_leaves():
    """The context's pool, queues, counters and events are shared by all its calls: agpt_set_stream waits for the stream it leaves
    before it stores the new one (include/agpt.h).  No GPU work races here whatever the library does: the delay and a tile kernel are
    queued on A, the context moves to B, and on return A must be idle.  Setting the handle it already has does nothing."""
    W, H, block = 40, 50, 8
    hip = hip_runtime.runtime()
    with Stage() as st:
        other = hip.stream_create()
        try:
            b_in = st.output((H, W, 4), 1.0, clear=False)
            b_out = st.output((H, W, 4), -7.0, clear=False)
            st.open([b_in, b_out])
            st.call("set_stream, same handle", st.ctx.set_stream, st.stream)
            assert hip.stream_query(st.stream) == hip_runtime.hipErrorNotReady         # (nothing was waited for)
            st.ctx.deinterleave_tiles(b_in.dst, W, H, block, 1, 0, b_out.dst)
            st.call("set_stream, another stream", st.ctx.set_stream, other)
            assert hip.stream_query(st.stream) == hip_runtime.hipSuccess
            assert (st.read(b_out) == 1.0).all()
        finally:
            st.ctx.set_stream(st.stream)
            hip.stream_destroy(other)
