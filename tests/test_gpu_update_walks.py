"""The per-frame update calls of a committed scene TOGETHER: every walk of update_walk_cases.py (seeded action lists over the front ends
of agpt_scene_update_mesh, the setters, the analytic updates, the snapshots, the readers of the host mirror and the refusals) is applied to
scene B, and after EVERY action B is observed only through calls that read the device and never the mirror:

    Intersect and IntersectP on the scene's fixed ray set, a 32x32 2-spp render with its three ray totals and -- after a snapshot action --
    the motion buffers at 32x32 (agpt_render_features_surface_motion after snapshot_surfaces: albedo, normal and depth, prev_point with its
    w, prev_normal; after snapshot_positions the shading generations are absent by contract and agpt_render_features_motion gives the
    first three).

Scene.bvh() is NOT part of the observation: agpt_mesh_get_bvh runs sync_mirror(s, false), which downloads the bounds and the spheres and
clears bounds_stale and spheres_stale -- an observation through it would reset the state under test at every step, and no stale flag
would survive from one call into the next (device_update_cases.snapshot does exactly that, which is fine for what it is used for).  bvh
and DbgLi run only where the walk draws them as actions of their own, and there their result is compared too.

Expected values:
  replay scene R   built from scratch at each step, the plainest way: the description with each mesh's BUILD-time arrays under the builder
                   the model recorded for it, the analytic records and radiances the model holds, then one host-pointer
                   update_mesh(..., "refit") for each mesh whose current arrays differ (normals mode GIVEN throughout: the model's
                   normals are passed).  For the motion buffers the same is done for the older generation (the analytic records moved
                   there by the host calls), the snapshot call the walk made then, the newer generation, and the walk's snapshot call
                   again.  R never sees a device pointer, a deform kernel, a cache or a stale flag; its host-pointer REFIT is pinned to
                   bvh_refit_model and the oracle by test_gpu_mesh_update.py.  All observed bytes of B equal R's.
  the oracle       an OracleScene of the model's current arrays: the hit flag and the bits of t of every closest-hit record, and the
                   any-hit flag.  (Triangle ids are compared with R only: where two triangles tie at one t the id depends on the tree.)

Only at the end of a walk, because they disturb the state: b.bvh(p) of every mesh equals R's, bytes and order; then every mesh is rebuilt
from the model's arrays (all 70 of them on the 70-primitive scene), and the render of B equals the render of a fresh scene of those
arrays and the oracle's, bit for bit.

A failure names the walk's seed, the step, the action and the first key that differs; update_walk_cases.walk(seed) is the walk."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import ag_pathtracer_amd as ag
import device_update_cases as dc
import update_walk_cases as uw
from helpers import bits, gpu_context, oracle_render
from oracle import binding as ob

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT = ag.PathTracer(dc.DEPTH)
N_DBG = 256
REFUSAL_TEXT = {"singular_joint": "joint 1 is singular (its determinant is exactly 0)", "last_row": "the last row of joint 0 is not (0, 0, 0, 1)",
                "weight": "non-finite weight (target ", "counts": "both counts stay",
                "radius": "the centre and the radius must be finite and the radius positive",
                "sphere_record": "a record has a non-finite value or a radius that is not positive"}


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
class _PerMeshBuilder:
    """SceneDesc.instantiate's target: every mesh is added under the builder recorded for its primitive"""

    def __init__(self, g, builders):
        self.g, self.builders, self.n = g, builders, 0

    def __getattr__(self, name):
        fn = getattr(self.g, name)
        if name not in ("add_mesh", "add_sphere", "add_plane", "add_area_light"):
            return fn

        def add(*args):
            if name == "add_mesh":
                self.g.set_bvh_builder(self.builders.get(self.n, "host"))
            self.n += 1
            return fn(*args)
        return add


def instantiate(desc, ctx, builders=None):
    g = ag.Scene(ctx)
    desc.instantiate(_PerMeshBuilder(g, builders or {}))
    g.set_bvh_builder("host")
    return g


def same_arrays(a, b):
    return all(x is y or (x is not None and y is not None and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


def replay(model, ctx, motion):
    """scene R of the module's docstring for the model's current scene (motion: with the two generations of model.snaps)"""
    stages = model.snaps if motion else [(None, model.frozen())]
    g = instantiate(model.desc("build", stages[0][1]), ctx, {p: m.builder for p, m in model.mesh.items()})
    held = {p: (m.BV, m.BN) for p, m in model.mesh.items()}
    analytic, radiance = dict(stages[0][1]["analytic"]), dict(stages[0][1]["radiance"])
    for kind, fz in stages:
        for p, (v, n) in fz["mesh"].items():
            if not same_arrays(held[p], (v, n)):
                g.update_mesh(p, v, n, "refit")
                held[p] = (v, n)
        for p, rec in fz["analytic"].items():
            if not (np.array_equal(rec[0], analytic[p][0]) and np.array_equal(rec[1], analytic[p][1])):
                (g.update_plane if p in model.layout.planes else g.update_sphere)(p, rec[0], rec[1])
                analytic[p] = rec
        for p, L in fz["radiance"].items():
            if not np.array_equal(L, radiance[p]):
                g.set_area_light_radiance(p, L)
                radiance[p] = L
        if kind:
            getattr(g, kind)()
    return g


# ---- one action on scene B ----------------------------------------------------------------------------------------------------------
class Pointers:
    """the device-memory inputs of one call as raw pointers of the context (freed when the call is over)"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def __call__(self, *arrays):
        out = []
        for a in arrays:
            a = np.ascontiguousarray(a)
            self.ptrs.append(self.ctx.alloc(max(a.nbytes, 16)))
            self.ctx.upload(self.ptrs[-1], a)
            out.append(self.ptrs[-1])
        return out

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)
        self.ptrs = []


def front_end(g, a, inp, tensors):
    kind, p, mode = a["kind"], a["prim"], a["mode"]
    if kind == "update_host":
        g.update_mesh(p, inp["V"], inp["N"], mode)
    elif kind == "transform":
        g.transform_mesh(p, inp["M"], mode)
    elif kind == "pose":
        g.pose_mesh(p, inp["mats"], mode)
    elif kind in ("morph", "morph_joints"):
        g.morph_mesh(p, inp["w"], inp.get("mats") if kind == "morph_joints" else None, mode)
    elif tensors:      # the device-pointer calls through torch tensors produced on the context's stream
        if kind == "update_device":
            tv, tn = tensors(inp["V"], inp["N"])
            g.update_mesh(p, tv, tn, mode)
        elif kind == "pose_device":
            g.pose_mesh(p, tensors(inp["mats"])[0], mode)
        else:
            tw, tm = tensors(inp["w"], inp["mats"] if kind == "morph_device_joints" else None)
            g.morph_mesh(p, tw, tm, mode)
    else:
        dev = Pointers(g.ctx)
        try:
            if kind == "update_device":
                pv, = dev(inp["V"])
                pn = None if inp["N"] is None else dev(inp["N"])[0]
                g.update_mesh_device(p, pv, len(inp["V"]), pn, 0 if inp["N"] is None else len(inp["N"]), mode)
                g.ctx.memset(pv, 0xFF, inp["V"].nbytes)     # the library has copied the arrays
            elif kind == "pose_device":
                g.pose_mesh_device(p, dev(inp["mats"].reshape(-1, 16))[0], len(inp["mats"]), mode)
            else:
                pw, = dev(inp["w"])
                pm = dev(inp["mats"].reshape(-1, 16))[0] if kind == "morph_device_joints" else None
                g.morph_mesh_device(p, pw, len(inp["w"]), pm, len(inp["mats"]) if pm else 0, mode)
        finally:
            dev.free()


def spheres_batch(g, prims, records, via, tensors):
    if via == "host":
        g.update_spheres(prims, records)
    elif via == "tensor" and tensors:
        g.update_spheres(prims, tensors(records)[0])
    else:
        dev = Pointers(g.ctx)
        try:
            g.update_spheres_device(prims, dev(records)[0])
        finally:
            dev.free()


def refuse(g, a, inp, tensors):
    """the refused call: the host call's error, by whichever door"""
    what, p, device = a["what"], a.get("prim"), a["via"] == "device"
    with pytest.raises(ag.AgptError) as e:
        if what in ("singular_joint", "last_row"):
            front_end(g, {"kind": "pose_device" if device else "pose", "prim": p, "mode": "refit"}, inp, tensors)
        elif what == "weight":
            front_end(g, {"kind": "morph_device" if device else "morph", "prim": p, "mode": "refit"}, inp, tensors)
        elif what == "counts":
            front_end(g, {"kind": "update_device" if device else "update_host", "prim": p, "mode": "refit"}, inp, tensors)
        elif what == "radius":
            g.update_sphere(p, inp["c"], inp["r"])
        else:
            spheres_batch(g, a["prims"], inp["records"], a["via"], tensors)
    assert REFUSAL_TEXT[what] in str(e.value), str(e.value)


def perform(g, a, inp, tensors, rays):
    """the action on scene g -> what a reader returned, as bytes (None for every other action)"""
    kind, p = a["kind"], a.get("prim")
    if kind in uw.FRONT_ENDS:
        front_end(g, a, inp, tensors)
    elif kind == "set_skin":
        s = inp["skin"]
        g.set_mesh_skin(p, s["J"], s["W"], s["nJ"], s["nW"], n_joints=s["n_joints"])
    elif kind == "set_targets":
        g.set_mesh_morph_targets(p, *inp["targets"])
    elif kind == "set_mode":
        g.set_mesh_normals_mode(p, a["value"])
    elif kind == "set_builder":
        g.set_bvh_builder(a["value"])
    elif kind == "update_sphere":
        g.update_sphere(p, inp["c"], inp["r"])
    elif kind == "update_plane":
        g.update_plane(p, inp["c"], inp["size"])
    elif kind == "set_radiance":
        g.set_area_light_radiance(p, inp["L"])
    elif kind == "update_spheres":
        spheres_batch(g, a["prims"], inp["records"], a["via"], tensors)
    elif kind in uw.SNAPSHOTS:
        getattr(g, kind)()
    elif kind == "refuse":
        refuse(g, a, inp, tensors)
    else:
        return read(g, a, rays)


def read(g, a, rays):
    if a["kind"] == "bvh":
        nodes, order = g.bvh(a["prim"])
        return nodes.tobytes() + order.tobytes()
    return PT.DbgLi(g, rays[:N_DBG]).tobytes()


# ---- the observation ------------------------------------------------------------------------------------------------------------------
def observe(g, rays, motion):
    out = {"closest": g.Intersect(rays)[0].tobytes(), "any": g.IntersectP(rays)[0].tobytes()}
    acc, st = PT.render_to_host(g, dc.W, dc.H, dc.SPP)
    out["render"], out["rays"] = acc.tobytes(), (st.rays, st.closest_rays, st.anyhit_rays)
    if motion == "snapshot_surfaces":
        names, buffers = ("albedo", "normal_depth", "prev_point", "prev_normal"), PT.render_features_surface_motion_to_host(g, dc.W, dc.H)
    elif motion:
        names, buffers = ("albedo", "normal_depth", "prev_point"), PT.render_features_motion_to_host(g, dc.W, dc.H)
    else:
        names, buffers = (), ()
    for k, x in zip(names, buffers):
        out[k] = x.tobytes()
    return out


def first_difference(a, b):
    assert list(a) == list(b), (list(a), list(b))
    return next((k for k in a if a[k] != b[k]), None)


def against_oracle(model, rays, seen, where):
    o = model.desc().instantiate(ob.OracleScene())
    oh, oa = o.intersect(rays)[0], o.intersect(rays, any_hit=True)[0]
    gh, ga = np.frombuffer(seen["closest"], ag.HIT_DTYPE), np.frombuffer(seen["any"], ag.HIT_DTYPE)
    assert np.array_equal(gh["hit"], oh["hit"]), "%s: closest-hit flags differ from the oracle's on rays %s" % (where, np.nonzero(gh["hit"] != oh["hit"])[0][:8])
    hit = oh["hit"] == 1
    assert np.array_equal(bits(gh["t"][hit]), bits(oh["t"][hit])), "%s: t differs from the oracle's on rays %s" % (where, np.nonzero(hit)[0][bits(gh["t"][hit]) != bits(oh["t"][hit])][:8])
    assert np.array_equal(ga["hit"], oa["hit"]), "%s: any-hit flags differ from the oracle's on rays %s" % (where, np.nonzero(ga["hit"] != oa["hit"])[0][:8])


# ---- a walk -------------------------------------------------------------------------------------------------------------------------------
def run_walk(w, ctx, tensors=None, check=True):
    """walk w on a fresh scene B of context ctx -> the observation after every step; check: against R and the oracle at every step, and
    the disturbing checks at the end"""
    lay, model = w.layout, uw.Model(w.layout)
    rays = dc.rays_for(lay.desc)
    b = instantiate(lay.desc, ctx)
    seen = []
    try:
        for i, a in enumerate(w.actions):
            where = "%r (seed %d) step %d: %s" % (w, w.seed, i, uw.describe(a))
            inp = model.inputs(a)
            try:
                got = perform(b, a, inp, tensors, rays)
            except ag.AgptError as e:
                raise AssertionError("%s: %s" % (where, e))
            model.apply(a, inp)
            motion = a["kind"] if a["kind"] in uw.SNAPSHOTS else None
            ob_b = observe(b, rays, motion)
            if got is not None:
                ob_b["reader"] = got
            seen.append(ob_b)
            if not check:
                continue
            r = replay(model, ctx, motion)
            try:
                ob_r = observe(r, rays, motion)
                if got is not None:
                    ob_r["reader"] = read(r, a, rays)
            finally:
                r.close()
            key = first_difference(ob_b, ob_r)
            assert key is None, "%s: '%s' differs from the replay scene's" % (where, key)
            against_oracle(model, rays, ob_b, where)
        if check:
            finish(w, model, b, ctx, rays)
    finally:
        b.close()
    return seen


def finish(w, model, b, ctx, rays):
    """the checks that read the mirror and rebuild: only at the end of a walk"""
    where = "%r (seed %d) at the end" % (w, w.seed)
    lay = w.layout
    r = replay(model, ctx, None)
    try:
        for p in lay.meshes:
            for (x, y), what in zip(zip(b.bvh(p), r.bvh(p)), ("nodes", "order")):
                assert x.tobytes() == y.tobytes(), "%s: bvh(%d) %s differ from the replay scene's" % (where, p, what)
    finally:
        r.close()
    for p in lay.meshes:
        m = model.mesh[p]
        b.set_mesh_normals_mode(p, "given")
        b.update_mesh(p, m.V, m.N, "rebuild")
    fresh = instantiate(model.desc(), ctx)
    try:
        acc, st = PT.render_to_host(b, dc.W, dc.H, dc.SPP)
        facc, fst = PT.render_to_host(fresh, dc.W, dc.H, dc.SPP)
    finally:
        fresh.close()
    assert acc.tobytes() == facc.tobytes() and (st.rays, st.closest_rays, st.anyhit_rays) == (fst.rays, fst.closest_rays, fst.anyhit_rays), \
        "%s: the rebuilt scene's render differs from a fresh scene's" % where
    oacc, ost = oracle_render(model.desc(), dc.W, dc.H, dc.SPP, max_depth=dc.DEPTH)
    assert np.array_equal(bits(acc[..., :3]), bits(oacc[..., :3])) and st.rays == ost.rays, "%s: the rebuilt scene's render differs from the oracle's" % where


@pytest.mark.parametrize("seed", uw.SEEDS)
def test_walk(seed):
    """every walk, on the shared null-stream context, device inputs as raw pointers (the sphere batch also as a host array)"""
    t0 = time.perf_counter()
    w = uw.walk(seed)
    run_walk(w, gpu_context())
    print("%r: %d actions in %.2f s" % (w, len(w.actions), time.perf_counter() - t0))


def test_a_walk_twice_gives_the_same_bytes_at_every_step():
    """two fresh scenes on one context, the same walk: an observation that depended on what an earlier call left in the context's or the
    scene's buffers would differ between the first run (cold buffers) and the second"""
    w = uw.walk(uw.SEEDS[0])
    first, second = (run_walk(w, gpu_context(), check=False) for _ in range(2))
    for i, (x, y) in enumerate(zip(first, second)):
        key = first_difference(x, y)
        assert key is None, "%r (seed %d) step %d: %s: '%s' differs between two runs" % (w, w.seed, i, uw.describe(w.actions[i]), key)


# ---- on a caller's non-blocking stream, inputs as torch tensors produced on it ----------------------------------------------------------
class StreamTensors:
    """the inputs of one call as torch tensors PRODUCED ON THE CONTEXT'S STREAM while the call is made (test_gpu_streams.py's pattern): the
    tensors first hold finite wrong values; a delay is enqueued on the stream that the host does not wait for; behind it device-to-device
    copies put the real values in place; the caller hands the tensors over at once.  A library that read them on any other stream, or
    before the stream's earlier work, sees the wrong values."""

    def __init__(self, torch, stream, delay):
        self.torch, self.stream, self.delay = torch, stream, delay

    def __call__(self, *arrays):
        torch = self.torch
        real = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
        out = [None if r is None else torch.full_like(r, 0.5) for r in real]
        self.stream.synchronize()
        self.delay.enqueue(self.stream.cuda_stream)
        for o, r in zip(out, real):
            if o is not None:
                o.copy_(r)
        return out


STREAM_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch                      # before the library touches the GPU (INTEGRATION.md section 3)
torch.zeros(1, device="cuda")
import ag_pathtracer_amd as ag
import hip_runtime
import update_walk_cases as uw
import test_gpu_update_walks as t

ag.lib()
runtimes = hip_runtime.mapped_runtimes()
assert len(runtimes) == 1, "torch and libagpt_hip.so are bound to different HIP runtime copies: %%s" %% (runtimes,)
s = torch.cuda.Stream()
ctx = ag.Context(0, stream=s.cuda_stream)
assert ctx.stream != 0
with torch.cuda.stream(s):
    delay = hip_runtime.Delay(ctx, s.cuda_stream)
    t.run_walk(uw.walk(%(seed)d), ctx, tensors=t.StreamTensors(torch, s, delay))
    s.synchronize()
    delay.free()
ctx.close()
print("walk-ok")
"""


def stream_walk(batches):
    """the first walk with (or without) a device batch of spheres handed over as a tensor"""
    for w in uw.walks():
        has = any(a["kind"] == "update_spheres" and a["via"] == "tensor" for a in w.actions)
        none = not any(a["kind"] == "update_spheres" or (a["kind"] == "refuse" and a["what"] == "sphere_record") for a in w.actions)
        if has if batches else none:
            return w
    raise AssertionError("no such walk")


@pytest.mark.parametrize("batches", [True, False], ids=["sphere_batches", "no_sphere_batch"])
def test_walk_on_a_non_blocking_stream(batches):
    """a walk with and one without device batches of spheres, repeated with the context on a torch.cuda.Stream() -- non-blocking, a
    non-zero handle -- and every device input a torch tensor produced on that stream behind a delay (StreamTensors); R and the oracle as
    in test_walk.  In a child process: torch must initialise the GPU before the library does, and the child first checks that both are
    bound to one HIP runtime copy (test_gpu_mesh_update_device.py's rule)."""
    w = stream_walk(batches)
    code = STREAM_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "seed": w.seed}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "walk-ok" in r.stdout, "%r (seed %d)\n%s%s" % (w, w.seed, r.stdout[-2000:], r.stderr[-4000:])
