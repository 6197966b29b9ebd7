"""Developer measurement: what the motion-vector calls cost (agpt_scene_snapshot_positions, agpt_render_features_motion,
agpt_temporal_accumulate_motion) beside the calls they extend, into profiles/motion_c3.json.

    python tools/motion_cost.py [--runs 9] [--out profiles/motion_c3.json] [--parent-lib TAG] [--rounds 3]

Every row is the host clock around one call that ends in a synchronise of the context's stream; the rows of a group take turns in one
process (row A, row B, row A, ...) after one warm-up turn, --runs timed turns, and are reported as median (min - max) in ms.
  snapshot   agpt_scene_snapshot_positions on C3 (258,672 triangles) and on the 999,698-triangle heightfield
  features   agpt_render_features against agpt_render_features_motion on C3 at 1080p
  temporal   agpt_temporal_accumulate against agpt_temporal_accumulate_motion with nothing moved (every w in {0, 2}) and with every
             hit pixel moved (w == 1, the point being the one seen now), on two 4-spp frames of C3 at 1080p one degree of orbit apart
--parent-lib TAG: agpt_temporal_accumulate of this build against the build `libagpt_hip_TAG.so` of the parent commit
(tools/build_variant.py run in a checkout of it, the file copied beside libagpt_hip.so): child processes, alternating parent / this
for --rounds rounds on the same GPU.
--surfaces: the previous-frame-normal calls beside those rows, into profiles/surface_motion_c3.json: agpt_scene_snapshot_surfaces beside
agpt_scene_snapshot_positions (the difference is a device copy of 64 B per triangle), agpt_render_features_surface_motion beside
agpt_render_features_motion, agpt_temporal_accumulate_surface_motion beside agpt_temporal_accumulate_motion and beside
agpt_temporal_accumulate_clamped (r = 2), with nothing moved and with every hit pixel moved (prev_normal = the current normal)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import ag_pathtracer_amd as ag  # noqa: E402

W, H, SPP = 1920, 1080, 4
HEIGHTFIELD_QUADS = 707   # 2 * 707^2 = 999,698 triangles


def turns(rows, runs):
    """rows: {name: callable}; one warm-up turn, then `runs` timed turns -> {name: {median_ms, min_ms, max_ms, runs_ms}}"""
    times = {name: [] for name in rows}
    for k in range(runs + 1):
        for name, fn in rows.items():
            t0 = time.perf_counter()
            fn()
            if k:
                times[name].append(1e3 * (time.perf_counter() - t0))
    return {name: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                   "runs_ms": [round(x, 4) for x in t]} for name, t in times.items()}


def show(group, res):
    for name, r in res.items():
        print("%-9s %-46s %8.3f ms (%.3f - %.3f)" % (group, name, r["median_ms"], r["min_ms"], r["max_ms"]), flush=True)


class Frames:
    """two 4-spp frames of C3 at 1080p, one degree of orbit apart, with their feature buffers on the device"""

    def __init__(self, ctx):
        self.ctx = ctx
        desc = ag.scenes.scene_c3(aspect=W / float(H))
        self.scene = desc.instantiate(ag.Scene(ctx))
        self.cams = [ag.scenes.orbit_camera(desc.camera, k) for k in (0.0, 1.0)]
        pt = ag.PathTracer(5)
        n16, n4 = W * H * 16, W * H * 4
        self.sets = []
        for k, cam in enumerate(self.cams):
            acc, m2, albedo, nd = ctx.alloc(n16), ctx.alloc(n4), ctx.alloc(n16), ctx.alloc(n16)
            ctx.memset(acc, 0, n16)
            ctx.memset(m2, 0, n4)
            self.scene.set_camera(*cam)
            pt.render_adaptive(self.scene, W, H, acc, m2, SPP, SPP, SPP, 0.0, seed_base=k)
            pt.render_features(self.scene, W, H, albedo, nd)
            self.sets.append((acc, m2, albedo, nd))
        self.out = (ctx.alloc(n16), ctx.alloc(n4))
        # frame 1 is the current one, frame 0 (its own history) the previous one
        self.params = ag.TemporalParams(W, H, ag.camera_desc(*self.cams[1]), ag.camera_desc(*self.cams[0]), 32.0, ag.TEMPORAL_DEPTH_TOL,
                                        ag.TEMPORAL_NORMAL_COS)
        self.buffers = self.sets[1] + self.sets[0] + self.out

    def accumulate(self):
        self.ctx.temporal_accumulate(self.params, *self.buffers)


def temporal_only(runs):
    """the child of --parent-lib: agpt_temporal_accumulate alone, through whichever library AGPT_LIB_VARIANT names"""
    ctx = ag.Context(0)
    f = Frames(ctx)
    print("RESULT " + json.dumps(turns({"agpt_temporal_accumulate": f.accumulate}, runs)), flush=True)


def compare_with_parent(tag, runs, rounds):
    sets = {"parent": [], "this": []}
    for _ in range(rounds):
        for which in ("parent", "this"):
            env = dict(os.environ)
            env.pop("AGPT_LIB_VARIANT", None)
            if which == "parent":
                env["AGPT_LIB_VARIANT"] = tag
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(runs)], env=env, capture_output=True, text=True,
                               timeout=900, check=True)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
            sets[which].append(json.loads(line[7:])["agpt_temporal_accumulate"])
            print(which, line[7:], flush=True)
    out = {"method": "child processes alternating parent / this on one GPU, %d rounds of %d timed calls each after one warm-up; per "
                     "build the median of the rounds' medians, the lowest min and the highest max" % (rounds, runs)}
    for which in ("parent", "this"):
        rs = sets[which]
        out[which] = {"median_ms": round(statistics.median(r["median_ms"] for r in rs), 4), "min_ms": min(r["min_ms"] for r in rs),
                      "max_ms": max(r["max_ms"] for r in rs), "rounds": rs}
    out["this_median_within_parent_spread"] = bool(out["parent"]["min_ms"] <= out["this"]["median_ms"] <= out["parent"]["max_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "motion_c3.json"))
    ap.add_argument("--parent-lib", default=None, metavar="TAG")
    ap.add_argument("--surfaces", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.surfaces and a.out == ap.get_default("out"):
        a.out = os.path.join(os.path.dirname(a.out), "surface_motion_c3.json")
    if a.runs < 9:
        ap.error("--runs: at least 9")
    if a.child:
        return temporal_only(a.runs)
    import hashlib
    import torch
    ctx = ag.Context(0)
    # (the command as far as it decides what is measured: where the file goes is left out)
    res = {"device": torch.cuda.get_device_name(0),
           "command": "python tools/motion_cost.py --runs %d --rounds %d%s%s" % (a.runs, a.rounds, " --surfaces" if a.surfaces else "",
                                                                                " --parent-lib " + a.parent_lib if a.parent_lib else ""),
           "library_sha256": hashlib.sha256(open(ag.library_path(), "rb").read()).hexdigest(),
           "method": "host clock around each synchronised call; the rows of a group take turns in one process, one warm-up turn, then "
                     "%d timed turns: median (min - max)" % a.runs,
           "config": dict(W=W, H=H, spp=SPP)}
    f = Frames(ctx)
    hf = ag.scenes.scene_heightfield(HEIGHTFIELD_QUADS, True, W, H).instantiate(ag.Scene(ctx))
    res["triangles"] = {"c3": ag.scenes.scene_c3(aspect=W / float(H)).n_tris, "heightfield": 2 * HEIGHTFIELD_QUADS ** 2}
    res["snapshot"] = turns({"agpt_scene_snapshot_positions c3": f.scene.snapshot_positions,
                             "agpt_scene_snapshot_positions heightfield": hf.snapshot_positions}, a.runs)
    show("snapshot", res["snapshot"])
    if a.surfaces:
        # (after the rows above: consecutive agpt_scene_snapshot_surfaces calls keep the shading generations allocated, as a frame loop does)
        res["snapshot_surfaces"] = turns({"agpt_scene_snapshot_surfaces c3": f.scene.snapshot_surfaces,
                                          "agpt_scene_snapshot_surfaces heightfield": hf.snapshot_surfaces}, a.runs)
        res["snapshot_surfaces"]["copy_bytes"] = {k: 64 * v for k, v in res["triangles"].items()}
        show("snapshot", {k: v for k, v in res["snapshot_surfaces"].items() if "median_ms" in v})
    hf.close()

    pt = ag.PathTracer(5)
    n16 = W * H * 16
    albedo, nd, point = ctx.alloc(n16), ctx.alloc(n16), ctx.alloc(n16)
    f.scene.set_camera(*f.cams[1])
    res["features"] = turns({"agpt_render_features": lambda: pt.render_features(f.scene, W, H, albedo, nd),
                             "agpt_render_features_motion": lambda: pt.render_features_motion(f.scene, W, H, albedo, nd, point)}, a.runs)
    if a.surfaces:
        normal = ctx.alloc(n16)
        f.scene.snapshot_surfaces()
        res["features"].update(turns({"agpt_render_features_motion (beside the next row)": lambda: pt.render_features_motion(f.scene, W, H, albedo, nd, point),
                                      "agpt_render_features_surface_motion": lambda: pt.render_features_surface_motion(f.scene, W, H, albedo, nd, point, normal)},
                                     a.runs))
    show("features", res["features"])

    pp = ctx.download(point, (H, W, 4))
    assert set(np.unique(pp[..., 3])) <= {0.0, 2.0}
    moved = pp.copy()
    moved[..., 3] = np.where(pp[..., 3] == 2, np.float32(1), pp[..., 3])
    point_moved = ctx.alloc(n16)
    ctx.upload(point_moved, moved)
    res["temporal"] = turns({"agpt_temporal_accumulate": f.accumulate,
                             "agpt_temporal_accumulate_motion, every w in {0, 2}": lambda: ctx.temporal_accumulate_motion(f.params, *f.buffers, point),
                             "agpt_temporal_accumulate_motion, every hit pixel w == 1": lambda: ctx.temporal_accumulate_motion(f.params, *f.buffers, point_moved)},
                            a.runs)
    if a.surfaces:
        same = np.concatenate([ctx.download(f.sets[1][3], (H, W, 4))[..., :3], pp[..., 3:]], -1)
        same_moved = np.concatenate([same[..., :3], moved[..., 3:]], -1)
        normal_same, normal_moved = ctx.alloc(n16), ctx.alloc(n16)
        ctx.upload(normal_same, same)
        ctx.upload(normal_moved, same_moved)
        clamp = ag.TemporalClampParams(2, 1, 1.0, 8.0)
        rows = {}
        for what, pt_, pn_ in (("every w in {0, 2}", point, normal_same), ("every hit pixel w == 1", point_moved, normal_moved)):
            rows["agpt_temporal_accumulate_motion, " + what + " (again)"] = lambda pt_=pt_: ctx.temporal_accumulate_motion(f.params, *f.buffers, pt_)
            rows["agpt_temporal_accumulate_surface_motion, " + what] = \
                lambda pt_=pt_, pn_=pn_: ctx.temporal_accumulate_surface_motion(f.params, None, *f.buffers, pt_, pn_)
            rows["agpt_temporal_accumulate_clamped r = 2, " + what] = lambda pt_=pt_: ctx.temporal_accumulate_clamped(f.params, clamp, *f.buffers, pt_)
            rows["agpt_temporal_accumulate_surface_motion clamp r = 2, " + what] = \
                lambda pt_=pt_, pn_=pn_: ctx.temporal_accumulate_surface_motion(f.params, clamp, *f.buffers, pt_, pn_)
        res["temporal_surfaces"] = turns(rows, a.runs)
        show("temporal", res["temporal_surfaces"])
    res["temporal"]["hit_pixels"] = int((pp[..., 3] == 2).sum())
    show("temporal", {k: v for k, v in res["temporal"].items() if isinstance(v, dict)})
    f.scene.close()
    ctx.close()
    if a.parent_lib:
        res["agpt_temporal_accumulate_parent_against_this"] = compare_with_parent(a.parent_lib, a.runs, a.rounds)
        c = res["agpt_temporal_accumulate_parent_against_this"]
        print("agpt_temporal_accumulate: parent %.3f ms (%.3f - %.3f), this %.3f ms (%.3f - %.3f)"
              % tuple(c[w][k] for w in ("parent", "this") for k in ("median_ms", "min_ms", "max_ms")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("->", a.out)


if __name__ == "__main__":
    main()
