"""Developer measurement: what moving a sphere, a plane or a light in a committed scene costs (agpt_scene_update_sphere,
agpt_scene_set_area_light_radiance, agpt_scene_update_spheres_device) beside the agpt_scene_commit they replace, into
profiles/analytic_update_times.json.

    python tools/analytic_update_time.py [--runs 9] [--out profiles/analytic_update_times.json] [--parent-lib TAG] [--rounds 3]

Every row is the host clock around one call that ends in a synchronise of the context's stream; the rows take turns in one process
(row A, row B, row A, ...) after one warm-up turn, --runs timed turns, and are reported as median (min - max) in ms.
  update_sphere / set_area_light_radiance   C3's first area light
  update_spheres_device                     n = 1, 64 and 2000 records, resident on the device, on a 2000-sphere scene
  agpt_scene_commit                         C3, in the same turns, and behind it a 4-byte agpt_device_memset: the first call after the
                                            commit's uploads, whichever it is, waits for work the runtime deferred
--parent-lib TAG: the calls this change touches without being asked to -- agpt_scene_snapshot_positions and
agpt_render_features_motion on C3 at 1080p, nothing moved -- of this build against the build `libagpt_hip_TAG.so` of the parent commit
(tools/build_variant.py run in a checkout of it, the file copied beside libagpt_hip.so): child processes, alternating parent / this
for --rounds rounds on the same GPU."""
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

W, H = 1920, 1080
N_SPHERES = 2000
PRIM_OPS = ("mesh", "sphere", "plane", "area_light")


def turns(rows, runs):
    """rows: {name: callable(k)}; one warm-up turn, then `runs` timed turns -> {name: {median_ms, min_ms, max_ms, runs_ms}}"""
    times = {name: [] for name in rows}
    for k in range(runs + 1):
        for name, fn in rows.items():
            t0 = time.perf_counter()
            fn(k)
            if k:
                times[name].append(1e3 * (time.perf_counter() - t0))
    return {name: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                   "runs_ms": [round(x, 4) for x in t]} for name, t in times.items()}


def show(res):
    for name, r in res.items():
        print("%-52s %9.4f ms (%.4f - %.4f)" % (name, r["median_ms"], r["min_ms"], r["max_ms"]), flush=True)


def sphere_field():
    """2000 spheres on a 50 x 40 grid above a plane, the last one a light"""
    d = ag.SceneDesc("spheres-%d" % N_SPHERES)
    m = d.add_material(ag.MAT_DIFFUSE_ONLY, (0.6, 0.6, 0.6))
    for k in range(N_SPHERES - 1):
        d.add_sphere((0.5 * (k % 50) - 12.25, 0.5 * (k // 50) + 0.3, 0.0), 0.2, m)
    d.add_area_light((0.0, 25.0, -10.0), 1.0, (200.0, 200.0, 200.0))
    d.add_plane((0.0, 0.0, 0.0), (40.0, 40.0), m)
    d.set_camera([0, 10, -30], [0, 10, 0], [0, 1, 0], W / float(H), 45.0, 0.0)
    return d


def unchanged_paths(runs):
    """the child of --parent-lib: the snapshot and the motion feature pass on C3 at 1080p, nothing moved, through whichever library
    AGPT_LIB_VARIANT names"""
    ctx = ag.Context(0)
    scene = ag.scenes.scene_c3(aspect=W / float(H)).instantiate(ag.Scene(ctx))
    pt = ag.PathTracer(5)
    bufs = [ctx.alloc(W * H * 16) for _ in range(3)]
    scene.snapshot_positions()
    res = turns({"agpt_scene_snapshot_positions": lambda k: scene.snapshot_positions(),
                 "agpt_render_features_motion": lambda k: pt.render_features_motion(scene, W, H, *bufs)}, runs)
    print("RESULT " + json.dumps(res), flush=True)


def compare_with_parent(tag, runs, rounds):
    names = ("agpt_scene_snapshot_positions", "agpt_render_features_motion")
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
            sets[which].append(json.loads(line[7:]))
            print(which, line[7:], flush=True)
    out = {"method": "child processes alternating parent / this on one GPU, %d rounds of %d timed calls each after one warm-up; per "
                     "build the median of the rounds' medians, the lowest min and the highest max" % (rounds, runs)}
    for name in names:
        out[name] = {}
        for which in ("parent", "this"):
            rs = [r[name] for r in sets[which]]
            out[name][which] = {"median_ms": round(statistics.median(r["median_ms"] for r in rs), 4), "min_ms": min(r["min_ms"] for r in rs),
                                "max_ms": max(r["max_ms"] for r in rs), "rounds_median_ms": [r["median_ms"] for r in rs]}
        out[name]["parent_slowest_round_ms"] = max(out[name]["parent"]["rounds_median_ms"])
        out[name]["this_median_within_parent_rounds"] = bool(out[name]["this"]["median_ms"] <= out[name]["parent_slowest_round_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "analytic_update_times.json"))
    ap.add_argument("--parent-lib", default=None, metavar="TAG")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.runs < 9:
        ap.error("--runs: at least 9")
    if a.child:
        return unchanged_paths(a.runs)
    import hashlib
    import torch
    ctx = ag.Context(0)
    res = {"device": torch.cuda.get_device_name(0),
           "command": "python tools/analytic_update_time.py --runs %d --rounds %d%s" % (a.runs, a.rounds, " --parent-lib " + a.parent_lib if a.parent_lib else ""),
           "library_sha256": hashlib.sha256(open(ag.library_path(), "rb").read()).hexdigest(),
           "method": "host clock around each synchronised call; the rows take turns in one process, one warm-up turn, then %d timed turns: "
                     "median (min - max)" % a.runs}
    c3 = ag.scenes.scene_c3(aspect=W / float(H))
    prims = [op for op in c3.ops if op[0] in PRIM_OPS]
    light = [k for k, op in enumerate(prims) if op[0] == "area_light"][0]
    centre, radius, L = prims[light][1], prims[light][2], prims[light][3]
    scene = c3.instantiate(ag.Scene(ctx))
    field = sphere_field().instantiate(ag.Scene(ctx))
    rng = np.random.RandomState(1)
    word = ctx.alloc(16)
    # (the commit comes first and a 4-byte memset behind it: the first call after the commit's large pageable uploads waits for what the
    # runtime deferred, whichever call it is; that wait is reported as a row of its own and not charged to the calls measured here)
    rows = {"agpt_scene_commit (C3)": lambda k: scene.commit(),
            "agpt_device_memset of 4 bytes, first call after the commit": lambda k: ctx.memset(word, 0, 4),
            "agpt_scene_update_sphere (C3's first light)": lambda k: scene.update_sphere(light, centre + np.float32(0.01 * k), radius),
            "agpt_scene_set_area_light_radiance (C3's first light)": lambda k: scene.set_area_light_radiance(light, L * np.float32(1 + 0.01 * k))}
    for n in (1, 64, N_SPHERES):
        ids = rng.permutation(N_SPHERES)[:n].astype(np.int32)
        rec = np.zeros((n, 4), np.float32)
        rec[:, 0], rec[:, 1], rec[:, 3] = 0.5 * (ids % 50) - 12.25, 0.5 * (ids // 50) + 0.3, 0.2
        ptr = ctx.alloc(rec.nbytes)
        ctx.upload(ptr, rec)
        rows["agpt_scene_update_spheres_device n = %d" % n] = lambda k, ids=ids, ptr=ptr: field.update_spheres_device(ids, ptr)
    res["triangles_c3"], res["primitives_c3"] = c3.n_tris, c3.n_prims
    res["update"] = turns(rows, a.runs)
    show(res["update"])
    commit = res["update"]["agpt_scene_commit (C3)"]["median_ms"]
    res["commit_over_call"] = {name: round(commit / r["median_ms"], 1) for name, r in res["update"].items() if name.startswith("agpt_scene_") and "commit" not in name}
    scene.close()
    field.close()
    ctx.close()
    if a.parent_lib:
        res["unchanged_paths_parent_against_this"] = compare_with_parent(a.parent_lib, a.runs, a.rounds)
        for name, c in res["unchanged_paths_parent_against_this"].items():
            if isinstance(c, dict):
                print("%s: parent %.3f ms (%.3f - %.3f), this %.3f ms (%.3f - %.3f)"
                      % ((name,) + tuple(c[w][k] for w in ("parent", "this") for k in ("median_ms", "min_ms", "max_ms"))))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("->", a.out)


if __name__ == "__main__":
    main()
