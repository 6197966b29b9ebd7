"""Host vs device BVH build time, and agpt_scene_commit (flatten + upload) time, on the C3 meshes, each of C5's 17 meshes and
a 5 M-triangle heightfield.  Every number is the median of `--runs` runs after one warm-up, host clock around synchronised
calls (agpt_bvh_build_device downloads its result, so its time is end to end: upload, build, download).

    python tools/bvh_build_time.py [--runs 5] [--out profiles/bvh_build_times.json] [--only-device]

--only-device times nothing but the device builds (for a `rocprofv3 --kernel-trace --stats` run of the kernels alone)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ag_pathtracer_amd as ag  # noqa: E402


def median_ms(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def meshes(desc):
    return [(op[1], op[4], op[6]) for op in desc.ops if op[0] == "mesh"]


def commit_ms(ctx, desc, runs):
    ts = []
    for r in range(runs + 1):
        s = ag.Scene(ctx)
        s.set_bvh_builder("device")
        for op in desc.ops:  # instantiate() without its commit
            k = op[0]
            if k == "material":
                s.add_material(op[1], op[2], op[3], op[4])
            elif k == "mesh":
                s.add_mesh(op[1], op[2], op[3], op[4], op[5], op[6])
            elif k == "sphere":
                s.add_sphere(op[1], op[2], op[3])
            elif k == "plane":
                s.add_plane(op[1], op[2], op[3])
            elif k == "area_light":
                s.add_area_light(op[1], op[2], op[3])
            elif k == "infinite_light":
                s.add_uniform_infinite_light(op[1])
            elif k == "env_light":
                s.add_infinite_area_light(op[1])
        if desc.camera is not None:
            s.set_camera(*desc.camera)
        t0 = time.perf_counter()
        s.commit()
        if r:
            ts.append((time.perf_counter() - t0) * 1e3)
        s.close()
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-device", action="store_true")
    a = ap.parse_args()
    ctx = ag.Context(0)
    hf = ag.scenes.heightfield(1581)
    sets = [("c3", ag.scenes.scene_c3()), ("c5", ag.scenes.scene_c5()), ("heightfield_5m", None)]
    out = {"runs": a.runs, "statistic": "median ms after one warm-up", "host_threads_env": os.environ.get("AGPT_BVH_THREADS"),
           "cpus": len(os.sched_getaffinity(0)), "scenes": {}}
    for name, desc in sets:
        ms = meshes(desc) if desc is not None else [(hf[0], hf[3], 1)]
        rows = []
        for k, (v, ix, mp) in enumerate(ms):
            if a.only_device:
                for _ in range(a.runs + 1):
                    assert ag.bvh_build_device(ctx, v, ix, mp)[3] == 1
                continue
            dev = ag.bvh_build_device(ctx, v, ix, mp)
            host = ag.bvh_build(v, ix, mp)
            assert dev[3] == 1 and dev[0].tobytes() == host[0].tobytes() and np.array_equal(dev[1], host[1])
            h = median_ms(lambda: ag.bvh_build(v, ix, mp), a.runs)
            d = median_ms(lambda: ag.bvh_build_device(ctx, v, ix, mp), a.runs)
            rows.append({"mesh": k, "tris": int(ix.shape[0] // 3), "nodes": int(len(host[0]) - 1), "host_ms": round(h, 3),
                         "device_ms": round(d, 3), "host_over_device": round(h / d, 3)})
            print("%s mesh %d: %d tris host %.2f ms device %.2f ms (x%.2f)" % (name, k, rows[-1]["tris"], h, d, h / d), flush=True)
        if a.only_device:
            continue
        entry = {"meshes": rows, "tris": sum(r["tris"] for r in rows), "host_ms": round(sum(r["host_ms"] for r in rows), 3),
                 "device_ms": round(sum(r["device_ms"] for r in rows), 3)}
        if desc is not None:
            entry["commit_ms"] = round(commit_ms(ctx, desc, a.runs), 3)
        else:
            sd = ag.scenes.scene_heightfield(1581)
            entry["commit_ms"] = round(commit_ms(ctx, sd, a.runs), 3)
        entry["host_over_device"] = round(entry["host_ms"] / entry["device_ms"], 3)
        out["scenes"][name] = entry
        print(name, json.dumps({k: v for k, v in entry.items() if k != "meshes"}), flush=True)
    ctx.close()
    if a.out and not a.only_device:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
