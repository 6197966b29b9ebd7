"""Developer measurement: exact against fast shading arithmetic (agpt_scene_set_shading_arith) in one process, on C3 at
1080p / 64 spp and on one rank's share of an 8-way split of C5 at 4K (64 spp), each mode run three times, alternating, after a
warm-up.  Per mode: step ms, trace ms, non-trace ms (k_shade, k_generate, k_accumulate and the iteration's small launches), shaded
vertices and non-trace ns per shaded vertex (medians).
    python tools/shade_arith_ab.py [--out profiles/shade_arith_ab.json] [--reps 3] [--scenes c3,c5] [--no-warmup]
(--scenes c3 --reps 1 --no-warmup: exactly one C3 render per mode, for a rocprofv3 run whose sums are per step)"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import ag_pathtracer_amd as ag  # noqa: E402
from ag_pathtracer_amd import tiles  # noqa: E402


def run(label, desc, W, H, spp, interleave, reps, warmup=True):
    ctx = ag.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    scene = desc.instantiate(ag.Scene(ctx))
    rows = tiles.max_local_rows(H, interleave[1]) if interleave else H
    local = torch.zeros((rows, W, 4), device="cuda")
    pt = ag.PathTracer(5)

    def step(mode):
        scene.set_shading_arith(mode)
        local.zero_()
        return pt.render(scene, W, H, spp, local.data_ptr(), accum_pitch=W, timing=True, interleave=interleave)

    for mode in ("exact", "fast") if warmup else ():   # warm-up
        step(mode)
    runs = {"exact": [], "fast": []}
    for _ in range(reps):
        for mode in ("exact", "fast"):
            st = step(mode)
            runs[mode].append(dict(step_ms=st.total_ms, trace_ms=st.trace_ms, non_trace_ms=st.total_ms - st.trace_ms,
                                   shaded=int(st.shaded_vertices), rays=int(st.rays)))
    out = {}
    for mode, rs in runs.items():
        med = {k: statistics.median(r[k] for r in rs) for k in ("step_ms", "trace_ms", "non_trace_ms")}
        med["shaded_vertices"] = rs[0]["shaded"]
        med["rays"] = rs[0]["rays"]
        med["non_trace_ns_per_shaded_vertex"] = med["non_trace_ms"] * 1e6 / max(1, med["shaded_vertices"])
        med["runs"] = rs
        out[mode] = med
        print("%-4s %-5s step %7.1f ms  trace %7.1f  non-trace %6.1f  shaded %6.1f M  %.3f ns/vertex" % (
            label, mode, med["step_ms"], med["trace_ms"], med["non_trace_ms"], med["shaded_vertices"] / 1e6,
            med["non_trace_ns_per_shaded_vertex"]), flush=True)
    out["non_trace_speedup"] = out["exact"]["non_trace_ms"] / out["fast"]["non_trace_ms"]
    out["step_speedup"] = out["exact"]["step_ms"] / out["fast"]["step_ms"]
    out["config"] = dict(W=W, H=H, spp=spp, interleave=list(interleave) if interleave else None, tris=desc.n_tris)
    scene.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", default="c3,c5")
    ap.add_argument("--no-warmup", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    for sc in a.scenes.split(","):
        if sc == "c3":
            res["c3"] = run("c3", ag.scenes.scene_c3(aspect=1920 / 1080.), 1920, 1080, 64, None, a.reps, not a.no_warmup)
        elif sc == "c5":
            res["c5"] = run("c5", ag.scenes.scene_c5(aspect=3840 / 2160.), 3840, 2160, 64, (tiles.BLOCK_ROWS, 8, 0), a.reps,
                            not a.no_warmup)
        else:
            raise SystemExit("unknown scene %r (c3, c5)" % sc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("->", a.out)


if __name__ == "__main__":
    main()
