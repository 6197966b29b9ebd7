"""Adaptive sampling on C3 at 1080p (agpt_render_adaptive) against uniform agpt_render: time, error and the round structure.

    python tools/adaptive_sampling.py [--out profiles/adaptive_c3.json] [--profile-only]

Reference image: a uniform 1024-spp render with another seed_base.  Uniform 64 spp is timed and its RMSE taken; adaptive renders
(min 16 / step 16 / max 256) are swept over rel_error, each from a fresh frame: time of one call, RMSE, samples, the count
histogram, and -- from a second run in calls of one round each (max_spp = 16, 32, ...; the frame continues exactly) -- the ms and
active pixels per round.  A full-tile round through the active list is compared with agpt_render at the same batch (16 spp).
--profile-only runs one adaptive render and one resolve, for `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ag_pathtracer_amd as ag  # noqa: E402

W, H = 1920, 1080
MIN, STEP, MAX = 16, 16, 256
FLOOR = 0.01
REF_SEED = 0x5EED1024


def rmse(img, ref):
    return float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))


def rmse_display(img, ref):
    """RMSE of the radiance clamped to [0, 1] (what CopyToSurface can show): the linear RMSE is dominated by a few very bright
    pixels (directly seen emitters, fireflies)"""
    # (tools/denoise_quality.py has its own rmse_display)
    return rmse(np.clip(img, 0, 1), np.clip(ref, 0, 1))


def traversed(st):
    return int(st.closest_rays + st.anyhit_rays - st.answered_rays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_c3.json"))
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--rel", type=float, nargs="*", default=[0.5, 0.35, 0.3, 0.27, 0.25, 0.18, 0.13, 0.09])
    args = ap.parse_args()
    ctx = ag.Context(0)
    scene = ag.scenes.scene_c3(aspect=W / float(H)).instantiate(ag.Scene(ctx))
    pt = ag.PathTracer(5)
    pa, pm = ctx.alloc(W * H * 16), ctx.alloc(W * H * 4)

    def fresh():
        ctx.memset(pa, 0, W * H * 16)
        ctx.memset(pm, 0, W * H * 4)

    if args.profile_only:
        for rel in (args.rel[len(args.rel) // 2],):
            fresh()
            st, ast = pt.render_adaptive(scene, W, H, pa, pm, MIN, MAX, STEP, rel, FLOOR)
            ctx.resolve_counts(pa, W * H)
            print("profile run: rel %.3f rounds %d samples %d ms %.1f" % (rel, ast.rounds, ast.samples, st.total_ms))
        # a full-tile round through the list, and agpt_render at the same batch
        fresh()
        pt.render_adaptive(scene, W, H, pa, pm, MIN, MIN, STEP, 0.0, FLOOR)
        pt.render_adaptive(scene, W, H, pa, pm, MIN, 2 * MIN, STEP, 0.0, FLOOR)
        pt.render(scene, W, H, STEP, pa, spp_begin=MIN, samples_per_batch=STEP)
        return

    out = {"scene": "C3 (BASELINE configs[2]) 1920x1080, MaxDepth 5", "min_spp": MIN, "step_spp": STEP, "max_spp": MAX, "abs_floor": FLOOR,
           "reference": "uniform 1024 spp, seed_base 0x%08X; RMSE over pixels and channels of linear radiance" % REF_SEED}
    # reference
    ctx.memset(pa, 0, W * H * 16)
    st = pt.render(scene, W, H, 1024, pa, seed_base=REF_SEED)
    ref = ctx.download(pa, (H, W, 4))[..., :3].astype(np.float64) / 1024
    out["reference_ms"] = st.total_ms
    # uniform 64 spp
    times = []
    for _ in range(4):
        ctx.memset(pa, 0, W * H * 16)
        st = pt.render(scene, W, H, 64, pa)
        times.append(st.total_ms)
    img = ctx.download(pa, (H, W, 4))[..., :3] / np.float32(64)
    out["uniform64"] = {"ms": float(np.median(times[1:])), "ms_runs": times, "rmse": rmse(img, ref), "rmse_display": rmse_display(img, ref), "samples": W * H * 64,
                        "traversed_rays": traversed(st)}
    print("uniform 64:", out["uniform64"], flush=True)
    # adaptive sweep
    sweep = []
    for rel in args.rel:
        fresh()
        pt.render_adaptive(scene, W, H, pa, pm, MIN, MAX, STEP, rel, FLOOR)   # (warm: pool and code objects)
        fresh()
        st, ast = pt.render_adaptive(scene, W, H, pa, pm, MIN, MAX, STEP, rel, FLOOR)
        acc = ctx.download(pa, (H, W, 4))
        counts = acc[..., 3].astype(np.int64)
        img = acc[..., :3] / acc[..., 3:4]
        levels, hist = np.unique(counts, return_counts=True)
        # the same render, one round per call
        fresh()
        rounds = []
        for m in range(MIN, MAX + 1, STEP):
            s1, a1 = pt.render_adaptive(scene, W, H, pa, pm, MIN, m, STEP, rel, FLOOR)
            if a1.rounds:
                rounds.append({"max_spp": m, "ms": round(s1.total_ms, 3), "active_pixels": a1.active_last, "samples": a1.samples,
                               "traversed_rays": traversed(s1)})
        split = ctx.download(pa, (H, W, 4))
        assert split.tobytes() == acc.tobytes(), "one-round-per-call render differs from the single call"
        few = [r for r in rounds if r["active_pixels"] < W * H // 10]
        rec = {"rel_error": rel, "ms": st.total_ms, "rmse": rmse(img, ref), "rmse_display": rmse_display(img, ref), "samples": int(ast.samples), "rounds": ast.rounds,
               "mean_spp": float(counts.mean()), "pixels_stopped": int(ast.pixels_stopped),
               "count_histogram": {str(int(k)): int(v) for k, v in zip(levels, hist)},
               "traversed_rays": traversed(st), "per_round": rounds,
               "per_round_ms_sum": round(sum(r["ms"] for r in rounds), 3),
               "tail_rounds_under_10pct_active": {"rounds": len(few), "ms": round(sum(r["ms"] for r in few), 3),
                                                  "share_of_per_round_ms": round(sum(r["ms"] for r in few) /
                                                                                 max(1e-9, sum(r["ms"] for r in rounds)), 4),
                                                  "samples": int(sum(r["samples"] for r in few))}}
        print("rel %.3f: ms %.1f rmse %.5f display %.5f mean spp %.1f rounds %d" % (rel, rec["ms"], rec["rmse"], rec["rmse_display"], rec["mean_spp"], rec["rounds"]), flush=True)
        sweep.append(rec)
    out["adaptive_sweep"] = sweep
    u = out["uniform64"]
    eq_time = min(sweep, key=lambda r: abs(r["ms"] - u["ms"]))
    out["equal_time"] = {"rel_error": eq_time["rel_error"], "ms": eq_time["ms"], "uniform64_ms": u["ms"]}
    for metric in ("rmse", "rmse_display"):
        out["equal_time"][metric] = eq_time[metric]
        out["equal_time"]["uniform64_" + metric] = u[metric]
        out["equal_time"][metric + "_ratio"] = eq_time[metric] / u[metric]
        reach = [r for r in sweep if r[metric] <= u[metric]]
        best = min(reach, key=lambda r: r["ms"]) if reach else None
        out["equal_error_" + metric] = ({"rel_error": best["rel_error"], "ms": best["ms"], metric: best[metric], "uniform64_ms": u["ms"],
                                         "time_ratio": best["ms"] / u["ms"]} if best else
                                        {"note": "no rel_error of the sweep reached uniform 64 spp's " + metric})
    # a full-tile round through the list against agpt_render at the same batch (16 spp of every pixel)
    rates = {"adaptive_full_round": [], "render_16spp_batch": []}
    for _ in range(4):
        fresh()
        pt.render_adaptive(scene, W, H, pa, pm, MIN, MIN, STEP, 0.0, FLOOR)
        s_a, a_a = pt.render_adaptive(scene, W, H, pa, pm, MIN, 2 * MIN, STEP, 0.0, FLOOR)
        assert a_a.active_last == W * H and a_a.rounds == 1
        s_r = pt.render(scene, W, H, STEP, pa, spp_begin=MIN, samples_per_batch=STEP)
        rates["adaptive_full_round"].append((traversed(s_a), s_a.total_ms))
        rates["render_16spp_batch"].append((traversed(s_r), s_r.total_ms))
    fr = {}
    for k, v in rates.items():
        ms = float(np.median([t for _, t in v[1:]]))
        fr[k] = {"ms": ms, "traversed_rays": v[-1][0], "traversed_mrays_s": v[-1][0] / ms / 1e3}
    fr["ratio"] = fr["adaptive_full_round"]["traversed_mrays_s"] / fr["render_16spp_batch"]["traversed_mrays_s"]
    out["full_round_vs_render"] = fr
    print("full round:", fr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.free(pa)
    ctx.free(pm)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
