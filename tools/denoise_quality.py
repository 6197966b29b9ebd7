"""The denoiser on C3 at 1080p (agpt_render_features + agpt_denoise): what a call costs against one sample per pixel, and what it
buys in display-range RMSE.

    python tools/denoise_quality.py [--out profiles/denoise_c3.json] [--profile-only] [--kernel-trace CSV]

Cost: HIP-event time of one agpt_denoise call (5 iterations, demodulated) and of one agpt_render_features call, warmed up, median of
repeats, alternated in the same loop with agpt_render at 16 spp (its total_ms / 16 = one sample per pixel, the yardstick).
Quality: uniform renders at 4, 16 and 64 spp through agpt_render_adaptive (rel_error 0, min_spp = max_spp), raw and denoised RMSE on
the display range (radiance clamped to [0, 1], the metric of DESIGN.md section 5.4) against a uniform 1024-spp render with another
seed_base; and the raw RMSE of a progressive uniform render at 16 .. 1024 spp, to place denoised 16 spp on that curve.
--profile-only runs one features call and one denoise call, for `rocprofv3 --kernel-trace --stats` in a run of its own;
--kernel-trace reads that run's kernel trace CSV and adds the per-pass kernel times to the JSON, each with the pass' unique bytes
(52 B per pixel: two float4 planes and the flag read, one float4 written) over its time as a share of the 8 TB/s HBM peak."""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ag_pathtracer_amd as ag  # noqa: E402
from adaptive_sampling import rmse  # noqa: E402  (tools/ is on the path of a script run from it)

W, H = 1920, 1080
ITER = 5
REF_SEED = 0x5EED1024
HBM_PEAK = 8.0e12
PASS_BYTES = 52


class HipEvents:
    """two HIP events on the null stream (the context's default), through the HIP runtime the library itself uses"""
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time(self, fn):
        assert self.hip.hipEventRecord(self.ev[0], None) == 0
        fn()
        assert self.hip.hipEventRecord(self.ev[1], None) == 0
        assert self.hip.hipEventSynchronize(self.ev[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return float(ms.value)


def rmse_display(img, ref):
    # (tools/adaptive_sampling.py has its own rmse_display, with the reason for the clamp)
    return rmse(np.clip(img, 0, 1), np.clip(ref, 0, 1))


def kernel_times(path):
    """per-dispatch rows of a rocprofv3 kernel trace CSV -> the denoise and feature kernels in launch order"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "k_denoise" in name or "k_feature" in name:
                rows.append((int(r["Start_Timestamp"]), name.split("(")[0].split()[-1], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    return [(n, us) for _, n, us in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_c3.json"))
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace CSV of a --profile-only run under rocprofv3")
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if args.kernel_trace:
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        k = kernel_times(args.kernel_trace)
        passes = [us for n, us in k if n == "k_denoise_pass"][-ITER:]
        out["kernel_trace"] = {
            "source": "rocprofv3 --kernel-trace --stats, tools/denoise_quality.py --profile-only (a run of its own)",
            "kernels_us": [{"kernel": n, "us": round(us, 2)} for n, us in k],
            "passes": [{"spacing": 1 << i, "us": round(us, 2), "unique_bytes": W * H * PASS_BYTES,
                        "unique_bytes_over_time_share_of_hbm_peak": round(W * H * PASS_BYTES / (us * 1e-6) / HBM_PEAK, 4)}
                       for i, us in enumerate(passes)]}
        json.dump(out, open(args.out, "w"), indent=1)
        print(json.dumps(out["kernel_trace"]["passes"], indent=1))
        return

    ctx = ag.Context(0)
    scene = ag.scenes.scene_c3(aspect=W / float(H)).instantiate(ag.Scene(ctx))
    pt = ag.PathTracer(5)
    n16 = W * H * 16
    pa, pm, pal, pnd, pout = ctx.alloc(n16), ctx.alloc(W * H * 4), ctx.alloc(n16), ctx.alloc(n16), ctx.alloc(n16)
    params = ag.DenoiseParams(W, H, ITER, 1, ag.DENOISE_SIGMA_Z, ag.DENOISE_SIGMA_N, ag.DENOISE_SIGMA_L)

    def uniform(spp):
        ctx.memset(pa, 0, n16)
        ctx.memset(pm, 0, W * H * 4)
        return pt.render_adaptive(scene, W, H, pa, pm, spp, spp, spp, 0.0)[0]

    uniform(16)
    pt.render_features(scene, W, H, pal, pnd)
    ctx.denoise(params, pa, pm, pal, pnd, pout)
    if args.profile_only:
        pt.render_features(scene, W, H, pal, pnd)
        ctx.denoise(params, pa, pm, pal, pnd, pout)
        print("profile run: one features call and one denoise call after the warm-up")
        return

    out = {"scene": "C3 (BASELINE configs[2]) 1920x1080, MaxDepth 5", "iterations": ITER, "demodulate": 1,
           "sigma_z": ag.DENOISE_SIGMA_Z, "sigma_n": ag.DENOISE_SIGMA_N, "sigma_l": ag.DENOISE_SIGMA_L,
           "reference": "uniform 1024 spp, seed_base 0x%08X; RMSE over pixels and channels, display range = clamped to [0, 1]" % REF_SEED}
    # ---- cost, alternated with the yardstick ------------------------------------------------------------------------
    ev = HipEvents()
    ptmp = ctx.alloc(n16)
    t_render, t_denoise, t_features = [], [], []
    for _ in range(args.reps + 1):
        ctx.memset(ptmp, 0, n16)
        t_render.append(pt.render(scene, W, H, 16, ptmp).total_ms)
        t_denoise.append(ev.time(lambda: ctx.denoise(params, pa, pm, pal, pnd, pout)))
        t_features.append(ev.time(lambda: pt.render_features(scene, W, H, pal, pnd)))
    ctx.free(ptmp)
    one_spp = float(np.median(t_render[1:])) / 16
    out["cost"] = {"render_16spp_ms_runs": t_render, "one_sample_per_pixel_ms": one_spp,
                   "denoise_ms_runs": t_denoise, "denoise_ms": float(np.median(t_denoise[1:])),
                   "features_ms_runs": t_features, "features_ms": float(np.median(t_features[1:])),
                   "timing": "HIP events on the context's stream around the call; agpt_render: its own total_ms; first repeat dropped, median"}
    out["cost"]["denoise_over_one_sample"] = out["cost"]["denoise_ms"] / one_spp
    out["cost"]["features_over_one_sample"] = out["cost"]["features_ms"] / one_spp
    print("cost:", {k: v for k, v in out["cost"].items() if not k.endswith("runs")}, flush=True)
    # ---- quality ------------------------------------------------------------------------------------------------
    ctx.memset(pa, 0, n16)
    pt.render(scene, W, H, 1024, pa, seed_base=REF_SEED)
    ref = ctx.download(pa, (H, W, 4))[..., :3].astype(np.float64) / 1024
    quality = []
    for spp in (4, 16, 64):
        st = uniform(spp)
        raw = ctx.download(pa, (H, W, 4))[..., :3] / np.float32(spp)
        ctx.denoise(params, pa, pm, pal, pnd, pout)
        den = ctx.download(pout, (H, W, 4))[..., :3]
        rec = {"spp": spp, "render_ms": st.total_ms, "raw_rmse_display": rmse_display(raw, ref), "denoised_rmse_display": rmse_display(den, ref),
               "raw_rmse": rmse(raw, ref), "denoised_rmse": rmse(den, ref)}
        rec["display_ratio"] = rec["denoised_rmse_display"] / rec["raw_rmse_display"]
        print(rec, flush=True)
        quality.append(rec)
    out["quality"] = quality
    # the raw curve: a progressive uniform render with the default seed
    ctx.memset(pa, 0, n16)
    curve, done = [], 0
    for spp in (16, 32, 64, 128, 256, 512, 1024):
        pt.render(scene, W, H, spp - done, pa, spp_begin=done)
        done = spp
        curve.append({"spp": spp, "raw_rmse_display": rmse_display(ctx.download(pa, (H, W, 4))[..., :3] / np.float32(spp), ref)})
    out["uniform_curve"] = curve
    target = quality[1]["denoised_rmse_display"]
    match = None
    for a, b in zip(curve, curve[1:]):
        if a["raw_rmse_display"] >= target >= b["raw_rmse_display"]:   # log-log interpolation between the two levels
            f = (np.log(a["raw_rmse_display"]) - np.log(target)) / (np.log(a["raw_rmse_display"]) - np.log(b["raw_rmse_display"]))
            match = float(np.exp(np.log(a["spp"]) + f * (np.log(b["spp"]) - np.log(a["spp"]))))
    out["uniform_spp_matching_denoised_16spp"] = match if match is not None else (
        "below %d" % curve[0]["spp"] if target > curve[0]["raw_rmse_display"] else "above %d" % curve[-1]["spp"])
    print("uniform spp whose raw display RMSE equals denoised 16 spp:", out["uniform_spp_matching_denoised_16spp"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    for p in (pa, pm, pal, pnd, pout):
        ctx.free(p)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
