"""Temporal reprojection on C3 at 1080p (agpt_temporal_accumulate): what the kernel costs beside one a-trous pass, and what the
history buys over an orbit.

    python tools/temporal_demo.py [--out profiles/temporal_c3.json] [--profile-only] [--kernel-trace CSV]

Quality: an orbit of 8 frames (--orbit degrees in all) at 4 spp per frame.  Per frame the display-range RMSE (denoise_model.display_rmse:
both images clamped to [0, 1]) against a 256-spp render of the same frame with another seed_base, of (a) agpt_denoise on the frame's own
samples, (b) agpt_temporal_accumulate + agpt_denoise, (c) the frame's samples unfiltered.  Call times are HIP-event times, medians.
--profile-only runs two frames after a warm-up, for `rocprofv3 --kernel-trace --stats` in a run of its own (no counters);
--kernel-trace reads that run's kernel trace CSV and adds k_temporal's time, the bytes it moves and the k_denoise_pass times of the
same run to the JSON."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ag_pathtracer_amd as ag  # noqa: E402
from denoise_model import display_rmse  # noqa: E402
from denoise_quality import HipEvents  # noqa: E402

W, H = 1920, 1080
FRAMES, SPP, REF_SPP, REF_SEED = 8, 4, 256, 0x5EED0256
MAX_HISTORY = 32.0
HBM_PEAK = 8.0e12
# per pixel, whole records: this frame's accum, moment2, albedo, normal_depth read (52 B), the previous frame's four likewise (52 B,
# each line shared by the pixels that land around it), the two outputs written (20 B)
TEMPORAL_BYTES = 52 + 52 + 20
PASS_BYTES = 52


def kernel_rows(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "k_temporal" in name or "k_denoise_pass" in name:
                rows.append((int(r["Start_Timestamp"]), name.split("(")[0].split()[-1], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    return [(n, us) for _, n, us in rows]


class FrameLoop:
    """the buffers of the frame loop: this frame's (accum, moment2), two sets of (history accum, history moment2, albedo,
    normal_depth) that alternate -- what frame k writes, frame k + 1 reads as prev -- and the denoised output"""

    def __init__(self, ctx, scene):
        self.ctx, self.scene, self.pt = ctx, scene, ag.PathTracer(5)
        n16, n4 = W * H * 16, W * H * 4
        self.acc, self.m2, self.out = ctx.alloc(n16), ctx.alloc(n4), ctx.alloc(n16)
        self.sets = [(ctx.alloc(n16), ctx.alloc(n4), ctx.alloc(n16), ctx.alloc(n16)) for _ in range(2)]
        self.denoise_params = ag.DenoiseParams(W, H, 5, 1, ag.DENOISE_SIGMA_Z, ag.DENOISE_SIGMA_N, ag.DENOISE_SIGMA_L)
        self.cam_prev, self.k = None, 0

    def frame(self, cam, ev=None):
        """-> dict of call times (ms) when ev is given; the results stay on the device"""
        ctx, cur, prev = self.ctx, self.sets[self.k & 1], self.sets[(self.k & 1) ^ 1]
        self.scene.set_camera(*cam)
        ctx.memset(self.acc, 0, W * H * 16)
        ctx.memset(self.m2, 0, W * H * 4)
        timed = (lambda fn: ev.time(fn)) if ev else (lambda fn: fn())
        t = {}
        t["render_ms"] = timed(lambda: self.pt.render_adaptive(self.scene, W, H, self.acc, self.m2, SPP, SPP, SPP, 0.0, seed_base=self.k))
        t["features_ms"] = timed(lambda: self.pt.render_features(self.scene, W, H, cur[2], cur[3]))
        first = self.cam_prev is None
        params = ag.TemporalParams(W, H, ag.camera_desc(*cam), ag.camera_desc(*(cam if first else self.cam_prev)), MAX_HISTORY,
                                   ag.TEMPORAL_DEPTH_TOL, ag.TEMPORAL_NORMAL_COS)
        t["temporal_ms"] = timed(lambda: ctx.temporal_accumulate(params, self.acc, self.m2, cur[2], cur[3],
                                                                 *((0, 0, 0, 0) if first else prev), cur[0], cur[1]))
        t["denoise_ms"] = timed(lambda: ctx.denoise(self.denoise_params, cur[0], cur[1], cur[2], cur[3], self.out))
        self.cam_prev, self.k = cam, self.k + 1
        return t

    def current(self):
        return self.sets[(self.k - 1) & 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_c3.json"))
    ap.add_argument("--orbit", type=float, default=-8.0,
                    help="degrees the camera turns about its lookat over the whole sequence (C3's camera stands 1.6 from a side wall: a "
                         "negative angle turns it towards the room's axis)")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--kernel-trace", default=None, help="kernel trace CSV of a --profile-only run under rocprofv3")
    args = ap.parse_args()
    if args.kernel_trace:
        out = json.load(open(args.out)) if os.path.exists(args.out) else {}
        k = kernel_rows(args.kernel_trace)
        temporal = [us for n, us in k if n == "k_temporal"]
        passes = [us for n, us in k if n == "k_denoise_pass"][-5:]
        us = temporal[-1]
        out["kernel_trace"] = {
            "source": "rocprofv3 --kernel-trace --stats, tools/temporal_demo.py --profile-only (a run of its own, no counters)",
            "k_temporal_us_all": [round(v, 2) for v in temporal],
            "k_temporal_us": round(us, 2), "k_temporal_bytes": W * H * TEMPORAL_BYTES,
            "k_temporal_bytes_over_time_share_of_hbm_peak": round(W * H * TEMPORAL_BYTES / (us * 1e-6) / HBM_PEAK, 4),
            "k_denoise_pass_us_same_run": [round(v, 2) for v in passes], "k_denoise_pass_bytes": W * H * PASS_BYTES,
            "k_temporal_over_slowest_pass": round(us / max(passes), 3), "k_temporal_over_fastest_pass": round(us / min(passes), 3)}
        json.dump(out, open(args.out, "w"), indent=1)
        print(json.dumps(out["kernel_trace"], indent=1))
        return

    ctx = ag.Context(0)
    desc = ag.scenes.scene_c3(aspect=W / float(H))
    scene = desc.instantiate(ag.Scene(ctx))
    cams = [ag.scenes.orbit_camera(desc.camera, args.orbit * k / (FRAMES - 1)) for k in range(FRAMES)]
    loop = FrameLoop(ctx, scene)
    if args.profile_only:
        for cam in cams[:3]:   # the first frame has no history; the third is the one to read
            loop.frame(cam)
        print("profile run: three frames (the last k_temporal and the last five k_denoise_pass are the ones to read)")
        return

    ev = HipEvents()
    pt = ag.PathTracer(5)
    pref, pden = ctx.alloc(W * H * 16), ctx.alloc(W * H * 16)
    loop.frame(cams[0])          # warm-up: code objects, pools
    loop = FrameLoop(ctx, scene)
    frames = []
    for k, cam in enumerate(cams):
        times = loop.frame(cam, ev)
        cur = loop.current()
        both = ctx.download(loop.out, (H, W, 4))[..., :3]
        hist_w = ctx.download(cur[0], (H, W, 4))[..., 3]
        raw = ctx.download(loop.acc, (H, W, 4))[..., :3] / np.float32(SPP)
        ctx.denoise(loop.denoise_params, loop.acc, loop.m2, cur[2], cur[3], pden)
        spatial = ctx.download(pden, (H, W, 4))[..., :3]
        ctx.memset(pref, 0, W * H * 16)
        pt.render(scene, W, H, REF_SPP, pref, seed_base=REF_SEED)
        ref = ctx.download(pref, (H, W, 4))[..., :3] / np.float32(REF_SPP)
        rec = {"frame": k, "denoise_alone_rmse_display": display_rmse(spatial, ref), "temporal_denoise_rmse_display": display_rmse(both, ref),
               "unfiltered_rmse_display": display_rmse(raw, ref), "mean_effective_count": float(hist_w.mean()),
               "pixels_without_history": int((hist_w <= SPP).sum()) if k else W * H}
        rec.update({n: round(v, 4) for n, v in times.items()})
        print(rec, flush=True)
        frames.append(rec)
    later = frames[1:]
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out.update({"scene": "C3 (BASELINE configs[2]) 1920x1080, MaxDepth 5", "frames": FRAMES, "orbit_degrees": args.orbit, "spp_per_frame": SPP,
                "max_history": MAX_HISTORY, "depth_tol": ag.TEMPORAL_DEPTH_TOL, "normal_cos": ag.TEMPORAL_NORMAL_COS,
                "reference": "uniform %d spp of the same frame, seed_base 0x%08X; RMSE over pixels and channels, clamped to [0, 1]" % (REF_SPP, REF_SEED),
                "timing": "HIP events on the context's stream around each call (the calls synchronise), per frame",
                "per_frame": frames,
                "temporal_ms_median_frames_1_on": float(np.median([f["temporal_ms"] for f in later])),
                "denoise_ms_median_frames_1_on": float(np.median([f["denoise_ms"] for f in later])),
                "temporal_below_denoise_alone_from_frame_1_on": bool(all(f["temporal_denoise_rmse_display"] < f["denoise_alone_rmse_display"]
                                                                         for f in later))})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
