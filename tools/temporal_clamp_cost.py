"""Developer measurement: what the neighbourhood clamp of temporal history costs (agpt_temporal_accumulate_clamped) beside the two
calls it extends, into profiles/temporal_clamp_c3.json.

    python tools/temporal_clamp_cost.py [--runs 9] [--out profiles/temporal_clamp_c3.json] [--parent-lib TAG] [--rounds 3]

Every row is the host clock around one call that ends in a synchronise of the context's stream; the rows take turns in one process
(row A, row B, ..., row A, ...) after one warm-up turn, --runs timed turns, and are reported as median (min - max) in ms.  The frames
are tools/motion_cost.py's: two 4-spp frames of C3 at 1080p one degree of orbit apart.  Rows: agpt_temporal_accumulate,
agpt_temporal_accumulate_motion (nothing moved: every w in {0, 2}), and the clamped call at radius 1, 2 and 3 (demodulated, gamma 1,
clamped_max_history 8) without and with prev_point.
--parent-lib TAG: agpt_temporal_accumulate of this build against the build `libagpt_hip_TAG.so` of the parent commit
(tools/build_variant.py run in a checkout of it, the file copied beside libagpt_hip.so), as tools/motion_cost.py compares them: child
processes, alternating parent / this for --rounds rounds on the same GPU."""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import numpy as np  # noqa: E402
import ag_pathtracer_amd as ag  # noqa: E402
import motion_cost as mc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "temporal_clamp_c3.json"))
    ap.add_argument("--parent-lib", default=None, metavar="TAG")
    a = ap.parse_args()
    if a.runs < 9:
        ap.error("--runs: at least 9")
    import torch
    W, H = mc.W, mc.H
    ctx = ag.Context(0)
    res = {"device": torch.cuda.get_device_name(0),
           "command": "python tools/temporal_clamp_cost.py --runs %d --rounds %d%s" % (a.runs, a.rounds, " --parent-lib " + a.parent_lib if a.parent_lib else ""),
           "library_sha256": hashlib.sha256(open(ag.library_path(), "rb").read()).hexdigest(),
           "method": "host clock around each synchronised call; the rows take turns in one process, one warm-up turn, then %d timed "
                     "turns: median (min - max)" % a.runs,
           "config": dict(W=W, H=H, spp=mc.SPP, demodulate=1, gamma=1.0, clamped_max_history=8.0)}
    f = mc.Frames(ctx)
    pt = ag.PathTracer(5)
    n16 = W * H * 16
    albedo, nd, point = ctx.alloc(n16), ctx.alloc(n16), ctx.alloc(n16)
    f.scene.snapshot_positions()
    f.scene.set_camera(*f.cams[1])
    pt.render_features_motion(f.scene, W, H, albedo, nd, point)
    rows = {"agpt_temporal_accumulate": f.accumulate,
            "agpt_temporal_accumulate_motion": lambda: ctx.temporal_accumulate_motion(f.params, *f.buffers, point)}
    for radius in (1, 2, 3):
        clamp = ag.TemporalClampParams(radius, 1, 1.0, 8.0)
        rows["agpt_temporal_accumulate_clamped r = %d" % radius] = lambda c=clamp: ctx.temporal_accumulate_clamped(f.params, c, *f.buffers)
        rows["agpt_temporal_accumulate_clamped r = %d, prev_point" % radius] = \
            lambda c=clamp: ctx.temporal_accumulate_clamped(f.params, c, *f.buffers, point)
    res["temporal"] = mc.turns(rows, a.runs)
    mc.show("temporal", res["temporal"])
    # how much of the film the clamp touched at radius 2: the count of a clamped pixel is capped at 8 + 4
    ctx.temporal_accumulate(f.params, *f.buffers)
    plain = ctx.download(f.out[0], (H, W, 4))
    ctx.temporal_accumulate_clamped(f.params, ag.TemporalClampParams(2, 1, 1.0, 8.0), *f.buffers)
    clamped = ctx.download(f.out[0], (H, W, 4))
    took = plain[..., 3] > mc.SPP
    changed = (plain.view(np.uint32) != clamped.view(np.uint32)).any(-1)
    res["pixels"] = {"film": W * H, "with_history": int(took.sum()), "clamped_at_radius_2": int(changed.sum())}
    print("pixels", res["pixels"], flush=True)
    f.scene.close()
    ctx.close()
    if a.parent_lib:
        c = res["agpt_temporal_accumulate_parent_against_this"] = mc.compare_with_parent(a.parent_lib, a.runs, a.rounds)
        print("agpt_temporal_accumulate: parent %.3f ms (%.3f - %.3f), this %.3f ms (%.3f - %.3f)"
              % tuple(c[w][k] for w in ("parent", "this") for k in ("median_ms", "min_ms", "max_ms")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("->", a.out)


if __name__ == "__main__":
    main()
