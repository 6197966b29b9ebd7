"""Developer measurement: what image textures cost.  C3 at 1080p / 64 spp untextured (k_shade) against the same scene with every
material pointed at a 256x256 texture (k_shade_textured) and, with --mapped, against that scene with every Disney material also
pointed at one 256x256 image for its roughness (g) and its metallic weight (b) (k_shade_mapped); with --sampled the mapped scene
with every texture read BILINEAR (k_shade_sampled) against the same scene with the default NEAREST samplers (k_shade_mapped), into
profiles/texture_filter_c3.json by default; the scenes live in one process, each
rendered --reps times, alternating, after a warm-up.  Per variant: step ms, trace ms, non-trace ms, the agpt_stats totals and non-trace ns per shaded vertex (medians).
    python tools/textures_cost.py [--out profiles/textures_c3.json] [--mapped | --sampled | --normal] [--reps 3] [--shading exact|fast] [--kernel-trace CSV]
(--reps 1 --no-warmup: exactly one render per variant, the run for rocprofv3 --kernel-trace --stats; --kernel-trace adds that
run's per-kernel times to the JSON, --kernel-trace-run JSON -- what that run wrote with --out -- its command and library hash)"""
import argparse
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ag_pathtracer_amd as ag  # noqa: E402


def textured_c3(desc, size=256, seed=7):
    """every material of the scene takes its own window of one size x size noise image scaled around the material's colour"""
    rng = np.random.RandomState(seed)
    noise = rng.uniform(0.6, 1.0, (size, size, 1)).astype(np.float32)
    colors = [op[2] for op in desc.ops if op[0] == "material"]
    for m, c in enumerate(colors):
        desc.set_material_texture(m, desc.add_texture(np.clip(noise * np.asarray(c, np.float32), 0, 1)))
    return desc


def mapped_c3(desc, size=256, seed=9):
    """textured_c3, then every Disney material takes one size x size noise image for both parameters: roughness from g, metallic
    from b, each scattered around the material's own value (so that the scene stays the kind of scene it was)"""
    desc = textured_c3(desc, size)
    rng = np.random.RandomState(seed)
    noise = rng.uniform(-0.2, 0.2, (size, size, 2))
    mats = [op for op in desc.ops if op[0] == "material"]
    for m, op in enumerate(mats):
        if op[1] != ag.MAT_DISNEY:
            continue
        image = np.zeros((size, size, 3), np.float32)
        image[..., 1] = np.clip(op[3] + noise[..., 0], 0, 1)
        image[..., 2] = np.clip(op[4] + noise[..., 1], 0, 1)
        tex = desc.add_texture(image)
        desc.set_material_param_texture(m, ag.PARAM_ROUGHNESS, tex, 1)
        desc.set_material_param_texture(m, ag.PARAM_METALLIC, tex, 2)
    return desc


def sampled_c3(desc, size=256):
    """mapped_c3 with every texture BILINEAR (repeat on both axes: the same texels are in reach, four of them per lookup)"""
    desc = mapped_c3(desc, size)
    for t in range(desc.n_textures):
        desc.set_texture_sampler(t, ag.FILTER_BILINEAR, ag.WRAP_REPEAT, ag.WRAP_REPEAT)
    return desc


def normal_c3(desc, size=256, seed=13):
    """sampled_c3 with one more size x size image, a random bump field read as a tangent-space normal map (tilts up to ~25 degrees),
    on every material (k_shade_normal)"""
    desc = sampled_c3(desc, size)
    g = np.random.RandomState(seed).uniform(-0.45, 0.45, (size, size, 2))
    n = np.concatenate([g, np.ones((size, size, 1))], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    tex = desc.add_texture((0.5 * n + 0.5).astype(np.float32))
    desc.set_texture_sampler(tex, ag.FILTER_BILINEAR, ag.WRAP_REPEAT, ag.WRAP_REPEAT)
    for m in range(desc.n_materials):
        desc.set_material_normal_texture(m, tex, 1.0)
    return desc


def library_build_id():
    """sha256 of the loaded library file: which kernel build the numbers belong to"""
    import hashlib
    return hashlib.sha256(open(ag.library_path(), "rb").read()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mapped", action="store_true", help="add the leg with roughness / metallic maps (k_shade_mapped)")
    ap.add_argument("--sampled", action="store_true", help="mapped with NEAREST (k_shade_mapped) against mapped with BILINEAR (k_shade_sampled)")
    ap.add_argument("--normal", action="store_true", help="the all-BILINEAR mapped scene (k_shade_sampled) against the same scene with a normal map on every material (k_shade_normal)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shading", default="exact", choices=["exact", "fast"])
    ap.add_argument("--no-warmup", action="store_true")
    ap.add_argument("--kernel-trace", default=None, metavar="CSV", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    ap.add_argument("--kernel-trace-run", default=None, metavar="JSON",
                    help="the JSON that the traced run itself wrote (--reps 1 --no-warmup --out JSON under rocprofv3): its command and its "
                         "library sha256 go into this run's JSON beside the kernel times, and the two libraries must be the same build")
    a = ap.parse_args()
    if a.sampled and a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "texture_filter_c3.json")
    if a.normal and a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "normal_map_c3.json")
    W, H, spp = 1920, 1080, 64
    ctx = ag.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    scenes = {}
    for name in ("sampled", "normal") if a.normal else ("mapped", "sampled") if a.sampled else ("untextured", "textured") + (("mapped",) if a.mapped else ()):
        d = ag.scenes.scene_c3(aspect=W / float(H))
        if name == "textured":
            d = textured_c3(d)
        elif name == "mapped":
            d = mapped_c3(d)
        elif name == "sampled":
            d = sampled_c3(d)
        elif name == "normal":
            d = normal_c3(d)
        scenes[name] = d.instantiate(ag.Scene(ctx))
        scenes[name].set_shading_arith(a.shading)
    film = torch.zeros((H, W, 4), device="cuda")
    pt = ag.PathTracer(5)

    def step(name):
        film.zero_()
        return pt.render(scenes[name], W, H, spp, film.data_ptr(), accum_pitch=W, timing=True)

    if not a.no_warmup:
        for name in scenes:
            step(name)
    runs = {name: [] for name in scenes}
    for _ in range(a.reps):
        for name in scenes:
            st = step(name)
            runs[name].append(dict(step_ms=st.total_ms, trace_ms=st.trace_ms, non_trace_ms=st.total_ms - st.trace_ms,
                                   shaded_vertices=int(st.shaded_vertices), rays=int(st.rays), closest_rays=int(st.closest_rays),
                                   anyhit_rays=int(st.anyhit_rays), answered_rays=int(st.answered_rays), iterations=int(st.iterations)))
    res = {"device": torch.cuda.get_device_name(0), "command": "python " + " ".join(sys.argv), "library_sha256": library_build_id(),
           "config": dict(W=W, H=H, spp=spp, shading=a.shading, texture="256x256 per material, 35 materials", reps=a.reps)}
    for name, rs in runs.items():
        med = {k: statistics.median(r[k] for r in rs) for k in ("step_ms", "trace_ms", "non_trace_ms")}
        med["non_trace_ns_per_shaded_vertex"] = med["non_trace_ms"] * 1e6 / max(1, rs[0]["shaded_vertices"])
        med["stats"] = {k: rs[0][k] for k in ("shaded_vertices", "rays", "closest_rays", "anyhit_rays", "answered_rays", "iterations")}
        med["spread"] = {k: [min(r[k] for r in rs), max(r[k] for r in rs)] for k in ("step_ms", "trace_ms", "non_trace_ms")}
        med["runs"] = rs
        res[name] = med
        print("%-10s step %7.1f ms  trace %7.1f  non-trace %6.1f  shaded %6.1f M  %.3f ns/vertex" % (
            name, med["step_ms"], med["trace_ms"], med["non_trace_ms"], rs[0]["shaded_vertices"] / 1e6,
            med["non_trace_ns_per_shaded_vertex"]), flush=True)
    if a.normal:
        # (the like-for-like figure is the one per shaded vertex: tilted normals end more paths, the two legs shade other vertex counts)
        res["normal_over_sampled"] = {k: res["normal"][k] / res["sampled"][k] for k in ("non_trace_ns_per_shaded_vertex", "non_trace_ms", "step_ms")}
    elif a.sampled:
        res["sampled_over_mapped"] = {k: res["sampled"][k] / res["mapped"][k] for k in ("step_ms", "non_trace_ms")}
    else:
        res["non_trace_ratio"] = res["textured"]["non_trace_ms"] / res["untextured"]["non_trace_ms"]
        res["step_ratio"] = res["textured"]["step_ms"] / res["untextured"]["step_ms"]
    if a.mapped and not a.sampled:
        for base in ("textured", "untextured"):
            res["mapped_over_%s" % base] = {k: res["mapped"][k] / res[base][k] for k in ("step_ms", "non_trace_ms")}
    if a.kernel_trace:
        rows = list(csv.DictReader(open(a.kernel_trace)))
        res["kernel_trace"] = {r["Name"].split("(")[0]: dict(calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) / 1e6)
                               for r in rows if "k_shade" in r["Name"] or r["Name"].startswith("k_accumulate(") or r["Name"].startswith("k_accumulate_fast(")}
        if a.kernel_trace_run:   # where the kernel times come from: another run of this tool, under the profiler
            run = json.load(open(a.kernel_trace_run))
            if run["library_sha256"] != res["library_sha256"]:
                sys.exit("--kernel-trace-run: the traced run used another build of the library")
            res["kernel_trace_run"] = {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- " + run["command"],
                                       "library_sha256": run["library_sha256"], "stats_csv": a.kernel_trace}
    for s in scenes.values():
        s.close()
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("->", a.out)


if __name__ == "__main__":
    main()
