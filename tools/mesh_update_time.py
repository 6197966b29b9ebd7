"""What one mesh update costs, per path: agpt_scene_update_mesh (host arrays), agpt_scene_update_mesh_device (device arrays),
agpt_scene_transform_mesh (16 floats), and REBUILD with the host and the device builder -- on C3's largest mesh inside C3 and on a
1 M-triangle heightfield.  Host clock around the synchronised calls; per operation the median and the min-max of `--runs` runs after
one warm-up, and the bytes that cross PCIe per call (up / down, from the sizes; REBUILD re-uploads the whole scene).

    python tools/mesh_update_time.py [--runs 9] [--out profiles/mesh_update_times.json] [--parent-lib TAG] [--rounds 3]
    python tools/mesh_update_time.py --pose [--runs 9] [--out profiles/mesh_pose_times.json]
    python tools/mesh_update_time.py --morph [--runs 9] [--out profiles/mesh_morph_times.json]
    python tools/mesh_update_time.py --normals [--runs 9] [--out profiles/mesh_normals_times.json]
    python tools/mesh_update_time.py --device-inputs [--runs 9] [--out profiles/mesh_device_inputs_times.json]

--pose times agpt_scene_pose_mesh instead (REFIT, 4 influences per vertex, 64 and 1,024 joints, the palette staged in LDS and read
from global memory -- AGPT_SKIN_GLOBAL_PALETTE), with, in the same process on the same GPU, agpt_scene_transform_mesh and the route a
host has without it: agpt_skin_arrays on the CPU, then agpt_scene_update_mesh with its output.

--morph times agpt_scene_morph_mesh (REFIT, 64 targets bound with normal deltas, 0 / 4 / 16 / 64 of them active; 16 active fused with a
64-joint skin of 4 influences) with, in the same process on the same GPU, agpt_scene_transform_mesh, agpt_scene_pose_mesh with the same
skin, and the route a host has without it: agpt_morph_arrays on the CPU, then agpt_scene_update_mesh with its output.

--normals times the AGPT_NORMALS_SMOOTH mode (agpt_scene_set_mesh_normals_mode): agpt_scene_update_mesh_device REFIT with the caller's
normals (the floor) against the same call in SMOOTH mode with NULL normals, agpt_scene_morph_mesh at 16 active targets once GIVEN with
normal deltas and once SMOOTH without, the rows taking turns in one process on the same GPU, and agpt_vertex_normals_arrays on one CPU
thread.

--device-inputs times Scene.pose_mesh (REFIT, 64 and 1,024 joints) three ways in turn -- host matrices, a torch tensor on the GPU
(agpt_scene_pose_mesh_device), and that tensor through .cpu().numpy() and the host call, the route a torch user had before -- and
Scene.morph_mesh at 16 of 64 targets active with host and with device weights, alone and fused with a 64-joint skin.

--parent-lib TAG compares the host-pointer REFIT of this build with the build `libagpt_hip_TAG.so` of the parent commit
(tools/build_variant.py run in a checkout of it, the file copied beside libagpt_hip.so): child processes, alternating parent / this
for `--rounds` rounds on the same GPU, each timing `--runs` updates per mesh; the new median must lie within the parent's own min-max
spread, and both sets of numbers go into the JSON.  With --pose or --morph it compares every GPU row of that leg the same way (each
child runs the whole leg) and writes only the comparison to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ag_pathtracer_amd as ag  # noqa: E402

F = np.float32
HEIGHTFIELD_QUADS = 707   # 2 * 707^2 = 999,698 triangles


def cases():
    """(name, scene description, primitive that moves)"""
    c3 = ag.scenes.scene_c3()
    meshes = [(len(op[4]) // 3, k) for k, op in enumerate(o for o in c3.ops if o[0] in ("mesh", "sphere", "plane", "area_light")) if op[0] == "mesh"]
    return [("c3_largest_mesh", c3, max(meshes)[1]), ("heightfield_1m", ag.scenes.scene_heightfield(HEIGHTFIELD_QUADS), 0)]


def arrays_of(desc, prim):
    op = [o for o in desc.ops if o[0] in ("mesh", "sphere", "plane", "area_light")][prim]
    return op[1], op[2], len(op[4]) // 3


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "runs": len(ts)}


def timed(fn, runs):
    fn(0)
    ts = []
    for k in range(1, runs + 1):
        t0 = time.perf_counter()
        fn(k)
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def wobble(v, k):
    """the pose of run k: the build pose with a small smooth displacement (every run uploads different bytes)"""
    return (v + F(0.002 * (k % 5)) * np.sin(v[:, ::-1] * F(3.0) + F(k))).astype(F)


def spin(v, k):
    c = 0.5 * (v.min(0).astype(np.float64) + v.max(0))
    a = 0.01 * k
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    t0, t1 = np.eye(4), np.eye(4)
    t0[:3, 3], t1[:3, 3] = -c, c
    return (t1 @ m @ t0).astype(F)


POSE_INFLUENCES = 4
POSE_ROUNDS = 3
SKIN_LDS_BYTES = 40 * 1024   # agpt_update.hip: the largest palette k_skin_mesh stages


def pose_binding(v, count, n_joints):
    """`count` rows of 4 influences: joints in bands along the mesh's longest axis (neighbours share joints, as on a rigged mesh),
    weights .4 .3 .2 .1 on the band and its neighbours"""
    axis = int(np.argmax(v.max(0) - v.min(0)))
    x = np.resize(v[:, axis], count).astype(np.float64)
    band = np.clip(((x - x.min()) / max(x.max() - x.min(), 1e-30) * n_joints).astype(np.int64), 0, n_joints - 1)
    J = np.clip(np.stack([band, band + 1, band - 1, band + 2], 1), 0, n_joints - 1).astype(np.int32)
    W = np.tile(np.array([.4, .3, .2, .1], F), (count, 1))
    return J, W


def pose_palette(v, n_joints, k):
    """run k: every joint a small turn about the vertical axis through the mesh's centre and a small lift, different per joint"""
    c = 0.5 * (v.min(0).astype(np.float64) + v.max(0))
    out = np.tile(np.eye(4), (n_joints, 1, 1))
    ang = 0.002 * (k + 1) * np.sin(0.37 * np.arange(n_joints) + k)
    out[:, 0, 0], out[:, 0, 2], out[:, 2, 0], out[:, 2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
    out[:, :3, 3] = c - np.einsum("jab,b->ja", out[:, :3, :3], c)
    out[:, 1, 3] += 0.001 * np.cos(0.11 * np.arange(n_joints) + k)
    return out.astype(F)


def pose_leg(runs):
    result = {"runs": runs, "influences": POSE_INFLUENCES,
              "statistic": "host clock around the synchronised call, ms: median and min-max of the runs after one warm-up (the warm-up "
                           "uploads the rest pose and the binding); all rows of a case from one process on one GPU; the pose rows are "
                           "%d rounds alternating the two palette routes: the median of the rounds' medians, the lowest min, the highest "
                           "max.  A palette over 40 KiB is not staged: its `lds` row took the global route too" % POSE_ROUNDS,
              "cases": {}}
    ctx = ag.Context(0)
    for name, desc, prim in cases():
        v, n, tris = arrays_of(desc, prim)
        nv, nn = len(v), 0 if n is None else len(n)
        g = desc.instantiate(ag.Scene(ctx))
        rows = {}
        mats = [spin(v, k) for k in range(runs + 1)]
        g.transform_mesh(prim, mats[0])
        rows["refit_transform"] = dict(timed(lambda k: g.transform_mesh(prim, mats[k]), runs), pcie_up=128, pcie_down=36)
        for n_joints in (64, 1024):
            J, W = pose_binding(v, nv, n_joints)
            nJ, nW = pose_binding(v, nn, n_joints) if nn and nn != nv else (None, None)
            g.set_mesh_skin(prim, J, W, nJ, nW, n_joints=n_joints)
            palettes = [pose_palette(v, n_joints, k) for k in range(runs + 1)]
            floats = n_joints * (21 if nn else 12)
            staged = 4 * n_joints * (21 if nn else 13) <= SKIN_LDS_BYTES
            per_route = {"lds": [], "global": []}
            for _ in range(POSE_ROUNDS):       # the two routes in turn, so that neither has the GPU in a better hour
                for route in ("lds", "global"):
                    if route == "global":
                        os.environ["AGPT_SKIN_GLOBAL_PALETTE"] = "1"
                    try:
                        per_route[route].append(timed(lambda k: g.pose_mesh(prim, palettes[k]), runs))
                    finally:
                        os.environ.pop("AGPT_SKIN_GLOBAL_PALETTE", None)
            for route, rs in per_route.items():
                rows["refit_pose_%d_joints_%s" % (n_joints, route)] = {
                    "median_ms": round(statistics.median(r["median_ms"] for r in rs), 4), "min_ms": min(r["min_ms"] for r in rs),
                    "max_ms": max(r["max_ms"] for r in rs), "runs": runs, "rounds": [r["median_ms"] for r in rs], "pcie_up": 4 * floats,
                    "pcie_down": 36, "palette_staged_in_lds": bool(staged and route == "lds")}
            # the route without the call: the blend on the CPU, then the arrays up
            t0 = time.perf_counter()
            posed = [ag.skin_arrays(palettes[k], v, J, W, n, nJ, nW) for k in range(2)]
            twin_ms = (time.perf_counter() - t0) * 1e3 / 2
            rows["host_skin_arrays_%d_joints" % n_joints] = {"mean_ms": round(twin_ms, 3), "runs": 2, "what": "agpt_skin_arrays on the CPU, one thread"}
            rows["refit_host_pointer_%d_joints" % n_joints] = dict(timed(lambda k: g.update_mesh(prim, posed[k & 1][0], posed[k & 1][1], "refit"), runs),
                                                                   pcie_up=12 * (nv + nn), pcie_down=32)
        g.close()
        result["cases"][name] = {"triangles": tris, "vertices": nv, "normals": nn, "scene_triangles": desc.n_tris, "operations": rows}
        for k, r in rows.items():
            if "median_ms" in r:
                print("%-16s %-36s median %9.3f ms  (%.3f .. %.3f)" % (name, k, r["median_ms"], r["min_ms"], r["max_ms"]), flush=True)
            else:
                print("%-16s %-36s mean   %9.3f ms" % (name, k, r["mean_ms"]), flush=True)
    ctx.close()
    return result


MORPH_TARGETS = 64
MORPH_ACTIVE = (0, 4, 16, 64)
MORPH_FUSED_ACTIVE = 16
MORPH_JOINTS = 64
MORPH_ROUNDS = 3


def morph_deltas(v, count, seed):
    """MORPH_TARGETS x count x 3 deltas of a few thousandths of the mesh's extent (the mesh stays where the camera and the tree expect it)"""
    scale = F(0.004 * float((v.max(0) - v.min(0)).max()))
    return (np.random.default_rng(seed).random((MORPH_TARGETS, count, 3), dtype=F) - F(0.5)) * scale


def morph_weights(active, k):
    """run k: `active` targets spread over the bound ones, every run with other values"""
    w = np.zeros(MORPH_TARGETS, F)
    if active:
        t = (np.arange(active) * MORPH_TARGETS) // active
        w[t] = 0.1 * (1 + (k + t) % 5)
    return w


def median_of_rounds(rs, runs):
    return {"median_ms": round(statistics.median(r["median_ms"] for r in rs), 4), "min_ms": min(r["min_ms"] for r in rs),
            "max_ms": max(r["max_ms"] for r in rs), "runs": runs, "rounds": [r["median_ms"] for r in rs]}


def morph_leg(runs):
    import torch
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    result = {"runs": runs, "targets_bound": MORPH_TARGETS, "influences": POSE_INFLUENCES, "joints": MORPH_JOINTS, "compute_units": num_cus,
              "statistic": "host clock around the synchronised call, ms: median and min-max of the runs after one warm-up (the warm-up "
                           "uploads the rest pose, the deltas and the binding); all rows of a case from one process on one GPU; every "
                           "row is %d rounds that take the operations in turn: the median of the rounds' medians, the lowest min, the "
                           "highest max.  kernel_bytes: what k_morph_mesh moves by its header, (vertices + normals) * (24 + 12 * active); "
                           "call_gb_per_s: those bytes over the median of the whole call (kernel, refit, flag and root box); "
                           "marginal_gb_per_s: the bytes and the time a row adds to the 0-active row" % MORPH_ROUNDS,
              "cases": {}}
    ctx = ag.Context(0)
    for name, desc, prim in cases():
        v, n, tris = arrays_of(desc, prim)
        nv, nn = len(v), 0 if n is None else len(n)
        g = desc.instantiate(ag.Scene(ctx))
        dP = morph_deltas(v, nv, 1)
        dN = morph_deltas(v, nn, 2) if nn else None
        g.set_mesh_morph_targets(prim, dP, dN)
        J, W = pose_binding(v, nv, MORPH_JOINTS)
        nJ, nW = pose_binding(v, nn, MORPH_JOINTS) if nn and nn != nv else (None, None)
        g.set_mesh_skin(prim, J, W, nJ, nW, n_joints=MORPH_JOINTS)
        mats = [spin(v, k) for k in range(runs + 1)]
        palettes = [pose_palette(v, MORPH_JOINTS, k) for k in range(runs + 1)]
        ws = {a: [morph_weights(a, k) for k in range(runs + 1)] for a in MORPH_ACTIVE}
        ops = {"refit_transform": lambda k: g.transform_mesh(prim, mats[k]),
               "refit_pose_%d_joints" % MORPH_JOINTS: lambda k: g.pose_mesh(prim, palettes[k])}
        for active in MORPH_ACTIVE:
            ops["refit_morph_%d_active" % active] = lambda k, a=active: g.morph_mesh(prim, ws[a][k])
        ops["refit_morph_%d_active_fused_%d_joints" % (MORPH_FUSED_ACTIVE, MORPH_JOINTS)] = \
            lambda k: g.morph_mesh(prim, ws[MORPH_FUSED_ACTIVE][k], palettes[k])
        # the launch shape of the morph-only kernel: its 8 blocks per CU against the skin kernel's 4 (AGPT_MORPH_MAX_BLOCKS lowers the cap)
        capped = "refit_morph_%d_active_4_blocks_per_cu" % MORPH_FUSED_ACTIVE
        ops[capped] = lambda k: g.morph_mesh(prim, ws[MORPH_FUSED_ACTIVE][k])
        per_op = {k: [] for k in ops}
        for _ in range(MORPH_ROUNDS):       # the operations in turn, so that none has the GPU in a better hour
            for op, fn in ops.items():
                if op == capped:
                    os.environ["AGPT_MORPH_MAX_BLOCKS"] = str(4 * num_cus)
                try:
                    per_op[op].append(timed(fn, runs))
                finally:
                    os.environ.pop("AGPT_MORPH_MAX_BLOCKS", None)
        rows = {op: median_of_rounds(rs, runs) for op, rs in per_op.items()}
        rows["refit_transform"].update(pcie_up=128, pcie_down=36)
        palette_bytes = 4 * MORPH_JOINTS * (21 if nn else 12)
        rows["refit_pose_%d_joints" % MORPH_JOINTS].update(pcie_up=palette_bytes, pcie_down=36)
        floor = rows["refit_morph_0_active"]["median_ms"]
        for op, r in rows.items():
            if not op.startswith("refit_morph"):
                continue
            active = int(op.split("_")[2])
            fused = "fused" in op
            r.update(pcie_up=8 * active + (palette_bytes if fused else 0), pcie_down=36)
            if not fused:
                r["kernel_bytes"] = (nv + nn) * (24 + 12 * active)
                r["call_gb_per_s"] = round(r["kernel_bytes"] / (r["median_ms"] * 1e-3) / 1e9, 1)
                if active and r["median_ms"] > floor:
                    r["marginal_gb_per_s"] = round((nv + nn) * 12 * active / ((r["median_ms"] - floor) * 1e-3) / 1e9, 1)
        # the route without the call: the blend on the CPU, then the arrays up
        t0 = time.perf_counter()
        blended = [ag.morph_arrays(w, v, dP, n, dN) for w in ws[MORPH_FUSED_ACTIVE][:2]]
        twin_ms = (time.perf_counter() - t0) * 1e3 / 2
        rows["host_morph_arrays_%d_active" % MORPH_FUSED_ACTIVE] = {
            "mean_ms": round(twin_ms, 3), "runs": 2, "what": "agpt_morph_arrays on the CPU, one thread; it also checks every delta of the %d targets for finiteness" % MORPH_TARGETS}
        rows["refit_host_pointer_%d_active" % MORPH_FUSED_ACTIVE] = dict(
            timed(lambda k: g.update_mesh(prim, blended[k & 1][0], blended[k & 1][1], "refit"), runs), pcie_up=12 * (nv + nn), pcie_down=32)
        g.close()
        result["cases"][name] = {"triangles": tris, "vertices": nv, "normals": nn, "scene_triangles": desc.n_tris,
                                 "delta_bytes_on_device": 12 * MORPH_TARGETS * (nv + nn), "operations": rows}
        for k, r in rows.items():
            if "median_ms" in r:
                print("%-16s %-44s median %9.3f ms  (%.3f .. %.3f)%s" % (name, k, r["median_ms"], r["min_ms"], r["max_ms"],
                      "  %s GB/s of the call, %s marginal" % (r["call_gb_per_s"], r.get("marginal_gb_per_s", "-")) if "kernel_bytes" in r else ""), flush=True)
            else:
                print("%-16s %-44s mean   %9.3f ms" % (name, k, r["mean_ms"]), flush=True)
    ctx.close()
    return result


NORMALS_TARGETS = 16   # all of them active
NORMALS_ROUNDS = 3


def normals_leg(runs):
    result = {"runs": runs, "targets_bound_and_active": NORMALS_TARGETS,
              "statistic": "host clock around the synchronised call, ms: median and min-max of the runs after one warm-up (the warm-up "
                           "uploads the adjacency, the rest pose and the deltas); all rows of a case from one process on one GPU, two "
                           "scenes of it -- one with the mesh in GIVEN, one in SMOOTH mode --; every GPU row is %d rounds that take the "
                           "operations in turn: the median of the rounds' medians, the lowest min, the highest max.  kernel_bytes: what "
                           "k_face_normals and k_vertex_normals move by their header: per triangle 36 B of indices, 36 B of positions "
                           "and 16 B of g written, per normal item 8 B of offsets and 12 B written, per corner 4 B of triangle id and a "
                           "16-byte gather" % NORMALS_ROUNDS,
              "cases": {}}
    ctx = ag.Context(0)
    for name, desc, prim in cases():
        op = [o for o in desc.ops if o[0] in ("mesh", "sphere", "plane", "area_light")][prim]
        v, n, ix = op[1], op[2], np.asarray(op[4], np.int32).reshape(-1, 3)
        nv, nn, tris = len(v), len(n), len(ix) // 3
        given, smooth = (desc.instantiate(ag.Scene(ctx)) for _ in range(2))
        smooth.set_mesh_normals_mode(prim, "smooth")
        dP = (np.random.default_rng(1).random((NORMALS_TARGETS, nv, 3), dtype=F) - F(0.5)) * F(0.004 * float((v.max(0) - v.min(0)).max()))
        dN = (np.random.default_rng(2).random((NORMALS_TARGETS, nn, 3), dtype=F) - F(0.5)) * F(0.01)
        given.set_mesh_morph_targets(prim, dP, dN)
        smooth.set_mesh_morph_targets(prim, dP, None)
        ws = [(0.1 * (1 + (k + np.arange(NORMALS_TARGETS)) % 5)).astype(F) for k in range(runs + 1)]
        poses = [wobble(v, k) for k in range(2)]
        pv = [ctx.alloc(12 * nv) for _ in poses]
        for p, pose in zip(pv, poses):
            ctx.upload(p, pose)
        pn = ctx.alloc(12 * nn)
        ctx.upload(pn, n)
        ops = {"refit_device_pointer_given_normals": lambda k: given.update_mesh_device(prim, pv[k & 1], nv, pn, nn, "refit"),
               "refit_device_pointer_smooth_null_normals": lambda k: smooth.update_mesh_device(prim, pv[k & 1], nv, None, nn, "refit"),
               "refit_morph_%d_active_given_normal_deltas" % NORMALS_TARGETS: lambda k: given.morph_mesh(prim, ws[k]),
               "refit_morph_%d_active_smooth_no_normal_deltas" % NORMALS_TARGETS: lambda k: smooth.morph_mesh(prim, ws[k])}
        per_op = {k: [] for k in ops}
        for _ in range(NORMALS_ROUNDS):       # the operations in turn, so that none has the GPU in a better hour
            for name_op, fn in ops.items():
                per_op[name_op].append(timed(fn, runs))
        rows = {k: median_of_rounds(rs, runs) for k, rs in per_op.items()}
        kernel_bytes = tris * (36 + 36 + 16) + nn * (8 + 12) + 3 * tris * (4 + 16)
        rows["refit_device_pointer_given_normals"].update(pcie_up=0, pcie_down=36)
        rows["refit_device_pointer_smooth_null_normals"].update(pcie_up=0, pcie_down=36, first_call_up=4 * (nn + 1 + 3 * tris), kernel_bytes=kernel_bytes)
        for k in rows:
            if "morph" in k:
                rows[k].update(pcie_up=8 * NORMALS_TARGETS, pcie_down=36)
        t0 = time.perf_counter()
        for pose in poses:
            ag.vertex_normals_arrays(pose, ix, nn)
        rows["host_vertex_normals_arrays"] = {"mean_ms": round((time.perf_counter() - t0) * 1e3 / len(poses), 3), "runs": len(poses),
                                              "what": "agpt_vertex_normals_arrays on the CPU, one thread; it builds the adjacency every call"}
        for p in pv + [pn]:
            ctx.free(p)
        given.close()
        smooth.close()
        result["cases"][name] = {"triangles": tris, "vertices": nv, "normals": nn, "scene_triangles": desc.n_tris, "operations": rows}
        for k, r in rows.items():
            if "median_ms" in r:
                print("%-16s %-48s median %9.3f ms  (%.3f .. %.3f)" % (name, k, r["median_ms"], r["min_ms"], r["max_ms"]), flush=True)
            else:
                print("%-16s %-48s mean   %9.3f ms" % (name, k, r["mean_ms"]), flush=True)
    ctx.close()
    return result


INPUTS_ROUNDS = 3
INPUTS_ACTIVE = 16


def device_inputs_leg(runs):
    """--device-inputs: pose_mesh / morph_mesh with the frame's matrices and weights as torch tensors on the GPU (agpt_scene_pose_mesh_device,
    agpt_scene_morph_mesh_device) against the host-array calls and against the route a torch user had before: tensor -> .cpu().numpy() ->
    the host call"""
    import torch
    torch.zeros(1, device="cuda")   # torch initialises the GPU before the library does
    result = {"runs": runs, "influences": POSE_INFLUENCES, "targets_bound": MORPH_TARGETS, "targets_active": INPUTS_ACTIVE, "morph_joints": MORPH_JOINTS,
              "statistic": "host clock around the synchronised call, ms: median and min-max of the runs after one warm-up; all rows of a case "
                           "from one process on one GPU; every row is %d rounds that take the rows of its group in turn (the three pose rows "
                           "of a joint count; the four morph rows): the median of the rounds' medians, the lowest min, the highest max.  The "
                           "context runs on the null stream, as torch's default stream does: Scene.pose_mesh synchronises it before a tensor "
                           "is handed over.  *_device_tensor: the tensors exist before the clock starts.  *_download_and_call: the same "
                           "tensor through .cpu().numpy() and the host call" % INPUTS_ROUNDS,
              "cases": {}}
    ctx = ag.Context(0)

    def in_turn(ops):
        per_op = {k: [] for k in ops}
        for _ in range(INPUTS_ROUNDS):
            for op, fn in ops.items():
                per_op[op].append(timed(fn, runs))
        return {op: median_of_rounds(rs, runs) for op, rs in per_op.items()}

    for name, desc, prim in cases():
        v, n, tris = arrays_of(desc, prim)
        nv, nn = len(v), 0 if n is None else len(n)
        g = desc.instantiate(ag.Scene(ctx))
        rows = {}
        for n_joints in (64, 1024):
            J, W = pose_binding(v, nv, n_joints)
            nJ, nW = pose_binding(v, nn, n_joints) if nn and nn != nv else (None, None)
            g.set_mesh_skin(prim, J, W, nJ, nW, n_joints=n_joints)
            palettes = [pose_palette(v, n_joints, k) for k in range(runs + 1)]
            tensors = [torch.from_numpy(p).cuda() for p in palettes]
            torch.cuda.synchronize()
            got = in_turn({"refit_pose_%d_joints_host_matrices" % n_joints: lambda k: g.pose_mesh(prim, palettes[k]),
                           "refit_pose_%d_joints_device_tensor" % n_joints: lambda k: g.pose_mesh(prim, tensors[k]),
                           "refit_pose_%d_joints_download_and_call" % n_joints: lambda k: g.pose_mesh(prim, tensors[k].cpu().numpy())})
            floats = n_joints * (21 if nn else 12)
            got["refit_pose_%d_joints_host_matrices" % n_joints].update(pcie_up=4 * floats, pcie_down=36)
            got["refit_pose_%d_joints_device_tensor" % n_joints].update(pcie_up=0, pcie_down=20 + 36)
            got["refit_pose_%d_joints_download_and_call" % n_joints].update(pcie_up=4 * floats, pcie_down=64 * n_joints + 36)
            rows.update(got)
        dP = morph_deltas(v, nv, 1)
        dN = morph_deltas(v, nn, 2) if nn else None
        g.set_mesh_morph_targets(prim, dP, dN)
        J, W = pose_binding(v, nv, MORPH_JOINTS)
        nJ, nW = pose_binding(v, nn, MORPH_JOINTS) if nn and nn != nv else (None, None)
        g.set_mesh_skin(prim, J, W, nJ, nW, n_joints=MORPH_JOINTS)
        palettes = [pose_palette(v, MORPH_JOINTS, k) for k in range(runs + 1)]
        ws = [morph_weights(INPUTS_ACTIVE, k) for k in range(runs + 1)]
        tp, tw = [torch.from_numpy(p).cuda() for p in palettes], [torch.from_numpy(w).cuda() for w in ws]
        torch.cuda.synchronize()
        tag = "refit_morph_%d_of_%d" % (INPUTS_ACTIVE, MORPH_TARGETS)
        got = in_turn({tag + "_host_weights": lambda k: g.morph_mesh(prim, ws[k]),
                       tag + "_device_tensor": lambda k: g.morph_mesh(prim, tw[k]),
                       tag + "_fused_%d_joints_host" % MORPH_JOINTS: lambda k: g.morph_mesh(prim, ws[k], palettes[k]),
                       tag + "_fused_%d_joints_device_tensors" % MORPH_JOINTS: lambda k: g.morph_mesh(prim, tw[k], tp[k])})
        palette_bytes = 4 * MORPH_JOINTS * (21 if nn else 12)
        got[tag + "_host_weights"].update(pcie_up=8 * INPUTS_ACTIVE, pcie_down=36)
        got[tag + "_device_tensor"].update(pcie_up=0, pcie_down=20 + 36)
        got[tag + "_fused_%d_joints_host" % MORPH_JOINTS].update(pcie_up=8 * INPUTS_ACTIVE + palette_bytes, pcie_down=36)
        got[tag + "_fused_%d_joints_device_tensors" % MORPH_JOINTS].update(pcie_up=0, pcie_down=20 + 36)
        rows.update(got)
        g.close()
        result["cases"][name] = {"triangles": tris, "vertices": nv, "normals": nn, "scene_triangles": desc.n_tris, "operations": rows}
        for k, r in rows.items():
            print("%-16s %-52s median %9.3f ms  (%.3f .. %.3f)" % (name, k, r["median_ms"], r["min_ms"], r["max_ms"]), flush=True)
    ctx.close()
    return result


def host_refit_only(runs):
    """the child of --parent-lib: the host-pointer REFIT alone, through whichever library AGPT_LIB_VARIANT names"""
    ctx = ag.Context(0)
    out = {}
    for name, desc, prim in cases():
        g = desc.instantiate(ag.Scene(ctx))
        v, n, _ = arrays_of(desc, prim)
        poses = [wobble(v, k) for k in range(runs + 1)]
        out[name] = timed(lambda k: g.update_mesh(prim, poses[k], n, "refit"), runs)
        g.close()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def leg_rows(result):
    """the child of --parent-lib with --pose / --morph: the leg's GPU rows as {case/operation: stats}"""
    out = {}
    for case, c in result["cases"].items():
        for op, r in c["operations"].items():
            if "median_ms" in r:
                out["%s/%s" % (case, op)] = {k: r[k] for k in ("median_ms", "min_ms", "max_ms")}
    print("RESULT " + json.dumps(out), flush=True)


def compare_with_parent(tag, runs, rounds, leg=()):
    sets = {"parent": [], "this": []}
    for _ in range(rounds):
        for which in ("parent", "this"):
            env = dict(os.environ)
            env.pop("AGPT_LIB_VARIANT", None)
            if which == "parent":
                env["AGPT_LIB_VARIANT"] = tag
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--runs", str(runs)] + list(leg), env=env, capture_output=True,
                               text=True, timeout=900, check=True)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
            sets[which].append(json.loads(line[7:]))
            print(which, line[7:], flush=True)
    out = {"method": "child processes alternating parent / this on one GPU, %d rounds of %d timed updates each after one warm-up; "
                     "per build the median of the rounds' medians, the lowest min and the highest max" % (rounds, runs)}
    for name in sets["this"][0]:
        row = {}
        for which in ("parent", "this"):
            rs = [s[name] for s in sets[which]]
            row[which] = {"median_ms": round(statistics.median(r["median_ms"] for r in rs), 4), "min_ms": min(r["min_ms"] for r in rs),
                          "max_ms": max(r["max_ms"] for r in rs), "rounds": rs}
        row["this_median_within_parent_spread"] = bool(row["parent"]["min_ms"] <= row["this"]["median_ms"] <= row["parent"]["max_ms"])
        row["this_median_not_above_parent_max"] = bool(row["this"]["median_ms"] <= row["parent"]["max_ms"])
        out[name] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, metavar="TAG")
    ap.add_argument("--pose", action="store_true", help="time agpt_scene_pose_mesh (see above) instead of the update paths")
    ap.add_argument("--morph", action="store_true", help="time agpt_scene_morph_mesh (see above) instead of the update paths")
    ap.add_argument("--normals", action="store_true", help="time the AGPT_NORMALS_SMOOTH mode (see above) instead of the update paths")
    ap.add_argument("--device-inputs", action="store_true", help="time pose_mesh / morph_mesh with torch tensors on the GPU (see above) instead of the update paths")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.runs < 7:
        ap.error("--runs: at least 7")
    if a.child:
        return leg_rows(morph_leg(a.runs) if a.morph else pose_leg(a.runs)) if a.pose or a.morph else host_refit_only(a.runs)
    if a.parent_lib and (a.pose or a.morph):
        result = compare_with_parent(a.parent_lib, a.runs, a.rounds, ["--morph" if a.morph else "--pose"])
        if a.out:
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
        slower = [k for k, r in result.items() if isinstance(r, dict) and not r["this_median_not_above_parent_max"]]
        if slower:
            sys.exit("slower than the parent's spread on: %s" % ", ".join(slower))
        return
    if a.pose or a.morph or a.normals or a.device_inputs:
        result = device_inputs_leg(a.runs) if a.device_inputs else normals_leg(a.runs) if a.normals else morph_leg(a.runs) if a.morph else pose_leg(a.runs)
        default = ("mesh_device_inputs_times.json" if a.device_inputs else "mesh_normals_times.json" if a.normals else
                   "mesh_morph_times.json" if a.morph else "mesh_pose_times.json")
        with open(a.out or os.path.join(ROOT, "profiles", default), "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return
    result = {"runs": a.runs, "statistic": "host clock around the synchronised call, ms: median and min-max of the runs after one warm-up",
              "pcie_bytes": "per call, from the sizes: up = host to device, down = device to host", "cases": {}}
    ctx = ag.Context(0)
    for name, desc, prim in cases():
        v, n, tris = arrays_of(desc, prim)
        nv, nn = len(v), 0 if n is None else len(n)
        arrays_bytes = 12 * (nv + nn)
        rows = {}
        g = desc.instantiate(ag.Scene(ctx))
        poses = [wobble(v, k) for k in range(a.runs + 1)]
        rows["refit_host_pointer"] = dict(timed(lambda k: g.update_mesh(prim, poses[k], n, "refit"), a.runs), pcie_up=arrays_bytes, pcie_down=32)
        pv, pn = ctx.alloc(12 * nv), (ctx.alloc(12 * nn) if nn else None)
        if nn:
            ctx.upload(pn, n)

        def device_refit(k):
            g.update_mesh_device(prim, pv, nv, pn, nn, "refit")
        ctx.upload(pv, poses[1])
        rows["refit_device_pointer"] = dict(timed(device_refit, a.runs), pcie_up=0, pcie_down=36)
        g.update_mesh(prim, v, n, "refit")   # the rest pose again
        mats = [spin(v, k) for k in range(a.runs + 1)]
        g.transform_mesh(prim, mats[0])      # (the one-time upload of the rest arrays is not part of a frame)
        rows["refit_transform"] = dict(timed(lambda k: g.transform_mesh(prim, mats[k]), a.runs), pcie_up=128, pcie_down=36,
                                       first_call_up=arrays_bytes)
        ctx.free(pv)
        if pn:
            ctx.free(pn)
        commit_bytes = None
        for builder in ("host", "device"):
            g.close()
            g = ag.Scene(ctx)
            g.set_bvh_builder(builder)
            desc.instantiate(g)
            rows["rebuild_%s_builder" % builder] = dict(timed(lambda k: g.update_mesh(prim, poses[k], n, "rebuild"), a.runs),
                                                        pcie="the arrays (device builder: up; its tree comes down) and the whole scene's "
                                                             "flattened records up again (agpt_scene_commit)")
        g.close()
        result["cases"][name] = {"triangles": tris, "vertices": nv, "normals": nn, "scene_triangles": desc.n_tris, "operations": rows}
        for k, r in rows.items():
            print("%-16s %-24s median %9.3f ms  (%.3f .. %.3f)" % (name, k, r["median_ms"], r["min_ms"], r["max_ms"]), flush=True)
    ctx.close()
    if a.parent_lib:
        result["host_pointer_refit_parent_against_this"] = compare_with_parent(a.parent_lib, a.runs, a.rounds)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    cmp_ = result.get("host_pointer_refit_parent_against_this", {})
    slower = [k for k, r in cmp_.items() if isinstance(r, dict) and not r["this_median_not_above_parent_max"]]
    if slower:
        sys.exit("host-pointer REFIT got slower than the parent's spread on: %s" % ", ".join(slower))


if __name__ == "__main__":
    main()
