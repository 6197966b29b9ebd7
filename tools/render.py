#!/usr/bin/env python3
"""Render one of the BASELINE scenes on the GPU and write a PNG (Accumulator::CopyToSurface resolve: gamma 2.2,
0x00RRGGBB) -- the presentation end of SURVEY.md section 8(f) rank 4.

    python tools/render.py --scene c3 --width 960 --height 540 --spp 64 --out gpurun_out/c3.png
    python tools/render.py --scene c3 --spp 4 --frames 8 --orbit 8 --temporal --out out/orbit.png   (out/orbit_0000.png ...)
    python tools/render.py --scene textured --spp 16 --spin 12 --out out/spin.png                  (out/spin_0000.png ...)
    python tools/render.py --scene textured --spp 4 --frames 8 --spin 12 --temporal --motion --out out/spin.png
    python tools/render.py --scene textured --spp 4 --frames 8 --spin 12 --temporal --motion --clamp 1.5 --clamp-radius 2 --out out/spin.png
    python tools/render.py --scene textured --spp 4 --frames 8 --spin 12 --temporal --motion --follow-normals --out out/spin.png
    python tools/render.py --scene c1 --spp 4 --frames 8 --light-orbit 10 --temporal --motion --clamp 1.5 --out out/light.png
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import ag_pathtracer_amd as ag  # noqa: E402


def stud_normal_map(studs_x=4, studs_y=4, cell=16, height=0.35):
    """rgb[studs_y * cell, studs_x * cell, 3]: the normals of studs_x x studs_y round bumps (a raised cosine each, cell x cell texels)
    over a flat ground, as n / 2 + 1 / 2"""
    y, x = np.mgrid[0:studs_y * cell, 0:studs_x * cell]
    cx, cy = ((x + .5) % cell) / cell - .5, ((y + .5) % cell) / cell - .5
    r = np.sqrt(cx * cx + cy * cy)
    slope = np.where(r < .4, height * np.pi / .4 * np.sin(np.pi * r / .4) * .5, 0.0)        # -d/dr of height / 2 * (1 + cos(pi r / .4))
    with np.errstate(invalid="ignore", divide="ignore"):
        gx, gy = np.where(r > 0, slope * cx / r, 0.0), np.where(r > 0, slope * cy / r, 0.0)
    n = np.stack([gx, gy, np.ones_like(gx)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return (0.5 * n + 0.5).astype(np.float32)


def render_sequence(a, ctx, scene, desc, W, H):
    """--frames: per frame render, features, (temporal accumulate,) denoise, resolve.  Between frames the host keeps the history
    buffers the frame wrote and the frame's feature buffers: two sets that alternate."""
    pt = ag.PathTracer(5)
    spp = max(2, a.spp)
    iterations = a.denoise if a.denoise is not None else 5
    n16, n4 = W * H * 16, W * H * 4
    acc, m2, out = ctx.alloc(n16), ctx.alloc(n4), ctx.alloc(n16)
    sets = [(ctx.alloc(n16), ctx.alloc(n4), ctx.alloc(n16), ctx.alloc(n16)) for _ in range(2)]   # history accum, moment2, albedo, normal_depth
    stem, ext = os.path.splitext(a.out)
    cam_prev = None
    for k in range(a.frames):
        cam = ag.scenes.orbit_camera(desc.camera, a.orbit * k / (a.frames - 1))
        cur, prev = sets[k & 1], sets[(k & 1) ^ 1]
        scene.set_camera(*cam)
        ctx.memset(acc, 0, n16)
        ctx.memset(m2, 0, n4)
        t0 = time.time()
        pt.render_adaptive(scene, W, H, acc, m2, spp, spp, spp, 0.0, seed_base=k)
        pt.render_features(scene, W, H, cur[2], cur[3])
        hist = (acc, m2)
        if a.temporal:
            params = ag.TemporalParams(W, H, ag.camera_desc(*cam), ag.camera_desc(*(cam_prev or cam)), a.max_history,
                                       ag.TEMPORAL_DEPTH_TOL, ag.TEMPORAL_NORMAL_COS)
            buffers = (acc, m2, cur[2], cur[3]) + (prev if cam_prev else (0, 0, 0, 0)) + (cur[0], cur[1])
            if a.clamp is not None:
                ctx.temporal_accumulate_clamped(params, clamp_params(a), *buffers)
            else:
                ctx.temporal_accumulate(params, *buffers)
            hist = cur[:2]
        ctx.denoise(ag.DenoiseParams(W, H, iterations, 1, ag.DENOISE_SIGMA_Z, ag.DENOISE_SIGMA_N, ag.DENOISE_SIGMA_L), hist[0], hist[1],
                    cur[2], cur[3], out)
        dt = time.time() - t0
        path = "%s_%04d%s" % (stem, k, ext)
        ag.binding.write_png(path, ctx.resolve_counts(out, W * H), W, H)
        print("frame %d: %d spp%s, %.1f ms -> %s" % (k, spp, " + history" if a.temporal and cam_prev else "", dt * 1e3, path))
        cam_prev = cam


def clamp_params(a):
    """--clamp [GAMMA] --clamp-radius R: the history is clamped to the current frame's neighbourhood (agpt_temporal_accumulate_clamped),
    on demodulated radiance like the denoiser's; a clamped pixel keeps at most a quarter of --max-history"""
    return ag.TemporalClampParams(a.clamp_radius, 1, a.clamp, max(1.0, a.max_history / 4))


def sequence_frames(a, n):
    """--spin / --bend / --morph N: all N frames of the cycle, or with --frames F its first F"""
    return min(n, a.frames) if a.frames > 1 else n


class FrameDrawer:
    """One frame of --spin / --bend / --morph after the frame's mesh update: --spp samples, resolved and written to OUT_kkkk.png.
    With --temporal the frame goes through the loop of render_sequence instead (uniform samples, features, the reprojected history
    of the frame before, the denoiser) under the scene's static camera; with --motion the history follows the moved mesh: a position
    snapshot behind the update, then agpt_render_features_motion and agpt_temporal_accumulate_motion.  The mean effective sample count
    over the moving mesh's pixels (prev_point.w == 1; the snapshot and prev_point are taken without --motion too, for this figure alone)
    is printed per frame.  With --follow-normals the three calls are agpt_scene_snapshot_surfaces, agpt_render_features_surface_motion and
    agpt_temporal_accumulate_surface_motion (with or without --clamp): a mesh that turned keeps its history."""

    def __init__(self, a, ctx, scene, desc, W, H):
        self.a, self.ctx, self.scene, self.W, self.H = a, ctx, scene, W, H
        self.stem, self.ext = os.path.splitext(a.out)
        self.cam = ag.camera_desc(*desc.camera)
        n16, n4 = W * H * 16, W * H * 4
        self.acc = ctx.alloc(n16)
        if a.temporal:
            self.m2, self.out, self.point = ctx.alloc(n4), ctx.alloc(n16), ctx.alloc(n16)
            self.normal = ctx.alloc(n16) if a.follow_normals else 0
            self.sets = [(ctx.alloc(n16), ctx.alloc(n4), ctx.alloc(n16), ctx.alloc(n16)) for _ in range(2)]

    def __call__(self, k):
        """-> (path, a note for the frame's line)"""
        a, ctx, scene, W, H = self.a, self.ctx, self.scene, self.W, self.H
        path = "%s_%04d%s" % (self.stem, k, self.ext)
        pt = ag.PathTracer(5)
        ctx.memset(self.acc, 0, W * H * 16)
        if not a.temporal:
            pt.render(scene, W, H, a.spp, self.acc)
            ag.binding.write_png(path, ctx.resolve(self.acc, W * H, a.spp), W, H)
            return path, ""
        spp = max(2, a.spp)
        cur, prev = self.sets[k & 1], self.sets[(k & 1) ^ 1]
        if a.follow_normals:
            scene.snapshot_surfaces()
        else:
            scene.snapshot_positions()
        ctx.memset(self.m2, 0, W * H * 4)
        pt.render_adaptive(scene, W, H, self.acc, self.m2, spp, spp, spp, 0.0, seed_base=k)
        if a.follow_normals:
            pt.render_features_surface_motion(scene, W, H, cur[2], cur[3], self.point, self.normal)
        else:
            pt.render_features_motion(scene, W, H, cur[2], cur[3], self.point)
        params = ag.TemporalParams(W, H, self.cam, self.cam, a.max_history, ag.TEMPORAL_DEPTH_TOL, ag.TEMPORAL_NORMAL_COS)
        buffers = (self.acc, self.m2, cur[2], cur[3]) + (prev if k else (0, 0, 0, 0)) + (cur[0], cur[1])
        if a.follow_normals:
            ctx.temporal_accumulate_surface_motion(params, clamp_params(a) if a.clamp is not None else None, *buffers, self.point, self.normal)
        elif a.clamp is not None:
            ctx.temporal_accumulate_clamped(params, clamp_params(a), *buffers, self.point if a.motion else 0)
        elif a.motion:
            ctx.temporal_accumulate_motion(params, *buffers, self.point)
        else:
            ctx.temporal_accumulate(params, *buffers)
        ctx.denoise(ag.DenoiseParams(W, H, a.denoise if a.denoise is not None else 5, 1, ag.DENOISE_SIGMA_Z, ag.DENOISE_SIGMA_N,
                                     ag.DENOISE_SIGMA_L), cur[0], cur[1], cur[2], cur[3], self.out)
        ag.binding.write_png(path, ctx.resolve_counts(self.out, W * H), W, H)
        moving = ctx.download(self.point, (H, W, 4))[..., 3] == 1
        counts = ctx.download(cur[0], (H, W, 4))[..., 3]
        note = ", %d moving pixels with %.2f effective samples on average" % (moving.sum(), counts[moving].mean()) if moving.any() else ""
        how = " with motion vectors and previous normals" if a.follow_normals else " with motion vectors" if a.motion else ""
        return path, " + history%s%s%s" % (how, ", clamped" if a.clamp is not None else "", note)


def render_light_orbit(a, ctx, scene, desc, W, H):
    """--light-orbit DEG: the scene's first area light moved DEG degrees further per frame about the vertical axis through the camera's
    lookat, each frame placed with Scene.update_sphere (20 bytes of one device record; nothing is uploaded again) and rendered at --spp
    into OUT_0000.png ...  With --temporal --motion the light's own pixels keep their history; --clamp is what keeps the shadows it
    moves from trailing."""
    prims = [op for op in desc.ops if op[0] in ("mesh", "sphere", "plane", "area_light")]
    lights = [k for k, op in enumerate(prims) if op[0] == "area_light"]
    if not lights:
        raise SystemExit("--light-orbit: the scene has no area light")
    prim, op = lights[0], prims[lights[0]]
    axis = np.asarray(desc.camera[1], np.float64)
    d = op[1].astype(np.float64) - axis
    draw = FrameDrawer(a, ctx, scene, desc, W, H)
    for k in range(a.frames):
        ang = np.deg2rad(a.light_orbit * k)
        c = axis + np.array([np.cos(ang) * d[0] + np.sin(ang) * d[2], d[1], np.cos(ang) * d[2] - np.sin(ang) * d[0]])
        t0 = time.time()
        scene.update_sphere(prim, c.astype(np.float32), op[2])
        t1 = time.time()
        path, note = draw(k)
        print("frame %d: light (primitive %d) at %.0f degrees in %.3f ms, %d spp%s in %.1f ms -> %s" %
              (k, prim, a.light_orbit * k, (t1 - t0) * 1e3, a.spp, note, (time.time() - t1) * 1e3, path))


def smooth_normals(a, scene, prim, op):
    """--smooth-normals: the moving mesh in "smooth" normals mode -- every frame's update recomputes its vertex normals on the GPU from
    the new positions (Scene.set_mesh_normals_mode) instead of turning, blending or keeping the rest normals"""
    if a.smooth_normals:
        if op[2] is None:
            raise SystemExit("--smooth-normals: primitive %d has no normals to write into" % prim)
        scene.set_mesh_normals_mode(prim, "smooth")


def render_spin(a, ctx, scene, desc, W, H):
    """--spin: the scene's last mesh turned once about the vertical axis through its centre over N frames, each frame placed with
    Scene.transform_mesh (16 floats up, the mesh's records rewritten on the GPU) and rendered at --spp into OUT_0000.png ..."""
    meshes = [(k, op) for k, op in enumerate(o for o in desc.ops if o[0] in ("mesh", "sphere", "plane", "area_light")) if op[0] == "mesh"]
    prim, op = meshes[-1] if a.spin_prim is None else [m for m in meshes if m[0] == a.spin_prim][0]
    c = 0.5 * (op[1].min(0).astype(np.float64) + op[1].max(0))
    smooth_normals(a, scene, prim, op)
    draw = FrameDrawer(a, ctx, scene, desc, W, H)
    for k in range(sequence_frames(a, a.spin)):
        ang = 2 * np.pi * k / a.spin
        m = np.eye(4)
        m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
        m[:3, 3] = c - m[:3, :3] @ c
        t0 = time.time()
        scene.transform_mesh(prim, m.astype(np.float32))
        t1 = time.time()
        path, note = draw(k)
        print("frame %d: primitive %d turned %.0f degrees in %.2f ms, %d spp%s in %.1f ms -> %s" %
              (k, prim, np.degrees(ang), (t1 - t0) * 1e3, a.spp, note, (time.time() - t1) * 1e3, path))


def render_bend(a, ctx, scene, desc, W, H):
    """--bend: the scene's last mesh bound to two joints -- the second one's weight grows smoothly from 0 to 1 along the mesh's x
    extent -- and bent to and fro about the z axis through its centre over N frames, each frame posed with Scene.pose_mesh (two
    matrices up, the blend and the mesh's records on the GPU) and rendered at --spp into OUT_0000.png ..."""
    meshes = [(k, op) for k, op in enumerate(o for o in desc.ops if o[0] in ("mesh", "sphere", "plane", "area_light")) if op[0] == "mesh"]
    prim, op = meshes[-1]
    v, n = op[1], op[2]
    if n is not None and len(n) != len(v):
        raise SystemExit("--bend: the mesh has %d normals for %d vertices; its normals need influences of their own" % (len(n), len(v)))
    smooth_normals(a, scene, prim, op)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    c = 0.5 * (lo + hi)
    t = (v[:, 0] - lo[0]) / max(hi[0] - lo[0], 1e-30)
    t = (t * t * (3 - 2 * t)).astype(np.float32)
    scene.set_mesh_skin(prim, np.tile(np.array([0, 1], np.int32), (len(v), 1)), np.stack([np.float32(1) - t, t], 1), n_joints=2)
    draw = FrameDrawer(a, ctx, scene, desc, W, H)
    for k in range(sequence_frames(a, a.bend)):
        ang = np.radians(50.0) * np.sin(2 * np.pi * k / a.bend)
        m = np.eye(4)
        m[0, 0], m[0, 1], m[1, 0], m[1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
        m[:3, 3] = c - m[:3, :3] @ c
        t0 = time.time()
        scene.pose_mesh(prim, np.stack([np.eye(4), m]).astype(np.float32))
        t1 = time.time()
        path, note = draw(k)
        print("frame %d: primitive %d bent %.0f degrees in %.2f ms, %d spp%s in %.1f ms -> %s" %
              (k, prim, np.degrees(ang), (t1 - t0) * 1e3, a.spp, note, (time.time() - t1) * 1e3, path))


def render_morph(a, ctx, scene, desc, W, H):
    """--morph: the scene's last mesh with two morph targets -- a swelling of its far half along x and a squash towards its middle height
    (position deltas only: the normals keep their rest values unless --smooth-normals recomputes them) -- whose weights swing out of phase over N frames, each frame morphed
    with Scene.morph_mesh (two weights up, the blend and the mesh's records on the GPU) and rendered at --spp into OUT_0000.png ..."""
    meshes = [(k, op) for k, op in enumerate(o for o in desc.ops if o[0] in ("mesh", "sphere", "plane", "area_light")) if op[0] == "mesh"]
    prim, op = meshes[-1]
    smooth_normals(a, scene, prim, op)
    v = op[1].astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    c = 0.5 * (lo + hi)
    t = np.clip((v[:, 0] - c[0]) / max(hi[0] - c[0], 1e-30), 0, 1)
    swell = 0.6 * (t * t * (3 - 2 * t))[:, None] * (v - c) * [0, 1, 1]
    squash = -0.5 * (v - c) * [0, 1, 0]
    scene.set_mesh_morph_targets(prim, np.stack([swell, squash]).astype(np.float32))
    draw = FrameDrawer(a, ctx, scene, desc, W, H)
    for k in range(sequence_frames(a, a.morph)):
        w = np.array([0.5 - 0.5 * np.cos(2 * np.pi * k / a.morph), np.sin(2 * np.pi * k / a.morph)], np.float32)
        t0 = time.time()
        scene.morph_mesh(prim, w)
        t1 = time.time()
        path, note = draw(k)
        print("frame %d: primitive %d morphed by weights (%.2f, %.2f) in %.2f ms, %d spp%s in %.1f ms -> %s" %
              (k, prim, w[0], w[1], (t1 - t0) * 1e3, a.spp, note, (time.time() - t1) * 1e3, path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3", choices=["c1", "c2", "c3", "c5", "simple", "heightfield", "textured", "mapped"])
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--out", default="gpurun_out/render.png")
    ap.add_argument("--pfm", default=None, help="also write the linear float image")
    ap.add_argument("--bvh-builder", default="host", choices=["host", "device"], help="where the mesh BVHs are built (same trees)")
    ap.add_argument("--shading", default="exact", choices=["exact", "fast"],
                    help="shading arithmetic: exact (bit-identical to the oracle) or fast (agpt_scene_set_shading_arith)")
    ap.add_argument("--adaptive", type=float, default=None, metavar="REL_ERROR",
                    help="adaptive sampling (agpt_render_adaptive) with this stop-test threshold instead of --spp uniform samples")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=256)
    ap.add_argument("--step-spp", type=int, default=16)
    ap.add_argument("--abs-floor", type=float, default=0.01, help="adaptive: luminance floor of the stop test")
    ap.add_argument("--counts-png", default=None, help="adaptive: also write a heat map of the per-pixel sample counts")
    ap.add_argument("--denoise", type=int, nargs="?", const=5, default=None, metavar="ITER",
                    help="denoise the render (agpt_render_features + agpt_denoise, ITER a-trous passes, default 5) before the resolve; "
                         "implies the adaptive entry point -- uniform at --spp when --adaptive is not given")
    ap.add_argument("--features-png", default=None, metavar="PREFIX", help="write PREFIX_albedo.png and PREFIX_normal.png (first-hit features)")
    ap.add_argument("--filter", default="nearest", choices=["nearest", "bilinear"],
                    help="scenes textured / mapped: how every texture is read (agpt_scene_set_texture_sampler)")
    ap.add_argument("--wrap", default="repeat", choices=["repeat", "clamp", "mirror"], help="scenes textured / mapped: wrap mode of both axes")
    ap.add_argument("--normal-map", type=float, nargs="?", const=1.0, default=None, metavar="SCALE",
                    help="scenes textured / mapped: a procedural bump image (a field of round studs) as tangent-space normal map on both mesh "
                         "materials, read like the other textures (agpt_scene_set_material_normal_texture)")
    ap.add_argument("--frames", type=int, default=1, metavar="N",
                    help="render a sequence of N frames at --spp each (uniform, denoised) into numbered files OUT_0000.png ...")
    ap.add_argument("--orbit", type=float, default=0.0, metavar="DEG", help="--frames: the camera turns DEG degrees about its lookat over the sequence")
    ap.add_argument("--temporal", action="store_true",
                    help="--frames: add each frame's reprojected history (agpt_temporal_accumulate) before the denoiser")
    ap.add_argument("--max-history", type=float, default=32.0, help="--temporal: cap on the reprojected sample count")
    ap.add_argument("--clamp", type=float, nargs="?", const=1.0, default=None, metavar="GAMMA",
                    help="--temporal: clamp the reprojected history to mean +- GAMMA standard deviations (default 1) of the frame's own "
                         "neighbourhood (agpt_temporal_accumulate_clamped): shadows and bounce light do not trail behind what moved")
    ap.add_argument("--clamp-radius", type=int, default=2, choices=(1, 2, 3), help="--clamp: the neighbourhood's half-width in pixels")
    ap.add_argument("--motion", action="store_true",
                    help="--temporal with --spin, --bend or --morph: the history follows the moved mesh (agpt_scene_snapshot_positions after "
                         "each frame's update, agpt_render_features_motion, agpt_temporal_accumulate_motion)")
    ap.add_argument("--follow-normals", action="store_true",
                    help="--temporal --motion: the normal test uses the normal the surface point had a frame ago, so a mesh that turns keeps "
                         "its history (agpt_scene_snapshot_surfaces, agpt_render_features_surface_motion, "
                         "agpt_temporal_accumulate_surface_motion); with or without --clamp")
    ap.add_argument("--spin", type=int, default=0, metavar="N",
                    help="N frames at --spp each with one mesh turned about its vertical axis by agpt_scene_transform_mesh (OUT_0000.png ...)")
    ap.add_argument("--spin-prim", type=int, default=None, metavar="PRIM", help="--spin: the mesh primitive that turns (default: the scene's last mesh)")
    ap.add_argument("--bend", type=int, default=0, metavar="N",
                    help="N frames at --spp each with the scene's last mesh (the blob of textured / mapped) bent by two joints through "
                         "agpt_scene_set_mesh_skin / agpt_scene_pose_mesh (OUT_0000.png ...)")
    ap.add_argument("--morph", type=int, default=0, metavar="N",
                    help="N frames at --spp each with the scene's last mesh (the blob of textured / mapped) morphed by two targets through "
                         "agpt_scene_set_mesh_morph_targets / agpt_scene_morph_mesh (OUT_0000.png ...)")
    ap.add_argument("--light-orbit", type=float, default=0.0, metavar="DEG",
                    help="--frames N: the scene's first area light moves DEG degrees per frame about the vertical axis through the camera's "
                         "lookat (agpt_scene_update_sphere); the camera stays")
    ap.add_argument("--smooth-normals", action="store_true",
                    help="--spin, --bend, --morph: the moving mesh in AGPT_NORMALS_SMOOTH mode (agpt_scene_set_mesh_normals_mode): its vertex "
                         "normals are recomputed on the GPU from every frame's positions")
    a = ap.parse_args()
    if a.smooth_normals and not (a.spin or a.bend or a.morph):
        ap.error("--smooth-normals applies to --spin, --bend and --morph")
    animated = a.spin or a.bend or a.morph or a.light_orbit
    if (a.spin > 0) + (a.bend > 0) + (a.morph > 0) + (a.light_orbit != 0) > 1:
        ap.error("--spin, --bend, --morph and --light-orbit are separate sequences")
    if a.light_orbit and a.frames < 2:
        ap.error("--light-orbit applies to a sequence (--frames N, N >= 2)")
    if animated and a.orbit:
        ap.error("--orbit applies to --frames alone: --spin, --bend and --morph keep the scene's camera (with --frames F they stop after F frames)")
    if a.orbit and a.frames < 2 or a.temporal and a.frames < 2 and not animated:
        ap.error("--temporal and --orbit apply to a sequence (--frames N, N >= 2; --temporal also to --spin, --bend and --morph)")
    if a.clamp is not None and not a.temporal:
        ap.error("--clamp applies to --temporal")
    if a.clamp is not None and not a.clamp >= 0:
        ap.error("--clamp GAMMA must be non-negative")
    if a.motion and not (a.temporal and animated):
        ap.error("--motion applies to --temporal with one of --spin, --bend, --morph and --light-orbit")
    if a.follow_normals and not (a.temporal and a.motion):
        ap.error("--follow-normals applies to --temporal --motion")
    W, H = a.width, a.height
    aspect = W / float(H)
    desc = {"c1": lambda: ag.scenes.scene_c1(), "c2": lambda: ag.scenes.scene_c2(aspect=aspect),
            "c3": lambda: ag.scenes.scene_c3(aspect=aspect), "c5": lambda: ag.scenes.scene_c5(aspect=aspect),
            "simple": lambda: ag.scenes.scene_simple_test(), "textured": lambda: ag.scenes.scene_textured(), "mapped": lambda: ag.scenes.scene_mapped(),
            "heightfield": lambda: ag.scenes.scene_heightfield(361, True, W, H)}[a.scene]()
    if a.normal_map is not None:
        if a.scene not in ("textured", "mapped"):
            ap.error("--normal-map applies to the scenes textured and mapped")
        # the floor and the blob (scenes.scene_textured).  The backdrop's u runs 0..36 along the sweep, the last unit of it over the ~32
        # units of flat floor, and v 0..1 across its 40 units: 48 x 60 studs per image are round and two thirds of a unit wide on the
        # floor (and far below a pixel on the wall behind, where the image repeats 35 times: no mip-mapping)
        desc.set_material_normal_texture(0, desc.add_texture(stud_normal_map(48, 60, 8)), a.normal_map)
        desc.set_material_normal_texture(2, desc.add_texture(stud_normal_map(8, 4)), a.normal_map)
    if (a.filter, a.wrap) != ("nearest", "repeat"):
        if a.scene not in ("textured", "mapped"):
            ap.error("--filter / --wrap apply to the scenes textured and mapped")
        wrap = {"repeat": ag.WRAP_REPEAT, "clamp": ag.WRAP_CLAMP, "mirror": ag.WRAP_MIRROR}[a.wrap]
        for t in range(desc.n_textures):
            desc.set_texture_sampler(t, ag.FILTER_BILINEAR if a.filter == "bilinear" else ag.FILTER_NEAREST, wrap, wrap)
    ctx = ag.Context(0)
    t0 = time.time()
    scene = ag.Scene(ctx)
    scene.set_bvh_builder(a.bvh_builder)
    scene.set_shading_arith(a.shading)
    scene = desc.instantiate(scene)
    print("scene build + BVH + upload: %.2f s" % (time.time() - t0))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.frames > 1 and not animated:
        return render_sequence(a, ctx, scene, desc, W, H)
    if a.spin:
        return render_spin(a, ctx, scene, desc, W, H)
    if a.bend:
        return render_bend(a, ctx, scene, desc, W, H)
    if a.morph:
        return render_morph(a, ctx, scene, desc, W, H)
    if a.light_orbit:
        return render_light_orbit(a, ctx, scene, desc, W, H)
    ptr = ctx.alloc(W * H * 16)
    ctx.memset(ptr, 0, W * H * 16)
    features = None
    if a.denoise is not None or a.features_png:
        features = (ctx.alloc(W * H * 16), ctx.alloc(W * H * 16))
        ag.PathTracer(5).render_features(scene, W, H, *features)
        if a.features_png:   # albedo as it is, the normal as n / 2 + 1/2 (black where nothing was hit), both through the display resolve
            for suffix, p in (("albedo", features[0]), ("normal", features[1])):
                img = ctx.download(p, (H, W, 4)).copy()
                if suffix == "normal":
                    img[..., :3] = np.where(img[..., 3:4] > 0, img[..., :3] * 0.5 + 0.5, 0.0) ** 2.2   # (the resolve applies 1 / 2.2)
                img[..., 3] = 1.0
                tmp = ctx.alloc(img.nbytes)
                ctx.upload(tmp, img)
                ag.binding.write_png("%s_%s.png" % (a.features_png, suffix), ctx.resolve_counts(tmp, W * H), W, H)
                ctx.free(tmp)
    if a.adaptive is not None or a.denoise is not None:
        mptr = ctx.alloc(W * H * 4)
        ctx.memset(mptr, 0, W * H * 4)
        t0 = time.time()
        if a.adaptive is not None:
            st, ast = ag.PathTracer(5).render_adaptive(scene, W, H, ptr, mptr, a.min_spp, a.max_spp, a.step_spp, a.adaptive, a.abs_floor)
        else:   # uniform through the adaptive entry point: it keeps the luminance second moment the denoiser reads
            a.min_spp = a.max_spp = spp = max(2, a.spp)
            st, ast = ag.PathTracer(5).render_adaptive(scene, W, H, ptr, mptr, spp, spp, spp, 0.0)
        dt = time.time() - t0
        if a.denoise is not None:
            out = ctx.alloc(W * H * 16)
            t1 = time.time()
            ctx.denoise(ag.DenoiseParams(W, H, a.denoise, 1, ag.DENOISE_SIGMA_Z, ag.DENOISE_SIGMA_N, ag.DENOISE_SIGMA_L), ptr, mptr,
                        features[0], features[1], out)
            print("denoise: %d passes, %.2f ms" % (a.denoise, (time.time() - t1) * 1e3))
            ag.binding.write_png(a.out, ctx.resolve_counts(out, W * H), W, H)
            if a.pfm:
                ag.binding.write_pfm(a.pfm, ctx.download(out, (H, W, 4)), 1)
                a.pfm = None
            ctx.free(out)
        else:
            ag.binding.write_png(a.out, ctx.resolve_counts(ptr, W * H), W, H)
        ctx.free(mptr)
        acc = ctx.download(ptr, (H, W, 4))
        counts = acc[..., 3]
        print("adaptive: %d rounds, %.1f spp on average (%d..%d), %d pixels stopped by the test" %
              (ast.rounds, counts.mean(), counts.min(), counts.max(), ast.pixels_stopped))
        if a.pfm:   # the PFM writer divides by one count: normalise here
            img = acc.copy()
            img[..., :3] /= np.maximum(counts, 1)[..., None]
            ag.binding.write_pfm(a.pfm, img, 1)
        if a.counts_png:   # black (min_spp) .. red .. yellow .. white (max_spp), in the order of the resolved image
            t = np.clip((counts - a.min_spp) / float(max(1, a.max_spp - a.min_spp)), 0, 1)
            rgb = (np.stack([np.clip(3 * t, 0, 1), np.clip(3 * t - 1, 0, 1), np.clip(3 * t - 2, 0, 1)], -1) * 255).astype(np.uint32)
            ag.binding.write_png(a.counts_png, ((rgb[..., 0] << 16) | (rgb[..., 1] << 8) | rgb[..., 2]).reshape(-1), W, H)
        a.spp = int(round(float(counts.mean())))
    else:
        t0 = time.time()
        st = ag.PathTracer(5).render(scene, W, H, a.spp, ptr)
        dt = time.time() - t0
        packed = ctx.resolve(ptr, W * H, a.spp)
        ag.binding.write_png(a.out, packed, W, H)
        if a.pfm:
            ag.binding.write_pfm(a.pfm, ctx.download(ptr, (H, W, 4)), a.spp)
    print("%s: %dx%d @%d spp, %d tris, %.2f s, %.1f Mrays/s -> %s" % (desc.name, W, H, a.spp, desc.n_tris, dt, st.rays / dt / 1e6, a.out))


if __name__ == "__main__":
    main()
