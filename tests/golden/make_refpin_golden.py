#!/usr/bin/env python3
"""Generates tests/golden/refpin_*.npz from the REFERENCE'S OWN hot path compiled in place (oracle/ref_hotpath.cpp ->
oracle/_ref/libref_hotpath.so, `make -C oracle ref`): DisneyMaterial / MirrorMaterial / BSDF, Scene::Intersect and IntersectP over
BVHTriMesh, Sphere and Plane, BVHTriMesh's node bytes, TriangleMesh::CreateBackdrop, Camera and PathTracer::Li, the last two in both trig
definitions.  The reference exists only in the build container, so this script runs there only:

    python tests/golden/make_refpin_golden.py        (rewrites tests/golden/refpin_*.npz; commit the result)

The fixtures are data only: seeded inputs and what the reference's code returned for them.  tests/test_refpin.py holds the oracle
(both trig modes), the host builders and the HIP path to them bit for bit, and -- where the library is present -- re-runs this script's
generate() and requires the committed bytes.  The input builders below need no reference and are what the tests import.
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import ag_pathtracer_amd as ag  # noqa: E402

F = np.float32
FLT_MAX = F(3.402823466e+38)
BELOW_ONE = np.nextafter(F(1), F(0))
DEPTHS = (0, 1, 5)
MODES = ("libm", "cr")     # oracle.TRIG_LIBM = 0, oracle.TRIG_CORRECTLY_ROUNDED = 1
LI_SCENES = ("mixed", "spheres_env", "gauntlet", "no_lights")
N_LI = 2048


def load(name):
    return np.load(os.path.join(HERE, name))


def save(name, arrays):
    """np.savez_compressed with fixed zip timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(os.path.join(HERE, name), "w") as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[key])
            np.lib.format.write_array(buf, a if a.flags.c_contiguous else a.copy(order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


# ---- BSDF -------------------------------------------------------------------------------------------------------------------------------
ROUGHNESS = (0.0, 0.02, 0.25, 0.5, 1.0)
METALLIC = (0.0, 0.5, 1.0)


def bsdf_materials(scene):
    """15 Disney materials (roughness x metallic), diffuse-only, mirror -> their ids, in this order."""
    mats = [scene.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], r, m) for r in ROUGHNESS for m in METALLIC]
    mats.append(scene.add_material(ag.MAT_DIFFUSE_ONLY, [.7, .6, .5]))
    mats.append(scene.add_material(ag.MAT_MIRROR, [.9, .8, .7]))
    return mats


def bsdf_inputs():
    """The 512 rows of make_golden.kat_inputs plus edge rows: every pair of nine special directions (the poles, three directions in
    the horizon plane z = 0, z = +-1e-4, one above and one below) -- which holds wi == wo, wi == -wo (zero half vector) and wi below
    the horizon -- with u cycling through (0,0), (.5,.5), the largest float below 1 in either slot and exactly 1 in either or both
    (RandomFloat can return 1); then one generic direction above and one below the horizon with each of those u."""
    import make_golden as mg
    wo, wi, u = mg.kat_inputs()
    n3 = lambda v: np.asarray(v, np.float64) / np.linalg.norm(v)
    special = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0.6, 0.8, 0], n3([1, 0, 1e-4]), n3([.6, .8, -1e-4]),
               n3([1, .3, 1]), n3([.6, -.2, -.8])]
    us = [[0, 0], [.5, .5], [BELOW_ONE, .3], [.3, BELOW_ONE], [1, 1], [1, .25], [.25, 1]]
    ewo, ewi, eu = [], [], []
    for a in special:
        for b in special:
            ewo.append(a)
            ewi.append(b)
            eu.append(us[len(eu) % len(us)])
    for a in (special[7], special[8]):
        for uu in us:
            ewo.append(a)
            ewi.append(special[7])
            eu.append(uu)
    return (np.concatenate([wo, np.asarray(ewo, F)]), np.concatenate([wi, np.asarray(ewi, F)]),
            np.concatenate([u, np.asarray(eu, F)]))


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def backdrop():
    g = load("refpin_backdrop.npz")
    return g["verts"], g["normals"], g["uvs"], g["indices"]


def intersect_scene(bd=None, lights=False):
    """The reference backdrop (radius 7.5, 32 segments), one-leaf meshes of 5 and 12 triangles (stacked_triangles of
    test_gpu_intersect.py), a mesh of one ordinary and one zero-area triangle, two overlapping spheres and a plane; with lights=True two
    sphere lights and a uniform sky as well (the first Li scene)."""
    from test_gpu_intersect import stacked_triangles
    d = ag.SceneDesc("refpin-mixed")
    floor = d.add_material(ag.MAT_DISNEY, ag.scenes.hex2lin(0xcbceb1), 1.0, 0.0)
    gold = d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], 0.5, 1.0)
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5])
    glossy = d.add_material(ag.MAT_DISNEY, [.8, .3, .2], .25, .5)
    mirror = d.add_material(ag.MAT_MIRROR, [.9, .9, .9])
    v, n, t, idx = bd if bd is not None else backdrop()
    d.add_mesh(v, n, t, idx, floor, 1)
    v5, i5 = stacked_triangles(5, [4, 1, 0], 1)
    d.add_mesh(v5, None, None, i5, grey, 1)
    v12, i12 = stacked_triangles(12, [0, 3, 0], 3)
    d.add_mesh(v12, None, None, i12, glossy, 1)
    vz = F([[-3, 0, -1], [-2, 0, -1], [-2.5, 1.5, -1.5], [-4, 2, 1], [-3, 2, 1], [-3.5, 2, 1]])   # the second triangle has no area
    d.add_mesh(vz, None, None, np.stack([np.arange(6, dtype=np.int32)] * 3, 1), grey, 1)
    d.add_sphere([0, 0, 0], 1.0, gold)
    d.add_sphere([0.8, 0.3, -0.4], 0.7, mirror)
    d.add_plane([0.5, -0.5, -1.0], [3.0, 2.0], glossy)
    if lights:
        d.add_area_light([0, 25, -20], 1.0, ag.scenes.KEY_LIGHT * F(200))
        d.add_area_light([-3, 4, -3], 0.5, ag.scenes.KEY_LIGHT * F(20))
        d.add_uniform_infinite_light([.4, .45, .5])
    d.set_camera([-1.46, 2.16, -6.64], [0, 0.5, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    return d


def intersect_rays(desc):
    """8,192 rays of helpers.random_rays, then rays that start on a triangle's plane (the floor y = -1, in-plane and leaving it), on a
    face of the backdrop's box (x = +-20, along the face and through it) and rays parallel to the plane primitive (D.y = 0, at its
    height and off it, and rays that graze its edges)."""
    from helpers import random_rays
    rays = random_rays(desc, 8192, seed=31)
    o = [[1, -1, 5], [1, -1, 5], [1, -1, 5], [-2, -1, 8], [20, 3, 4], [20, 3, 4], [20, 3, 4], [-20, 0, 10], [-20, -1, 10],
         [-4, -0.5, -1], [-4, -0.5, -1.5], [-4, 0.2, -1], [0.5, 3, -1], [2.0, 3, -1], [2.0, 3, 0], [0.5, -3, 0.0], [-1, 3, -2]]
    dd = [[1, 0, 0], [0, 1, 0], [1, 1, -1], [0, 0, -1], [0, 0, -1], [-1, 0, 0], [0, -1, 1], [1, 0, 0], [1, 0, 1],
          [1, 0, 0], [1, 0, .2], [1, 0, 0], [0, -1, 0], [0, -1, 0], [0, -1, 0], [0, 1, 0], [0, -1, 0]]
    extra = np.zeros(len(o), ag.RAY_DTYPE)
    extra["o"], extra["d"], extra["tmax"] = o, dd, FLT_MAX
    return np.concatenate([rays, extra])


def env_image():
    """synthetic_hdr(16, 8) rounded to what an RGBE pixel holds: the reference reads its map from an .hdr file."""
    from oracle.ref_binding import rgbe_exact
    return rgbe_exact(ag.scenes.synthetic_hdr(16, 8))


def li_scene(name, bd=None):
    bd = bd if bd is not None else backdrop()
    if name == "mixed":
        return intersect_scene(bd, lights=True)
    if name == "spheres_env":    # analytic primitives only: a mirror, a polished and a rough metal, a dielectric ground; env map; thin lens
        d = ag.SceneDesc("refpin-spheres-env")
        d.add_sphere([0, 0, 0], 1.0, d.add_material(ag.MAT_MIRROR, [.9, .9, .9]))
        d.add_sphere([2.1, 0, 0.3], 1.0, d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], 0.02, 1.0))
        d.add_sphere([-2.1, 0, 0.3], 1.0, d.add_material(ag.MAT_DISNEY, [.7, .75, .8], 0.5, 1.0))
        d.add_sphere([0, -101, 0], 100.0, d.add_material(ag.MAT_DISNEY, [.2, .6, .8], .8, 0.))
        d.add_infinite_area_light(env_image())
        d.set_camera([0, 1.5, -6], [0, 0, 0], [0, 1, 0], 1.0, 40.0, 0.15)
        return d
    if name == "gauntlet":       # emitter_gauntlet() of test_gpu_render.py on the reference's backdrop
        from test_gpu_render import emitter_gauntlet
        d = ag.scenes.scene_c1(backdrop=bd)
        d.name = "refpin-gauntlet"
        for op in [op for op in emitter_gauntlet().ops if op[0] == "area_light"][1:]:
            d.add_area_light(op[1], op[2], op[3])
        return d
    d = ag.SceneDesc("refpin-no-lights")
    floor = d.add_material(ag.MAT_DISNEY, ag.scenes.hex2lin(0xcbceb1), 1.0, 0.0)
    gold = d.add_material(ag.MAT_DISNEY, [0.944, 0.776, 0.373], 0.5, 1.0)
    d.add_mesh(*bd, floor, 1)
    d.add_sphere([0, 0, 0], 1.0, gold)
    d.set_camera([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.0)
    return d


def li_film_inputs(k):
    rng = np.random.RandomState(100 + k)
    return rng.uniform(size=(N_LI, 2)).astype(F), rng.randint(1, 2 ** 31 - 1, N_LI).astype(np.uint32)


# ---- BVH --------------------------------------------------------------------------------------------------------------------------------
def bvh_meshes():
    from test_gpu_intersect import deep_mesh, stacked_triangles
    hv, _, _, hi = ag.scenes.heightfield(15)
    dv, di, _, _ = deep_mesh()
    sv, si = stacked_triangles(20, [-4, 1, 1], 2)
    rng = np.random.RandomState(77)
    c = rng.uniform(-1, 1, (300, 3))
    v = (c[:, None, :] + rng.normal(scale=0.05, size=(300, 3, 3))).astype(F)
    v[::20, 1] = v[::20, 0]          # 5 %: two corners equal
    v[7::20, 2] = v[7::20, 1] = v[7::20, 0]   # 5 %: a point
    soup_i = np.stack([np.arange(900, dtype=np.int32)] * 3, 1)
    # none of the four above ever takes the leaf branch of bvhtrimesh.h:291 (a split is always cheaper): 15 clumps of four large,
    # nearly coincident triangles do, at maxPrimsInNode 4
    cc = rng.uniform(-10, 10, (15, 1, 1, 3))
    clumps = (cc + rng.normal(scale=1.0, size=(15, 1, 3, 3)) + rng.normal(scale=0.01, size=(15, 4, 3, 3))).astype(F).reshape(-1, 3)
    clump_i = np.stack([np.arange(180, dtype=np.int32)] * 3, 1)
    return {"heightfield15": (hv, hi), "deep40": (dv, di), "stacked20": (sv, si), "soup300": (v.reshape(-1, 3), soup_i),
            "clumps60": (clumps, clump_i)}


# ---- camera -----------------------------------------------------------------------------------------------------------------------------
CAMERAS = [([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.0),
           ([-1.46, 1.16, -4.64], [0, 0, 0], [0, 1, 0], 1.0, 45.0, 0.15),
           ([-13.2, 4.2, 5.4], [6.0, 4.0, -1.5], [0, 1, 0], 16.0 / 9.0, 58.0, 0.0),
           ([-13.2, 4.2, 5.4], [6.0, 4.0, -1.5], [0, 1, 0], 16.0 / 9.0, 58.0, 0.15),
           ([0, 2.2, -4.2], [0, 0, 0], [0, 1, 0], 16.0 / 9.0, 25.0, 0.0),
           ([3, .5, 2], [0, 0, 0], [0.1, 1, 0.05], 1.0, 70.0, 0.15),
           ([0, 8, 0], [0, 0, 1e-3], [0, 1, 0], 1.0, 30.0, 0.0),        # straight down: vup and the view direction nearly parallel
           ([0, 8, 0], [1e-3, 0, 0], [0, 1, 0], 16.0 / 9.0, 60.0, 0.15)]
N_CAMERA_RAYS = 64


def camera_film_inputs(k):
    rng = np.random.RandomState(200 + k)
    st = rng.uniform(size=(N_CAMERA_RAYS, 2)).astype(F)
    st[:4] = [[0, 0], [1, 1], [0.5, 0.5], [0, 1]]
    return st, rng.randint(1, 2 ** 31 - 1, N_CAMERA_RAYS).astype(np.uint32)


# ---- trig probe -------------------------------------------------------------------------------------------------------------------------
def find_trig_probe(rb):
    """The first u2 = k / 20000 at which the reference's slope sampling (microfacet.h:38-40) differs between the two trig modes."""
    for k in range(1, 20000):
        u2 = F(k / 20000.0)
        rb.set_trig_mode(0)
        a = rb.trig_probe(u2).copy()
        rb.set_trig_mode(1)
        b = rb.trig_probe(u2).copy()
        rb.set_trig_mode(0)
        if a.tobytes() != b.tobytes():
            return u2, a, b
    raise AssertionError("no input separates the trig modes")


# ---- generation (needs the reference) ---------------------------------------------------------------------------------------------------
def generate(only=None):
    """-> {file name: {array name: array}} from the reference harness.  `only`: a collection of file names to produce."""
    from oracle import ref_binding as rb
    out = {}
    want = lambda name: only is None or name in only
    rb.set_trig_mode(0)
    bd = rb.create_backdrop([0, -1, 20], [40, 20, 40], 7.5, 32)     # host-side scene prep: the C library's trig, as in the oracle
    if want("refpin_backdrop.npz"):
        out["refpin_backdrop.npz"] = dict(verts=bd[0], normals=bd[1], uvs=bd[2], indices=bd[3])

    if want("refpin_misc.npz"):
        u2, a, b = find_trig_probe(rb)
        misc = dict(probe_u2=u2, probe_libm=a, probe_cr=b, rng_first=rb.rng_floats(0x12345678, 4))
        for k, cam in enumerate(CAMERAS):
            misc["camera_%d" % k] = rb.camera_vectors(*cam)
            s = rb.RefScene()
            s.set_camera(*cam)
            st, states = camera_film_inputs(k)
            misc["camera_rays_%d" % k], misc["camera_states_%d" % k] = s.camera_rays(st, states)
        out["refpin_misc.npz"] = misc

    if want("refpin_bvh.npz"):
        b = {}
        for name, (v, idx) in bvh_meshes().items():
            for mp in (1, 2, 4):
                b["%s_mp%d_nodes" % (name, mp)], b["%s_mp%d_order" % (name, mp)] = rb.bvh(v, idx, mp)
        out["refpin_bvh.npz"] = b

    if any(want(n) for n in ("refpin_bsdf_eval.npz", "refpin_bsdf_sample_libm.npz", "refpin_bsdf_sample_cr.npz")):
        s = rb.RefScene()
        mats = bsdf_materials(s)
        wo, wi, u = bsdf_inputs()
        ev = dict(wo=wo, wi=wi, u=u)
        for m in mats:
            ev["f_%d" % m], ev["pdf_%d" % m] = s.bsdf_eval(m, wo, wi)
        rb.set_trig_mode(1)
        for m in mats:   # BSDF::f and Pdf call no trigonometric function
            f, pdf = s.bsdf_eval(m, wo, wi)
            assert f.tobytes() == ev["f_%d" % m].tobytes() and pdf.tobytes() == ev["pdf_%d" % m].tobytes()
        out["refpin_bsdf_eval.npz"] = ev
        for mode, name in enumerate(MODES):
            rb.set_trig_mode(mode)
            sm = {}
            for m in mats:
                sm["wi_%d" % m], sm["f_%d" % m], sm["pdf_%d" % m], sm["spec_%d" % m] = s.bsdf_sample(m, wo, u)
            out["refpin_bsdf_sample_%s.npz" % name] = sm
        rb.set_trig_mode(0)

    if want("refpin_hits.npz"):
        desc = intersect_scene(bd)
        s = desc.instantiate(rb.RefScene())
        rays = intersect_rays(desc)
        closest, uv, amb = s.intersect(rays)
        anyhit, _, _ = s.intersect(rays, any_hit=True)
        hits = dict(rays=rays, closest=closest, uv=uv, ambiguous=amb, anyhit=anyhit["hit"])
        for mode, name in enumerate(MODES):      # the sphere's uv goes through atan2 and acos (intersectable.h:186-190)
            rb.set_trig_mode(mode)
            hits["dbg_" + name] = s.dbg_li(rays)
            again, _, _ = s.intersect(rays)
            assert again.tobytes() == closest.tobytes()     # the hit record itself calls no trigonometric function
        rb.set_trig_mode(0)
        out["refpin_hits.npz"] = hits

    for k, name in enumerate(LI_SCENES):
        fname = "refpin_li_%s.npz" % name
        if not want(fname):
            continue
        rb.set_trig_mode(0)      # scene construction (InfiniteAreaLight's sin(theta) weights) is host-side
        s = li_scene(name, bd).instantiate(rb.RefScene())
        st, states = li_film_inputs(k)
        rays, start = s.camera_rays(st, states)
        li = dict(rays=rays, states=start)
        for mode, mname in enumerate(MODES):
            rb.set_trig_mode(mode)
            for depth in DEPTHS:
                L, after, draws, calls = s.li(rays, start, depth)
                key = "%s_d%d" % (mname, depth)
                li["L_" + key], li["after_" + key], li["draws_" + key], li["calls_" + key] = L, after, draws.astype(np.int16), np.int64(calls)
        rb.set_trig_mode(0)
        out[fname] = li
    return out


FILES = ["refpin_backdrop.npz", "refpin_misc.npz", "refpin_bvh.npz", "refpin_bsdf_eval.npz", "refpin_bsdf_sample_libm.npz",
         "refpin_bsdf_sample_cr.npz", "refpin_hits.npz"] + ["refpin_li_%s.npz" % n for n in LI_SCENES]


def main():
    for name, arrays in generate().items():
        save(name, arrays)
        print(name, os.path.getsize(os.path.join(HERE, name)))


if __name__ == "__main__":
    main()
