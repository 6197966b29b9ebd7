"""Shared test helpers: instantiate one SceneDesc on the CPU oracle (checker) and on the GPU (product), render it on either, build the
C and C++ programs the tests run against include/, and the comparisons more than one test file makes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import ag_pathtracer_amd as ag
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_scene(desc, max_depth=None):
    s = desc.instantiate(ob.OracleScene())
    if max_depth is not None:
        s.set_max_depth(max_depth)
    return s


def oracle_render_on(o, W, H, spp, **kw):
    """o.render on the GPU's per-(pixel, sample) RNG streams, with correctly-rounded trig -- what the kernels compute -- for the call"""
    kw.setdefault("threads", 8)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        return o.render(W, H, spp, rng_mode=ob.RNG_PER_SAMPLE, **kw)
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)


def oracle_render(desc, W, H, spp, max_depth=5, **kw):
    """(accumulator, stats) of oracle_render_on for a fresh oracle scene of desc"""
    return oracle_render_on(oracle_scene(desc, max_depth), W, H, spp, **kw)


def oracle_samples(desc, W, H, n, first=0, tile=None, max_depth=5):
    """[n, H, W, 3]: the oracle's radiance of samples first .. first + n - 1 of every pixel (of the tile; zero elsewhere), one by one"""
    o = oracle_scene(desc, max_depth)
    return np.stack([oracle_render_on(o, W, H, 1, spp_begin=first + s, tile=tile)[0][..., :3] for s in range(n)])


def deinterleave_np(compact, H, block, world, rank, full):
    """rank's compact rows -> their places in the full buffer (row H-1-y), for any per-pixel element shape"""
    j = 0
    while True:
        yb = (j * world + rank) * block
        if yb >= H:
            return
        hb = min(block, H - yb)
        full[H - yb - hb:H - yb] = compact[j * block:j * block + hb]
        j += 1


_CTX = None


def gpu_context():
    global _CTX
    if _CTX is None:
        _CTX = ag.Context(0)
    return _CTX


def gpu_scene(desc):
    return desc.instantiate(ag.Scene(gpu_context()))


def render(g, W, H, spp, depth=5, arith="exact"):
    g.set_shading_arith(arith)
    return ag.PathTracer(depth).render_to_host(g, W, H, spp)


def compare_render_with_oracle(desc, W, H, spp):
    """a depth-5 render of desc on the GPU and on the oracle (correctly rounded trig): the same bits in every pixel, the same ray count"""
    g = gpu_scene(desc)
    acc, st = ag.PathTracer(5).render_to_host(g, W, H, spp)
    g.close()
    o = oracle_scene(desc)
    ob.set_trig_mode(ob.TRIG_CORRECTLY_ROUNDED)
    try:
        oacc, ost = o.render(W, H, spp, threads=8)
    finally:
        ob.set_trig_mode(ob.TRIG_LIBM)
    same = np.all(acc[..., :3].view(np.uint32) == oacc[..., :3].view(np.uint32), axis=-1)
    close = np.all(np.abs(acc[..., :3] - oacc[..., :3]) <= 1e-4 * np.abs(oacc[..., :3]) + 1e-6, axis=-1)
    print(desc.name, "bit-exact %.5f close %.5f rays %d/%d" % (same.mean(), close.mean(), st.rays, ost.rays))
    assert same.all()
    assert st.rays == ost.rays
    assert acc[..., :3].mean() > 0.01


def scene_c1():
    return ag.scenes.scene_c1()


def scene_bounds(desc):
    lo = np.full(3, np.inf)
    hi = np.full(3, -np.inf)
    for op in desc.ops:
        if op[0] == "mesh":
            lo = np.minimum(lo, op[1].min(0))
            hi = np.maximum(hi, op[1].max(0))
        elif op[0] in ("sphere", "area_light"):
            lo = np.minimum(lo, op[1] - op[2])
            hi = np.maximum(hi, op[1] + op[2])
        elif op[0] == "plane":
            half = np.array([op[2][0] / 2, 0, op[2][1] / 2])
            lo = np.minimum(lo, op[1] - half)
            hi = np.maximum(hi, op[1] + half)
    return lo, hi


def random_rays(desc, n, seed=1, tmax=None):
    """A mix that exercises hits, misses, grazing and axis-parallel directions, rays starting inside the scene box
    and short (shadow-like) rays."""
    rng = np.random.RandomState(seed)
    lo, hi = scene_bounds(desc)
    ext = hi - lo
    c = 0.5 * (lo + hi)
    rays = np.zeros(n, ag.RAY_DTYPE)
    o = c + (rng.uniform(-1, 1, (n, 3)) * ext * 0.9)
    # half of the rays aim at a random vertex neighbourhood (guaranteed near-hits / edge hits)
    verts = np.concatenate([op[1] for op in desc.ops if op[0] == "mesh"])
    tgt = verts[rng.randint(len(verts), size=n)] + rng.normal(0, 0.002, (n, 3)) * np.linalg.norm(ext)
    d = rng.normal(size=(n, 3))
    aim = rng.uniform(size=n) < 0.6
    d[aim] = (tgt - o)[aim]
    # exact vertex aims (hits on shared vertices/edges -> tie handling)
    exact = rng.uniform(size=n) < 0.05
    d[exact] = (verts[rng.randint(len(verts), size=n)] - o)[exact]
    # axis-parallel directions (zero components: the reference's inf/NaN slab path)
    ax = rng.uniform(size=n) < 0.05
    axis = rng.randint(3, size=n)
    sign = rng.choice([-1.0, 1.0], size=n)
    dax = np.zeros((n, 3))
    dax[np.arange(n), axis] = sign
    d[ax] = dax[ax]
    # two-zero-component and one-zero-component mixes
    one0 = rng.uniform(size=n) < 0.03
    d[one0, rng.randint(3)] = 0.0
    d[np.all(d == 0, axis=1)] = [0, 0, 1]
    rays["o"] = o.astype(np.float32)
    rays["d"] = d.astype(np.float32)
    t = np.full(n, np.float32(3.402823466e+38), np.float32)
    short = rng.uniform(size=n) < 0.3
    t[short] = (rng.uniform(0.05, 1.5, n) * np.linalg.norm(ext)).astype(np.float32)[short]
    if tmax is not None:
        t[:] = tmax
    rays["tmax"] = t
    return rays


def signed_zero_grid(n):
    """(verts, indices) of an n x n grid of quads (2 n^2 triangles) in the plane y = 0 whose zeros carry both signs: y is -0 at every
    third vertex and +0 elsewhere, x = 0 is -0.  The two triangles of a quad share their box, hence their centroid, so every leaf of
    the grid's BVH holds two of them whatever max_prims_in_node is."""
    g = np.linspace(-1, 1, n + 1).astype(np.float32)
    X, Z = np.meshgrid(g, g, indexing="ij")
    Y = np.where((np.arange(X.size) % 3).reshape(X.shape) == 0, np.float32(-0.0), np.float32(0.0))
    X = np.where(X == 0, np.float32(-0.0), X)
    verts = np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32)
    tri = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, i * (n + 1) + j + 1, (i + 1) * (n + 1) + j + 1
            tri += [a, b, c, c, b, d]
    idx = np.zeros((len(tri), 3), np.int32)
    idx[:, 0] = tri
    assert np.signbit(verts).any()
    return verts, idx


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def film_point(P, s, t, depth):
    """the world point at distance `depth` from the camera P (temporal_model.camera's dict) through its film position (s, t), in float64"""
    d = (P["llc"].astype(np.float64) + s * P["horizontal"].astype(np.float64) + t * P["vertical"].astype(np.float64)) - P["origin"].astype(np.float64)
    return P["origin"].astype(np.float64) + depth * d / np.linalg.norm(d)


def close_fraction(a, b, rel):
    """the share of pixels with every channel within rel |b| + 1e-6"""
    return float(np.all(np.abs(a - b) <= rel * np.abs(b) + 1e-6, axis=-1).mean())


def compare_with_model(out, model, what):
    """the denoiser against tests/denoise_model.py, within the bound that model states"""
    differ = (out != model).any(-1)
    n = int(differ.sum())
    err = np.abs(out.astype(np.float64) - model.astype(np.float64))
    bound = 2.0 ** -18 * np.abs(model.astype(np.float64)) + 1e-7
    print("%s: %d of %d pixels differ from the model, max abs difference %.3g" % (what, n, differ.size, err.max()))
    assert n <= 4, (what, n, np.argwhere(differ)[:8])
    assert (err <= bound).all(), (what, err.max(), np.argwhere(err > bound)[:8])


def denoise_edge(out, model, what):
    """the denoiser against tests/denoise_model.py on a synthetic film (tests/denoise_cases.py): no pixel may differ.  The figures
    compare_with_model would judge by are printed first."""
    differ = (out != model).any(-1)
    err = np.abs(out.astype(np.float64) - model.astype(np.float64))
    bound = 2.0 ** -18 * np.abs(model.astype(np.float64)) + 1e-7
    print("%s: %d of %d pixels differ from the model, max abs difference %.3g, %d channels beyond rel 2^-18"
          % (what, int(differ.sum()), differ.size, err.max(), int((err > bound).sum())))
    assert out.tobytes() == model.tobytes(), (what, np.argwhere(differ)[:8])


def tile_rows(acc, H, tile):
    """the rgb rows [h, w, 3] of tile (x0, y0, w, h) in an accumulator of height H (row 0 = top)"""
    x0, y0, w, h = tile
    return acc[H - y0 - h:H - y0, x0:x0 + w, :3]


def build_cpp_example(tmp_path, name, wall=True):
    """examples/NAME.cpp -- or, for a path, that C++ file -- compiled against include/ and linked to the built library; the executable"""
    src = name if os.path.isabs(str(name)) else os.path.join(ROOT, "examples", name + ".cpp")
    exe = str(tmp_path / os.path.splitext(os.path.basename(str(src)))[0])
    lib = ag.library_path()
    subprocess.check_call(["g++", "-std=c++17"] + ["-Wall"] * wall +
                          ["-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)])
    return exe


FAKE_RCCL_SOURCE = os.path.join(ROOT, "tests", "fake_rccl", "fake_rccl.cpp")


def build_fake_rccl(tmp_path):
    """tests/fake_rccl/fake_rccl.cpp -- the stand-in transport of test_gpu_fake_rccl_gather.py -- as a shared object in tmp_path whose SONAME is
    librccl.so.1, against the headers and the HIP runtime of the ROCm that hipcc belongs to; the file.  It is loaded by this path only."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))))
    out = str(tmp_path / "libfake_rccl.so")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-O1", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), FAKE_RCCL_SOURCE, "-o", out, "-Wl,-soname,librccl.so.1",
                           "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    return out


def struct_layout(tmp_path, structs):
    """{C struct name: ctypes class}: sizeof and every offsetof, printed by a C probe compiled against include/agpt.h, are the class's"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "agpt.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in cls._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {}
    for ln in subprocess.check_output([exe]).decode().split("\n"):
        if ln:
            s, f, v = ln.split()
            got[(s, f)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "sizeof")] == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert got[(cname, f)] == getattr(cls, f).offset, (cname, f)


def assert_exported(names):
    """every name is declared in include/agpt.h, listed in ag.EXPORTS and exported by the built library"""
    header = open(os.path.join(ROOT, "include", "agpt.h")).read()
    L = ag.lib()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in ag.EXPORTS, name
        assert hasattr(L, name), name
