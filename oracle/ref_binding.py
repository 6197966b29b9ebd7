"""ctypes binding of oracle/_ref/libref_hotpath.so: the reference's own hot path, compiled in place (oracle/ref_hotpath.cpp).

TEST INFRASTRUCTURE ONLY.  The library exists only where the reference does (the build container); tests/golden/make_refpin_golden.py
and the regeneration test of tests/test_refpin.py are its only users.  RefScene takes the calls SceneDesc.instantiate replays, like
oracle.binding.OracleScene.
"""
import ctypes as C
import os
import tempfile

import numpy as np

from .binding import HIT_DTYPE, NODE_DTYPE, RAY_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(_HERE, "_ref", "libref_hotpath.so")
_LIB = None

TRIG_LIBM, TRIG_CORRECTLY_ROUNDED = 0, 1
fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int32)
up = C.POINTER(C.c_uint32)


def available():
    return os.path.exists(PATH)


ENV_LIGHT = ("ref_env_le", "ref_env_pdf_li", "ref_env_sample_li")


def has_env_light():
    """The library is there and exports InfiniteAreaLight's three functions: one built from an earlier ref_hotpath.cpp does not (build
    products are not tracked; __graft_entry__.build() rebuilds such a file where the reference is).  Read from the file, not from a
    loaded handle: a library that was replaced on disk stays what it was in a process that has loaded it."""
    if not available():
        return False
    with open(PATH, "rb") as f:
        data = f.read()
    return all(name.encode() + b"\0" in data for name in ENV_LIGHT)


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(PATH)
        L.ref_scene_new.restype = C.c_void_p
        L.ref_scene_free.argtypes = [C.c_void_p]
        L.ref_set_trig_mode.argtypes = [C.c_int]
        L.ref_set_draws.argtypes = [fp, C.c_int]
        L.ref_draws_used.restype = C.c_longlong
        L.ref_rng_floats.argtypes = [C.c_uint32, C.c_int, fp]
        L.ref_trig_probe.argtypes = [C.c_float, fp]
        L.ref_add_material.argtypes = [C.c_void_p, C.c_int, fp, C.c_float, C.c_float]
        L.ref_add_mesh.argtypes = [C.c_void_p, fp, C.c_int, fp, C.c_int, fp, C.c_int, ip, C.c_int, C.c_int, C.c_int]
        L.ref_add_sphere.argtypes = [C.c_void_p, fp, C.c_float, C.c_int]
        L.ref_add_plane.argtypes = [C.c_void_p, fp, fp, C.c_int]
        L.ref_add_area_light.argtypes = [C.c_void_p, fp, C.c_float, fp]
        L.ref_add_uniform_infinite_light.argtypes = [C.c_void_p, fp]
        L.ref_add_infinite_area_light.argtypes = [C.c_void_p, C.c_char_p]
        L.ref_load_hdr.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), fp, C.c_int]
        L.ref_set_camera.argtypes = [C.c_void_p, fp, fp, fp, C.c_float, C.c_float, C.c_float]
        L.ref_bsdf_eval.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, fp, fp, fp]
        L.ref_bsdf_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, fp, fp, fp, fp, ip]
        L.ref_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, fp, ip, C.c_int]
        L.ref_dbg_li.argtypes = [C.c_void_p, C.c_void_p, C.c_int, fp]
        L.ref_bvh.argtypes = [fp, C.c_int, ip, C.c_int, C.c_int, C.c_void_p, C.c_int, ip]
        L.ref_backdrop.argtypes = [fp, fp, C.c_float, C.c_int, fp, fp, fp, ip, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ref_camera.argtypes = [fp, fp, fp, C.c_float, C.c_float, C.c_float, fp]
        L.ref_camera_rays.argtypes = [C.c_void_p, fp, C.c_int, up, C.c_void_p]
        L.ref_li.argtypes = [C.c_void_p, C.c_void_p, up, C.c_int, C.c_int, fp, up, ip, C.POINTER(C.c_longlong)]
        if all(hasattr(L, name) for name in ENV_LIGHT):     # (absent from a library built before they were added: has_env_light)
            L.ref_env_le.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, fp]
            L.ref_env_pdf_li.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, fp]
            L.ref_env_sample_li.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, fp, fp, fp, ip]
        _LIB = L
    return _LIB


def _f(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(fp)


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ip)


def set_trig_mode(mode):
    lib().ref_set_trig_mode(int(mode))


def rng_floats(seed, n):
    out = np.zeros(n, np.float32)
    lib().ref_rng_floats(C.c_uint32(seed), n, out.ctypes.data_as(fp))
    return out


def trig_probe(u2):
    """TrowbridgeReitzSample11 at normal incidence with U1 = .5 -> (cos(phi), sin(phi)) for phi = 6.28318530718f * u2."""
    out = np.zeros(2, np.float32)
    lib().ref_trig_probe(C.c_float(u2), out.ctypes.data_as(fp))
    return out


def create_backdrop(origin, size, radius, steps):
    nv = 2 * (steps + 5)
    verts = np.zeros((nv, 3), np.float32)
    normals = np.zeros((nv, 3), np.float32)
    uvs = np.zeros((nv, 2), np.float32)
    idx = np.zeros((6 * (steps + 4), 3), np.int32)
    _, po = _f(origin)
    _, ps = _f(size)
    n_v, n_i = C.c_int(0), C.c_int(0)
    lib().ref_backdrop(po, ps, float(radius), int(steps), verts.ctypes.data_as(fp), normals.ctypes.data_as(fp), uvs.ctypes.data_as(fp),
                       idx.ctypes.data_as(ip), C.byref(n_v), C.byref(n_i))
    assert n_v.value == nv and n_i.value == idx.shape[0]
    return verts, normals, uvs, idx


def bvh(verts, indices, max_prims_in_node=1):
    v, pv = _f(np.asarray(verts).reshape(-1, 3))
    ix, pi = _i(np.asarray(indices).reshape(-1, 3))
    n_tris = ix.shape[0] // 3
    nodes = np.zeros(2 * n_tris + 2, NODE_DTYPE)
    order = np.zeros(n_tris, np.int32)
    total = lib().ref_bvh(pv, v.shape[0], pi, ix.shape[0], int(max_prims_in_node), nodes.ctypes.data_as(C.c_void_p), len(nodes),
                          order.ctypes.data_as(ip))
    assert total > 0
    return nodes[:total + 1].copy(), order


def camera_vectors(lookfrom, lookat, vup, aspect_ratio, vfov, aperture):
    out = np.zeros(22, np.float32)
    _, a = _f(lookfrom)
    _, b = _f(lookat)
    _, c = _f(vup)
    lib().ref_camera(a, b, c, float(aspect_ratio), float(vfov), float(aperture), out.ctypes.data_as(fp))
    return out


def load_hdr(path, cap=1 << 20):
    w, h = C.c_int(0), C.c_int(0)
    out = np.zeros(cap * 3, np.float32)
    assert lib().ref_load_hdr(os.fsencode(path), C.byref(w), C.byref(h), out.ctypes.data_as(fp), cap)
    return out[:w.value * h.value * 3].reshape(h.value, w.value, 3).copy()


def to_rgbe(rgb):
    """rgb[H, W, 3] float -> rgbe[H, W, 4] uint8 (shared exponent of the largest channel, mantissas truncated)."""
    rgb = np.asarray(rgb, np.float64)
    m = rgb.max(-1)
    mant, e = np.frexp(m)
    scale = np.where(m > 1e-32, mant * 256.0 / np.where(m > 1e-32, m, 1.0), 0.0)
    out = np.zeros(rgb.shape[:-1] + (4,), np.uint8)
    out[..., :3] = np.floor(rgb * scale[..., None]).astype(np.uint8)
    out[..., 3] = np.where(m > 1e-32, e + 128, 0).astype(np.uint8)
    return out


def rgbe_exact(rgb):
    """rgb rounded down to what a Radiance RGBE pixel holds: byte * 2^(e - 136), the value an .hdr reader returns."""
    q = to_rgbe(rgb)
    f = np.ldexp(1.0, q[..., 3].astype(np.int64) - 136)
    return np.where(q[..., 3:] == 0, 0.0, q[..., :3] * f[..., None]).astype(np.float32)


def flat_hdr_bytes(rgbe):
    """A Radiance .hdr file with flat (not run-length encoded) scanlines from rgbe[H, W, 4] uint8."""
    h, w = rgbe.shape[:2]
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w) + np.ascontiguousarray(rgbe, np.uint8).tobytes()


class RefScene:
    def __init__(self):
        self.L = lib()
        self.h = C.c_void_p(self.L.ref_scene_new())

    def __del__(self):
        try:
            if self.h:
                self.L.ref_scene_free(self.h)
                self.h = None
        except Exception:
            pass

    def add_material(self, mtype, color, roughness=0.5, metallic=0.0):
        _, p = _f(color)
        return self.L.ref_add_material(self.h, int(mtype), p, float(roughness), float(metallic))

    def add_mesh(self, verts, normals, uvs, indices, material, max_prims_in_node=1):
        v, pv = _f(np.asarray(verts).reshape(-1, 3))
        n, pn = _f(np.zeros((0, 3), np.float32) if normals is None else np.asarray(normals).reshape(-1, 3))
        t, pt = _f(np.zeros((0, 2), np.float32) if uvs is None else np.asarray(uvs).reshape(-1, 2))
        ix, pi = _i(np.asarray(indices).reshape(-1, 3))
        return self.L.ref_add_mesh(self.h, pv, v.shape[0], pn, n.shape[0], pt, t.shape[0], pi, ix.shape[0], int(material),
                                   int(max_prims_in_node))

    def add_sphere(self, center, radius, material):
        _, p = _f(center)
        return self.L.ref_add_sphere(self.h, p, float(radius), int(material))

    def add_plane(self, o, size, material):
        _, pa = _f(o)
        _, pb = _f(size)
        return self.L.ref_add_plane(self.h, pa, pb, int(material))

    def add_area_light(self, center, radius, L):
        _, p = _f(center)
        _, pl = _f(L)
        return self.L.ref_add_area_light(self.h, p, float(radius), pl)

    def add_uniform_infinite_light(self, L):
        _, pl = _f(L)
        return self.L.ref_add_uniform_infinite_light(self.h, pl)

    def add_infinite_area_light(self, rgb):
        """The reference loads its environment map from a file: `rgb` must be exactly representable in RGBE (what rgbe_exact
        returns), so that the file written here decodes to the same floats."""
        rgb = np.ascontiguousarray(rgb, np.float32)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "env.hdr")
            with open(path, "wb") as f:
                f.write(flat_hdr_bytes(to_rgbe(rgb)))
            back = load_hdr(path)
            assert back.tobytes() == rgb.tobytes(), "environment map is not RGBE-exact"
            return self.L.ref_add_infinite_area_light(self.h, os.fsencode(path))

    def set_camera(self, lookfrom, lookat, vup, aspect_ratio, vfov=45.0, aperture=0.0):
        _, a = _f(lookfrom)
        _, b = _f(lookat)
        _, c = _f(vup)
        self.L.ref_set_camera(self.h, a, b, c, float(aspect_ratio), float(vfov), float(aperture))

    def bsdf_eval(self, material, wo, wi):
        wo, pwo = _f(np.asarray(wo).reshape(-1, 3))
        wi, pwi = _f(np.asarray(wi).reshape(-1, 3))
        n = wo.shape[0]
        f = np.zeros((n, 3), np.float32)
        pdf = np.zeros(n, np.float32)
        self.L.ref_bsdf_eval(self.h, int(material), n, pwo, pwi, f.ctypes.data_as(fp), pdf.ctypes.data_as(fp))
        return f, pdf

    def bsdf_sample(self, material, wo, u):
        wo, pwo = _f(np.asarray(wo).reshape(-1, 3))
        u, pu = _f(np.asarray(u).reshape(-1, 2))
        n = wo.shape[0]
        wi = np.zeros((n, 3), np.float32)
        f = np.zeros((n, 3), np.float32)
        pdf = np.zeros(n, np.float32)
        spec = np.zeros(n, np.int32)
        self.L.ref_bsdf_sample(self.h, int(material), n, pwo, pu, wi.ctypes.data_as(fp), f.ctypes.data_as(fp), pdf.ctypes.data_as(fp),
                               spec.ctypes.data_as(ip))
        return wi, f, pdf, spec

    def intersect(self, rays, any_hit=False):
        """-> (hits, uv[n, 2], ambiguous[n]); see ref_intersect in ref_hotpath.cpp."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        n = rays.shape[0]
        out = np.zeros(n, HIT_DTYPE)
        uv = np.zeros((n, 2), np.float32)
        amb = np.zeros(n, np.int32)
        self.L.ref_intersect(self.h, rays.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(fp),
                             amb.ctypes.data_as(ip), int(bool(any_hit)))
        return out, uv, amb

    def dbg_li(self, rays):
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        out = np.zeros((rays.shape[0], 3), np.float32)
        self.L.ref_dbg_li(self.h, rays.ctypes.data_as(C.c_void_p), rays.shape[0], out.ctypes.data_as(fp))
        return out

    def camera_rays(self, st, states):
        """Camera::GetRay(s, t) per row of st[n, 2], each on its own xorshift32 state -> (rays, states after)."""
        st, pst = _f(np.asarray(st).reshape(-1, 2))
        states = np.array(states, np.uint32)
        rays = np.zeros(st.shape[0], RAY_DTYPE)
        self.L.ref_camera_rays(self.h, pst, st.shape[0], states.ctypes.data_as(up), rays.ctypes.data_as(C.c_void_p))
        return rays, states

    def env_le(self, light, d):
        """InfiniteAreaLight::Le of light `light` of the scene's list for directions d[n, 3], taken as given -> rgb[n, 3]."""
        d, pd = _f(np.asarray(d).reshape(-1, 3))
        out = np.zeros_like(d)
        if self.L.ref_env_le(self.h, int(light), d.shape[0], pd, out.ctypes.data_as(fp)) != 1:
            raise ValueError("light %d is no InfiniteAreaLight" % light)
        return out

    def env_pdf_li(self, light, wi):
        """InfiniteAreaLight::Pdf_Li for wi[n, 3] -> pdf[n]."""
        wi, pw = _f(np.asarray(wi).reshape(-1, 3))
        out = np.zeros(wi.shape[0], np.float32)
        if self.L.ref_env_pdf_li(self.h, int(light), wi.shape[0], pw, out.ctypes.data_as(fp)) != 1:
            raise ValueError("light %d is no InfiniteAreaLight" % light)
        return out

    def env_sample_li(self, light, u):
        """InfiniteAreaLight::Sample_Li, one call per draw u[i] (what its RandomFloat() returns) -> (wi[n, 3], pdf[n], Le[n, 3], ok[n]);
        ok = 0 where the call returned before it wrote wi and pdf (both 0 there)."""
        u, pu = _f(np.asarray(u).reshape(-1))
        n = u.shape[0]
        wi, pdf, le, ok = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        rc = self.L.ref_env_sample_li(self.h, int(light), n, pu, wi.ctypes.data_as(fp), pdf.ctypes.data_as(fp), le.ctypes.data_as(fp),
                                      ok.ctypes.data_as(ip))
        if rc != 1:
            raise ValueError("light %d is no InfiniteAreaLight" % light if rc == 0 else "Sample_Li did not take exactly one draw")
        return wi, pdf, le, ok

    def li(self, rays, states, max_depth):
        """PathTracer(max_depth).Li per ray -> (radiance[n, 3], states after, draws[n], (Scene::Intersect calls, IntersectP calls))."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        states = np.ascontiguousarray(states, np.uint32)
        n = rays.shape[0]
        L = np.zeros((n, 3), np.float32)
        after = np.zeros(n, np.uint32)
        draws = np.zeros(n, np.int32)
        calls = (C.c_longlong * 2)()
        self.L.ref_li(self.h, rays.ctypes.data_as(C.c_void_p), states.ctypes.data_as(up), n, int(max_depth), L.ctypes.data_as(fp),
                      after.ctypes.data_as(up), draws.ctypes.data_as(ip), calls)
        return L, after, draws, (int(calls[0]), int(calls[1]))
