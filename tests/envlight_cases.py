"""The cases of the environment-light pins (tests/golden/make_envlight_golden.py writes their answers from the reference's own
InfiniteAreaLight, tests/test_envlight_pins.py and tests/test_gpu_envlight_pins.py hold the oracle and the kernels to them).

Ten maps, rebuilt from seeds and rounded to what an RGBE pixel holds (the reference reads its map from an .hdr file); per map the draws
handed to Sample_Li and the directions handed to Le and Pdf_Li; two Li scenes.  Nothing here needs the reference or a GPU.

The draws depend on the map's cdf, and the cdf on sin(theta) of every row as the C library of the generating machine rounded it.  The
fixture therefore stores those row weights, and the cases are built from the STORED weights: func = max(r, g, b) * weight[row], cdf =
Distribution1D(func) -- fp32 sums and divisions, the same on every machine (the oracle's, pinned to the reference's header by
tests/test_dist1d.py).  The product's own binding of that constructor needs a device context, which the generator does not have.
"""
import hashlib

import numpy as np

import ag_pathtracer_amd as ag
from oracle import binding as ob
from oracle.ref_binding import rgbe_exact

F = np.float32
MAPS = ("1x1", "1x7", "7x1", "5x3", "16x8", "33x17", "33x17_sun", "33x17_black", "8x4_black", "500x250")
SMALL = 561                 # up to this many texels every cdf entry is a draw
N_RANDOM_DIRS = 2048
N_UNIFORM_DRAWS = 4096      # 500x250
N_ROUND_TRIP = 512          # 500x250: cdf[i] draws with fl(fl(i / n) * n) < i, and as many without
BOUNDARY_CAP = 64
FIXED_DRAWS = F([0.0, 1e-45, 0.5, 1.0 - 2.0 ** -24, 1.0])     # 1e-45 rounds to the smallest subnormal
SUN_TEXEL = (4, 20)         # (row, column) of the 33x17 sun
BLACK_ROWS, BLACK_COLS = (3, 11), (7, 32)


def map_size(name):
    w, h = name.split("_")[0].split("x")
    return int(w), int(h)


def map_image(name):
    """rgb[H, W, 3] float32, exactly representable in RGBE"""
    w, h = map_size(name)
    if name.endswith("_black") and (w, h) == (8, 4):
        return np.zeros((h, w, 3), F)
    if name == "33x17_sun":
        rng = np.random.RandomState(1733)
        img = rng.uniform(0.04, 0.06, (h, w, 3))
        img[SUN_TEXEL] = [5.0e4, 4.6e4, 4.1e4]
        return rgbe_exact(img)
    img = ag.scenes.synthetic_hdr(w, h, seed=1000 + 7 * w + h) if (w, h) != (16, 8) else ag.scenes.synthetic_hdr(16, 8)
    if name == "33x17_black":
        img[list(BLACK_ROWS)] = 0
        img[:, list(BLACK_COLS)] = 0
    return rgbe_exact(img)


def map_sha256(name):
    return hashlib.sha256(np.ascontiguousarray(map_image(name)).tobytes()).hexdigest()


def oracle_row_weights(h):
    """sin(theta) of the h rows as THIS machine's C library rounds it, read from the table the oracle's InfiniteAreaLight constructor
    builds for a map of ones (1 * sin(theta) is sin(theta))"""
    s = ob.OracleScene()
    return s.env_table(s.add_infinite_area_light(np.ones((h, 1, 3), F)))[0]


def map_table(name, weights):
    """(func[n], cdf[n + 1], funcInt) of the map from the fixture's row weights"""
    img = map_image(name)
    func = (img.max(-1) * np.asarray(weights, F)[:, None]).astype(F).reshape(-1)
    cdf, fi = ob.distribution1d(func, np.zeros(0, F))[:2]
    return func, cdf, fi


def round_trip_misses(n):
    """the i in [0, n) for which fl(fl(i / n) * n) < i: a draw that equals cdf[i] lights from texel i - 1"""
    i = np.arange(n)
    return i[((i.astype(F) / F(n)) * F(n)).astype(F) < i]


def pick(a, k):
    """k entries of a, evenly spaced (all of them if there are fewer)"""
    a = np.asarray(a)
    return a if len(a) <= k else a[np.linspace(0, len(a) - 1, k).astype(np.int64)]


def draws(name, weights):
    """-> (u[k] float32, of_cdf[k] int32: the i for which u[k] is exactly cdf[i], else -1)"""
    w, h = map_size(name)
    n = w * h
    cdf = map_table(name, weights)[1]
    u, of = [FIXED_DRAWS], [np.full(len(FIXED_DRAWS), -1)]
    if n <= SMALL:
        c = cdf[:n]
        mid = ((cdf[:n].astype(np.float64) + cdf[1:]) / 2).astype(F)     # with the three above alone a texel can go unselected:
        u += [c, np.nextafter(c, F(-1)), np.nextafter(c, F(2)), mid]     # each of its neighbours' draws may round away from it
        of += [np.arange(n), np.full(n, -1), np.full(n, -1), np.full(n, -1)]
    else:
        u.append(np.random.RandomState(n).uniform(size=N_UNIFORM_DRAWS).astype(F))
        of.append(np.full(N_UNIFORM_DRAWS, -1))
        miss = round_trip_misses(n)
        rest = np.setdiff1d(np.arange(1, n), miss)
        for sel in (pick(miss, N_ROUND_TRIP), pick(rest, N_ROUND_TRIP)):
            u.append(cdf[sel])
            of.append(sel)
    return np.concatenate(u).astype(F), np.concatenate(of).astype(np.int32)


def _spherical(theta, phi):
    """(sin(theta) cos(phi), cos(theta), sin(theta) sin(phi)) in fp64, rounded: the direction Sample_Li builds for these angles"""
    theta, phi = np.broadcast_arrays(np.asarray(theta, np.float64), np.asarray(phi, np.float64))
    return np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], -1).astype(F)


def _three_steps(x):
    """fp32(x), and one fp32 step to either side"""
    x = np.asarray(x, np.float64).astype(F)
    return np.concatenate([np.nextafter(x, F(-10)), x, np.nextafter(x, F(10))])


def directions(name):
    """d[n, 3] float32, finite and not of zero length: random directions of random length, the axes with every sign of zero, both sides
    of (up to 64 of) the column and the row boundaries, phi just below 2 pi, theta a few steps from 0 and from pi"""
    w, h = map_size(name)
    rng = np.random.RandomState(4000 + 31 * w + h)
    d = rng.standard_normal((N_RANDOM_DIRS, 3))
    d *= (10.0 ** rng.uniform(-3, 3, (N_RANDOM_DIRS, 1))) / np.linalg.norm(d, axis=1, keepdims=True)
    out = [d.astype(F)]
    axes = []
    for a in range(3):
        for s in (1.0, -1.0):
            for z0 in (0.0, -0.0):
                for z1 in (0.0, -0.0):
                    v = [z0, z1]
                    v.insert(a, s)
                    axes.append(v)
    out.append(np.array(axes, F))
    cols = pick(np.arange(w + 1), BOUNDARY_CAP)
    rows = pick(np.arange(h + 1), BOUNDARY_CAP)
    out.append(_spherical(1.1, _three_steps(2 * np.pi * cols / w)))
    out.append(_spherical(_three_steps(np.pi * rows / h), 2.0))
    x = np.array([1.0, 0.5, 1e-3, 37.0])
    for c in (0.0, 0.3, -2.0):       # phi = atan2(D.z, D.x) just below 2 pi
        out.append(np.stack([x, c * x, -1e-7 * x], -1).astype(F))
    tiny = np.sqrt(2.0 * np.arange(1, 5)) * 2.0 ** -12      # acos(1 - k 2^-24), k = 1 .. 4
    for phi in (0.3, 2.5, 5.9):
        out.append(_spherical(tiny, phi))
        out.append(_spherical(np.pi - tiny, phi))
    d = np.concatenate(out)
    assert np.isfinite(d).all() and (np.abs(d).max(-1) > 0).all()
    return d


def same(got, want):
    """bit-identical float arrays, NaN matching NaN by class"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def assert_same(got, want, what):
    ok = same(got, want)
    assert ok.all(), "%s: %d of %d values differ, first at %s" % (what, (~ok).sum(), ok.size, np.argwhere(~ok)[0])


def texel_of(wi, w, h):
    """the texel (row, column) whose centre direction wi is, for directions Sample_Li returned"""
    wi = np.asarray(wi, np.float64)
    theta = np.arctan2(np.hypot(wi[:, 0], wi[:, 2]), wi[:, 1])
    phi = np.arctan2(wi[:, 2], wi[:, 0]) % (2 * np.pi)
    row = np.rint(theta / np.pi * h - .5).astype(np.int64)
    col = np.rint(phi / (2 * np.pi) * w - .5).astype(np.int64) % w
    return row, col


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
LI_SCENES = ("sun", "two_maps")
N_LI = 256
LI_DEPTH = 5
TWO_MAPS = ("5x3", None, "33x17_black")      # the light list of the two-map scene: its first and third entries are maps


def map_scene(name):
    """one small sphere under the map, the scene of the function-level calls"""
    d = ag.SceneDesc("envpin-" + name)
    d.add_sphere([0, 0, 0], 1.0, d.add_material(ag.MAT_DIFFUSE_ONLY, [.5, .5, .5]))
    d.add_infinite_area_light(map_image(name))
    d.set_camera([0, 1.5, -6], [0, 0, 0], [0, 1, 0], 1.0, 40.0, 0.0)
    return d


def li_scene(name):
    d = ag.SceneDesc("envpin-li-" + name)
    if name == "sun":        # a rough Disney floor and a mirror sphere under the 33x17 sun map
        d.add_sphere([0, -101, 0], 100.0, d.add_material(ag.MAT_DISNEY, [.6, .55, .5], 0.9, 0.0))
        d.add_sphere([0, 0, 0], 1.0, d.add_material(ag.MAT_MIRROR, [.9, .9, .9]))
        d.add_infinite_area_light(map_image("33x17_sun"))
    else:                    # a diffuse floor lit by the 5x3 map, an area light and the 33x17 black-rows map, in this order
        d.add_sphere([0, -101, 0], 100.0, d.add_material(ag.MAT_DIFFUSE_ONLY, [.7, .7, .7]))
        d.add_sphere([0, 0, 0], 1.0, d.add_material(ag.MAT_DISNEY, [.8, .3, .2], .5, 0.))
        d.add_infinite_area_light(map_image(TWO_MAPS[0]))
        d.add_area_light([2, 4, -2], 0.5, [30, 28, 25])
        d.add_infinite_area_light(map_image(TWO_MAPS[2]))
    d.set_camera([0, 1.5, -6], [0, 0, 0], [0, 1, 0], 1.0, 40.0, 0.0)
    return d


def li_film_inputs(k):
    rng = np.random.RandomState(900 + k)
    return rng.uniform(size=(N_LI, 2)).astype(F), rng.randint(1, 2 ** 31 - 1, N_LI).astype(np.uint32)
