"""The cases of test_gpu_textured_paths.py -- whole paths through images that vary inside triangles, against the textured oracle -- shared
with the CPU tests of test_oracle_textures.py, which prove on the oracle alone that every case exercises what it claims (the census) and
that its images matter (the sensitivities).  The scenes are the existing constructions of the texture test files, imported, not copied."""
import collections
import copy
import functools

import numpy as np

import ag_pathtracer_amd as ag
import test_gpu_normal_map as t_normal
import test_gpu_texture_filter as t_filter
import test_gpu_textures as t_textures
from helpers import oracle_render
from oracle import binding as ob
from texture_cases import varying_lights_and_camera, varying_mesh

F = np.float32
W = H = 64
SPP = 3
DEPTH = 5
BILINEAR, NEAREST = ag.FILTER_BILINEAR, ag.FILTER_NEAREST
REPEAT, CLAMP, MIRROR = ag.WRAP_REPEAT, ag.WRAP_CLAMP, ag.WRAP_MIRROR

# name; texturing level (agpt_shade_kernels.h: the highest one a material needs); build() -> SceneDesc; the census counters
# (oracle.binding.CENSUS_NAMES) the case promises to make non-zero
Case = collections.namedtuple("Case", "name level build promises")

LOOKUPS = {1: ("lookup_colour",), 2: ("lookup_colour", "lookup_roughness", "lookup_metallic")}
DEEP = ("lookup_deep",)


def with_env(desc):
    """desc plus synthetic_hdr(16, 8) as an infinite area light: the ENV instantiation of its level"""
    d = copy.copy(desc)
    d.ops = list(desc.ops)
    d.name = desc.name + "+env"
    d.add_infinite_area_light(ag.scenes.synthetic_hdr(16, 8))
    return d


# ---- level 2: parameter texels at the edges of the Disney constructor, varying inside triangles -----------------------------------
# (roughness, metallic) texels: metallic exactly 0 and 1 (1 drops the diffuse and the retro lobe), roughness 0 and .02 (below the .001
# clamp of alpha = r * r), 1, and 1.5 -- above 1, which nothing clamps (alpha = 2.25)
PARAM_EDGE_VALUES = np.array([[0.0, 0.0], [0.0, 1.0], [.02, 0.0], [.02, 1.0], [1.0, 0.0], [1.0, 1.0], [1.5, 0.0], [1.5, 1.0],
                              [.35, .5], [.6, 0.0], [.25, 1.0], [.8, .3]], F)


def param_edge_image(size=8):
    """size x size texels (0, roughness, metallic) drawn from PARAM_EDGE_VALUES, every value present"""
    rng = np.random.RandomState(41)
    pick = np.concatenate([np.arange(len(PARAM_EDGE_VALUES)), rng.randint(len(PARAM_EDGE_VALUES), size=size * size - len(PARAM_EDGE_VALUES))])
    rng.shuffle(pick)
    img = np.zeros((size, size, 3), F)
    img[..., 1:] = PARAM_EDGE_VALUES[pick].reshape(size, size, 2)
    return img


def param_edge_scene():
    """the varying mesh -- its uvs leave [0, 1] and cross many texels per triangle -- with a colour image and param_edge_image() in the
    glTF layout on its one Disney material, both through the default sampler (level 2)"""
    d = ag.SceneDesc("param-edges")
    m = d.add_material(ag.MAT_DISNEY, [.5, .5, .5], .7, .2)
    d.add_mesh(*varying_mesh(), m, 1)
    d.set_material_texture(m, d.add_texture(np.random.RandomState(42).uniform(0.05, 0.95, (16, 16, 3)).astype(F)))
    p = d.add_texture(param_edge_image())
    d.set_material_param_texture(m, ag.PARAM_ROUGHNESS, p, 1)
    d.set_material_param_texture(m, ag.PARAM_METALLIC, p, 2)
    return varying_lights_and_camera(d)


# ---- level 4 on the varying mesh ------------------------------------------------------------------------------------------------
NORMAL_SAMPLERS = [("16x16", BILINEAR, MIRROR, CLAMP), ("5x3", NEAREST, REPEAT, REPEAT), ("5x3", BILINEAR, CLAMP, REPEAT),
                   ("16x16", NEAREST, CLAMP, MIRROR)]


def normal_case(kind, scale, with_normals, which):
    image, filter, wu, wv = NORMAL_SAMPLERS[which % len(NORMAL_SAMPLERS)]
    return t_normal.varying_scene(kind, (t_normal.IMAGES[image], filter, wu, wv, scale), with_normals)


def shared_taps_scene():
    """a Disney material whose normal map IS its colour image, BILINEAR: one set of taps serves both slots"""
    d = t_normal.varying_scene("disney", (t_normal.IMAGES["16x16"], BILINEAR, REPEAT, MIRROR, 1.0), True)
    d.ops = list(d.ops)
    d.set_material_texture(0, 0)
    d.name = "varying-normal-shared"
    return d


def flat_patches_image():
    """a tilt image with every third texel exactly (.5, .5, 1): hits there fall under the no-op rule, their neighbours do not"""
    img = t_normal.tilt_image(8, 8, 23).copy()
    img.reshape(-1, 3)[::3] = [.5, .5, 1]
    return img


def flat_patches_scene():
    return t_normal.varying_scene("disney", (flat_patches_image(), NEAREST, REPEAT, REPEAT, 2.0), True)


def _cases():
    out = [
        Case("varying-colour", 1, lambda: t_textures.varying_scene()[0], LOOKUPS[1] + DEEP),
        Case("c1-textured", 1, ag.scenes.scene_textured, LOOKUPS[1] + DEEP),
        Case("c1-mapped", 2, ag.scenes.scene_mapped, LOOKUPS[2] + DEEP + ("rebuild_fewer_lobes",)),
        Case("param-edges", 2, param_edge_scene, LOOKUPS[2] + DEEP + ("rebuild_fewer_lobes",)),
    ]
    for name, wrap in t_filter.WRAPS.items():
        out.append(Case("c1-mapped-bilinear-" + name, 3, functools.partial(t_filter.scene_mapped_bilinear, wrap),
                        LOOKUPS[2] + DEEP + ("bilinear_fractional",)))
    out.append(Case("varying-filtered", 3, lambda: t_filter.varying_scene(t_filter.IMAGES["5x3"], BILINEAR, CLAMP, MIRROR),
                    LOOKUPS[1] + DEEP + ("bilinear_fractional",)))
    out.append(Case("c1-mapped-bilinear-normal", 4, t_normal.scene_mapped_bilinear_normal,
                    LOOKUPS[2] + DEEP + ("lookup_normal", "normal_applied", "bilinear_fractional")))
    which = 0
    for kind in t_normal.KINDS:
        for scale in (1.0, 3.0):
            for with_normals in (True, False):
                out.append(Case("varying-normal-%s-x%g-%s" % (kind, scale, "vn" if with_normals else "flat"), 4,
                                functools.partial(normal_case, kind, scale, with_normals, which), ("lookup_normal", "normal_applied") + DEEP))
                which += 1
    out.append(Case("varying-normal-shared", 4, shared_taps_scene, LOOKUPS[1] + DEEP + ("lookup_normal", "normal_applied", "bilinear_fractional")))
    out.append(Case("varying-normal-flat-patches", 4, flat_patches_scene, ("lookup_normal", "normal_applied", "normal_noop") + DEEP))
    return out


BASE_CASES = _cases()
# one case per level (two at level 4) again under the environment map
ENV_OF = ["varying-colour", "param-edges", "varying-filtered", "varying-normal-shared", "c1-mapped-bilinear-normal"]


def _env_case(c):
    return Case(c.name + "+env", c.level, lambda: with_env(c.build()), c.promises)


CASES = BASE_CASES + [_env_case(c) for c in BASE_CASES if c.name in ENV_OF]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
TABLES = ("lds", "global")       # "global": AGPT_SHADE_GLOBAL_TABLES=1


def has_env(case):
    return case.name.endswith("+env")


def variant(case, tables):
    """(level, fast, lds, env) as Scene.shade_variant() reports the exact instantiation the case runs"""
    return (case.level, 0, int(tables == "lds"), int(has_env(case)))


# one case per level for the fast arithmetic, and the level-4 cases of the other entry points
FAST_CASES = ["varying-colour", "param-edges", "varying-filtered", "varying-normal-shared"]
LI_CASE = "varying-normal-shared"
ADAPTIVE_CASE = "varying-normal-disney-x3-vn"


@functools.lru_cache(None)
def desc_of(name):
    return BY_NAME[name].build()


@functools.lru_cache(None)
def oracle_reference(name, spp=SPP, w=W, h=H):
    """(read-only accumulator, stats as a dict, census) of the textured oracle's render of the case, once per process"""
    acc, st = oracle_render(desc_of(name), w, h, spp, DEPTH)
    acc.setflags(write=False)
    return acc, st.as_dict(), ob.census()


# ---- the same case with one thing changed: what the sensitivity tests render ----------------------------------------------------
def _mapped_ops(desc, f):
    d = copy.copy(desc)
    d.ops = [f(op) for op in desc.ops]
    return d


def rolled(desc):
    """every image rolled by one texel along both axes"""
    return _mapped_ops(desc, lambda op: ("texture", np.roll(op[1], (1, 1), (0, 1))) if op[0] == "texture" else op)


def nearest(desc):
    """every BILINEAR sampler turned to NEAREST, the wraps kept"""
    return _mapped_ops(desc, lambda op: (op[0], op[1], NEAREST, op[3], op[4]) if op[0] == "texture_sampler" else op)


def negated(desc):
    """every normal map's scale negated"""
    return _mapped_ops(desc, lambda op: (op[0], op[1], op[2], -op[3]) if op[0] == "material_normal_texture" else op)


def has_bilinear(desc):
    return any(op[0] == "texture_sampler" and op[2] == BILINEAR for op in desc.ops)


def has_normal_map(desc):
    return any(op[0] == "material_normal_texture" and op[2] >= 0 for op in desc.ops)
