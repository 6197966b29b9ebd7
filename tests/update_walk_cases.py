"""Seeded walks over the per-frame update calls of a committed scene, and the model of what include/agpt.h says the scene is after
each of them (test_update_walk_cases.py on the CPU, test_gpu_update_walks.py on the GPU).  Nothing here needs a GPU or a context.

An ACTION is a dict: {"kind": ..., "prim": ..., "mode": "refit" | "rebuild", "k": a number its inputs are derived from, ...}.
  front ends       FRONT_ENDS on a mesh, in REFIT or REBUILD; update_host with "nan": the non-finite fallback
  setters          set_skin (route "lds": 3 joints, or "global": 800 joints, a palette beyond the LDS cap), set_targets, set_mode, set_builder
  analytic         update_sphere, update_plane, set_radiance, update_spheres (a device batch: "via" tensor / pointer / host)
  snapshots        snapshot_positions, snapshot_surfaces
  mirror readers   bvh, dbg_li -- and, among the front ends, every REBUILD, every fallback and the first transform / pose / morph of a
                   mesh after explicit arrays (DESIGN.md section 5.7's reader table)
  refusals         refuse: "what" of REFUSALS through the host ("via": "host") or the device-pointer call ("device")

Model holds the ARRAYS (what every reader of the device must see); its new arrays come from skin_model, morph_model, normals_model and
agpt_transform_arrays (the host twin that test_transform_arrays.py pins to the OBJ loader).  Flags holds the library's PREDICTED
bookkeeping (stale flags, rest pose, cache) -- it decides nothing about expected values; the generator steers by it and the census of
conditions 1-7 is counted with it.

The walks are steered, not purely random: the generator keeps the census cells no walk has covered yet, proposes for a few of them a
short recipe of actions that reaches the cell from the walk's current state, simulates the recipes on a copy of Flags, appends the one
that covers most new cells per action, and between recipes draws actions at random."""
import copy
import functools
import types

import numpy as np

import ag_pathtracer_amd as ag
import device_update_cases as dc
import morph_model
import normals_model
import skin_model
from morph_cases import targets, weights
from skin_cases import binding

F = np.float32
FRONT_ENDS = ("update_host", "update_device", "transform", "pose", "pose_device", "morph", "morph_joints", "morph_device", "morph_device_joints")
DEFORMS = FRONT_ENDS[2:]
POSES = ("pose", "pose_device", "morph_joints", "morph_device_joints")      # need a skin
MORPHS = ("morph", "morph_joints", "morph_device", "morph_device_joints")   # need targets
READERS = ("bvh", "rebuild_other", "fallback", "dbg_li", "first_deform")
STATES = ("bounds", "arrays", "spheres", "none", "other")
REFUSALS = ("singular_joint", "last_row", "weight", "counts", "radius", "sphere_record")
SPHERE_REFUSALS = ("radius", "sphere_record")
BETWEEN = ("rebuild", "fallback", "device_only")
SNAPSHOTS = ("snapshot_positions", "snapshot_surfaces")
PRIM_OPS = ("mesh", "sphere", "plane", "area_light")
GLOBAL_JOINTS = 800        # above both LDS caps of agpt_update.hip (487 joints with normals, 787 without)
N_ZOO_WALKS, ZOO_LENGTH, N_LONG_WALKS, LONG_LENGTH = 16, 48, 2, 24


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------
def walk_zoo():
    """device_update_cases' zoo (floor, eight meshes, sphere light, sky) plus two spheres and a plane in front of it"""
    d = dc.zoo_scene()
    d.name = "update-walk-zoo"
    blue = d.add_material(ag.MAT_DISNEY, [0.2, 0.3, 0.8], 0.5, 0.0)
    grey = d.add_material(ag.MAT_DIFFUSE_ONLY, [.7, .7, .7])
    d.add_sphere([-0.9, -0.5, -3.4], 0.5, blue)      # primitive 10
    d.add_sphere([1.0, -0.55, -3.9], 0.45, grey)     # 11
    d.add_plane([0.0, -0.8, -5.0], [1.6, 1.0], grey)   # 12
    return d


def walk_seventy():
    d = dc.seventy_prims()
    d.name = "update-walk-70"
    return d


class Layout:
    """which primitive of a description is what, and the meshes the walks act on"""

    def __init__(self, desc, active_sets, long_list):
        self.desc = desc
        self.long = long_list
        self.op_of = [i for i, op in enumerate(desc.ops) if op[0] in PRIM_OPS]
        kinds = [desc.ops[i][0] for i in self.op_of]
        self.meshes = [p for p, k in enumerate(kinds) if k == "mesh"]
        self.spheres = [p for p, k in enumerate(kinds) if k == "sphere"]
        self.planes = [p for p, k in enumerate(kinds) if k == "plane"]
        self.lights = [p for p, k in enumerate(kinds) if k == "area_light"]
        self.active_sets = active_sets
        self.spare = {}            # mesh -> a vertex that no triangle references (where the fallback's NaN goes)
        for p in self.meshes:
            v, corners = self.op(p)[1], self.op(p)[4]
            free = np.setdiff1d(np.arange(len(v)), corners[:, 0])
            if len(free):
                self.spare[p] = int(free[0])

    def op(self, prim):
        return self.desc.ops[self.op_of[prim]]

    def has_normals(self, prim):
        return self.op(prim)[2] is not None

    def centre(self, prim):
        v = self.op(prim)[1].astype(np.float64)
        return 0.5 * (v.min(0) + v.max(0))


@functools.lru_cache(maxsize=None)
def zoo_layout():
    # every set has a grid with normals (SMOOTH mode, the fallback's spare vertex) and a mesh without normals
    sets = [(5, 4, 2), (7, 6, 3), (5, 8, 1), (7, 4, 6), (5, 6, 3), (7, 8, 2), (5, 2, 8), (7, 3, 4)]
    return Layout(walk_zoo(), sets, False)


@functools.lru_cache(maxsize=None)
def long_layout():
    return Layout(walk_seventy(), [(7, 33, 66), (0, 40, 69)], True)


# ---- the inputs of an action ------------------------------------------------------------------------------------------------------------
def pose_arrays(v0, n0, k):
    """explicit arrays number k of a mesh: a smooth deformation of the description's, the normals rolled"""
    p = v0.astype(np.float64)
    a = 0.07 + 0.03 * (k % 4)
    p = p + a * np.stack([np.sin(2.1 * p[:, 1] + k), np.cos(1.7 * p[:, 0] + 0.5 * k), np.sin(1.3 * p[:, 2] - k)], 1)
    return p.astype(F), (None if n0 is None else np.roll(n0, k % max(len(n0), 1), axis=0).copy())


def affine(k):
    """a rotation, a non-uniform scale with a little shear and a small translation, all depending on k (float64, 4x4)"""
    a, axis = 0.2 + 0.13 * (k % 5), k % 3
    c, s = np.cos(a), np.sin(a)
    R = np.eye(3)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    S = np.diag([1.0 + 0.1 * ((k // 3) % 3), 1.0 - 0.06 * (k % 4), 1.0 + 0.07 * (k % 2)])
    S[0, 1] = 0.05 * (k % 3)
    M = np.eye(4)
    M[:3, :3] = R @ S
    M[:3, 3] = 0.12 * np.array([np.sin(k), np.cos(2.0 * k), np.sin(3.0 * k)])
    return M


def matrix_about(centre, k, projective=False):
    """T(c) affine(k) T(-c) in float32; projective: a last row with w != 1 as well"""
    t0, t1 = np.eye(4), np.eye(4)
    t0[:3, 3], t1[:3, 3] = -np.asarray(centre), np.asarray(centre)
    A = affine(k)
    if projective:
        A[3] = [0.01, -0.02, 0.015, 1.0 + 0.05 * (k % 3)]
    return (t1 @ A @ t0).astype(F)


def joint_matrices(centre, n_joints, k):
    base = [matrix_about(centre, k + 3 * j) for j in range(5)]
    for m in base:
        m[3] = [0, 0, 0, 1]
    return np.stack([base[(7 * j + k) % 5] for j in range(n_joints)])


def morph_weights(T, k):
    active = ([0], [0, T - 1], list(range(T)), [T - 1, 0])[k % 4]
    return (weights(T, k, sorted(set(active))) * F(1.0 + 0.015625 * (k % 61))).astype(F)     # (exact in float32, another factor at every step of a walk)


def sphere_record(base_c, base_r, k):
    c = np.asarray(base_c, np.float64) + 0.25 * np.array([np.sin(k), 0.4 + 0.4 * np.cos(1.3 * k), np.sin(2.0 * k)])
    return c.astype(F), float(F(base_r * (1.0 + 0.2 * np.sin(3.0 * k))))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class Model:
    """the scene after each call, by the contract of include/agpt.h:
      mesh[p]     V, N: the current arrays; RV, RN: the arrays it last received explicitly (the rest pose of transform / pose / morph);
                  BV, BN, builder: the arrays and the builder of its last build (they fix the tree's topology); mode; skin; targets
      analytic[p] (centre, radius) of a sphere or an area light's sphere, (o, size) of a plane;  radiance[p] of an area light
      snaps       (kind, frozen scene) of the last two snapshot actions: the two generations the scene keeps"""

    def __init__(self, layout):
        self.layout = layout
        self.builder = "host"
        self.mesh = {}
        for p in layout.meshes:
            op = layout.op(p)
            self.mesh[p] = types.SimpleNamespace(V=op[1], N=op[2], RV=op[1], RN=op[2], BV=op[1], BN=op[2], builder="host", mode="given",
                                                 skin=None, targets=None, corners=op[4])
        self.analytic = {p: (layout.op(p)[1], layout.op(p)[2]) for p in layout.spheres + layout.planes + layout.lights}
        self.radiance = {p: layout.op(p)[3] for p in layout.lights}
        self.snaps = []

    def frozen(self):
        return {"mesh": {p: (m.V, m.N) for p, m in self.mesh.items()}, "analytic": dict(self.analytic), "radiance": dict(self.radiance)}

    def desc(self, arrays="current", frozen=None):
        """the description with the meshes' build-time ("build") or current arrays -- or those of a frozen scene -- and that scene's
        analytic records; same name, so the same fixed ray set"""
        fz = frozen or self.frozen()
        d = copy.copy(self.layout.desc)
        d.ops = list(d.ops)
        for p, i in enumerate(self.layout.op_of):
            op = d.ops[i]
            if op[0] == "mesh":
                v, n = (self.mesh[p].BV, self.mesh[p].BN) if arrays == "build" else fz["mesh"][p]
                d.ops[i] = (op[0], v, n) + op[3:]
            elif op[0] == "sphere":
                d.ops[i] = (op[0], fz["analytic"][p][0], fz["analytic"][p][1], op[3])
            elif op[0] == "plane":
                d.ops[i] = (op[0], fz["analytic"][p][0], fz["analytic"][p][1], op[3])
            elif op[0] == "area_light":
                d.ops[i] = (op[0], fz["analytic"][p][0], fz["analytic"][p][1], fz["radiance"][p])
        return d

    # -- inputs: the arrays an action hands to the library, from the state BEFORE it
    def inputs(self, a):
        kind, k, lay = a["kind"], a.get("k", 0), self.layout
        p = a.get("prim")
        if kind == "refuse":
            return self._refusal_inputs(a)
        if kind in ("update_host", "update_device"):
            op = lay.op(p)
            v, n = pose_arrays(op[1], op[2], k)
            if a.get("nan"):
                v[lay.spare[p], 1] = np.nan
            return {"V": v, "N": n}
        if kind == "transform":
            return {"M": matrix_about(lay.centre(p), k, projective=k % 4 == 3)}
        inp = {}
        if kind in POSES:
            inp["mats"] = joint_matrices(lay.centre(p), self.mesh[p].skin["n_joints"], k)
        if kind in MORPHS:
            inp["w"] = morph_weights(len(self.mesh[p].targets[0]), k)
        if kind == "set_skin":
            op = lay.op(p)
            nv, nn = len(op[1]), 0 if op[2] is None else len(op[2])
            n_joints, K = (GLOBAL_JOINTS, 2) if a["route"] == "global" else (3, 4)
            J, W = binding(nv, K, seed=100 * k + p, n_joints=n_joints)
            nJ, nW = binding(nn, K, seed=100 * k + p + 50, n_joints=n_joints) if nn and nn != nv else (None, None)
            inp["skin"] = {"J": J, "W": W, "nJ": nJ, "nW": nW, "n_joints": n_joints}
        if kind == "set_targets":
            op = lay.op(p)
            dP = targets(len(op[1]), a["T"], 100 * k + p, extent=1.5)
            dN = targets(len(op[2]), a["T"], 100 * k + p + 1, extent=5.0) if op[2] is not None and a["normal_deltas"] else None
            inp["targets"] = (dP, dN)
        if kind in ("update_sphere", "update_plane"):
            op = lay.op(p)
            if kind == "update_sphere":
                inp["c"], inp["r"] = sphere_record(op[1], op[2], k)
            else:
                inp["c"] = sphere_record(op[1], 1.0, k)[0]
                inp["size"] = (np.asarray(op[2], F) * F(1.0 + 0.2 * np.sin(2.0 * k))).astype(F)
        if kind == "set_radiance":
            inp["L"] = (np.asarray(lay.op(p)[3], F) * F(1.0 + 0.3 * np.sin(1.0 * k))).astype(F)
        if kind == "update_spheres":
            inp["records"] = np.array([list(c) + [r] for c, r in (sphere_record(lay.op(q)[1], lay.op(q)[2], k + 5 * i) for i, q in enumerate(a["prims"]))], F)
        return inp

    def _refusal_inputs(self, a):
        what, p, k, lay = a["what"], a.get("prim"), a.get("k", 0), self.layout
        if what in ("singular_joint", "last_row"):
            mats = joint_matrices(lay.centre(p), self.mesh[p].skin["n_joints"], k)
            if what == "singular_joint":
                mats[1, 2, :3] = 0        # a zero row: every term of the cofactor expansion is a product with 0
            else:
                mats[0, 3] = [0, 0, 0, 2]
            return {"mats": mats}
        if what == "weight":
            w = morph_weights(len(self.mesh[p].targets[0]), k)
            w[-1] = np.nan
            return {"w": w}
        if what == "counts":
            op = lay.op(p)
            v, n = pose_arrays(op[1], op[2], k)
            return {"V": v[:-1].copy(), "N": n}
        if what == "radius":
            return {"c": sphere_record(lay.op(p)[1], lay.op(p)[2], k)[0], "r": (0.0, -0.5)[k % 2]}
        rec = np.array([list(c) + [r] for c, r in (sphere_record(lay.op(q)[1], lay.op(q)[2], k) for q in a["prims"])], F)
        rec[len(rec) - 1, k % 4] = (np.nan, np.inf)[k % 2]
        return {"records": rec}

    # -- apply: the scene after the action
    def apply(self, a, inp):
        kind, p = a["kind"], a.get("prim")
        if kind in FRONT_ENDS:
            m = self.mesh[p]
            smooth = m.mode == "smooth"
            RN = None if smooth else m.RN
            if kind in ("update_host", "update_device"):
                V, N = inp["V"], inp["N"]
            elif kind == "transform":
                V, N = ag.transform_arrays(inp["M"], m.RV, RN)
            elif kind in ("pose", "pose_device"):
                s = m.skin
                V, N = skin_model.skin_arrays(inp["mats"], m.RV, s["J"], s["W"], RN, s["nJ"], s["nW"])
            elif kind in ("morph", "morph_device"):
                V, N = morph_model.morph_arrays(inp["w"], m.RV, m.targets[0], RN, m.targets[1])
            else:
                s = m.skin
                V, N = morph_model.morph_then_skin(inp["w"], inp["mats"], m.RV, m.targets[0], s["J"], s["W"], RN, m.targets[1], s["nJ"], s["nW"])
            if smooth:
                N = normals_model.vertex_normals_arrays(V, m.corners, len(m.RN))
            m.V, m.N = V, N
            if kind in ("update_host", "update_device"):
                m.RV, m.RN = V, N       # (SMOOTH: the mirror, hence the next rest pose, holds the recomputed normals)
            if a["mode"] == "rebuild":
                m.BV, m.BN, m.builder = V, N, self.builder
        elif kind == "set_skin":
            self.mesh[p].skin = inp["skin"]
        elif kind == "set_targets":
            self.mesh[p].targets = inp["targets"]
        elif kind == "set_mode":
            self.mesh[p].mode = a["value"]
        elif kind == "set_builder":
            self.builder = a["value"]
        elif kind == "update_sphere":
            self.analytic[p] = (inp["c"], inp["r"])
        elif kind == "update_plane":
            self.analytic[p] = (inp["c"], inp["size"])
        elif kind == "set_radiance":
            self.radiance[p] = inp["L"]
        elif kind == "update_spheres":
            for q, rec in zip(a["prims"], inp["records"]):
                self.analytic[q] = (rec[:3].copy(), float(rec[3]))
        elif kind in SNAPSHOTS:
            self.snaps = (self.snaps + [(kind, self.frozen())])[-2:]
        # bvh, dbg_li and refusals change nothing


CHANGES_GEOMETRY = FRONT_ENDS + ("update_sphere", "update_plane", "update_spheres")   # the actions condition 7 is about


# ---- the predicted bookkeeping and the census ----------------------------------------------------------------------------------------
class Flags:
    """what DESIGN.md section 5.7 says the library keeps per mesh -- bounds_stale, arrays_stale, the rest pose, the cache -- and per scene
    (spheres_stale, the builder), advanced action by action; step() returns the census cells the action covers in the state it meets"""

    def __init__(self, layout):
        self.layout = layout
        self.m = {p: types.SimpleNamespace(bounds=False, arrays=False, rest=False, finite=True, skin=None, targets=0, mode="given", cache=False,
                                           after=None, chain=None, switched=None, over=None) for p in layout.meshes}
        self.spheres = False
        self.builder = "host"
        self.prev = None
        self.last_snapshot = None
        self.between = set()
        self.refused = {}

    def stale(self, p):
        return self.m[p].bounds or self.m[p].arrays

    def states(self, p, others_only=False):
        """the STATES a mirror reader that names mesh p (None: no mesh) meets now.  others_only: "bounds" and "arrays" are counted from the
        meshes other than p -- for a REBUILD or a fallback of p, whose own stale state the call overwrites: the commit behind it reads
        the mirror of the OTHER meshes"""
        seen = [x for q, x in self.m.items() if not (others_only and q == p)]
        any_b, any_a = any(x.bounds for x in seen), any(x.arrays for x in seen)
        s = set()
        if any_b and not any_a:
            s.add("bounds")
        if any_a:
            s.add("arrays")
        if self.spheres:
            s.add("spheres")
        if not (any_b or any_a or self.spheres):
            s.add("none")
        if any(self.stale(q) for q in self.m if q != p) and (p is None or not self.stale(p)):
            s.add("other")
        return s

    def _sync(self, arrays):
        for x in self.m.values():
            x.bounds = False
            if arrays:
                x.arrays = False
        self.spheres = False

    def _reader_between(self):
        for x in self.m.values():
            x.chain = None

    def step(self, a):
        kind, p = a["kind"], a.get("prim")
        cells = set()
        if kind in FRONT_ENDS:
            st, mode = self.m[p], a["mode"]
            explicit = kind in ("update_host", "update_device")
            finite = not a.get("nan") if explicit else st.finite
            host_path = mode == "rebuild" or not finite
            fallback = mode == "refit" and not finite
            first = not explicit and not st.rest
            reader = "first_deform" if first else "rebuild_other" if mode == "rebuild" else "fallback" if fallback and explicit else None
            if reader:
                cells |= {("reader", reader, s) for s in self.states(p, others_only=reader != "first_deform")}
            if st.chain and not host_path:
                cells.add(("pair", st.chain, kind))
            if st.after:
                cells.add(("after_" + st.after, kind))
            if self.prev == "set_builder":
                cells.add(("after_builder", kind))
            if st.mode == "smooth":
                cells.add(("smooth", kind))
            if st.switched:
                cells.add(("first_after_mode", st.switched, kind))
            if mode == "rebuild":
                cells.add(("rebuild_mode", kind))
            if kind in POSES:
                cells.add(("route", kind, st.skin))
            if self.layout.long and not host_path:
                cells.add(("long", kind))
            if first or host_path:       # sync_mirror(s, true) runs: it meets the meshes whose stale arrays a host path overwrote
                cells |= {("overwritten", x.over) for x in self.m.values() if x.over}
                for x in self.m.values():
                    x.over = None
                self._reader_between()
            if first:
                self._sync(True)
                st.rest = True
            if host_path and st.arrays:     # update_on_host replaces arrays that existed only on the device: arrays_stale must go with them
                st.over = "rebuild" if mode == "rebuild" else "fallback"
            if explicit:
                st.rest, st.finite = False, finite
            if host_path:
                self._sync(True)
                st.cache = st.cache and mode != "rebuild"
            else:
                st.bounds, st.arrays, st.cache, st.over = True, not (kind == "update_host" and st.mode == "given"), True, None
            st.chain = None if host_path else kind
            st.after = "rebuild" if mode == "rebuild" else "fallback" if fallback and explicit else None
            st.switched = None
            self.between |= {"rebuild"} if mode == "rebuild" else {"fallback"} if fallback else {"device_only"} if kind != "update_host" else set()
        elif kind in ("set_skin", "set_targets", "set_mode"):
            st = self.m[p]
            st.chain = st.after = None
            if kind == "set_skin":
                if st.skin and st.cache:
                    cells.add(("setter_replaced", "skin"))
                st.skin = a["route"]
            elif kind == "set_targets":
                if st.targets and st.cache:
                    cells.add(("setter_replaced", "targets"))
                st.targets = a["T"]
            elif a["value"] != st.mode:
                st.mode, st.switched = a["value"], "to_" + a["value"]
        elif kind == "set_builder":
            self.builder = a["value"]
        elif kind in ("bvh", "dbg_li"):
            cells |= {("reader", kind, s) for s in self.states(p)}
            self._reader_between()
            self._sync(False)
            if kind == "bvh":
                self.m[p].after = None
        elif kind in ("update_sphere", "update_plane", "set_radiance"):
            cells.add(("analytic", kind))
        elif kind == "update_spheres":
            cells.add(("spheres_via", a["via"]))
            self.spheres = True
        elif kind in SNAPSHOTS:
            if self.last_snapshot:
                cells |= {("snap", kind, b) for b in self.between}
                if self.last_snapshot != kind:
                    cells.add(("alternate", self.last_snapshot + ">" + kind))
            self.last_snapshot, self.between = kind, set()
        elif kind == "refuse":
            what = a["what"]
            self.refused[what] = self.refused.get(what, 0) + 1
            cells.add(("refusal", what, min(self.refused[what], 2)))
            if (self.spheres or any(self.stale(q) for q in self.m)) if what in SPHERE_REFUSALS else self.stale(p):
                cells.add(("refusal_stale", what))
            if p in self.m:      # a refusal that names a mesh is an action on it (the device-pointer ones launch its front-end kernels)
                self.m[p].chain = self.m[p].after = None
        self.prev = kind
        return cells


def zoo_universe():
    """every census cell the zoo walks together must cover: conditions 1 - 6, and the routes, modes and variants beside them"""
    u = {("pair", x, y) for x in FRONT_ENDS for y in FRONT_ENDS}
    u |= {("after_" + w, k) for w in ("rebuild", "fallback", "builder") for k in FRONT_ENDS}
    u |= {("reader", r, s) for r in READERS for s in STATES}
    u |= {("smooth", k) for k in FRONT_ENDS} | {("first_after_mode", d, k) for d in ("to_smooth", "to_given") for k in FRONT_ENDS}
    u |= {("snap", s, b) for s in SNAPSHOTS for b in BETWEEN}
    u |= {("alternate", "snapshot_positions>snapshot_surfaces"), ("alternate", "snapshot_surfaces>snapshot_positions")}
    u |= {("refusal", w, n) for w in REFUSALS for n in (1, 2)} | {("refusal_stale", w) for w in REFUSALS}
    u |= {("rebuild_mode", k) for k in FRONT_ENDS} | {("route", k, r) for k in POSES for r in ("lds", "global")}
    u |= {("spheres_via", v) for v in ("tensor", "pointer", "host")} | {("analytic", k) for k in ("update_sphere", "update_plane", "set_radiance")}
    u |= {("setter_replaced", "skin"), ("setter_replaced", "targets")}
    # a REBUILD and a fallback of a mesh whose new arrays existed only on the device, then a commit behind another call
    u |= {("overwritten", "rebuild"), ("overwritten", "fallback")}
    return u


def long_universe():
    """the 70-primitive scene: every front end in REFIT (the top-level tree is uploaded again) and the readers behind a device-only REFIT"""
    return {("long", k) for k in FRONT_ENDS} | {("reader", r, "arrays") for r in ("bvh", "rebuild_other", "dbg_li", "first_deform")}


def census(walks, layout_long):
    """the cells a list of walks covers, counted from the action lists alone"""
    covered = set()
    for w in walks:
        if w.layout.long != layout_long:
            continue
        fl = Flags(w.layout)
        for a in w.actions:
            covered |= fl.step(a)
    return covered


# ---- the generator --------------------------------------------------------------------------------------------------------------------
class Walk:
    def __init__(self, seed, layout, actions):
        self.seed, self.layout, self.actions = seed, layout, actions

    def __repr__(self):
        return "walk-%d%s" % (self.seed, "-long" if self.layout.long else "")


class _Generator:
    def __init__(self, seed, layout, active, limit, universe, covered):
        self.rng = np.random.RandomState(seed)
        self.lay, self.active, self.limit, self.universe, self.covered = layout, list(active), limit, universe, covered
        self.fl = Flags(layout)
        self.actions = []
        self.k = 0

    # -- single actions
    def pick(self, xs):
        xs = list(xs)
        return xs[self.rng.randint(len(xs))]

    def fe(self, kind, p, mode="refit", nan=False):
        return {"kind": kind, "prim": p, "mode": mode, "nan": nan}

    def spheres_batch(self, via=None):
        prims = self.lay.spheres + (self.lay.lights if self.rng.rand() < 0.5 else [])
        return {"kind": "update_spheres", "prims": prims, "via": via or self.pick(("tensor", "pointer", "host"))}

    def meshes(self, normals=None, spare=None, given=None, finite=None, fl=None):
        fl = fl or self.fl
        out = [p for p in self.active if (normals is None or self.lay.has_normals(p) == normals) and (spare is None or (p in self.lay.spare) == spare)
               and (given is None or (fl.m[p].mode == "given") == given) and (finite is None or fl.m[p].finite == finite)]
        return out

    def refusal(self, what, p=None):
        if what in SPHERE_REFUSALS:
            if what == "radius":
                return {"kind": "refuse", "what": what, "prim": self.pick(self.lay.spheres + self.lay.lights), "via": "host"}
            return {"kind": "refuse", "what": what, "prims": list(self.lay.spheres), "via": self.pick(("tensor", "pointer"))}
        return {"kind": "refuse", "what": what, "prim": p if p is not None else self.pick(self.active), "via": self.pick(("host", "device"))}

    # -- recipes: a short list of actions that reaches a cell from the current state (or None)
    def recipe(self, cell):
        lay, fl, tag = self.lay, self.fl, cell[0]
        p = self.pick(self.active)
        explicit_rebuild = lambda q: self.fe("update_host", q, "rebuild")    # clears every flag and the rest pose of q
        finite = self.meshes(finite=True)
        if tag == "pair":
            have = [q for q in finite if fl.m[q].chain == cell[1]]
            if have:
                return [self.fe(cell[2], self.pick(have))]
            if not finite:
                return [self.fe("update_host", p), self.fe(cell[1], p), self.fe(cell[2], p)]
            q = self.pick(finite)
            return [self.fe(cell[1], q), self.fe(cell[2], q)]
        if tag == "after_rebuild":
            return [self.fe(self.pick(FRONT_ENDS), p, "rebuild"), self.fe(cell[1], p, self.pick(("refit", "refit", "rebuild")))]
        if tag == "after_fallback":
            q = self.pick(self.meshes(spare=True))
            return [self.fe("update_host", q, nan=True), self.fe(cell[1], q)]
        if tag == "after_builder":
            return [{"kind": "set_builder", "value": "switch"}, self.fe(cell[1], p, self.pick(("refit", "rebuild")))]
        if tag == "reader":
            r, state = cell[1], cell[2]
            if lay.long:
                p = self.pick(self.active)
            if r == "fallback":
                p = self.pick(self.meshes(spare=True))
            others = [q for q in self.active if q != p]
            q = self.pick([x for x in others if fl.m[x].mode == "given"] or others)
            pre = [explicit_rebuild(p)]
            if state == "bounds":
                if fl.m[q].mode != "given":
                    pre.append({"kind": "set_mode", "prim": q, "value": "given"})
                pre.append(self.fe("update_host", q))
            elif state in ("arrays", "other"):
                pre.append(self.fe("update_device", q))
            elif state == "spheres":
                pre.append(self.spheres_batch())
            act = {"bvh": {"kind": "bvh", "prim": p}, "dbg_li": {"kind": "dbg_li"}, "rebuild_other": self.fe(self.pick(FRONT_ENDS[:2]), p, "rebuild"),
                   "fallback": self.fe("update_host", p, nan=True), "first_deform": self.fe(self.pick(DEFORMS), p)}[r]
            return pre + [act]
        if tag in ("smooth", "first_after_mode"):
            with_n = self.meshes(normals=True)
            if not with_n:
                return None
            target = "smooth" if tag == "smooth" or cell[1] == "to_smooth" else "given"
            kind = cell[-1]
            ready = [x for x in with_n if fl.m[x].mode == target and (tag == "smooth" or fl.m[x].switched == "to_" + target)]
            if ready:
                return [self.fe(kind, self.pick(ready))]
            q = self.pick([x for x in with_n if fl.m[x].mode != target] or with_n)
            pre = [] if fl.m[q].mode != target else [{"kind": "set_mode", "prim": q, "value": "given" if target == "smooth" else "smooth"}]
            return pre + [{"kind": "set_mode", "prim": q, "value": target}, self.fe(kind, q)]
        if tag == "snap":
            mid = {"rebuild": lambda: self.fe(self.pick(FRONT_ENDS), p, "rebuild"),
                   "fallback": lambda: self.fe("update_host", self.pick(self.meshes(spare=True)), nan=True),
                   "device_only": lambda: self.fe(self.pick(FRONT_ENDS[1:]), self.pick(finite or [p]))}[cell[2]]()
            first = [] if fl.prev in SNAPSHOTS else [{"kind": self.pick(SNAPSHOTS)}]
            return first + [mid, {"kind": cell[1]}]
        if tag == "alternate":
            a, b = cell[1].split(">")
            return ([] if fl.last_snapshot == a else [{"kind": a}]) + [self.fe(self.pick(FRONT_ENDS), p), {"kind": b}]
        if tag == "refusal":
            return [self.refusal(cell[1])]
        if tag == "refusal_stale":
            if cell[1] in SPHERE_REFUSALS:
                return [self.spheres_batch(), self.refusal(cell[1])]
            return [self.fe("update_device", p), self.refusal(cell[1], p)]
        if tag == "rebuild_mode":
            return [self.fe(cell[1], p, "rebuild")]
        if tag == "route":
            have = [q for q in finite if fl.m[q].skin == cell[2]]
            if have:
                return [self.fe(cell[1], self.pick(have))]
            return [{"kind": "set_skin", "prim": p, "route": cell[2]}, self.fe(cell[1], p)]
        if tag == "long":
            return [self.fe(cell[1], self.pick(finite or [p]))]
        if tag == "spheres_via":
            return [self.spheres_batch(cell[1])] if lay.spheres else None
        if tag == "analytic":
            target = {"update_sphere": lay.spheres + lay.lights, "update_plane": lay.planes, "set_radiance": lay.lights}[cell[1]]
            return [{"kind": cell[1], "prim": self.pick(target)}] if target else None
        if tag == "overwritten":
            q = self.pick(self.meshes(spare=True)) if cell[1] == "fallback" else p
            over = self.fe("update_host", q, nan=True) if cell[1] == "fallback" else self.fe(self.pick(FRONT_ENDS[:2]), q, "rebuild")
            return [self.fe("update_device", q), over, explicit_rebuild(self.pick([x for x in self.active if x != q]))]
        if tag == "setter_replaced":
            if cell[1] == "skin":
                return [self.fe("pose", p), {"kind": "set_skin", "prim": p, "route": self.pick(("lds", "global"))}, self.fe("pose_device", p)]
            return [self.fe("morph", p), {"kind": "set_targets", "prim": p, "T": self.pick((2, 3)), "normal_deltas": bool(self.rng.randint(2))},
                    self.fe("morph_device", p)]
        return None

    def random_action(self):
        lay, fl = self.lay, self.fl
        r = self.rng.rand()
        p = self.pick(self.active)
        if r < 0.5 or not lay.spheres:
            kind = self.pick(FRONT_ENDS)
            nan = kind == "update_host" and p in lay.spare and self.rng.rand() < 0.15
            return self.fe(kind, p, "rebuild" if self.rng.rand() < 0.2 and not nan else "refit", nan)
        if r < 0.62:
            return self.pick([{"kind": "update_sphere", "prim": self.pick(lay.spheres + lay.lights)}, {"kind": "update_plane", "prim": self.pick(lay.planes)},
                              {"kind": "set_radiance", "prim": self.pick(lay.lights)}, self.spheres_batch()])
        if r < 0.74:
            return self.pick([{"kind": "bvh", "prim": p}, {"kind": "dbg_li"}])
        if r < 0.82:
            return {"kind": self.pick(SNAPSHOTS)}
        if r < 0.9:
            with_n = self.meshes(normals=True)
            if with_n and self.rng.rand() < 0.6:
                q = self.pick(with_n)
                return {"kind": "set_mode", "prim": q, "value": "given" if fl.m[q].mode == "smooth" else "smooth"}
            return {"kind": "set_builder", "value": "switch"}
        return self.refusal(self.pick(REFUSALS))

    # -- what an action needs before it, the simulation
    def complete(self, actions, fl):
        """the actions with the setters their front ends and refusals need put in front, on the state fl (which is advanced)"""
        out = []
        for a in actions:
            a = dict(a)
            p = a.get("prim")
            needs_skin = a["kind"] in POSES or (a["kind"] == "refuse" and a["what"] in ("singular_joint", "last_row"))
            needs_targets = a["kind"] in MORPHS or (a["kind"] == "refuse" and a["what"] == "weight")
            pre = []
            if needs_skin and not fl.m[p].skin:
                pre.append({"kind": "set_skin", "prim": p, "route": "lds"})
            if needs_targets and not fl.m[p].targets:
                pre.append({"kind": "set_targets", "prim": p, "T": 3, "normal_deltas": True})
            if a["kind"] == "set_builder" and a["value"] == "switch":
                a["value"] = "device" if fl.builder == "host" else "host"
            for x in pre + [a]:
                out.append(x)
                fl.step(x)
        return out

    def simulate(self, actions):
        fl = copy.deepcopy(self.fl)
        done = self.complete(actions, fl)
        fl2 = copy.deepcopy(self.fl)
        gained = set()
        for a in done:
            gained |= fl2.step(a)
        return done, (gained & self.universe) - self.covered

    def append(self, done):
        for a in done:
            self.k += 1
            a = dict(a, k=self.k)
            self.covered |= self.fl.step(a) & self.universe
            self.actions.append(a)

    def run(self, noise=0.2):
        stuck = 0
        setup = []
        for p in self.active:     # every mesh of the walk can be posed and morphed from the start
            setup += [{"kind": "set_skin", "prim": p, "route": self.pick(("lds", "lds", "global"))},
                      {"kind": "set_targets", "prim": p, "T": self.pick((2, 3)), "normal_deltas": bool(self.rng.randint(2))}]
        self.append(setup)
        while len(self.actions) < self.limit and stuck < 20:
            missing = sorted(self.universe - self.covered, key=repr)
            best = None
            if missing and self.rng.rand() >= noise:
                for i in self.rng.permutation(len(missing))[:10]:
                    rec = self.recipe(missing[i])
                    if not rec:
                        continue
                    done, gained = self.simulate(rec)
                    if gained and len(self.actions) + len(done) <= self.limit and (best is None or len(gained) / len(done) > best[1]):
                        best = (done, len(gained) / len(done))
            if best is None:
                done, _ = self.simulate([self.random_action()])
                if len(self.actions) + len(done) > self.limit:
                    stuck += 1
                    continue
                best = (done, 0)
            self.append(best[0])
        return self.actions


@functools.lru_cache(maxsize=None)
def walks():
    """the fixed walk set: N_ZOO_WALKS walks of at most ZOO_LENGTH actions on the zoo, then N_LONG_WALKS of at most LONG_LENGTH on the
    70-primitive scene; walk i has seed SEEDS[i] and is reproduced by it (together with the walks before it, whose cells it skips)"""
    out = []
    for lay, n, limit, universe, first_seed in ((zoo_layout(), N_ZOO_WALKS, ZOO_LENGTH, zoo_universe(), 1000),
                                                (long_layout(), N_LONG_WALKS, LONG_LENGTH, long_universe(), 7000)):
        covered = set()
        for i in range(n):
            g = _Generator(first_seed + i, lay, lay.active_sets[i % len(lay.active_sets)], limit, universe, covered)
            out.append(Walk(first_seed + i, lay, g.run()))
    return out


SEEDS = [1000 + i for i in range(N_ZOO_WALKS)] + [7000 + i for i in range(N_LONG_WALKS)]


def walk(seed):
    return walks()[SEEDS.index(seed)]


def __getattr__(name):
    if name == "WALKS":
        return walks()
    raise AttributeError(name)


def describe(a):
    """an action in a failure message"""
    return " ".join("%s=%s" % (k, a[k]) for k in ("kind", "what", "prim", "prims", "mode", "nan", "route", "T", "value", "via", "k") if a.get(k) not in (None, False))
