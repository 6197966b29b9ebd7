// agpt_analytic.h -- spheres, planes and lights of a committed scene, moved in place (agpt_analytic.hip: agpt_scene_update_sphere,
// agpt_scene_update_plane, the two radiance calls, agpt_scene_update_spheres_device), and the analytic half of the motion vectors
// (agpt_motion.hip).  The only device copy of a sphere or a plane is DevPrim::{cx, cy, cz, r, r2} (agpt_scene.h); the trace, shading
// and feature kernels read it at every launch, so rewriting those 20 bytes moves the primitive.  One definition of the record for the
// host calls, agpt_scene_add_sphere and k_update_spheres.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "agpt_scene.h"

struct agpt_scene;

// what a sphere leaves in DevPrim / HostSphere
struct AnalyticRecord {
    float cx, cy, cz, r, r2;
};

// Sphere ctor (intersectable.h:161-162): the radius and its square, each rounded on its own
AGPT_HD AnalyticRecord sphere_record(float cx, float cy, float cz, float radius) {
    AnalyticRecord a;
    a.cx = cx;
    a.cy = cy;
    a.cz = cz;
    a.r = radius;
    a.r2 = radius * radius;
    return a;
}

// the update calls' rule, stricter than agpt_scene_add_sphere's: every value finite and radius > 0 (a NaN radius fails the comparison)
AGPT_HD bool analytic_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }
AGPT_HD bool sphere_record_refused(float cx, float cy, float cz, float radius) {
    return !(analytic_finite(cx) && analytic_finite(cy) && analytic_finite(cz) && analytic_finite(radius) && radius > 0.f);
}

// One generation of agpt_scene_snapshot_positions' analytic records: two float4 per primitive index k,
//   [2k] = (cx, cy, cz, r)   [2k + 1] = (r2, type as bits, 0, 0)      (a mesh: its DevPrim's zeros)
// The 20 record bytes are [2k].xyzw and [2k + 1].x; the type never changes between generations.
#define AGPT_ANALYTIC_GEN_STRIDE 2

namespace agpt {
// gen[2k], gen[2k + 1] from prims[k] for the n_prims primitives of the scene
void launch_snapshot_analytic(hipStream_t stream, const DevPrim* prims, uint32_t n_prims, float4* gen);
// the host's spheres from the device's records, if agpt_scene_update_spheres_device left them behind (sync_mirror, agpt_scene_api.hip)
int download_spheres(agpt_scene* s);
}  // namespace agpt
