// agpt_motion.hip -- per-object motion vectors for the temporal reprojection (include/agpt.h): the kernels of
// agpt_scene_snapshot_positions and agpt_render_features_motion (the entry point is in agpt_api.hip, beside agpt_render_features).
// agpt_scene_snapshot_surfaces is defined here too: the same snapshot plus a device-to-device copy of the tri_shade records, no kernel
// of its own.  The call that reprojects the points, agpt_temporal_accumulate_motion, is in agpt_temporal.hip with the other temporal calls.
//
// k_snapshot_positions copies the world-space positions the update calls left in tri_verts (BVH slot order) into a buffer indexed by
// the global triangle id, so two snapshots compare triangle by triangle whatever a rebuild did to the slot order.  k_motion turns a
// feature-pass hit into the point the hit surface had in the older snapshot.  One thread per item, fixed order, no atomics, no LDS:
// tests/motion_model.py reproduces each operation by operation.  Compiled with the library's common flags (-ffp-contract=off, IEEE
// divide / sqrt).
// Both are bandwidth kernels.  k_snapshot_positions: 48 B read contiguous per wave, 48 B written to 3 * gid -- scattered within
// a mesh's range by its leaf order.  k_motion: per pixel 16 B of hit and 32 B of ray, contiguous, and on a mesh hit 2 x 48 B gathered at
// the hit triangle (a wave's pixels share a few triangles), 16 B written.
#include <hip/hip_runtime.h>

#include <string>

#include "agpt_analytic.h"
#include "agpt_internal.h"
#include "agpt_motion.h"

using agpt::fail;

__global__ void __launch_bounds__(AGPT_BLOCK)
k_snapshot_positions(const float4* __restrict__ tri_verts, uint32_t n_tris, float4* __restrict__ gen) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_tris) return;
    float4 v0 = tri_verts[3 * (size_t)s], v1 = tri_verts[3 * (size_t)s + 1], v2 = tri_verts[3 * (size_t)s + 2];
    const uint32_t gid = __float_as_uint(v0.w);
    if (gid >= n_tris) return;   // (no record of a committed scene: pack_tri_verts writes ids below the triangle count)
    v0.w = 0.f; v1.w = 0.f; v2.w = 0.f;
    float4* out = gen + 3 * (size_t)gid;
    out[0] = v0;
    out[1] = v1;
    out[2] = v2;
}

// prev_point = (p.xyz, w): w = 0 a miss (p = 0); w = 2 a surface that did not move between the two snapshots -- a triangle whose 36
// position bytes, a sphere or a plane whose 20 record bytes are the same in both --, p = O + t * D; w = 1 a triangle that moved, p = its
// older positions at this hit's barycentrics.
// A sphere or a plane k (an_old / an_new: the analytic generations, agpt_analytic.h; n_prims == 0 without them) whose 20 record bytes
// differ: w = 1 and p = c_old + (p - c_new) * s per component, s = (q, q, q) with q = r_old / r_new for a sphere and
// (r_old / r_new, 1, r2_old / r2_new) -- the half-sizes -- for a plane; a component of s or of that point that is not finite leaves
// w = 2 and p = O + t * D.
__global__ void __launch_bounds__(AGPT_BLOCK)
k_motion(RenderConsts rc, const DevHit* __restrict__ hits, const float4* __restrict__ ray_o, const float4* __restrict__ ray_d,
         const float4* __restrict__ gen_old, const float4* __restrict__ gen_new, uint32_t n_tris, const float4* __restrict__ an_old,
         const float4* __restrict__ an_new, uint32_t n_prims, float4* __restrict__ prev_point) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rc.NP) return;
    int x, y;
    size_t ai;
    pixel_of(rc, i, x, y, ai);
    const DevHit h = hits[i];
    float4 m;
    m.x = 0.f; m.y = 0.f; m.z = 0.f; m.w = 0.f;
    if (h.id != AGPT_HIT_MISS) {
        const float4 o4 = ray_o[i], d4 = ray_d[i];
        const v3 O = V3(o4.x, o4.y, o4.z), D = V3(d4.x, d4.y, d4.z);
        v3 p = O + h.t * D;
        m.w = 2.f;
        if (!(h.id & AGPT_HIT_SPHERE) && h.id < n_tris) {
            const float4* a = gen_old + 3 * (size_t)h.id;
            const float4* b = gen_new + 3 * (size_t)h.id;
            const float4 a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
            // the bytes, not the values: -0 against +0 counts as moved, a NaN against itself does not
            const uint32_t differ = (__float_as_uint(a0.x) ^ __float_as_uint(b0.x)) | (__float_as_uint(a0.y) ^ __float_as_uint(b0.y)) |
                                    (__float_as_uint(a0.z) ^ __float_as_uint(b0.z)) | (__float_as_uint(a1.x) ^ __float_as_uint(b1.x)) |
                                    (__float_as_uint(a1.y) ^ __float_as_uint(b1.y)) | (__float_as_uint(a1.z) ^ __float_as_uint(b1.z)) |
                                    (__float_as_uint(a2.x) ^ __float_as_uint(b2.x)) | (__float_as_uint(a2.y) ^ __float_as_uint(b2.y)) |
                                    (__float_as_uint(a2.z) ^ __float_as_uint(b2.z));
            if (differ) {
                const float w0 = (1.f - h.b1) - h.b2;
                p = (V3(a0.x, a0.y, a0.z) * w0 + V3(a1.x, a1.y, a1.z) * h.b1) + V3(a2.x, a2.y, a2.z) * h.b2;
                m.w = 1.f;
            }
        } else if ((h.id & AGPT_HIT_SPHERE) && (h.id & 0x7FFFFFFFu) < n_prims) {
            const size_t k = AGPT_ANALYTIC_GEN_STRIDE * (size_t)(h.id & 0x7FFFFFFFu);
            const float4 a0 = an_old[k], a1 = an_old[k + 1], b0 = an_new[k], b1 = an_new[k + 1];
            const uint32_t differ = (__float_as_uint(a0.x) ^ __float_as_uint(b0.x)) | (__float_as_uint(a0.y) ^ __float_as_uint(b0.y)) |
                                    (__float_as_uint(a0.z) ^ __float_as_uint(b0.z)) | (__float_as_uint(a0.w) ^ __float_as_uint(b0.w)) |
                                    (__float_as_uint(a1.x) ^ __float_as_uint(b1.x));
            if (differ) {
                const float q = a0.w / b0.w;
                const bool plane = __float_as_uint(b1.y) == (uint32_t)AGPT_PRIM_PLANE;
                const v3 s = plane ? V3(q, 1.f, a1.x / b1.x) : V3(q, q, q);
                const v3 was = V3(a0.x, a0.y, a0.z) + (p - V3(b0.x, b0.y, b0.z)) * s;
                if (analytic_finite(s.x) && analytic_finite(s.z) && analytic_finite(was.x) && analytic_finite(was.y) && analytic_finite(was.z)) {
                    p = was;
                    m.w = 1.f;
                }
            }
        }
        m.x = p.x; m.y = p.y; m.z = p.z;
    }
    prev_point[ai] = m;
}

namespace agpt {

void launch_snapshot_positions(hipStream_t stream, const float4* tri_verts, uint32_t n_tris, float4* gen) {
    hipLaunchKernelGGL(k_snapshot_positions, agpt_blocks(n_tris), dim3(AGPT_BLOCK), 0, stream, tri_verts, n_tris, gen);
}
void launch_motion(hipStream_t stream, const RenderConsts& rc, const DevHit* hits, const float4* ray_o, const float4* ray_d,
                   const float4* gen_old, const float4* gen_new, uint32_t n_tris, const float4* an_old, const float4* an_new, uint32_t n_prims,
                   float4* prev_point) {
    hipLaunchKernelGGL(k_motion, agpt_blocks(rc.NP), dim3(AGPT_BLOCK), 0, stream, rc, hits, ray_o, ray_d, gen_old, gen_new, n_tris, an_old,
                       an_new, n_prims, prev_point);
}

}  // namespace agpt

// The newer generation becomes the older one; the newer one is filled from what the update calls left in tri_verts and -- the spheres
// and planes -- in d_prims.  The first call allocates both and fills both with the same bytes.
// surfaces (agpt_scene_snapshot_surfaces, `fn` names the entry point that was called): the tri_shade records as well, one device-to-device
// copy behind the updates; without it the shading generations are freed.
static int snapshot(const char* fn, bool surfaces, agpt_scene* s) {
    const std::string f(fn);
    if (!s) return fail(AGPT_ERR_INVALID, f + ": NULL scene");
    if (!s->committed) return fail(AGPT_ERR_INVALID, f + ": the scene is not committed");
    size_t n_tris = 0, n_prims = 0;
    for (const agpt::HostMesh& m : s->meshes) n_tris += m.prim_index.size();
    if (!s->spheres.empty()) n_prims = s->prims.size();   // (records by primitive index; none for a scene of meshes only)
    agpt_scene::PositionSnapshots& ps = s->snapshots;
    if (n_tris == 0 && n_prims == 0) {   // nothing to hold: every hit of such a scene is a miss
        ps.valid = true;
        ps.surfaces = surfaces;
        return AGPT_OK;
    }
    if (3 * n_tris > s->d_tri_verts.n || n_tris > 0x7FFFFFFFull || n_prims > s->d_prims.n || (surfaces && 4 * n_tris > s->d_tri_shade.n))
        return fail(AGPT_ERR_DEVICE, f + ": the scene's records do not cover its meshes and primitives");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const bool first = !ps.valid;
    const size_t n_analytic = AGPT_ANALYTIC_GEN_STRIDE * n_prims;
    if (first) {
        bool ok = true;
        for (int g = 0; g < 2; g++) {
            if (n_tris) ok = ok && ps.gen[g].alloc(3 * n_tris) == hipSuccess;
            if (n_prims) ok = ok && ps.analytic[g].alloc(n_analytic) == hipSuccess;
        }
        if (!ok) {
            ps.drop();
            return fail(AGPT_ERR_NOMEM, f + ": out of device memory");
        }
        ps.n_tris = n_tris;
        ps.n_prims = n_prims;
        ps.newest = 0;
    } else {
        ps.newest ^= 1;
    }
    if (n_tris) agpt::launch_snapshot_positions(c->stream, s->d_tri_verts.p, (uint32_t)n_tris, ps.gen[ps.newest].p);
    if (n_prims) agpt::launch_snapshot_analytic(c->stream, s->d_prims.p, (uint32_t)n_prims, ps.analytic[ps.newest].p);
    HIP_TRY(hipGetLastError());
    if (first && n_tris)
        HIP_TRY(hipMemcpyAsync(ps.gen[ps.newest ^ 1].p, ps.gen[ps.newest].p, 3 * n_tris * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    if (first && n_prims)
        HIP_TRY(hipMemcpyAsync(ps.analytic[ps.newest ^ 1].p, ps.analytic[ps.newest].p, n_analytic * sizeof(float4), hipMemcpyDeviceToDevice,
                               c->stream));
    if (!surfaces) {
        ps.drop_surfaces();
    } else if (n_tris) {
        // absent (no snapshot yet, or the last one was agpt_scene_snapshot_positions'): both generations get the current bytes.
        // d_tri_shade.p is read now: an AGPT_UPDATE_REBUILD may have reallocated it.
        const bool absent = !ps.surfaces;
        const size_t bytes = 4 * n_tris * sizeof(float4);
        if (absent && (ps.shade[0].alloc(4 * n_tris) != hipSuccess || ps.shade[1].alloc(4 * n_tris) != hipSuccess)) {
            ps.drop_surfaces();
            (void)hipStreamSynchronize(c->stream);
            ps.valid = true;   // (the positions were taken)
            return fail(AGPT_ERR_NOMEM, f + ": out of device memory");
        }
        HIP_TRY(hipMemcpyAsync(ps.shade[ps.newest].p, s->d_tri_shade.p, bytes, hipMemcpyDeviceToDevice, c->stream));
        if (absent) HIP_TRY(hipMemcpyAsync(ps.shade[ps.newest ^ 1].p, s->d_tri_shade.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    ps.valid = true;
    ps.surfaces = surfaces;
    return AGPT_OK;
}

extern "C" {

int agpt_scene_snapshot_positions(agpt_scene* s) { return snapshot("agpt_scene_snapshot_positions", false, s); }

// agpt_scene_snapshot_positions plus two generations of the tri_shade records (PositionSnapshots::shade)
int agpt_scene_snapshot_surfaces(agpt_scene* s) { return snapshot("agpt_scene_snapshot_surfaces", true, s); }

}  // extern "C"
