// agpt_analytic.hip -- spheres, planes and lights of a committed scene moved in place (include/agpt.h): agpt_scene_update_sphere,
// agpt_scene_update_plane, agpt_scene_set_area_light_radiance, agpt_scene_set_infinite_light_radiance and
// agpt_scene_update_spheres_device, plus k_snapshot_analytic, the analytic half of agpt_scene_snapshot_positions (agpt_motion.hip).
//
// A sphere or a plane exists on the device as five floats of its DevPrim, a light's radiance as three floats of its DevLight; the trace
// kernels stage or read the primitives at every launch and the shading kernels copy both tables per launch, so the host calls rewrite
// those bytes with one small copy and the batch call with one lane per record.  Nothing else is derived from them: the prefilter, the
// top-level tree, the root pairs and mdiv_coords_ok cover meshes, the analytic masks and n_infinite depend on types only.
//   k_check_spheres    one lane per (cx, cy, cz, radius) record: one flag word set if any value is Inf or NaN or radius <= 0
//   k_update_spheres   one lane per record: prims[ids[i]].{cx, cy, cz, r, r2} = sphere_record(record i); the host has checked that the
//                      ids are distinct spheres of the scene, so no two lanes write one record
//   k_snapshot_analytic  one lane per primitive: its record into a generation (agpt_analytic.h)
// All three move a few KiB; their cost is the launch.  Compiled with the library's common flags (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "agpt_analytic.h"
#include "agpt_internal.h"

using agpt::fail;

__global__ void __launch_bounds__(AGPT_BLOCK)
k_check_spheres(const float4* __restrict__ records, uint32_t n, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const float4 q = records[i];
        bad = sphere_record_refused(q.x, q.y, q.z, q.w);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) *flag = 1u;   // (every wave that sees one stores the same word)
}

__global__ void __launch_bounds__(AGPT_BLOCK)
k_update_spheres(const float4* __restrict__ records, const int32_t* __restrict__ ids, uint32_t n, DevPrim* __restrict__ prims,
                 uint32_t n_prims) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = (uint32_t)ids[i];
    if (k >= n_prims) return;   // (no id of a checked list)
    const float4 q = records[i];
    const AnalyticRecord a = sphere_record(q.x, q.y, q.z, q.w);
    DevPrim& P = prims[k];
    P.cx = a.cx;
    P.cy = a.cy;
    P.cz = a.cz;
    P.r = a.r;
    P.r2 = a.r2;
}

__global__ void __launch_bounds__(AGPT_BLOCK)
k_snapshot_analytic(const DevPrim* __restrict__ prims, uint32_t n_prims, float4* __restrict__ gen) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_prims) return;
    const DevPrim& P = prims[k];
    gen[AGPT_ANALYTIC_GEN_STRIDE * (size_t)k] = make_float4(P.cx, P.cy, P.cz, P.r);
    gen[AGPT_ANALYTIC_GEN_STRIDE * (size_t)k + 1] = make_float4(P.r2, __uint_as_float((uint32_t)P.type), 0.f, 0.f);
}

namespace agpt {

void launch_snapshot_analytic(hipStream_t stream, const DevPrim* prims, uint32_t n_prims, float4* gen) {
    hipLaunchKernelGGL(k_snapshot_analytic, agpt_blocks(n_prims), dim3(AGPT_BLOCK), 0, stream, prims, n_prims, gen);
}

int download_spheres(agpt_scene* s) {
    if (!s->spheres_stale) return AGPT_OK;
    // the records of the last commit: primitives added since then (the scene is then uncommitted) have none, and keep their index
    std::vector<DevPrim> prims(std::min(s->prims.size(), (size_t)s->dev.n_prims));
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipMemcpyAsync(prims.data(), s->d_prims.p, prims.size() * sizeof(DevPrim), hipMemcpyDeviceToHost, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    for (size_t k = 0; k < prims.size(); k++)
        if (s->prims[k].type == AGPT_PRIM_SPHERE) {
            HostSphere& sp = s->spheres[(size_t)s->prims[k].index];
            sp.center = V3(prims[k].cx, prims[k].cy, prims[k].cz);
            sp.r = prims[k].r;
            sp.r2 = prims[k].r2;
        }
    s->spheres_stale = false;
    return AGPT_OK;
}

}  // namespace agpt

// the checks the host calls share, in the header's order: NULL arguments, a committed scene, a primitive of type `type`
static int check_prim(const std::string& f, const agpt_scene* s, const void* a, const void* b, int prim, int type, const char* what) {
    if (!s || !a || !b) return fail(AGPT_ERR_INVALID, f + "NULL argument");
    if (!s->committed) return fail(AGPT_ERR_INVALID, f + "the scene is not committed");
    if (prim < 0 || prim >= (int)s->prims.size() || s->prims[prim].type != type)
        return fail(AGPT_ERR_INVALID, f + "primitive " + std::to_string(prim) + " is not a " + what + " of this scene");
    return AGPT_OK;
}

// the host record and the five floats of d_prims[prim]
static int write_record(agpt_scene* s, int prim, const AnalyticRecord& a) {
    static_assert(offsetof(DevPrim, r2) == offsetof(DevPrim, cx) + 4 * sizeof(float) && sizeof(AnalyticRecord) == 5 * sizeof(float),
                  "cx, cy, cz, r, r2 are one run of DevPrim");
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(s->d_prims.p + prim) + offsetof(DevPrim, cx), &a, sizeof(a), hipMemcpyHostToDevice, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    agpt::HostSphere& sp = s->spheres[(size_t)s->prims[prim].index];
    sp.center = V3(a.cx, a.cy, a.cz);
    sp.r = a.r;
    sp.r2 = a.r2;
    return AGPT_OK;
}

static int write_radiance(agpt_scene* s, int light, const float L[3]) {
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(s->d_lights.p + light) + offsetof(DevLight, L), L, 3 * sizeof(float), hipMemcpyHostToDevice,
                           s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    s->lights[(size_t)light].L = V3(L[0], L[1], L[2]);
    return AGPT_OK;
}

extern "C" {

int agpt_scene_update_sphere(agpt_scene* s, int prim, const float center[3], float radius) {
    const std::string f = "agpt_scene_update_sphere: ";
    if (const int rc = check_prim(f, s, center, center, prim, AGPT_PRIM_SPHERE, "sphere")) return rc;
    if (sphere_record_refused(center[0], center[1], center[2], radius))
        return fail(AGPT_ERR_INVALID, f + "the centre and the radius must be finite and the radius positive");
    return write_record(s, prim, sphere_record(center[0], center[1], center[2], radius));
}

int agpt_scene_update_plane(agpt_scene* s, int prim, const float o[3], const float size[2]) {
    const std::string f = "agpt_scene_update_plane: ";
    if (const int rc = check_prim(f, s, o, size, prim, AGPT_PRIM_PLANE, "plane")) return rc;
    for (float x : {o[0], o[1], o[2], size[0], size[1]})
        if (!analytic_finite(x)) return fail(AGPT_ERR_INVALID, f + "the origin and the size must be finite");
    if (!(size[0] > 0.f) || !(size[1] > 0.f)) return fail(AGPT_ERR_INVALID, f + "the size must be positive");
    AnalyticRecord a;   // agpt_scene_add_plane's record: centre = O, r = HalfSize.x, r2 = HalfSize.y
    a.cx = o[0];
    a.cy = o[1];
    a.cz = o[2];
    a.r = size[0] / 2;
    a.r2 = size[1] / 2;
    return write_record(s, prim, a);
}

int agpt_scene_set_area_light_radiance(agpt_scene* s, int prim, const float L[3]) {
    const std::string f = "agpt_scene_set_area_light_radiance: ";
    if (const int rc = check_prim(f, s, L, L, prim, AGPT_PRIM_SPHERE, "sphere")) return rc;
    const int light = s->prims[prim].arealight;
    if (light < 0 || light >= (int)s->lights.size()) return fail(AGPT_ERR_INVALID, f + "primitive " + std::to_string(prim) + " has no area light");
    for (int j = 0; j < 3; j++)
        if (!analytic_finite(L[j])) return fail(AGPT_ERR_INVALID, f + "the radiance must be finite");
    return write_radiance(s, light, L);
}

int agpt_scene_set_infinite_light_radiance(agpt_scene* s, int light, const float L[3]) {
    const std::string f = "agpt_scene_set_infinite_light_radiance: ";
    if (!s || !L) return fail(AGPT_ERR_INVALID, f + "NULL argument");
    if (!s->committed) return fail(AGPT_ERR_INVALID, f + "the scene is not committed");
    if (light < 0 || light >= (int)s->lights.size() || s->lights[light].type != AGPT_LIGHT_UNIFORM_INFINITE)
        return fail(AGPT_ERR_INVALID, f + "light " + std::to_string(light) + " is not a uniform infinite light of this scene");
    for (int j = 0; j < 3; j++)
        if (!analytic_finite(L[j])) return fail(AGPT_ERR_INVALID, f + "the radiance must be finite");
    return write_radiance(s, light, L);
}

int agpt_scene_update_spheres_device(agpt_scene* s, const int32_t* prims, int n, const float* center_radius_dev) {
    const std::string f = "agpt_scene_update_spheres_device: ";
    if (!s || !prims || !center_radius_dev) return fail(AGPT_ERR_INVALID, f + "NULL argument");
    if (!s->committed) return fail(AGPT_ERR_INVALID, f + "the scene is not committed");
    if (n < 0) return fail(AGPT_ERR_INVALID, f + "n is negative");
    if (reinterpret_cast<uintptr_t>(center_radius_dev) & 15u) return fail(AGPT_ERR_INVALID, f + "center_radius_dev is not 16-byte aligned");
    {
        std::vector<char> seen(s->prims.size(), 0);
        for (int i = 0; i < n; i++) {
            const int k = prims[i];
            if (k < 0 || k >= (int)s->prims.size() || s->prims[k].type != AGPT_PRIM_SPHERE)
                return fail(AGPT_ERR_INVALID, f + "primitive " + std::to_string(k) + " is not a sphere of this scene");
            if (seen[k]) return fail(AGPT_ERR_INVALID, f + "primitive " + std::to_string(k) + " is listed twice");
            seen[k] = 1;
        }
    }
    if (n == 0) return AGPT_OK;
    if (s->prims.size() > s->d_prims.n) return fail(AGPT_ERR_DEVICE, f + "the scene's primitive records do not cover its primitives");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = s->d_sphere_ids.ensure((size_t)n)) return rc;
    if (const int rc = s->d_sphere_flag.ensure(1)) return rc;
    const float4* records = reinterpret_cast<const float4*>(center_radius_dev);
    uint32_t flag = 0;
    HIP_TRY(hipMemsetAsync(s->d_sphere_flag.p, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemcpyAsync(s->d_sphere_ids.p, prims, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_check_spheres, agpt_blocks((uint32_t)n), dim3(AGPT_BLOCK), 0, c->stream, records, (uint32_t)n, s->d_sphere_flag.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&flag, s->d_sphere_flag.p, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (`prims` has been read by now as well)
    if (flag) return fail(AGPT_ERR_INVALID, f + "a record has a non-finite value or a radius that is not positive");
    hipLaunchKernelGGL(k_update_spheres, agpt_blocks((uint32_t)n), dim3(AGPT_BLOCK), 0, c->stream, records, s->d_sphere_ids.p, (uint32_t)n,
                       s->d_prims.p, (uint32_t)s->prims.size());
    HIP_TRY(hipGetLastError());
    s->spheres_stale = true;   // (set before the wait: a failed wait leaves the device's state unknown, not the mirror current)
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

}  // extern "C"
