// agpt_kat.hip -- the known-answer entry points of include/agpt.h and their kernels: one piece of the device arithmetic each (the
// BSDF functions, the surface reconstruction and the normal-map perturbation of agpt_shade.h, the environment map's sampler and the environment light's three functions, the RNG streams), run on caller-supplied
// cases, one lane per case.  The exact arithmetic; the fast-arithmetic BSDF and environment-light kernels are compiled in their own unit
// (agpt_shade_kernels_fast.hip).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "agpt_internal.h"
#include "agpt_shade.h"

using agpt::fail;

// known-answer kernels (one lane per case)
__global__ void k_kat_bsdf_eval(DevScene sc, int material, int n, const float* __restrict__ wo3, const float* __restrict__ wi3,
                                float* __restrict__ f3o, float* __restrict__ pdfo) {
    kat_bsdf_eval_lane(sc, material, n, wo3, wi3, f3o, pdfo);
}
__global__ void k_kat_bsdf_sample(DevScene sc, int material, int n, const float* __restrict__ wo3, const float* __restrict__ u2,
                                  float* __restrict__ wi3o, float* __restrict__ f3o, float* __restrict__ pdfo,
                                  int32_t* __restrict__ speco) {
    kat_bsdf_sample_lane(sc, material, n, wo3, u2, wi3o, f3o, pdfo, speco);
}
// agpt_kat_env_light: env_Le, env_pdf_li and env_sample_li (agpt_shade.h) on one light's map, one lane per direction or draw
__global__ void k_kat_env_light(DevScene sc, int light, int n_dirs, const float* __restrict__ d3, float* __restrict__ le3o,
                                float* __restrict__ pdf_li_o, int n_draws, const float* __restrict__ u, float* __restrict__ wi3o,
                                float* __restrict__ pdfo, float* __restrict__ sle3o, int32_t* __restrict__ oko) {
    kat_env_light_lane(sc, light, n_dirs, d3, le3o, pdf_li_o, n_draws, u, wi3o, pdfo, sle3o, oko);
}
// known-answer kernel: Distribution1D::SampleContinuous (env_sample_continuous) for k draws, one lane each
// agpt_kat_normal_map: surface_apply_normal_map (agpt_shade.h) alone, one lane per item
__global__ void k_kat_normal_map(int n, const float* __restrict__ ns3, const float* __restrict__ ss3, const float* __restrict__ rgb3, float scale,
                                 float* __restrict__ out3) {
    kat_normal_map_lane(n, ns3, ss3, rgb3, scale, out3);
}
__global__ void k_kat_distribution1d(DevEnv e, const float* __restrict__ u, int k, float* __restrict__ x_out, float* __restrict__ pdf_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    float pdf;
    x_out[i] = env_sample_continuous(e, u[i], &pdf);
    pdf_out[i] = pdf;
}
__global__ void k_kat_rng(uint32_t pixel, uint32_t wh, uint32_t sample, uint32_t seed_base, int n, float* __restrict__ out,
                          uint32_t* __restrict__ seed_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t s = sample_seed(pixel, wh, sample, seed_base);
    *seed_out = s;
    for (int i = 0; i < n; i++) out[i] = rng_float(s);
}

// agpt_kat_surface: surface_from_triangle (agpt_shade.h) alone on the records at tri_shade -- the scene's, or a generation of
// agpt_scene_snapshot_surfaces --, one lane per item; the ray (origin 0, direction +z, t = 1) reaches p and wo only, which are not returned
__global__ void k_kat_surface(DevScene sc, const float4* __restrict__ tri_shade, int n, const uint32_t* __restrict__ tri_ids,
                              const float* __restrict__ b1, const float* __restrict__ b2, float* __restrict__ ns3, float* __restrict__ ss3) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DevScene from = sc;
    from.tri_shade = tri_shade;
    Surface s;
    surface_from_triangle(from, tri_ids[i], b1[i], b2[i], V3s(0.f), V3(0.f, 0.f, 1.f), 1.f, s);
    ns3[3 * i] = s.ns.x; ns3[3 * i + 1] = s.ns.y; ns3[3 * i + 2] = s.ns.z;
    ss3[3 * i] = s.ss_bsdf.x; ss3[3 * i + 1] = s.ss_bsdf.y; ss3[3 * i + 2] = s.ss_bsdf.z;
}

// what follows every launch here: its launch error, then its completion
static int launched(agpt_ctx* c) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AGPT_OK;
}

extern "C" {

int agpt_kat_bsdf_eval(agpt_scene* s, int material, int n, const float* wo3, const float* wi3, float* f3_out, float* pdf_out) {
    if (!s || !s->committed || material < 0 || material >= (int)s->materials.size() || n <= 0 || !wo3 || !wi3 || !f3_out || !pdf_out)
        return fail(AGPT_ERR_INVALID, "agpt_kat_bsdf_eval: bad argument");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_wo, d_wi, d_f, d_p;
    int rc;
    if ((rc = d_wo.in(wo3, 3 * (size_t)n)) || (rc = d_wi.in(wi3, 3 * (size_t)n))) return rc;
    HIP_TRY(d_f.alloc(3 * (size_t)n));
    HIP_TRY(d_p.alloc((size_t)n));
    if (s->shading_arith == AGPT_SHADING_FAST)
        agpt::launch_kat_bsdf_eval_fast(c->stream, s->dev, material, n, d_wo.p, d_wi.p, d_f.p, d_p.p);
    else
        hipLaunchKernelGGL(k_kat_bsdf_eval, dim3((n + 63) / 64), dim3(64), 0, c->stream, s->dev, material, n, d_wo.p, d_wi.p, d_f.p, d_p.p);
    if ((rc = launched(c)) || (rc = d_f.out(f3_out, 3 * (size_t)n))) return rc;
    return d_p.out(pdf_out, (size_t)n);
}

int agpt_kat_bsdf_sample(agpt_scene* s, int material, int n, const float* wo3, const float* u2, float* wi3_out, float* f3_out,
                         float* pdf_out, int32_t* specular_out) {
    if (!s || !s->committed || material < 0 || material >= (int)s->materials.size() || n <= 0 || !wo3 || !u2 || !wi3_out ||
        !f3_out || !pdf_out || !specular_out)
        return fail(AGPT_ERR_INVALID, "agpt_kat_bsdf_sample: bad argument");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_wo, d_u, d_wi, d_f, d_p;
    DevBuf<int32_t> d_s;
    int rc;
    if ((rc = d_wo.in(wo3, 3 * (size_t)n)) || (rc = d_u.in(u2, 2 * (size_t)n))) return rc;
    HIP_TRY(d_wi.alloc(3 * (size_t)n));
    HIP_TRY(d_f.alloc(3 * (size_t)n));
    HIP_TRY(d_p.alloc((size_t)n));
    HIP_TRY(d_s.alloc((size_t)n));
    if (s->shading_arith == AGPT_SHADING_FAST)
        agpt::launch_kat_bsdf_sample_fast(c->stream, s->dev, material, n, d_wo.p, d_u.p, d_wi.p, d_f.p, d_p.p, d_s.p);
    else
        hipLaunchKernelGGL(k_kat_bsdf_sample, dim3((n + 63) / 64), dim3(64), 0, c->stream, s->dev, material, n, d_wo.p, d_u.p, d_wi.p, d_f.p,
                           d_p.p, d_s.p);
    if ((rc = launched(c)) || (rc = d_wi.out(wi3_out, 3 * (size_t)n)) || (rc = d_f.out(f3_out, 3 * (size_t)n)) ||
        (rc = d_p.out(pdf_out, (size_t)n)))
        return rc;
    return d_s.out(specular_out, (size_t)n);
}

int agpt_kat_env_light(agpt_scene* s, int light, int n_dirs, const float* d3, float* le3_out, float* pdf_li_out, int n_draws, const float* u,
                       float* wi3_out, float* pdf_out, float* sample_le3_out, int32_t* ok_out) {
    if (!s || !s->committed || light < 0 || light >= (int)s->lights.size() || n_dirs < 0 || n_draws < 0 || n_dirs + (long long)n_draws <= 0 ||
        n_dirs + (long long)n_draws > (1 << 28) || (n_dirs && (!d3 || !le3_out || !pdf_li_out)) ||
        (n_draws && (!u || !wi3_out || !pdf_out || !sample_le3_out || !ok_out)))
        return fail(AGPT_ERR_INVALID, "agpt_kat_env_light: bad argument");
    const agpt::HostLight& hl = s->lights[light];
    if (hl.type != AGPT_LIGHT_INFINITE_AREA || hl.env < 0 || hl.env >= (int)s->envs.size())
        return fail(AGPT_ERR_INVALID, "agpt_kat_env_light: the light is no infinite-area light");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_d, d_le, d_pl, d_u, d_wi, d_p, d_sle;
    DevBuf<int32_t> d_ok;
    int rc;
    if (n_dirs) {
        if ((rc = d_d.in(d3, 3 * (size_t)n_dirs))) return rc;
        HIP_TRY(d_le.alloc(3 * (size_t)n_dirs));
        HIP_TRY(d_pl.alloc((size_t)n_dirs));
    }
    if (n_draws) {
        if ((rc = d_u.in(u, (size_t)n_draws))) return rc;
        HIP_TRY(d_wi.alloc(3 * (size_t)n_draws));
        HIP_TRY(d_p.alloc((size_t)n_draws));
        HIP_TRY(d_sle.alloc(3 * (size_t)n_draws));
        HIP_TRY(d_ok.alloc((size_t)n_draws));
    }
    const int n = n_dirs + n_draws;
    if (s->shading_arith == AGPT_SHADING_FAST)
        agpt::launch_kat_env_light_fast(c->stream, s->dev, light, n_dirs, d_d.p, d_le.p, d_pl.p, n_draws, d_u.p, d_wi.p, d_p.p, d_sle.p, d_ok.p);
    else
        hipLaunchKernelGGL(k_kat_env_light, dim3((n + 63) / 64), dim3(64), 0, c->stream, s->dev, light, n_dirs, d_d.p, d_le.p, d_pl.p, n_draws,
                           d_u.p, d_wi.p, d_p.p, d_sle.p, d_ok.p);
    if ((rc = launched(c))) return rc;
    if (n_dirs && ((rc = d_le.out(le3_out, 3 * (size_t)n_dirs)) || (rc = d_pl.out(pdf_li_out, (size_t)n_dirs)))) return rc;
    if (n_draws && ((rc = d_wi.out(wi3_out, 3 * (size_t)n_draws)) || (rc = d_p.out(pdf_out, (size_t)n_draws)) ||
                    (rc = d_sle.out(sample_le3_out, 3 * (size_t)n_draws)) || (rc = d_ok.out(ok_out, (size_t)n_draws))))
        return rc;
    return AGPT_OK;
}

int agpt_kat_normal_map(agpt_ctx* c, int n, const float* ns3, const float* ss3, const float* rgb3, float scale, float* ns_out3) {
    if (!c || n <= 0 || !ns3 || !ss3 || !rgb3 || !ns_out3) return fail(AGPT_ERR_INVALID, "agpt_kat_normal_map: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_ns, d_ss, d_rgb, d_o;
    int rc;
    if ((rc = d_ns.in(ns3, 3 * (size_t)n)) || (rc = d_ss.in(ss3, 3 * (size_t)n)) || (rc = d_rgb.in(rgb3, 3 * (size_t)n))) return rc;
    HIP_TRY(d_o.alloc(3 * (size_t)n));
    hipLaunchKernelGGL(k_kat_normal_map, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, d_ns.p, d_ss.p, d_rgb.p, scale, d_o.p);
    if ((rc = launched(c))) return rc;
    return d_o.out(ns_out3, 3 * (size_t)n);
}

int agpt_kat_surface(agpt_scene* s, int generation, int n, const uint32_t* tri_ids, const float* b1, const float* b2, float* ns3_out,
                     float* ss3_out) {
    if (!s || !s->committed || generation < -1 || generation > 1 || n <= 0 || !tri_ids || !b1 || !b2 || !ns3_out || !ss3_out)
        return fail(AGPT_ERR_INVALID, "agpt_kat_surface: bad argument");
    size_t n_tris = 0;
    for (const agpt::HostMesh& m : s->meshes) n_tris += m.prim_index.size();
    const agpt_scene::PositionSnapshots& ps = s->snapshots;
    const float4* records = s->d_tri_shade.p;
    if (generation >= 0) {
        if (!ps.surfaces || !n_tris) return fail(AGPT_ERR_INVALID, "agpt_kat_surface: the scene has no such generation of shading records");
        records = ps.shade[ps.newest ^ generation].p;
    }
    if (4 * n_tris > s->d_tri_shade.n) return fail(AGPT_ERR_DEVICE, "agpt_kat_surface: the scene's records do not cover its meshes");
    for (int i = 0; i < n; i++)
        if (tri_ids[i] >= n_tris) return fail(AGPT_ERR_INVALID, "agpt_kat_surface: triangle id out of range");
    agpt_ctx* c = s->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> d_id;
    DevBuf<float> d_b1, d_b2, d_ns, d_ss;
    int rc;
    if ((rc = d_id.in(tri_ids, (size_t)n)) || (rc = d_b1.in(b1, (size_t)n)) || (rc = d_b2.in(b2, (size_t)n))) return rc;
    HIP_TRY(d_ns.alloc(3 * (size_t)n));
    HIP_TRY(d_ss.alloc(3 * (size_t)n));
    hipLaunchKernelGGL(k_kat_surface, dim3((n + 63) / 64), dim3(64), 0, c->stream, s->dev, records, n, d_id.p, d_b1.p, d_b2.p, d_ns.p, d_ss.p);
    if ((rc = launched(c)) || (rc = d_ns.out(ns3_out, 3 * (size_t)n))) return rc;
    return d_ss.out(ss3_out, 3 * (size_t)n);
}

int agpt_kat_rng(agpt_ctx* c, uint32_t pixel, uint32_t wh, uint32_t sample, uint32_t seed_base, int n, float* out,
                 uint32_t* seed_out) {
    if (!c || n <= 0 || !out || !seed_out) return fail(AGPT_ERR_INVALID, "agpt_kat_rng: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_o;
    DevBuf<uint32_t> d_s;
    HIP_TRY(d_o.alloc((size_t)n));
    HIP_TRY(d_s.alloc(1));
    hipLaunchKernelGGL(k_kat_rng, dim3(1), dim3(64), 0, c->stream, pixel, wh, sample, seed_base, n, d_o.p, d_s.p);
    int rc;
    if ((rc = launched(c)) || (rc = d_o.out(out, (size_t)n))) return rc;
    return d_s.out(seed_out, 1);
}

int agpt_kat_distribution1d(agpt_ctx* c, const float* func, int n, const float* u, int k, float* cdf_out, float* func_int_out,
                            float* x_out, float* pdf_out) {
    if (!c || !func || n <= 0 || k < 0 || (k && (!u || !x_out || !pdf_out)))
        return fail(AGPT_ERR_INVALID, "agpt_kat_distribution1d: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float> cdf((size_t)n + 1);
    const float func_int = agpt::build_distribution1d(func, n, cdf.data());
    if (cdf_out) memcpy(cdf_out, cdf.data(), 4 * cdf.size());
    if (func_int_out) *func_int_out = func_int;
    if (k == 0) return AGPT_OK;
    DevBuf<float> d_f, d_c, d_u, d_x, d_p;
    int rc;
    if ((rc = d_f.in(func, (size_t)n)) || (rc = d_c.in(cdf.data(), cdf.size())) || (rc = d_u.in(u, (size_t)k))) return rc;
    HIP_TRY(d_x.alloc((size_t)k));
    HIP_TRY(d_p.alloc((size_t)k));
    DevEnv e{};
    e.func = d_f.p;
    e.cdf = d_c.p;
    e.n = n;
    e.funcInt = func_int;
    hipLaunchKernelGGL(k_kat_distribution1d, dim3((k + 63) / 64), dim3(64), 0, c->stream, e, d_u.p, k, d_x.p, d_p.p);
    if ((rc = launched(c)) || (rc = d_x.out(x_out, (size_t)k))) return rc;
    return d_p.out(pdf_out, (size_t)k);
}

// the two front-end kernels of the device-pointer mesh calls (agpt_update.hip), launched as MeshUpdate::device_inputs launches them
int agpt_kat_skin_palette(agpt_ctx* c, const float* joints16, int n_joints, int with_normals, float* palette_out, uint32_t status_out[3]) {
    if (!c || !joints16 || n_joints < 1 || n_joints > agpt::kSkinMaxJoints || !palette_out || !status_out)
        return fail(AGPT_ERR_INVALID, "agpt_kat_skin_palette: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)n_joints * (size_t)agpt::skin_palette_stride(with_normals != 0);
    DevBuf<float> d_j, d_p;
    DevBuf<uint32_t> d_s;
    int rc;
    if ((rc = d_j.in(joints16, 16 * (size_t)n_joints))) return rc;
    HIP_TRY(d_p.alloc(n));
    HIP_TRY(d_s.alloc(3));
    HIP_TRY(hipMemsetAsync(d_s.p, 0xFF, 3 * sizeof(uint32_t), c->stream));
    if ((rc = agpt::launch_pack_palette(c->stream, d_j.p, n_joints, with_normals != 0, d_p.p, d_s.p)) || (rc = launched(c)) ||
        (rc = d_p.out(palette_out, n)))
        return rc;
    return d_s.out(status_out, 3);
}

int agpt_kat_morph_active(agpt_ctx* c, const float* weights, int n_targets, int32_t* targets_out, float* weights_out, uint32_t status_out[2]) {
    if (!c || !weights || n_targets < 1 || n_targets > agpt::kMorphMaxTargets || !targets_out || !weights_out || !status_out)
        return fail(AGPT_ERR_INVALID, "agpt_kat_morph_active: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<float> d_w;
    DevBuf<agpt::MorphActive> d_a;
    DevBuf<uint32_t> d_s;
    int rc;
    if ((rc = d_w.in(weights, (size_t)n_targets))) return rc;
    HIP_TRY(d_a.alloc((size_t)n_targets));
    HIP_TRY(d_s.alloc(2));
    if ((rc = agpt::launch_morph_active(c->stream, d_w.p, n_targets, d_a.p, d_s.p)) || (rc = launched(c)) || (rc = d_s.out(status_out, 2))) return rc;
    if (status_out[0] > (uint32_t)n_targets) return fail(AGPT_ERR_DEVICE, "agpt_kat_morph_active: the kernel reports more pairs than targets");
    std::vector<agpt::MorphActive> active(status_out[0]);
    if (!active.empty())
        if ((rc = d_a.out(active.data(), active.size()))) return rc;
    for (size_t k = 0; k < active.size(); k++) {
        targets_out[k] = active[k].target;
        weights_out[k] = active[k].weight;
    }
    return AGPT_OK;
}

}  // extern "C"
