// oracle/ref_hotpath.cpp -- TEST INFRASTRUCTURE ONLY (never linked by the product).
//
// Harness around the reference's own hot path, compiled from where it lies (`make -C oracle ref`, output oracle/_ref/libref_hotpath.so):
// template/precomp.h, disney.h, integrator.h, bvhtrimesh.h, texture.h, scene.h and sampling.h are included here unmodified, and
// reflection.cpp, Intersectable.cpp, lights.cpp and trianglemesh.cpp are compiled as translation units of their own (precomp.h has no
// include guard).  The platform headers precomp.h includes unconditionally are the empty-or-nearly-empty files of oracle/ref_standins.
// This file only CALLS the reference's classes (DisneyMaterial, MirrorMaterial, BSDF, BVHTriMesh, Sphere, Plane, Scene, Camera,
// PathTracer, DbgIntegrator, the lights -- InfiniteAreaLight's Le, Pdf_Li and Sample_Li also one by one, ref_env_* --,
// TriangleMesh::CreateBackdrop); it restates none of their bodies.  Where a value is a protected
// member, a derived class with an accessor reads it.  tests/golden/make_refpin_golden.py turns its outputs into tests/golden/refpin_*.npz,
// tests/golden/make_envlight_golden.py into tests/golden/envlight_cases.npz.
//
// What the harness itself supplies, because the reference gets it from files that are not compiled here:
//   RandomUInt / RandomFloat   (template.cpp, full of GL): xorshift32 on the state the caller passes per ray, or draws from a
//                              caller-supplied array; draws are counted
//   sinf / cosf / acosf / atan2f: the four functions oracle.c's trig switch covers.  The library is built with -fno-builtin and linked
//                              with -Bsymbolic-functions, so every call the reference makes lands here; mode 0 forwards to the C
//                              library's function, mode 1 returns the correctly rounded value through fp64 (what the kernels compute)
//   a material with ONE DisneyDiffuse lobe (MAT_DIFFUSE_ONLY): the reference has no such Material class; its lobe and BSDF are used
#define STB_IMAGE_IMPLEMENTATION
#define TINYOBJLOADER_IMPLEMENTATION
#define TINYOBJLOADER_USE_MAPBOX_EARCUT
#include "precomp.h"
#include "disney.h"
#include "integrator.h"
#include "bvhtrimesh.h"
#include "texture.h"
#include "sampling.h"

#include <dlfcn.h>
#include <stdint.h>

// ---- trig switch ------------------------------------------------------------------------------------------------------------------
static int g_trig_mode = 0;
typedef float (*f1_t)(float);
typedef float (*f2_t)(float, float);
template <class T> static T next_symbol(const char* name) {
    T f = (T)dlsym(RTLD_NEXT, name);
    if (!f) { fprintf(stderr, "ref_hotpath: the C library has no %s\n", name); abort(); }
    return f;
}
extern "C" {
float sinf(float x) noexcept { static f1_t f = next_symbol<f1_t>("sinf"); return g_trig_mode ? (float)::sin((double)x) : f(x); }
float cosf(float x) noexcept { static f1_t f = next_symbol<f1_t>("cosf"); return g_trig_mode ? (float)::cos((double)x) : f(x); }
float acosf(float x) noexcept { static f1_t f = next_symbol<f1_t>("acosf"); return g_trig_mode ? (float)::acos((double)x) : f(x); }
float atan2f(float y, float x) noexcept {
    static f2_t f = next_symbol<f2_t>("atan2f");
    return g_trig_mode ? (float)::atan2((double)y, (double)x) : f(y, x);
}
}

// ---- random numbers ---------------------------------------------------------------------------------------------------------------
static uint32_t g_rng_state = 0x12345678u;
static const float* g_draw_array = nullptr;
static int g_draw_count = 0;
static long long g_draws_used = 0;

uint RandomUInt() {
    uint32_t x = g_rng_state;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    g_rng_state = x;
    g_draws_used++;
    return x;
}
float RandomFloat() {
    if (g_draw_array) {
        long long i = g_draws_used++;
        return i < g_draw_count ? g_draw_array[i] : 0.f;
    }
    return RandomUInt() * 2.3283064365387e-10f;
}

// ---- accessors to protected members -----------------------------------------------------------------------------------------------
namespace {

struct PeekTriMesh : TriangleMesh {
    using TriangleMesh::TriangleMesh;
    bool Tri(const Ray& ray, int tridx, SurfaceInteraction& hit) const { return TriangleIntersect(ray, tridx, hit); }
    const vector<float3>& V() const { return vertices; }
    const vector<float3>& N() const { return normals; }
    const vector<float2>& T() const { return texcoords; }
    const vector<index_type>& I() const { return indices; }
};

struct PeekBVH : BVHTriMesh {
    using BVHTriMesh::BVHTriMesh;
    bool Tri(const Ray& ray, int tridx, SurfaceInteraction& hit) const { return TriangleIntersect(ray, tridx, hit); }
    int NumPrims() const { return (int)primitives.size(); }
    int PrimIndex(int i) const { return primitives[i].index; }
    const BVHNode* Nodes() const { return nodes; }
};

struct PeekCamera : Camera {
    using Camera::Camera;
    void Vectors(float out[22]) const {
        const float3 v3[7] = {origin, u, v, w, lower_left_corner, horizontal, vertical};
        for (int i = 0; i < 7; i++) { out[3 * i] = v3[i].x; out[3 * i + 1] = v3[i].y; out[3 * i + 2] = v3[i].z; }
        out[21] = lens_radius;
    }
};

// MAT_DIFFUSE_ONLY: one DisneyDiffuse lobe of the given colour
struct DiffuseOnlyMaterial : Material {
    DiffuseOnlyMaterial(const float3& c) : lobe(make_shared<DisneyDiffuse>(c)) {}
    void SetupBSDF(BSDF* bsdf) const { bsdf->AddBxDF(lobe.get()); }
    shared_ptr<DisneyDiffuse> lobe;
};

// never hit; placed in front of Scene::primitives while Li runs, it sees every Scene::Intersect and every Scene::IntersectP call
struct CallCounter : Intersectable {
    CallCounter() : Intersectable(nullptr) {}
    bool Intersect(const Ray&, SurfaceInteraction&) const { closest++; return false; }
    bool IntersectP(const Ray&) const { any++; return false; }
    mutable long long closest = 0, any = 0;
};

struct RefScene {
    Scene scene;
    vector<shared_ptr<Material>> materials;
    vector<PeekBVH*> mesh_of_prim;              // per scene primitive, nullptr for spheres and planes
    vector<shared_ptr<PeekTriMesh>> bary_twin;  // per scene primitive: the same triangles with texcoords that make uv = (b1, b2)
    bool has_camera = false;
};

struct ref_ray { float o[3]; float d[3]; float tmax; };
struct ref_hit { int32_t hit, prim, tri; float t, b1, b2; };
struct ref_node { float bmin[3]; float bmax[3]; int32_t first, count; };

float3 F3(const float* p) { return float3(p[0], p[1], p[2]); }
Ray make_ray(const ref_ray& r) { return Ray(F3(r.o), F3(r.d), r.tmax); }
uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
bool same3(const float3& a, const float3& b) { return bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y) && bits(a.z) == bits(b.z); }

shared_ptr<TriangleMesh> mesh_from_arrays(const float* verts, int n_verts, const float* normals, int n_normals, const float* uvs,
                                          int n_uvs, const int32_t* indices, int n_indices, shared_ptr<Material> mat) {
    vector<float3> v, n;
    vector<float2> t;
    vector<index_type> ix;
    for (int i = 0; i < n_verts; i++) v.push_back(F3(verts + 3 * i));
    for (int i = 0; i < n_normals; i++) n.push_back(F3(normals + 3 * i));
    for (int i = 0; i < n_uvs; i++) t.push_back(float2(uvs[2 * i], uvs[2 * i + 1]));
    for (int i = 0; i < n_indices; i++) ix.push_back(index_type(indices[3 * i], indices[3 * i + 1], indices[3 * i + 2]));
    return make_shared<TriangleMesh>(ix, v, n, t, mat);
}

struct QuietCerr {   // BVHTriMesh's constructor reports its timings on cerr
    QuietCerr() { cerr.setstate(ios_base::failbit); }
} quiet_cerr;

}  // namespace

extern "C" {

void ref_set_trig_mode(int mode) { g_trig_mode = mode; }
// draws from an array instead of the xorshift32 stream (nullptr: back to the stream); ref_draws_used() counts from this call on
void ref_set_draws(const float* draws, int n) { g_draw_array = draws; g_draw_count = n; g_draws_used = 0; }
long long ref_draws_used(void) { return g_draws_used; }
// first floats of the stand-in stream (the reference's first RandomFloat() is pinned in tests/test_oracle_pins.py)
void ref_rng_floats(uint32_t seed, int n, float* out) {
    g_rng_state = seed;
    for (int i = 0; i < n; i++) out[i] = RandomFloat();
}
// TrowbridgeReitzSample11 (microfacet.h:34-42) at normal incidence with U1 = .5: r = 1, so out = (cos(phi), sin(phi)), phi = 2 pi U2
void ref_trig_probe(float u2, float out[2]) { TrowbridgeReitzSample11(1.f, .5f, u2, &out[0], &out[1]); }

void* ref_scene_new(void) { return new RefScene(); }
void ref_scene_free(void* s) { delete (RefScene*)s; }

int ref_add_material(void* s_, int type, const float color[3], float roughness, float metallic) {
    RefScene* s = (RefScene*)s_;
    if (type == 0) s->materials.push_back(DisneyMaterial::Make(F3(color), roughness, metallic));
    else if (type == 1) s->materials.push_back(MirrorMaterial::Make(F3(color)));
    else s->materials.push_back(make_shared<DiffuseOnlyMaterial>(F3(color)));
    return (int)s->materials.size() - 1;
}

static int push_prim(RefScene* s, shared_ptr<Intersectable> p, PeekBVH* mesh, shared_ptr<PeekTriMesh> twin) {
    s->scene.primitives.push_back(p);
    s->mesh_of_prim.push_back(mesh);
    s->bary_twin.push_back(twin);
    return (int)s->scene.primitives.size() - 1;
}

int ref_add_mesh(void* s_, const float* verts, int n_verts, const float* normals, int n_normals, const float* uvs, int n_uvs,
                 const int32_t* indices, int n_indices, int material, int max_prims_in_node) {
    RefScene* s = (RefScene*)s_;
    shared_ptr<Material> mat = material >= 0 ? s->materials[material] : nullptr;
    auto bvh = make_shared<PeekBVH>(mesh_from_arrays(verts, n_verts, normals, n_normals, uvs, n_uvs, indices, n_indices, mat), mat,
                                    max_prims_in_node);
    // twin: the same vertices, no normals, texcoords (0,0) (1,0) (0,1) at the three corners of every triangle, so that
    // TriangleIntersect's interpolated uv (trianglemesh.cpp:57) is uv0*b0 + uv1*b1 + uv2*b2 = (b1, b2)
    vector<float3> v;
    vector<float3> none;
    vector<float2> t = {float2(0, 0), float2(1, 0), float2(0, 1)};
    vector<index_type> ix;
    for (int i = 0; i < n_verts; i++) v.push_back(F3(verts + 3 * i));
    for (int i = 0; i < n_indices; i++) ix.push_back(index_type(indices[3 * i], 0, i % 3));
    auto twin = make_shared<PeekTriMesh>(ix, v, none, t, mat);
    return push_prim(s, bvh, bvh.get(), twin);
}
int ref_add_sphere(void* s_, const float center[3], float radius, int material) {
    RefScene* s = (RefScene*)s_;
    return push_prim(s, make_shared<Sphere>(F3(center), radius, material >= 0 ? s->materials[material] : nullptr), nullptr, nullptr);
}
int ref_add_plane(void* s_, const float o[3], const float size[2], int material) {
    RefScene* s = (RefScene*)s_;
    return push_prim(s, make_shared<Plane>(F3(o), float2(size[0], size[1]), material >= 0 ? s->materials[material] : nullptr), nullptr,
                     nullptr);
}
int ref_add_area_light(void* s_, const float center[3], float radius, const float L[3]) {
    RefScene* s = (RefScene*)s_;
    s->scene.addAreaLight(make_shared<Sphere>(F3(center), radius, nullptr), F3(L));
    s->mesh_of_prim.push_back(nullptr);
    s->bary_twin.push_back(nullptr);
    return (int)s->scene.primitives.size() - 1;
}
int ref_add_uniform_infinite_light(void* s_, const float L[3]) {
    RefScene* s = (RefScene*)s_;
    s->scene.lights.push_back(make_shared<UniformInfiniteLight>(F3(L)));
    return (int)s->scene.lights.size() - 1;
}
// InfiniteAreaLight(texmap): the reference loads the image itself (HDRTexture, stbi_loadf)
int ref_add_infinite_area_light(void* s_, const char* hdr_path) {
    RefScene* s = (RefScene*)s_;
    s->scene.lights.push_back(make_shared<InfiniteAreaLight>(string(hdr_path)));
    return (int)s->scene.lights.size() - 1;
}
// the pixels HDRTexture gets from the same file: rgb_out[w * h * 3]; returns 0 when the file cannot be read or is larger than cap
int ref_load_hdr(const char* hdr_path, int* w, int* h, float* rgb_out, int cap_pixels) {
    int n = 0;
    float* data = stbi_loadf(hdr_path, w, h, &n, 0);
    if (!data) return 0;
    int ok = (*w) * (*h) <= cap_pixels && n >= 3;
    if (ok)
        for (int i = 0; i < (*w) * (*h); i++)
            for (int c = 0; c < 3; c++) rgb_out[3 * i + c] = data[i * n + c];
    stbi_image_free(data);
    return ok;
}
void ref_set_camera(void* s_, const float lookfrom[3], const float lookat[3], const float vup[3], float aspect_ratio, float vfov,
                    float aperture) {
    RefScene* s = (RefScene*)s_;
    s->scene.camera.lookfrom = F3(lookfrom);
    s->scene.camera.lookat = F3(lookat);
    s->scene.camera.vup = F3(vup);
    s->scene.camera.aspect_ratio = aspect_ratio;
    s->scene.camera.vfov = vfov;
    s->scene.camera.aperture = aperture;
    s->has_camera = true;
}

// ---- BSDF: frame convention of agpt_kat_bsdf_eval / agpt_kat_bsdf_sample (ng = ns = +z, ss = +x) -------------------------------------
static BSDF canonical_bsdf(RefScene* s, int material, const Intersectable* shape) {
    SurfaceInteraction si(float3(0.f), float2(0, 0), float3(0, 0, 1), float3(1, 0, 0), float3(0, 1, 0), shape);
    BSDF b(si);
    s->materials[material]->SetupBSDF(&b);
    return b;
}
// BSDF::f and BSDF::Pdf with skipSpecular = true (the calls of EstimateDirect, integrator.h:46-47)
void ref_bsdf_eval(void* s_, int material, int n, const float* wo, const float* wi, float* f_out, float* pdf_out) {
    RefScene* s = (RefScene*)s_;
    Sphere shape(float3(0.f), 1.f, s->materials[material]);
    BSDF b = canonical_bsdf(s, material, &shape);
    for (int i = 0; i < n; i++) {
        float3 f = b.f(F3(wo + 3 * i), F3(wi + 3 * i), true);
        f_out[3 * i] = f.x; f_out[3 * i + 1] = f.y; f_out[3 * i + 2] = f.z;
        pdf_out[i] = b.Pdf(F3(wo + 3 * i), F3(wi + 3 * i), true);
    }
}
// BSDF::Sample_f with skipSpecular = false (the call of PathTracer::Li, integrator.h:174); wi and pdf start at 0
void ref_bsdf_sample(void* s_, int material, int n, const float* wo, const float* u, float* wi_out, float* f_out, float* pdf_out,
                     int32_t* specular_out) {
    RefScene* s = (RefScene*)s_;
    Sphere shape(float3(0.f), 1.f, s->materials[material]);
    BSDF b = canonical_bsdf(s, material, &shape);
    for (int i = 0; i < n; i++) {
        float3 wi(0.f);
        float pdf = 0;
        bool spec = false;
        float3 f = b.Sample_f(F3(wo + 3 * i), &wi, float2(u[2 * i], u[2 * i + 1]), &pdf, false, &spec);
        wi_out[3 * i] = wi.x; wi_out[3 * i + 1] = wi.y; wi_out[3 * i + 2] = wi.z;
        f_out[3 * i] = f.x; f_out[3 * i + 1] = f.y; f_out[3 * i + 2] = f.z;
        pdf_out[i] = pdf;
        specular_out[i] = spec ? 1 : 0;
    }
}

// ---- Scene::Intersect / Scene::IntersectP ---------------------------------------------------------------------------------------------
// SurfaceInteraction carries the shape, the point and uv, not the triangle or its barycentrics.  For a mesh hit those are recovered by
// calling the reference's own TriangleIntersect on every triangle of the hit mesh with a ray that ends one ulp beyond the hit: the
// triangle that returns the hit's t and the hit's p, uv, n and shading normal is the one; b1, b2 are the uv the twin mesh returns for it.
// ambiguous_out[i] = number of triangles that qualify, minus one (0 for every unambiguous row); -1 where the twin disagrees.
void ref_intersect(void* s_, const ref_ray* rays, int n, ref_hit* out, float* uv_out, int32_t* ambiguous_out, int any_hit) {
    RefScene* s = (RefScene*)s_;
    for (int i = 0; i < n; i++) {
        ref_hit* h = &out[i];
        memset(h, 0, sizeof(*h));
        h->prim = -1; h->tri = -1;
        uv_out[2 * i] = uv_out[2 * i + 1] = 0;
        ambiguous_out[i] = 0;
        Ray ray = make_ray(rays[i]);
        if (any_hit) {
            h->hit = s->scene.IntersectP(ray) ? 1 : 0;
            continue;
        }
        SurfaceInteraction si;
        if (!s->scene.Intersect(ray, si)) continue;
        h->hit = 1;
        h->t = ray.t;
        uv_out[2 * i] = si.uv.x; uv_out[2 * i + 1] = si.uv.y;
        for (size_t k = 0; k < s->scene.primitives.size(); k++)
            if (s->scene.primitives[k].get() == si.shape) h->prim = (int)k;
        PeekBVH* mesh = h->prim >= 0 ? s->mesh_of_prim[h->prim] : nullptr;
        if (!mesh) continue;
        int found = 0;
        for (int j = 0; j < mesh->NumPrims(); j++) {
            Ray probe = ray;
            probe.t = nextafterf(ray.t, INFINITY);
            SurfaceInteraction cand;
            if (!mesh->Tri(probe, 3 * j, cand) || bits(probe.t) != bits(ray.t)) continue;
            if (!same3(cand.p, si.p) || !same3(cand.n, si.n) || !same3(cand.shading.n, si.shading.n) ||
                bits(cand.uv.x) != bits(si.uv.x) || bits(cand.uv.y) != bits(si.uv.y))
                continue;
            if (found++ == 0) {
                h->tri = 3 * j;
                Ray probe2 = ray;
                probe2.t = nextafterf(ray.t, INFINITY);
                SurfaceInteraction bary;
                if (s->bary_twin[h->prim]->Tri(probe2, 3 * j, bary) && bits(probe2.t) == bits(ray.t)) {
                    h->b1 = bary.uv.x; h->b2 = bary.uv.y;
                } else {
                    ambiguous_out[i] = -1;
                }
            }
        }
        if (ambiguous_out[i] == 0) ambiguous_out[i] = found - 1;
    }
}
// DbgIntegrator::Li: the hit's uv as a colour
void ref_dbg_li(void* s_, const ref_ray* rays, int n, float* out) {
    RefScene* s = (RefScene*)s_;
    DbgIntegrator dbg;
    for (int i = 0; i < n; i++) {
        float3 L = dbg.Li(make_ray(rays[i]), s->scene);
        out[3 * i] = L.x; out[3 * i + 1] = L.y; out[3 * i + 2] = L.z;
    }
}

// ---- BVHTriMesh's tree in the layout of OracleScene.bvh / ag.bvh_build: nodes[total + 1] (slot 1, which the reference leaves
// uninitialised, zeroed) and Primitive::index in leaf order.  Returns total, or -1 when it exceeds cap_nodes - 1. ---------------------
int ref_bvh(const float* verts, int n_verts, const int32_t* indices, int n_indices, int max_prims_in_node, ref_node* nodes_out,
            int cap_nodes, int32_t* order_out) {
    PeekBVH bvh(mesh_from_arrays(verts, n_verts, nullptr, 0, nullptr, 0, indices, n_indices, nullptr), nullptr, max_prims_in_node);
    const BVHNode* nodes = bvh.Nodes();
    // the array is as long as the last child pair reaches: follow the interior nodes
    int last = 0;
    vector<int> todo = {0};
    while (!todo.empty()) {
        int k = todo.back();
        todo.pop_back();
        if (k > last) last = k;
        if (nodes[k].count == 0) { todo.push_back(nodes[k].first); todo.push_back(nodes[k].first + 1); }
    }
    int total = last == 0 ? 1 : last;   // root alone: 1 node; otherwise slots 0, 2 .. last
    if (total + 1 > cap_nodes) return -1;
    memset(nodes_out, 0, sizeof(ref_node) * (size_t)(total + 1));
    for (int k = 0; k <= last; k++) {
        if (k == 1) continue;
        memcpy(nodes_out[k].bmin, nodes[k].bounds.bmin3, 12);
        memcpy(nodes_out[k].bmax, nodes[k].bounds.bmax3, 12);
        nodes_out[k].first = nodes[k].first;
        nodes_out[k].count = nodes[k].count;
    }
    for (int i = 0; i < bvh.NumPrims(); i++) order_out[i] = bvh.PrimIndex(i);
    return total;
}

// ---- TriangleMesh::CreateBackdrop: capacities as oracle_create_backdrop ----------------------------------------------------------------
void ref_backdrop(const float origin[3], const float size[3], float radius, int steps, float* verts, float* normals, float* uvs,
                  int32_t* indices, int* n_verts, int* n_indices) {
    auto made = TriangleMesh::CreateBackdrop(F3(origin), F3(size), radius, steps, nullptr);
    PeekTriMesh m(made, nullptr);
    for (size_t i = 0; i < m.V().size(); i++) { verts[3 * i] = m.V()[i].x; verts[3 * i + 1] = m.V()[i].y; verts[3 * i + 2] = m.V()[i].z; }
    for (size_t i = 0; i < m.N().size(); i++) { normals[3 * i] = m.N()[i].x; normals[3 * i + 1] = m.N()[i].y; normals[3 * i + 2] = m.N()[i].z; }
    for (size_t i = 0; i < m.T().size(); i++) { uvs[2 * i] = m.T()[i].x; uvs[2 * i + 1] = m.T()[i].y; }
    for (size_t i = 0; i < m.I().size(); i++) {
        indices[3 * i] = m.I()[i].vertex_index; indices[3 * i + 1] = m.I()[i].normal_index; indices[3 * i + 2] = m.I()[i].texcoord_index;
    }
    *n_verts = (int)m.V().size();
    *n_indices = (int)m.I().size();
}

// ---- Camera: the 22 floats of agpt_camera_vectors -------------------------------------------------------------------------------------
void ref_camera(const float lookfrom[3], const float lookat[3], const float vup[3], float aspect_ratio, float vfov, float aperture,
                float out[22]) {
    PeekCamera cam(F3(lookfrom), F3(lookat), F3(vup), aspect_ratio, vfov, aperture);
    cam.Vectors(out);
}
// Camera::GetRay(s, t) for n film positions with the scene's camera; each ray draws from its own xorshift32 state (left updated)
void ref_camera_rays(void* s_, const float* st, int n, uint32_t* states, ref_ray* out) {
    RefScene* s = (RefScene*)s_;
    Camera cam(s->scene.camera);
    for (int i = 0; i < n; i++) {
        g_rng_state = states[i];
        Ray r = cam.GetRay(st[2 * i], st[2 * i + 1]);
        states[i] = g_rng_state;
        out[i].o[0] = r.O.x; out[i].o[1] = r.O.y; out[i].o[2] = r.O.z;
        out[i].d[0] = r.D.x; out[i].d[1] = r.D.y; out[i].d[2] = r.D.z;
        out[i].tmax = r.t;
    }
}

// ---- PathTracer::Li for n rays, each on the xorshift32 stream rng_states[i] defines (as agpt_li_batch).  calls_out[2] = Scene::Intersect
// and Scene::IntersectP calls over the whole batch. ----------------------------------------------------------------------------------
void ref_li(void* s_, const ref_ray* rays, const uint32_t* rng_states, int n, int max_depth, float* L_out, uint32_t* states_out,
            int32_t* draws_out, long long calls_out[2]) {
    RefScene* s = (RefScene*)s_;
    auto counter = make_shared<CallCounter>();
    s->scene.primitives.insert(s->scene.primitives.begin(), counter);
    PathTracer pt(max_depth);
    for (int i = 0; i < n; i++) {
        g_rng_state = rng_states[i];
        g_draws_used = 0;
        float3 L = pt.Li(make_ray(rays[i]), s->scene);
        L_out[3 * i] = L.x; L_out[3 * i + 1] = L.y; L_out[3 * i + 2] = L.z;
        states_out[i] = g_rng_state;
        draws_out[i] = (int32_t)g_draws_used;
    }
    s->scene.primitives.erase(s->scene.primitives.begin());
    calls_out[0] = counter->closest;
    calls_out[1] = counter->any;
}

// ---- InfiniteAreaLight::Le / Pdf_Li / Sample_Li of entry `light` of the scene's light list, through its public members only.  Each
// returns 0 when that entry is no InfiniteAreaLight. ----------------------------------------------------------------------------------
static const InfiniteAreaLight* env_light(RefScene* s, int light) {
    if (light < 0 || light >= (int)s->scene.lights.size()) return nullptr;
    return dynamic_cast<const InfiniteAreaLight*>(s->scene.lights[light].get());
}
// Le(ray) with ray.D = d as given (Ray's constructor would normalize it a first time; PathTracer::Li hands Le a ray it made itself)
int ref_env_le(void* s_, int light, int n, const float* d3, float* rgb_out) {
    const InfiniteAreaLight* l = env_light((RefScene*)s_, light);
    if (!l) return 0;
    for (int i = 0; i < n; i++) {
        Ray ray;
        ray.O = float3(0.f);
        ray.D = F3(d3 + 3 * i);
        ray.t = FLT_MAX;
        float3 L = l->Le(ray);
        rgb_out[3 * i] = L.x; rgb_out[3 * i + 1] = L.y; rgb_out[3 * i + 2] = L.z;
    }
    return 1;
}
int ref_env_pdf_li(void* s_, int light, int n, const float* wi3, float* pdf_out) {
    const InfiniteAreaLight* l = env_light((RefScene*)s_, light);
    if (!l) return 0;
    SurfaceInteraction si;
    for (int i = 0; i < n; i++) pdf_out[i] = l->Pdf_Li(si, F3(wi3 + 3 * i));
    return 1;
}
// Sample_Li, one call per draw: u[i] is what its one RandomFloat() returns.  wi and pdf start at a sentinel; a call that leaves them
// untouched (the return before the texel is chosen) is recorded as ok = 0 with wi = pdf = 0.  le3_out is the returned radiance.
int ref_env_sample_li(void* s_, int light, int n, const float* u, float* wi3_out, float* pdf_out, float* le3_out, int32_t* ok_out) {
    const InfiniteAreaLight* l = env_light((RefScene*)s_, light);
    if (!l) return 0;
    const float sentinel = -12345.f;
    SurfaceInteraction ref(float3(0.f), float2(0, 0), float3(0, 0, 1), float3(1, 0, 0), float3(0, 1, 0), nullptr);
    for (int i = 0; i < n; i++) {
        ref_set_draws(u + i, 1);
        float3 wi(sentinel);
        float pdf = sentinel;
        VisibilityTester vis;
        float3 L = l->Sample_Li(ref, float2(0, 0), &wi, &pdf, &vis);
        const bool ok = !(bits(wi.x) == bits(sentinel) && bits(wi.y) == bits(sentinel) && bits(wi.z) == bits(sentinel) &&
                          bits(pdf) == bits(sentinel));
        if (g_draws_used != 1) { ref_set_draws(nullptr, 0); return -1; }
        ok_out[i] = ok ? 1 : 0;
        wi3_out[3 * i] = ok ? wi.x : 0.f; wi3_out[3 * i + 1] = ok ? wi.y : 0.f; wi3_out[3 * i + 2] = ok ? wi.z : 0.f;
        pdf_out[i] = ok ? pdf : 0.f;
        le3_out[3 * i] = L.x; le3_out[3 * i + 1] = L.y; le3_out[3 * i + 2] = L.z;
    }
    ref_set_draws(nullptr, 0);
    return 1;
}
}
