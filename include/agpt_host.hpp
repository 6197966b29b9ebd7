// include/agpt_host.hpp -- C++ host adapter over the C ABI of include/agpt.h.
//
// Header-only mirror of the reference's host-side surface for the path-tracing hot path, so that code written
// like MyApp::Init / MyApp::Tick (myapp.cpp:13-135,141-190) keeps its shape while the per-pixel loop, BVH traversal
// and shading run on the MI355X:
//
//   reference (paths relative to the reference checkout)            this header
//   ---------------------------------------------------------------------------------------------------------
//   DisneyMaterial::Make(color, rough, metallic)  material.h:60     agpt::DisneyMaterial::Make(scene, ...)
//   MirrorMaterial::Make(r)                        material.h:83     agpt::MirrorMaterial::Make(scene, r)
//   TriangleMesh::CreateBackdrop(...)              trianglemesh.cpp:232   agpt::TriangleMesh::CreateBackdrop(...)
//   TriangleMesh::LoadObj(file, mat, transform)    trianglemesh.cpp:157   agpt::TriangleMesh::LoadObj(file, transform16)
//   make_shared<BVHTriMesh>(mesh, mat, 1)          bvhtrimesh.h:154  scene.primitives_push_back(mesh, mat, 1)
//   make_shared<Sphere>(c, r, mat)                 intersectable.h:161    scene.primitives_push_back(Sphere{c, r}, mat)
//   scene->addAreaLight(sphere, L)                 scene.h:21        scene.addAreaLight(Sphere{c, r}, L)
//   scene->lights.push_back(UniformInfiniteLight)  lights.h:37       scene.lights_push_back(UniformInfiniteLight{L})
//   scene->lights.push_back(InfiniteAreaLight(hdr)) lights.h:53      scene.lights_push_back(InfiniteAreaLight("x.hdr"))
//   scene->camera = CameraDesc{...}                camera.h:17       scene.camera = ...; (applied at commit)
//   Scene::Intersect / IntersectP                  scene.h:5-19      scene.Intersect(rays, n, hits) / IntersectP
//   PathTracer(maxDepth).Li per pixel + Accumulator::AddSample       agpt::PathTracer(maxDepth).Render(scene, accum, spp)
//   Accumulator (sum buffer, y flip, sample count) myapp.h:8-68      agpt::Accumulator
//   RotatingCamera(desc).update(angle)             camera.h:109-162  agpt::RotatingCamera(desc).update(dx, dy) -> CameraDesc
//   DbgIntegrator().Li(ray, scene)                 integrator.h:107  agpt::DbgIntegrator().Li(scene, ray)
//
// Errors: the reference has no error returns (bool hit/miss, exit() on load failure); here every failing C call
// throws agpt::Error carrying agpt_last_error().
#pragma once

#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "agpt.h"

namespace agpt {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what + ": " + agpt_last_error()), code(c) {}
};
inline int check(int rc, const char* what) {
    if (rc < 0) throw Error(rc, what);
    return rc;
}

struct float3 {
    float x, y, z;
};

class Context {
public:
    explicit Context(int device = 0, void* hip_stream = nullptr) {
        check(agpt_init(device, &h_), "agpt_init");
        if (hip_stream) check(agpt_set_stream(h_, hip_stream), "agpt_set_stream");
    }
    ~Context() { agpt_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    agpt_ctx* handle() const { return h_; }

private:
    agpt_ctx* h_ = nullptr;
};

// TriangleMesh (trianglemesh.h:14-57): AoS arrays + (v, n, t) index triplets
struct TriangleMesh {
    std::vector<float> vertices, normals, texcoords;
    std::vector<int32_t> indices;

    // TriangleMesh::LoadObj(inputfile, mat, transform, ignore_normals) (trianglemesh.cpp:157-230); transform16 is a
    // row-major mat4 or nullptr for identity.  Throws agpt::Error where the reference calls exit(1).
    static TriangleMesh LoadObj(const std::string& inputfile, const float* transform16 = nullptr, bool ignore_normals = false) {
        agpt_obj_mesh* h = nullptr;
        if (agpt_obj_load(inputfile.c_str(), transform16, ignore_normals ? 1 : 0, &h) < 0)
            throw std::runtime_error(std::string("agpt_obj_load: ") + agpt_obj_last_error());
        TriangleMesh m;
        int nv = 0, nn = 0, nt = 0, ni = 0;
        agpt_obj_counts(h, &nv, &nn, &nt, &ni);
        m.vertices.resize(3 * (size_t)nv);
        m.normals.resize(3 * (size_t)nn);
        m.texcoords.resize(2 * (size_t)nt);
        m.indices.resize(3 * (size_t)ni);
        agpt_obj_get(h, m.vertices.data(), m.normals.data(), m.texcoords.data(), m.indices.data());
        agpt_obj_free(h);
        return m;
    }

    // this mesh with its positions and normals through a row-major mat4 (agpt_transform_arrays: the arithmetic of LoadObj's transform
    // and of Scene::TransformMesh), on the host
    TriangleMesh Transformed(const float transform16[16]) const {
        TriangleMesh m = *this;
        if (agpt_transform_arrays(transform16, vertices.data(), (int)vertices.size() / 3, normals.data(), (int)normals.size() / 3,
                                  m.vertices.data(), m.normals.data()) < 0)
            throw std::runtime_error(std::string("agpt_transform_arrays: ") + agpt_last_error());
        return m;
    }
    static TriangleMesh CreateBackdrop(float3 origin, float3 size, float radius, int steps) {
        TriangleMesh m;
        const int nv = 2 * (steps + 5), ni = 6 * (steps + 4);
        m.vertices.resize(3 * nv);
        m.normals.resize(3 * nv);
        m.texcoords.resize(2 * nv);
        m.indices.resize(3 * ni);
        const float o[3] = {origin.x, origin.y, origin.z}, s[3] = {size.x, size.y, size.z};
        int n_v = 0, n_i = 0;
        check(agpt_create_backdrop(o, s, radius, steps, m.vertices.data(), m.normals.data(), m.texcoords.data(),
                                   m.indices.data(), &n_v, &n_i),
              "agpt_create_backdrop");
        return m;
    }
};

struct Sphere {
    float3 center;
    float radius;
};
// Plane (intersectable.h:119-157): XZ rectangle with +Y normal, size = full extents
struct Plane {
    float3 o;
    float size_x, size_z;
};
struct UniformInfiniteLight {
    float3 L;
};
// InfiniteAreaLight (lights.h:53-70): the HDR environment map as width*height RGB floats (what stbi_loadf returns)
// Built from a Radiance .hdr file as in the reference (myapp.cpp:113: InfiniteAreaLight("small_workshop_1k.hdr"); HDRTexture's
// stbi_loadf, texture.h:41-52 = agpt_hdr_load) or from pixels already in memory.
struct InfiniteAreaLight {
    const float* rgb = nullptr;
    int width = 0, height = 0;
    InfiniteAreaLight(const float* pixels, int w, int h) : rgb(pixels), width(w), height(h) {}
    explicit InfiniteAreaLight(const std::string& filename) {
        float* p = nullptr;
        check(agpt_hdr_load(filename.c_str(), &width, &height, &p), "agpt_hdr_load");
        owned_.reset(p, agpt_hdr_free);
        rgb = p;
    }

private:
    std::shared_ptr<float> owned_;
};
using CameraDesc = agpt_camera_desc;

// agpt_scene_set_bvh_builder: where the BVH of later primitives_push_back(mesh) calls is built; both give the same bytes
enum class BvhBuilder { Host = AGPT_BVH_BUILDER_HOST, Device = AGPT_BVH_BUILDER_DEVICE };
// agpt_scene_set_shading_arith: exact (default, bit-identical to the oracle) or fast shading arithmetic for later renders
// agpt_scene_update_mesh: keep the tree and refit its boxes, or build a new one
enum class MeshUpdate { Refit = AGPT_UPDATE_REFIT, Rebuild = AGPT_UPDATE_REBUILD };
// agpt_scene_set_mesh_normals_mode: a mesh's normals come from the caller / its rest normals, or are recomputed from every update's positions
enum class MeshNormals { Given = AGPT_NORMALS_GIVEN, Smooth = AGPT_NORMALS_SMOOTH };
enum class ShadingArith { Exact = AGPT_SHADING_EXACT, Fast = AGPT_SHADING_FAST };
// AdaptiveAccumulator::TemporalAccumulate: reproject the point a pixel sees now (agpt_temporal_accumulate), or where a moved mesh's
// surface point was a frame ago (agpt_temporal_accumulate_motion, with the features of PathTracer::RenderFeaturesMotion), or that
// and, in the normal test, the shading normal that point had a frame ago, so that a surface which turned keeps its history
// (agpt_temporal_accumulate_surface_motion, with Scene::SnapshotSurfaces and PathTracer::RenderFeaturesSurfaceMotion)
enum class Motion { Ignore, Follow, FollowSurfaces };

class Scene {
public:
    explicit Scene(Context& ctx) : ctx_(ctx) {
        check(agpt_scene_create(ctx.handle(), &h_), "agpt_scene_create");
        camera = CameraDesc{{0, 0, 1}, {0, 0, 0}, {0, 1, 0}, 1.f, 45.f, 0.f};
    }
    ~Scene() { agpt_scene_destroy(h_); }
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;

    int add_material(int type, float3 color, float roughness, float metallic) {
        const float c[3] = {color.x, color.y, color.z};
        return check(agpt_scene_add_material(h_, type, c, roughness, metallic), "agpt_scene_add_material");
    }
    void SetBvhBuilder(BvhBuilder b) { check(agpt_scene_set_bvh_builder(h_, (int)b), "agpt_scene_set_bvh_builder"); }
    void SetShadingArith(ShadingArith m) { check(agpt_scene_set_shading_arith(h_, (int)m), "agpt_scene_set_shading_arith"); }
    // scene->primitives.push_back(make_shared<BVHTriMesh>(mesh, material, maxPrimsInNode))
    int primitives_push_back(const TriangleMesh& m, int material, int maxPrimsInNode = 1) {
        return check(agpt_scene_add_mesh(h_, m.vertices.data(), (int)m.vertices.size() / 3, m.normals.data(),
                                         (int)m.normals.size() / 3, m.texcoords.data(), (int)m.texcoords.size() / 2,
                                         m.indices.data(), (int)m.indices.size() / 3, material, maxPrimsInNode),
                     "agpt_scene_add_mesh");
    }
    // scene->primitives.push_back(make_shared<Sphere>(center, radius, material)); material -1 = nullptr
    int primitives_push_back(const Sphere& s, int material) {
        const float c[3] = {s.center.x, s.center.y, s.center.z};
        return check(agpt_scene_add_sphere(h_, c, s.radius, material), "agpt_scene_add_sphere");
    }
    int primitives_push_back(const Plane& p, int material) {
        const float o[3] = {p.o.x, p.o.y, p.o.z}, sz[2] = {p.size_x, p.size_z};
        return check(agpt_scene_add_plane(h_, o, sz, material), "agpt_scene_add_plane");
    }
    int addAreaLight(const Sphere& s, float3 L) {
        const float c[3] = {s.center.x, s.center.y, s.center.z}, l[3] = {L.x, L.y, L.z};
        return check(agpt_scene_add_area_light(h_, c, s.radius, l), "agpt_scene_add_area_light");
    }
    int lights_push_back(const UniformInfiniteLight& l) {
        const float c[3] = {l.L.x, l.L.y, l.L.z};
        return check(agpt_scene_add_uniform_infinite_light(h_, c), "agpt_scene_add_uniform_infinite_light");
    }
    int lights_push_back(const InfiniteAreaLight& l) {
        return check(agpt_scene_add_infinite_area_light(h_, l.rgb, l.width, l.height), "agpt_scene_add_infinite_area_light");
    }
    // An image for materials (agpt_scene_add_texture): width * height linear RGB floats, row 0 = top -- HDRTexture's pixels
    // (texture.h:41-84) handed over in memory; returns the texture id
    int textures_push_back(const float* rgb, int width, int height) {
        return check(agpt_scene_add_texture(h_, rgb, width, height), "agpt_scene_add_texture");
    }
    // the material's colour at a mesh hit becomes Texture::value(u, v) of `texture` (-1: its constant colour again)
    void SetMaterialTexture(int material, int texture) {
        check(agpt_scene_set_material_texture(h_, material, texture), "agpt_scene_set_material_texture");
    }
    // how `texture` is read in every slot that names it: AGPT_FILTER_NEAREST / _BILINEAR, each axis AGPT_WRAP_REPEAT / _CLAMP / _MIRROR
    // (the default: nearest, repeat, repeat = Texture::value)
    void SetTextureSampler(int texture, int filter, int wrap_u, int wrap_v) {
        check(agpt_scene_set_texture_sampler(h_, texture, filter, wrap_u, wrap_v), "agpt_scene_set_texture_sampler");
    }
    // a Disney material's roughness (AGPT_PARAM_ROUGHNESS) / metallic (AGPT_PARAM_METALLIC) at a mesh hit becomes channel `channel`
    // (0 = r, 1 = g, 2 = b) of Texture::value(u, v) of `texture` (-1: its constant again), and the material what DisneyMaterial::Make
    // builds from it
    void SetMaterialParamTexture(int material, int param, int texture, int channel) {
        check(agpt_scene_set_material_param_texture(h_, material, param, texture, channel), "agpt_scene_set_material_param_texture");
    }
    // the material's shading normal at a mesh hit is perturbed by `texture` read as a tangent-space normal map: x = (2r - 1) * scale along
    // the tangent, y = (2g - 1) * scale along cross(normal, tangent), z = 2b - 1 along the normal (-1: no normal map)
    void SetMaterialNormalTexture(int material, int texture, float scale = 1.f) {
        check(agpt_scene_set_material_normal_texture(h_, material, texture, scale), "agpt_scene_set_material_normal_texture");
    }
    // upload to HBM; call once after the scene is built (and again after changing `camera`)
    void commit() {
        check(agpt_scene_set_camera(h_, &camera), "agpt_scene_set_camera");
        check(agpt_scene_commit(h_), "agpt_scene_commit");
    }
    // geometry moved (agpt_scene_update_mesh): new positions -- and vertex normals, if the mesh has any -- for mesh primitive `prim` of
    // the committed scene; indices, texture coordinates and material stay.  Refit keeps the BVH's topology and rewrites the mesh's
    // records on the GPU; Rebuild builds a new tree and uploads the scene again.  The host applies the result like a camera move:
    // `scene.UpdateMesh(prim, mesh); accumulator.Clear();`
    void UpdateMesh(int prim, const TriangleMesh& m, MeshUpdate mode = MeshUpdate::Refit) {
        check(agpt_scene_update_mesh(h_, prim, m.vertices.data(), (int)m.vertices.size() / 3, m.normals.empty() ? nullptr : m.normals.data(),
                                     (int)m.normals.size() / 3, (int)mode),
              "agpt_scene_update_mesh");
    }
    // the same with the arrays in DEVICE memory of the context's GPU (agpt_scene_update_mesh_device): packed xyz floats of the mesh's
    // own counts, complete when the call is made or produced on the context's stream; the library copies them before it returns
    void UpdateMeshDevice(int prim, const float* vertices_dev, int n_vertices, const float* normals_dev, int n_normals,
                          MeshUpdate mode = MeshUpdate::Refit) {
        check(agpt_scene_update_mesh_device(h_, prim, vertices_dev, n_vertices, normals_dev, n_normals, (int)mode), "agpt_scene_update_mesh_device");
    }
    // a rigid (or any affine / projective) placement, applied on the GPU to the mesh's rest pose -- the arrays it last received from
    // primitives_push_back / UpdateMesh / UpdateMeshDevice (agpt_scene_transform_mesh): transform16 is a row-major mat4, absolute, not
    // cumulative; 16 floats per object per frame instead of the mesh.  `scene.TransformMesh(prim, m); accumulator.Clear();`
    void TransformMesh(int prim, const float transform16[16], MeshUpdate mode = MeshUpdate::Refit) {
        check(agpt_scene_transform_mesh(h_, prim, transform16, (int)mode), "agpt_scene_transform_mesh");
    }
    // an articulated mesh: SetMeshSkin gives the binding once (agpt_scene_set_mesh_skin) -- `influences` (joint, weight) slots per
    // vertex, flat arrays of n_vertices * influences; the normals' own slots, or none when the mesh has as many normals as vertices and
    // they share the vertices' --, PoseMesh the n_joints row-major mat4 of a frame (agpt_scene_pose_mesh), applied on the GPU to the
    // rest pose TransformMesh uses: absolute, not cumulative.  `scene.PoseMesh(prim, joints); accumulator.Clear();`
    void SetMeshSkin(int prim, int influences, int n_joints, const std::vector<int32_t>& vertex_joints, const std::vector<float>& vertex_weights,
                     const std::vector<int32_t>& normal_joints = {}, const std::vector<float>& normal_weights = {}) {
        check(agpt_scene_set_mesh_skin(h_, prim, influences, n_joints, vertex_joints.data(), vertex_weights.data(),
                                       normal_joints.empty() ? nullptr : normal_joints.data(), normal_weights.empty() ? nullptr : normal_weights.data()),
              "agpt_scene_set_mesh_skin");
    }
    void PoseMesh(int prim, const std::vector<float>& joints16, MeshUpdate mode = MeshUpdate::Refit) {
        check(agpt_scene_pose_mesh(h_, prim, joints16.data(), (int)(joints16.size() / 16), (int)mode), "agpt_scene_pose_mesh");
    }
    // PoseMesh for an animation system that leaves its joint matrices on the GPU (agpt_scene_pose_mesh_device): n_joints row-major mat4
    // in device memory, 16-byte aligned, complete or produced on the context's stream; the GPU forms the palette and checks the matrices,
    // nothing of them crosses the bus, and the same bytes result.
    void PoseMeshDevice(int prim, const float* joints16_dev, int n_joints, MeshUpdate mode = MeshUpdate::Refit) {
        check(agpt_scene_pose_mesh_device(h_, prim, joints16_dev, n_joints, (int)mode), "agpt_scene_pose_mesh_device");
    }
    // morph targets (blend shapes): SetMeshMorphTargets gives the deltas once (agpt_scene_set_mesh_morph_targets) -- target-major,
    // n_targets * n_vertices * 3 floats, and the normals' n_targets * n_normals * 3 or none --, MorphMesh the weights of a frame and,
    // for a skinned mesh, its joints (agpt_scene_morph_mesh): morph, then skin, in one kernel from the rest pose TransformMesh and
    // PoseMesh use: absolute, not cumulative.  `scene.MorphMesh(prim, weights, joints); accumulator.Clear();`
    void SetMeshMorphTargets(int prim, int n_targets, const std::vector<float>& position_deltas, const std::vector<float>& normal_deltas = {}) {
        check(agpt_scene_set_mesh_morph_targets(h_, prim, n_targets, position_deltas.data(), normal_deltas.empty() ? nullptr : normal_deltas.data()),
              "agpt_scene_set_mesh_morph_targets");
    }
    void MorphMesh(int prim, const std::vector<float>& weights, const std::vector<float>& joints16 = {}, MeshUpdate mode = MeshUpdate::Refit) {
        check(agpt_scene_morph_mesh(h_, prim, weights.data(), (int)weights.size(), joints16.empty() ? nullptr : joints16.data(),
                                    (int)(joints16.size() / 16), (int)mode),
              "agpt_scene_morph_mesh");
    }
    // MorphMesh with the frame's weights and, for a skinned mesh, its joints in device memory (agpt_scene_morph_mesh_device; joints16_dev
    // may be NULL): the GPU compacts the weights into the active list itself.  Ordering and alignment as for PoseMeshDevice.
    void MorphMeshDevice(int prim, const float* weights_dev, int n_targets, const float* joints16_dev = nullptr, int n_joints = 0,
                         MeshUpdate mode = MeshUpdate::Refit) {
        check(agpt_scene_morph_mesh_device(h_, prim, weights_dev, n_targets, joints16_dev, n_joints, (int)mode), "agpt_scene_morph_mesh_device");
    }
    // smooth vertex normals recomputed on the GPU (agpt_scene_set_mesh_normals_mode): with MeshNormals::Smooth every later UpdateMesh,
    // UpdateMeshDevice, TransformMesh, PoseMesh and MorphMesh of the mesh writes its normals from the new positions -- area-weighted face
    // vectors summed per normal in corner order, normalised; (0, 0, 0), "use the geometric normal", where that sum has no direction --
    // and the normals those calls are given (normals_dev may be NULL) are not read.  Changes nothing by itself.
    // `scene.SetMeshNormalsMode(prim, MeshNormals::Smooth);` once, then `scene.UpdateMesh(prim, mesh); accumulator.Clear();` per frame.
    void SetMeshNormalsMode(int prim, MeshNormals mode) {
        check(agpt_scene_set_mesh_normals_mode(h_, prim, (int)mode), "agpt_scene_set_mesh_normals_mode");
    }
    // spheres, planes and lights of the committed scene moved in place (agpt_scene_update_sphere and the calls beside it): `prim` is what
    // primitives_push_back / addAreaLight returned, `light` what lights_push_back(UniformInfiniteLight) returned.  The values are absolute;
    // the scene is what building it with them gives.  Non-finite values, a radius <= 0 and a plane size <= 0 are refused.
    // `scene.updateSphere(light, Sphere{c, r}); accumulator.Clear();`
    void updateSphere(int prim, const Sphere& s) {
        const float c[3] = {s.center.x, s.center.y, s.center.z};
        check(agpt_scene_update_sphere(h_, prim, c, s.radius), "agpt_scene_update_sphere");
    }
    void updatePlane(int prim, const Plane& p) {
        const float o[3] = {p.o.x, p.o.y, p.o.z}, sz[2] = {p.size_x, p.size_z};
        check(agpt_scene_update_plane(h_, prim, o, sz), "agpt_scene_update_plane");
    }
    void setAreaLightRadiance(int prim, float3 L) {
        const float l[3] = {L.x, L.y, L.z};
        check(agpt_scene_set_area_light_radiance(h_, prim, l), "agpt_scene_set_area_light_radiance");
    }
    void setInfiniteLightRadiance(int light, float3 L) {
        const float l[3] = {L.x, L.y, L.z};
        check(agpt_scene_set_infinite_light_radiance(h_, light, l), "agpt_scene_set_infinite_light_radiance");
    }
    // n spheres at once from DEVICE memory of the context's GPU (agpt_scene_update_spheres_device): prims are distinct sphere ids,
    // center_radius_dev one 16-byte record (cx, cy, cz, radius) each, complete when the call is made or produced on the context's stream
    void updateSpheresDevice(const std::vector<int32_t>& prims, const float* center_radius_dev) {
        if (prims.empty()) return;
        check(agpt_scene_update_spheres_device(h_, prims.data(), (int)prims.size(), center_radius_dev), "agpt_scene_update_spheres_device");
    }
    // camera moved (RotatingCamera::update): re-derive the camera only, geometry stays in HBM
    // motion vectors (agpt_scene_snapshot_positions): once per frame, after the frame's UpdateMesh / TransformMesh / PoseMesh / MorphMesh /
    // updateSphere / updatePlane calls and before PathTracer::RenderFeaturesMotion -- the scene keeps the triangle positions and the sphere
    // and plane records of this frame and of the one before
    void SnapshotPositions() { check(agpt_scene_snapshot_positions(h_), "agpt_scene_snapshot_positions"); }
    // agpt_scene_snapshot_surfaces: SnapshotPositions plus two generations of the per-triangle shading records (128 B per triangle), in its
    // place, before PathTracer::RenderFeaturesSurfaceMotion
    void SnapshotSurfaces() { check(agpt_scene_snapshot_surfaces(h_), "agpt_scene_snapshot_surfaces"); }
    void set_camera() { check(agpt_scene_set_camera(h_, &camera), "agpt_scene_set_camera"); }
    void Intersect(const agpt_ray* rays, int n, agpt_hit* hits) const {
        check(agpt_intersect_batch(h_, rays, n, hits, 0, nullptr), "agpt_intersect_batch");
    }
    void IntersectP(const agpt_ray* rays, int n, agpt_hit* hits) const {
        check(agpt_intersect_batch(h_, rays, n, hits, 1, nullptr), "agpt_intersect_batch");
    }
    // single-ray convenience for picking / debugging (myapp.cpp:200-201)
    bool Intersect(const agpt_ray& ray, agpt_hit& hit) const {
        Intersect(&ray, 1, &hit);
        return hit.hit != 0;
    }

    CameraDesc camera;
    agpt_scene* handle() const { return h_; }
    Context& context() const { return ctx_; }

private:
    Context& ctx_;
    agpt_scene* h_ = nullptr;
};

// RotatingCamera (camera.h:109-162): orbit around lookat at a fixed distance.  The elevation angle is clamped to
// [-(pi/2 - 1e-4), 0] and lookfrom = RotateY(yAngle) * RotateX(xAngle) * (0,0,1) * dist + lookat.  The host applies the
// result with `scene.camera = cam.update(dx, dy); scene.set_camera(); accumulator.Clear();` (myapp.cpp:143-149).
class RotatingCamera {
public:
    explicit RotatingCamera(const CameraDesc& d) : desc_(d) {
        const float fx = d.lookfrom[0] - d.lookat[0], fy = d.lookfrom[1] - d.lookat[1], fz = d.lookfrom[2] - d.lookat[2];
        dist_ = std::sqrt(fx * fx + fy * fy + fz * fz);
        const float inv = 1.0f / dist_;
        const float nx = fx * inv, ny = fy * inv, nz = fz * inv;
        const float horiz = std::sqrt(nx * nx + nz * nz);
        xAngle_ = std::acos(horiz);
        if (ny > 0) xAngle_ = -xAngle_;
        yAngle_ = std::acos(nz / horiz);
        if (nx < 0) yAngle_ = -yAngle_;
    }
    const CameraDesc& update(float dxAngle, float dyAngle) {
        const float lim = 3.14159265358979323846f / 2 - 0.0001f;
        xAngle_ += dxAngle;
        xAngle_ = xAngle_ < -lim ? -lim : (xAngle_ > 0.f ? 0.f : xAngle_);
        yAngle_ += dyAngle;
        const float cx = std::cos(xAngle_), sx = std::sin(xAngle_), cy = std::cos(yAngle_), sy = std::sin(yAngle_);
        // third column of RotateY * RotateX (row-major mat4, template/precomp.h:875-876)
        desc_.lookfrom[0] = sy * cx * dist_ + desc_.lookat[0];
        desc_.lookfrom[1] = -sx * dist_ + desc_.lookat[1];
        desc_.lookfrom[2] = cy * cx * dist_ + desc_.lookat[2];
        return desc_;
    }
    const CameraDesc& desc() const { return desc_; }
    float xAngle() const { return xAngle_; }
    float yAngle() const { return yAngle_; }

private:
    CameraDesc desc_;
    float dist_, xAngle_, yAngle_;
};

struct DisneyMaterial {
    static int Make(Scene& s, float3 color, float roughness, float metallic) {
        return s.add_material(AGPT_MAT_DISNEY, color, roughness, metallic);
    }
};
struct MirrorMaterial {
    static int Make(Scene& s, float3 r) { return s.add_material(AGPT_MAT_MIRROR, r, 0.f, 0.f); }
};

// Accumulator (myapp.h:8-68): float sum buffer in HBM (float4 per pixel, row H-1-y), sample count, clear, resolve
class Accumulator {
public:
    Accumulator(Context& ctx, int w, int h) : width(w), height(h), ctx_(ctx) {
        check(agpt_device_alloc(ctx.handle(), (size_t)w * h * 16, &pixels_), "agpt_device_alloc");
        Clear();
    }
    ~Accumulator() { agpt_device_free(ctx_.handle(), pixels_); }
    Accumulator(const Accumulator&) = delete;
    Accumulator& operator=(const Accumulator&) = delete;
    void Clear() {
        check(agpt_device_memset(ctx_.handle(), pixels_, 0, (size_t)width * height * 16), "agpt_device_memset");
        samples_ = 0;
    }
    int NumSamples() const { return samples_; }
    void AddSamples(int n) { samples_ += n; }
    void SetSamples(int n) { samples_ = n; }
    float* device_pixels() const { return static_cast<float*>(pixels_); }
    // CopyToSurface: gamma 2.2 + 0x00RRGGBB (myapp.h:34-41)
    std::vector<uint32_t> CopyToSurface() const {
        std::vector<uint32_t> out((size_t)width * height);
        check(agpt_resolve(ctx_.handle(), device_pixels(), width * height, samples_, out.data()), "agpt_resolve");
        return out;
    }
    std::vector<float> Download() const {
        std::vector<float> out((size_t)width * height * 4);
        check(agpt_device_download(ctx_.handle(), out.data(), pixels_, out.size() * 4), "agpt_device_download");
        return out;
    }
    const int width, height;

private:
    Context& ctx_;
    void* pixels_ = nullptr;
    int samples_ = 0;
};

// First-hit feature buffers (agpt_render_features): albedo = (material colour, flag 0 miss / 1 surface / 2 emitter) and
// normal_depth = (shading normal, hit distance), float4 per pixel in Accumulator::pixels order.  They guide AdaptiveAccumulator::Denoise.
class FeatureBuffers {
public:
    FeatureBuffers(Context& ctx, int w, int h) : width(w), height(h), ctx_(ctx) {
        check(agpt_device_alloc(ctx.handle(), (size_t)w * h * 16, &albedo_), "agpt_device_alloc");
        check(agpt_device_alloc(ctx.handle(), (size_t)w * h * 16, &normal_depth_), "agpt_device_alloc");
    }
    ~FeatureBuffers() {
        if (prev_normal_) agpt_device_free(ctx_.handle(), prev_normal_);
        if (prev_point_) agpt_device_free(ctx_.handle(), prev_point_);
        agpt_device_free(ctx_.handle(), normal_depth_);
        agpt_device_free(ctx_.handle(), albedo_);
    }
    FeatureBuffers(const FeatureBuffers&) = delete;
    FeatureBuffers& operator=(const FeatureBuffers&) = delete;
    float* device_albedo() const { return static_cast<float*>(albedo_); }
    float* device_normal_depth() const { return static_cast<float*>(normal_depth_); }
    // prev_point of agpt_render_features_motion: (where the hit surface point was a frame ago, w: 0 miss / 1 moved / 2 not moved);
    // allocated by the first call, null until PathTracer::RenderFeaturesMotion has filled it
    float* device_prev_point() {
        if (!prev_point_) check(agpt_device_alloc(ctx_.handle(), (size_t)width * height * 16, &prev_point_), "agpt_device_alloc");
        return static_cast<float*>(prev_point_);
    }
    const float* prev_point_or_null() const { return static_cast<const float*>(prev_point_); }
    // prev_normal of agpt_render_features_surface_motion: (the shading normal the hit surface point had a frame ago, prev_point's w);
    // allocated by the first call, null until PathTracer::RenderFeaturesSurfaceMotion has filled it
    float* device_prev_normal() {
        if (!prev_normal_) check(agpt_device_alloc(ctx_.handle(), (size_t)width * height * 16, &prev_normal_), "agpt_device_alloc");
        return static_cast<float*>(prev_normal_);
    }
    const float* prev_normal_or_null() const { return static_cast<const float*>(prev_normal_); }
    std::vector<float> DownloadAlbedo() const { return download(albedo_); }
    std::vector<float> DownloadNormalDepth() const { return download(normal_depth_); }
    std::vector<float> DownloadPrevPoint() const { return prev_point_ ? download(prev_point_) : std::vector<float>(); }
    std::vector<float> DownloadPrevNormal() const { return prev_normal_ ? download(prev_normal_) : std::vector<float>(); }
    const int width, height;

private:
    std::vector<float> download(const void* src) const {
        std::vector<float> out((size_t)width * height * 4);
        check(agpt_device_download(ctx_.handle(), out.data(), src, out.size() * 4), "agpt_device_download");
        return out;
    }
    Context& ctx_;
    void* albedo_ = nullptr;
    void* normal_depth_ = nullptr;
    void* prev_point_ = nullptr;
    void* prev_normal_ = nullptr;
};

// The buffers of an adaptive render (agpt_render_adaptive): the float4 sums with each pixel's own sample count in w, and the
// per-pixel luminance second moment the stop test reads.  Keep both between RenderAdaptive calls to continue a frame.
class AdaptiveAccumulator {
public:
    AdaptiveAccumulator(Context& ctx, int w, int h) : width(w), height(h), ctx_(ctx) {
        check(agpt_device_alloc(ctx.handle(), (size_t)w * h * 16, &pixels_), "agpt_device_alloc");
        check(agpt_device_alloc(ctx.handle(), (size_t)w * h * 4, &moment2_), "agpt_device_alloc");
        Clear();
    }
    ~AdaptiveAccumulator() {
        agpt_device_free(ctx_.handle(), moment2_);
        agpt_device_free(ctx_.handle(), pixels_);
    }
    AdaptiveAccumulator(const AdaptiveAccumulator&) = delete;
    AdaptiveAccumulator& operator=(const AdaptiveAccumulator&) = delete;
    void Clear() {
        check(agpt_device_memset(ctx_.handle(), pixels_, 0, (size_t)width * height * 16), "agpt_device_memset");
        check(agpt_device_memset(ctx_.handle(), moment2_, 0, (size_t)width * height * 4), "agpt_device_memset");
    }
    float* device_pixels() const { return static_cast<float*>(pixels_); }
    float* device_moment2() const { return static_cast<float*>(moment2_); }
    // CopyToSurface with each pixel's own count (agpt_resolve_counts)
    std::vector<uint32_t> CopyToSurface() const {
        std::vector<uint32_t> out((size_t)width * height);
        check(agpt_resolve_counts(ctx_.handle(), device_pixels(), width * height, out.data()), "agpt_resolve_counts");
        return out;
    }
    std::vector<float> Download() const {
        std::vector<float> out((size_t)width * height * 4);
        check(agpt_device_download(ctx_.handle(), out.data(), pixels_, out.size() * 4), "agpt_device_download");
        return out;
    }
    // agpt_denoise: the a-trous filter over this frame, guided by `features`, into `out` as the mean radiance of ONE sample (its
    // CopyToSurface then displays it).  A uniform render for denoising is RenderAdaptive with rel_error <= 0 and min_spp = max_spp.
    void Denoise(const FeatureBuffers& features, Accumulator& out, int iterations = 5, bool demodulate = true,
                 float sigma_z = AGPT_DENOISE_SIGMA_Z, float sigma_n = AGPT_DENOISE_SIGMA_N, float sigma_l = AGPT_DENOISE_SIGMA_L) const {
        agpt_denoise_params p{};
        p.width = width;
        p.height = height;
        p.iterations = iterations;
        p.demodulate = demodulate ? 1 : 0;
        p.sigma_z = sigma_z;
        p.sigma_n = sigma_n;
        p.sigma_l = sigma_l;
        check(agpt_denoise(ctx_.handle(), &p, device_pixels(), device_moment2(), features.device_albedo(), features.device_normal_depth(),
                           out.device_pixels()),
              "agpt_denoise");
        out.SetSamples(1);
    }
    // agpt_temporal_accumulate: this frame -- these buffers and `features`, both rendered with cam_cur -- plus the history the previous
    // frame's call left (prev_history, with that frame's prev_features and cam_prev; both null on the first frame), reprojected,
    // into history_out.  history_out has this class' form (its w an effective, possibly fractional count): Denoise and CopyToSurface
    // apply to it, RenderAdaptive must not continue it.  The host keeps history_out and `features` for the next frame.
    // clamp (agpt_temporal_accumulate_clamped): the reprojected history is clamped to mean +- gamma standard deviations of this frame's
    // own neighbourhood, so that lighting which changed on unchanged geometry -- the shadow a moved mesh left -- does not trail.
    void TemporalAccumulate(const FeatureBuffers& features, const agpt_camera_desc& cam_cur, const AdaptiveAccumulator* prev_history,
                            const FeatureBuffers* prev_features, const agpt_camera_desc& cam_prev, AdaptiveAccumulator& history_out,
                            float max_history = 32.f, float depth_tol = AGPT_TEMPORAL_DEPTH_TOL,
                            float normal_cos = AGPT_TEMPORAL_NORMAL_COS, Motion motion = Motion::Ignore,
                            const agpt_temporal_clamp_params* clamp = nullptr) const {
        agpt_temporal_params p{};
        p.width = width;
        p.height = height;
        p.cam_cur = cam_cur;
        p.cam_prev = cam_prev;
        p.max_history = max_history;
        p.depth_tol = depth_tol;
        p.normal_cos = normal_cos;
        const float* hp = prev_history ? prev_history->device_pixels() : nullptr;
        const float* hm = prev_history ? prev_history->device_moment2() : nullptr;
        const float* pa = prev_features ? prev_features->device_albedo() : nullptr;
        const float* pn = prev_features ? prev_features->device_normal_depth() : nullptr;
        if (motion == Motion::FollowSurfaces) {
            // agpt_temporal_accumulate_surface_motion: `features` were rendered by PathTracer::RenderFeaturesSurfaceMotion; with or
            // without clamp (missing buffers are refused by the call)
            check(agpt_temporal_accumulate_surface_motion(ctx_.handle(), &p, clamp, device_pixels(), device_moment2(), features.device_albedo(),
                                                          features.device_normal_depth(), hp, hm, pa, pn, history_out.device_pixels(),
                                                          history_out.device_moment2(), features.prev_point_or_null(),
                                                          features.prev_normal_or_null()),
                  "agpt_temporal_accumulate_surface_motion");
            return;
        }
        if (clamp && (motion == Motion::Ignore || features.prev_point_or_null())) {
            // (Motion::Follow without a prev_point buffer is left to agpt_temporal_accumulate_motion below, which refuses it)
            check(agpt_temporal_accumulate_clamped(ctx_.handle(), &p, clamp, device_pixels(), device_moment2(), features.device_albedo(),
                                                   features.device_normal_depth(), hp, hm, pa, pn, history_out.device_pixels(),
                                                   history_out.device_moment2(),
                                                   motion == Motion::Follow ? features.prev_point_or_null() : nullptr),
                  "agpt_temporal_accumulate_clamped");
            return;
        }
        if (motion == Motion::Follow) {
            // agpt_temporal_accumulate_motion: `features` were rendered by PathTracer::RenderFeaturesMotion, whose prev_point says per
            // pixel where a moved mesh's surface point was a frame ago -- that point is reprojected instead of the one seen now
            check(agpt_temporal_accumulate_motion(ctx_.handle(), &p, device_pixels(), device_moment2(), features.device_albedo(),
                                                  features.device_normal_depth(), hp, hm, pa, pn, history_out.device_pixels(),
                                                  history_out.device_moment2(), features.prev_point_or_null()),
                  "agpt_temporal_accumulate_motion");
            return;
        }
        check(agpt_temporal_accumulate(ctx_.handle(), &p, device_pixels(), device_moment2(), features.device_albedo(),
                                       features.device_normal_depth(), hp, hm, pa, pn, history_out.device_pixels(),
                                       history_out.device_moment2()),
              "agpt_temporal_accumulate");
    }
    std::vector<float> DownloadMoment2() const {
        std::vector<float> out((size_t)width * height);
        check(agpt_device_download(ctx_.handle(), out.data(), moment2_, out.size() * 4), "agpt_device_download");
        return out;
    }
    const int width, height;

private:
    Context& ctx_;
    void* pixels_ = nullptr;
    void* moment2_ = nullptr;
};

// Integrator / PathTracer (integrator.h:28-31,120-196).  Li is evaluated for whole frames: one Render() call is
// `spp` iterations of MyApp::Tick's per-pixel loop (myapp.cpp:161-175).
// One rank's share of a film split over `world` GPUs: the 8-row blocks k with k % world == rank.
// The rank's Accumulator then holds only its own rows, compacted (Accumulator(ctx, width, RowsOfRank(height, ...))).
struct RankShare {
    int block_rows = 8, world = 1, rank = 0;
    // rows of a `film_height`-row film that belong to this rank
    int Rows(int film_height) const {
        int rows = 0;
        for (int y0 = 0, k = 0; y0 < film_height; y0 += block_rows, k++)
            if (k % world == rank) rows += (film_height - y0 < block_rows) ? film_height - y0 : block_rows;
        return rows;
    }
};

// The RCCL communicator of a multi-GPU render (one process and one Context per GPU).  Rank 0 obtains a 128-byte id with
// Comm::UniqueId() and passes it to the other ranks by the host application's own means (MPI_Bcast, a file, ...); every rank
// then constructs Comm(ctx, id, world, rank) collectively.  GatherTiles brings every rank's compact Accumulator to rank 0's
// full-film Accumulator (agpt_gather_tiles: grouped send/recv over xGMI + de-interleave), once per displayed frame.
class Comm {
public:
    static std::vector<unsigned char> UniqueId() {
        std::vector<unsigned char> id(128);
        check(agpt_comm_unique_id(id.data()), "agpt_comm_unique_id");
        return id;
    }
    Comm(Context& ctx, const std::vector<unsigned char>& id, int world, int rank) {
        check(agpt_comm_init(ctx.handle(), world > 1 ? id.data() : nullptr, world, rank, &h_), "agpt_comm_init");
    }
    ~Comm() { agpt_comm_destroy(h_); }
    Comm(const Comm&) = delete;
    Comm& operator=(const Comm&) = delete;
    // local: this rank's compact accumulator; full: the whole film on rank 0 (ignored, may be null, elsewhere)
    void GatherTiles(const Accumulator& local, int film_height, const RankShare& share, Accumulator* full) {
        check(agpt_gather_tiles(h_, local.device_pixels(), local.width, film_height, share.block_rows, full ? full->device_pixels() : nullptr),
              "agpt_gather_tiles");
        if (full) full->SetSamples(local.NumSamples());
    }
    // adaptive renders: the counts travel in w, so the full film resolves with its CopyToSurface as it is
    void GatherTiles(const AdaptiveAccumulator& local, int film_height, const RankShare& share, AdaptiveAccumulator* full) {
        check(agpt_gather_tiles(h_, local.device_pixels(), local.width, film_height, share.block_rows, full ? full->device_pixels() : nullptr),
              "agpt_gather_tiles");
    }

private:
    agpt_comm* h_ = nullptr;
};

class PathTracer {
public:
    explicit PathTracer(int maxDepth = 5) : MaxDepth(maxDepth) {}
    // multi-GPU: `acc` is this rank's compact accumulator (width x share.Rows(film_height)); seeds depend on the global
    // pixel index, so the gathered film is bit-identical to a single-GPU render
    agpt_stats Render(Scene& scene, Accumulator& acc, int film_height, const RankShare& share, int spp, uint32_t seed_base = 0) const {
        agpt_render_params p{};
        p.width = acc.width;
        p.height = film_height;
        p.w = acc.width;
        p.h = film_height;
        p.spp_begin = acc.NumSamples();
        p.spp_count = spp;
        p.seed_base = seed_base;
        p.max_depth = MaxDepth;
        p.accum_pitch = acc.width;
        p.interleave_block = share.block_rows;
        p.interleave_world = share.world;
        p.interleave_rank = share.rank;
        agpt_stats st{};
        check(agpt_render(scene.handle(), &p, acc.device_pixels(), &st), "agpt_render");
        acc.AddSamples(spp);
        return st;
    }
    agpt_stats Render(Scene& scene, Accumulator& acc, int spp, uint32_t seed_base = 0) const {
        agpt_render_params p{};
        p.width = acc.width;
        p.height = acc.height;
        p.x0 = 0;
        p.y0 = 0;
        p.w = acc.width;
        p.h = acc.height;
        p.spp_begin = acc.NumSamples();
        p.spp_count = spp;
        p.seed_base = seed_base;
        p.max_depth = MaxDepth;
        p.accum_pitch = acc.width;
        agpt_stats st{};
        check(agpt_render(scene.handle(), &p, acc.device_pixels(), &st), "agpt_render");
        acc.AddSamples(spp);
        return st;
    }
    // agpt_render_adaptive over the whole film (or, with `share`, this rank's rows of a film_height-row film into its compact
    // accumulator): rounds of params.step_spp samples for the pixels whose stop test fails, from the counts in acc
    agpt_stats RenderAdaptive(Scene& scene, AdaptiveAccumulator& acc, int film_height, const RankShare& share, const agpt_adaptive_params& params,
                              uint32_t seed_base = 0, agpt_adaptive_stats* astats = nullptr) const {
        agpt_render_params p{};
        p.width = acc.width;
        p.height = film_height;
        p.w = acc.width;
        p.h = film_height;
        p.seed_base = seed_base;
        p.max_depth = MaxDepth;
        p.accum_pitch = acc.width;
        p.interleave_block = share.block_rows;
        p.interleave_world = share.world;
        p.interleave_rank = share.rank;
        agpt_stats st{};
        check(agpt_render_adaptive(scene.handle(), &p, &params, acc.device_pixels(), acc.device_moment2(), &st, astats),
              "agpt_render_adaptive");
        return st;
    }
    agpt_stats RenderAdaptive(Scene& scene, AdaptiveAccumulator& acc, const agpt_adaptive_params& params, uint32_t seed_base = 0,
                              agpt_adaptive_stats* astats = nullptr) const {
        agpt_render_params p{};
        p.width = acc.width;
        p.height = acc.height;
        p.w = acc.width;
        p.h = acc.height;
        p.seed_base = seed_base;
        p.max_depth = MaxDepth;
        p.accum_pitch = acc.width;
        agpt_stats st{};
        check(agpt_render_adaptive(scene.handle(), &p, &params, acc.device_pixels(), acc.device_moment2(), &st, astats),
              "agpt_render_adaptive");
        return st;
    }
    // agpt_render_features over the whole film: one unjittered closest-hit query per pixel (no RNG, lens offset zero)
    void RenderFeatures(Scene& scene, FeatureBuffers& features) const {
        agpt_render_params p{};
        p.width = features.width;
        p.height = features.height;
        p.w = features.width;
        p.h = features.height;
        p.accum_pitch = features.width;
        check(agpt_render_features(scene.handle(), &p, features.device_albedo(), features.device_normal_depth()), "agpt_render_features");
    }
    // agpt_render_features_motion: RenderFeatures plus features.device_prev_point() from the same hits (Scene::SnapshotPositions first)
    void RenderFeaturesMotion(Scene& scene, FeatureBuffers& features) const {
        agpt_render_params p{};
        p.width = features.width;
        p.height = features.height;
        p.w = features.width;
        p.h = features.height;
        p.accum_pitch = features.width;
        check(agpt_render_features_motion(scene.handle(), &p, features.device_albedo(), features.device_normal_depth(), features.device_prev_point()),
              "agpt_render_features_motion");
    }
    // agpt_render_features_surface_motion: RenderFeaturesMotion plus features.device_prev_normal() (Scene::SnapshotSurfaces first)
    void RenderFeaturesSurfaceMotion(Scene& scene, FeatureBuffers& features) const {
        agpt_render_params p{};
        p.width = features.width;
        p.height = features.height;
        p.w = features.width;
        p.h = features.height;
        p.accum_pitch = features.width;
        check(agpt_render_features_surface_motion(scene.handle(), &p, features.device_albedo(), features.device_normal_depth(),
                                                  features.device_prev_point(), features.device_prev_normal()),
              "agpt_render_features_surface_motion");
    }
    // Integrator::Li(const Ray&, const Scene&) (integrator.h:28-31) for n rays -- what MyApp::Tick calls per pixel (myapp.cpp:168)
    // and the mouse-pick overlay per click (myapp.cpp:197-201).  rng[i] is the RandomFloat() state path i starts from and receives
    // the state it ends with (the reference keeps ONE such state, template/template.cpp:667: pass it for a single ray and store it
    // back to continue its stream).  radiance[i] is Li's return value, unfiltered.
    void Li(Scene& scene, const agpt_ray* rays, uint32_t* rng, int n, float3* radiance) const {
        std::vector<float> out(3 * (size_t)n);
        check(agpt_li_batch(scene.handle(), rays, rng, n, MaxDepth, out.data(), rng, nullptr), "agpt_li_batch");
        for (int i = 0; i < n; i++) radiance[i] = float3{out[3 * i], out[3 * i + 1], out[3 * i + 2]};
    }
    float3 Li(Scene& scene, const agpt_ray& ray, uint32_t& rng) const {
        float3 L{0.f, 0.f, 0.f};
        Li(scene, &ray, &rng, 1, &L);
        return L;
    }
    int MaxDepth;
};

// DbgIntegrator (integrator.h:107-118), the uv view MyApp can put on the left half of the split screen (myapp.cpp:129-130)
class DbgIntegrator {
public:
    void Li(Scene& scene, const agpt_ray* rays, int n, float3* radiance) const {
        std::vector<float> out(3 * (size_t)n);
        check(agpt_dbg_li_batch(scene.handle(), rays, n, out.data()), "agpt_dbg_li_batch");
        for (int i = 0; i < n; i++) radiance[i] = float3{out[3 * i], out[3 * i + 1], out[3 * i + 2]};
    }
    float3 Li(Scene& scene, const agpt_ray& ray) const {
        float3 L{0.f, 0.f, 0.f};
        Li(scene, &ray, 1, &L);
        return L;
    }
};

}  // namespace agpt
