// agpt_update.h -- agpt_scene_update_mesh's device path (agpt_update.hip): the records of ONE mesh of a committed scene -- its
// triangles' tri_verts / tri_shade entries, the bounds of its BVH nodes, its root box wherever the scene keeps a copy -- rewritten
// on the GPU for new vertex positions and normals, byte for byte what flatten_scene (agpt_host_scene.cpp) writes for them: both call
// the record writers of agpt_records.h and the box arithmetic of agpt_bvh_arith.h.  MeshUpdate is the one owner of what a mesh keeps
// between such calls, on the host and on the device; MeshUpdate::deform is the one launcher of the kernels that make new arrays from
// the rest pose.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "agpt_host_scene.hpp"
#include "agpt_morph.h"
#include "agpt_records.h"
#include "agpt_skin.h"
#include "agpt_transform.h"

namespace agpt {

// Where one mesh lives in the committed scene's device arrays (agpt_scene.h).
struct UpdateTarget {
    float4* nodes;
    float4* tri_verts;
    float4* tri_shade;
    DevPrim* prim;         // the mesh's own record
    float4* rootpair;      // its root-pair record (4 float4), or NULL
    float4* prefilter;     // its prefilter record (2 float4), or NULL
    uint32_t node_base, tri_base, prim_id;
};

// What a frame asks of MeshUpdate::deform.  One of three shapes: M and N (agpt_scene_transform_mesh: N = inverse_transpose(M)); `palette`
// (agpt_scene_pose_mesh: agpt_skin.h's packed palette for the state's binding); `active` (agpt_scene_morph_mesh: the frame's (target,
// weight) pairs for the state's targets), with `palette` as well when the morph runs on through the skin.  Either of the two may come
// in its device-pointer form instead.  The caller keeps what the pointers name until the stream is synchronised.
// The status words of a request whose joint matrices or weights are in device memory (k_pack_palette, k_morph_active): each the lowest
// offending index, kNoItem for none; 20 bytes, the one download of MeshUpdate::device_inputs.  The order of the first three is the
// order in which agpt_scene_pose_mesh refuses.
constexpr uint32_t kNoItem = 0xFFFFFFFFu;
struct DeviceInputStatus {
    uint32_t nonfinite_joint = kNoItem, bad_row_joint = kNoItem, singular_joint = kNoItem;
    uint32_t n_active = 0;     // the pairs k_morph_active wrote
    uint32_t nonfinite_weight = kNoItem;
    bool clean() const { return nonfinite_joint == kNoItem && bad_row_joint == kNoItem && singular_joint == kNoItem && nonfinite_weight == kNoItem; }
};

struct DeformRequest {
    const char* fn;            // the entry point, named in the messages
    const Mat4 *M = nullptr, *N = nullptr;
    const std::vector<float>* palette = nullptr;
    const std::vector<MorphActive>* active = nullptr;
    // The device-pointer forms of `palette` and `active` (agpt_scene_pose_mesh_device, agpt_scene_morph_mesh_device): n_joints row-major
    // 4x4 (16-byte aligned) and n_targets weights in device memory, complete or produced on the stream.  MeshUpdate::device_inputs turns
    // them into the cache's palette and active list and fills *status; deform takes the request only with a clean status.
    const float* joints16_dev = nullptr;
    int n_joints = 0;
    const float* weights_dev = nullptr;
    int n_targets = 0;
    DeviceInputStatus* status = nullptr;
    bool with_normals = true;  // false for a mesh in AGPT_NORMALS_SMOOTH mode: the normal halves get an item count of zero and the palette
                               // carries M only (stride 13)
    int num_cus = 1;           // sizes the grids of k_skin_mesh and k_morph_mesh
};

struct MeshDeviceCache;   // agpt_update.hip

// Everything agpt_scene_update_mesh and its front ends keep per mesh between calls, behind ONE owner (one per mesh of a scene, added
// with it by agpt_scene_add_mesh).
//   host    the rest pose of transform / pose / morph (a copy of the arrays the mesh last received explicitly, taken by the first of
//           those calls after them), the binding of agpt_scene_set_mesh_skin, the targets of agpt_scene_set_mesh_morph_targets, the
//           normals mode, and what the mirror (HostMesh) lacks: bounds_stale -- the bounds of HostMesh::nodes are behind the device's,
//           root box excepted --, arrays_stale -- HostMesh::vertices / normals are as well (a REFIT whose new arrays exist only on the
//           device).  The scene's sync_mirror brings both up to date (DESIGN.md section 5.7 lists who reads the mirror).
//   device  the cache, created by the mesh's first REFIT: indices, texture coordinates, prim_index, the tree's topology and per-level
//           node lists, positions / normals, the bounds in the reference layout, and -- each uploaded by the first call that needs it
//           and kept -- the rest pose, the binding, the targets' deltas, the CSR adjacency of smooth normals; per call the palette, the
//           active list and the face vectors.
// The host copies change only through the four methods below, and each drops the device copies that were made from them: no caller
// can invalidate one side without the other.  The methods that free device memory need the scene's device current (on_device()).
class MeshUpdate {
public:
    bool bounds_stale = false, arrays_stale = false;
    int normals_mode = 0;   // AGPT_NORMALS_GIVEN / _SMOOTH (agpt_scene_set_mesh_normals_mode)

    MeshUpdate();
    MeshUpdate(MeshUpdate&& o) noexcept;
    ~MeshUpdate();

    bool has_rest() const { return rest_valid_; }
    const SkinBinding& skin() const { return skin_; }
    const MorphTargets& morph() const { return morph_; }
    bool on_device() const { return dev_ != nullptr; }

    void arrays_given();                                                                   // explicit arrays: the rest pose is forgotten
    void rest_taken(const std::vector<v3>& vertices, const std::vector<v3>& normals);     // ... and these are the new one
    void skin_changed(SkinBinding&& skin);
    void morph_changed(MorphTargets&& morph);
    void topology_changed();   // a REBUILD: the whole cache goes; the mirror has just been written, so nothing of it is stale

    // The device path.  Every call returns AGPT_OK or AGPT_ERR_DEVICE / _NOMEM / _INVALID with the message recorded; the cache is created
    // by the first that needs it.
    // update: uploads the new arrays and rewrites the mesh's records on `stream`; root6 receives the new root box (bmin, bmax).
    // Synchronises with the stream.
    int update(hipStream_t stream, const HostMesh& mesh, const float* vertices, const float* normals, const UpdateTarget& target, float root6[6]);
    // The front ends of the same rewrite leave the new arrays in the cache's own buffers without synchronising:
    //   copy_arrays       device-to-device copies of the caller's packed xyz arrays; normals_dev == NULL (SMOOTH mode): room is made,
    //                     nothing is copied
    //   upload_positions  its host-array form for SMOOTH mode (the caller keeps `vertices` until the stream is synchronised)
    //   deform            k_transform_mesh, k_skin_mesh or k_morph_mesh by the request, from the rest pose
    //   smooth_normals    then writes the normals buffer from the positions: k_face_normals and k_vertex_normals (agpt_normals.h)
    // refit then rewrites the mesh's records from those buffers like update; *finite is false if any of the 3 * n_vertices coordinates
    // is Inf or NaN (k_check_finite), and the caller must then replace the records through the host path.  Only the flag and the root
    // box come back.
    int copy_arrays(hipStream_t stream, const HostMesh& mesh, const float* vertices_dev, const float* normals_dev);
    int upload_positions(hipStream_t stream, const HostMesh& mesh, const float* vertices);
    int deform(hipStream_t stream, const HostMesh& mesh, const DeformRequest& rq);
    // The front end of a request with device pointers, ahead of deform (k_check_spheres -> synchronise -> k_update_spheres' shape,
    // agpt_analytic.hip): k_pack_palette writes the cache's palette from rq.joints16_dev, k_morph_active its active list from
    // rq.weights_dev, and the status words come back in one download (*rq.status).  Synchronises with the stream.  Reads rq.with_normals;
    // touches nothing but the palette, the active list and the status words, which every call overwrites.
    int device_inputs(hipStream_t stream, const HostMesh& mesh, const DeformRequest& rq);
    int smooth_normals(hipStream_t stream, const HostMesh& mesh);
    int refit(hipStream_t stream, const HostMesh& mesh, const UpdateTarget& target, float root6[6], bool* finite);
    // the buffers' contents (vertices / normals keep their sizes), and mesh.nodes' bounds from the last refit
    int download_arrays(hipStream_t stream, std::vector<v3>& vertices, std::vector<v3>& normals) const;
    int download_bounds(hipStream_t stream, HostMesh& mesh) const;

private:
    int ensure_cache(hipStream_t stream, const HostMesh& mesh);
    int ensure_rest(const char* fn, hipStream_t stream, const HostMesh& mesh);

    bool rest_valid_ = false;
    std::vector<v3> rest_vertices_, rest_normals_;
    SkinBinding skin_;
    MorphTargets morph_;
    std::unique_ptr<MeshDeviceCache> dev_;
};

// The launches of the two front-end kernels, for device_inputs and for the known-answer entry points (agpt_kat.hip), which run the very
// kernels the scene calls run.  Everything is device memory; nothing is synchronised.
//   launch_pack_palette  joints16_dev (16-byte aligned) -> palette_dev, n_joints * skin_palette_stride(with_normals) floats in
//                        skin_pack_palette's layout; status3_dev must hold kNoItem three times and receives DeviceInputStatus' first three.
//   launch_morph_active  weights_dev (1 .. kMorphMaxTargets) -> active_dev (room for n_targets pairs), morph_active_list's bytes;
//                        status2_dev receives n_active and the lowest index of a non-finite weight (kNoItem: none).
int launch_pack_palette(hipStream_t stream, const float* joints16_dev, int n_joints, bool with_normals, float* palette_dev, uint32_t* status3_dev);
int launch_morph_active(hipStream_t stream, const float* weights_dev, int n_targets, MorphActive* active_dev, uint32_t* status2_dev);

}  // namespace agpt
