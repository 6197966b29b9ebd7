// agpt_update.h -- agpt_scene_update_mesh's device path (agpt_update.hip): the records of ONE mesh of a committed scene -- its
// triangles' tri_verts / tri_shade entries, the bounds of its BVH nodes, its root box wherever the scene keeps a copy -- rewritten
// on the GPU for new vertex positions and normals, byte for byte what flatten_scene (agpt_host_scene.cpp) writes for them: both call
// the record writers of agpt_records.h and the box arithmetic of agpt_bvh_arith.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
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

// What the device path keeps per mesh between updates: indices, texture coordinates, prim_index, the tree's topology and per-level
// node lists (uploaded on the first update), positions / normals, the rest pose of agpt_scene_transform_mesh, agpt_scene_pose_mesh
// and agpt_scene_morph_mesh, the binding and palette of a skin, the deltas and active list of morph targets, the adjacency and face
// vectors of smooth normals, and the bounds in the reference layout.
struct MeshUpdater;
void mesh_updater_destroy(MeshUpdater*);

// Uploads the new arrays and rewrites the mesh's records on `stream`; *cache is created on the first call.  root6 receives the new
// root box (bmin, bmax).  Synchronises with the stream.  AGPT_OK or AGPT_ERR_DEVICE / _NOMEM / _INVALID with the message recorded.
int update_mesh_device(hipStream_t stream, MeshUpdater** cache, const HostMesh& mesh, const float* vertices, const float* normals,
                       const UpdateTarget& target, float root6[6]);
// The four device-resident front ends of the same rewrite (agpt_scene_update_mesh_device, agpt_scene_transform_mesh,
// agpt_scene_pose_mesh, agpt_scene_morph_mesh).  Each leaves the new arrays in the cache's own buffers without synchronising:
//   copy_arrays_device       device-to-device copies of the caller's packed xyz arrays, enqueued on `stream`;
//   transform_arrays_device  k_transform_mesh: the rest pose through M (positions) and N = inverse_transpose(M) (normals).  The rest
//                            arrays are uploaded from the host vectors when the cache holds none (the first call, and the first
//                            after drop_rest) and kept; otherwise the vectors are only measured.
//   skin_arrays_device       k_skin_mesh: the rest pose through the palette (agpt_skin.h) and the binding's influences.  The rest
//                            arrays as above; the binding is uploaded when the cache holds none (the first pose, the first after drop_skin
//                            or after the cache was destroyed) and kept; the palette goes up with every call, and the caller keeps
//                            it until the stream is synchronised.  num_cus sizes the grid.
//   morph_arrays_device      k_morph_mesh: the rest pose plus the active targets' deltas (agpt_morph.h) and, with `skin` and `palette`
//                            (both or neither), through the skin in the same kernel.  Rest arrays and binding as above; the targets'
//                            deltas are uploaded when the cache holds none (the first morph, the first after drop_morph or after the
//                            cache was destroyed) and kept; `active` (and the palette) go up with every call, and the caller keeps
//                            them until the stream is synchronised.
// refit_device_arrays then rewrites the mesh's records from those buffers like update_mesh_device; *finite is false if any of the
// 3 * n_vertices coordinates is Inf or NaN (k_check_finite), and the caller must then replace the records through the host path.
// Only the flag and the root box come back.  download_arrays fetches the buffers' contents (vertices / normals keep their sizes).
int copy_arrays_device(hipStream_t stream, MeshUpdater** cache, const HostMesh& mesh, const float* vertices_dev, const float* normals_dev);
int transform_arrays_device(hipStream_t stream, MeshUpdater** cache, const HostMesh& mesh, const std::vector<v3>& rest_vertices,
                            const std::vector<v3>& rest_normals, const Mat4& M, const Mat4& N, bool with_normals);
int skin_arrays_device(hipStream_t stream, MeshUpdater** cache, const HostMesh& mesh, const std::vector<v3>& rest_vertices,
                       const std::vector<v3>& rest_normals, const SkinBinding& skin, const std::vector<float>& palette, int num_cus,
                       bool with_normals);
int morph_arrays_device(hipStream_t stream, MeshUpdater** cache, const HostMesh& mesh, const std::vector<v3>& rest_vertices,
                        const std::vector<v3>& rest_normals, const MorphTargets& morph, const std::vector<MorphActive>& active,
                        const SkinBinding* skin, const std::vector<float>* palette, int num_cus, bool with_normals);
// AGPT_NORMALS_SMOOTH.  The three kernels above take with_normals == false for a mesh in that mode: their normal halves get an item
// count of zero and the palette carries M only (stride 13).  copy_arrays_device accepts normals_dev == NULL (room is made, nothing is
// copied), and upload_positions_device is its host-array form (the caller keeps `vertices` until the stream is synchronised).
// smooth_normals_device then writes the cache's normals buffer from its positions: k_face_normals and k_vertex_normals
// (agpt_normals.h), enqueued on `stream` without synchronising.  The CSR adjacency of the normal items is built on the host and
// uploaded when the cache holds none (the mesh's first smooth update, and the first after a REBUILD destroyed the cache) and kept.
int upload_positions_device(hipStream_t stream, MeshUpdater** cache, const HostMesh& mesh, const float* vertices);
int smooth_normals_device(hipStream_t stream, MeshUpdater* cache, const HostMesh& mesh);
int refit_device_arrays(hipStream_t stream, MeshUpdater* cache, const HostMesh& mesh, const UpdateTarget& target, float root6[6], bool* finite);
void drop_rest(MeshUpdater* cache);   // the rest pose changed (NULL is fine)
void drop_skin(MeshUpdater* cache);   // the binding changed: its device copies are freed (NULL is fine)
void drop_morph(MeshUpdater* cache);  // the targets changed: their device copies are freed (NULL is fine)
int download_arrays(hipStream_t stream, const MeshUpdater* cache, std::vector<v3>& vertices, std::vector<v3>& normals);
// mesh.nodes' bounds from the last update_mesh_device of this cache (the host mirror is brought up to date on demand)
int download_bounds(hipStream_t stream, const MeshUpdater* cache, HostMesh& mesh);

}  // namespace agpt
