// agpt_bvh_device.h -- the binned-SAH BVH of agpt_host_scene.cpp's build_bvh, built on the GPU (agpt_bvh_device.hip).
// The output is byte-identical to the host builder's for every input, max_prims_in_node and launch configuration.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/agpt.h"

namespace agpt {

// Builds the tree of the n_tris triangles (indices: (v, n, t) triplets, 3 per triangle, vertex ids already validated) on
// `stream`.  nodes_out needs 2 * n_tris + 2 entries of capacity (total + 1 are written, slot 1 zero), prim_index_out n_tris;
// either may be NULL.  *on_device = 0 when the input holds a non-finite referenced coordinate or its extent overflows,
// the one case the host builder runs instead (the folds of the device build are exact only on finite input).
// Returns AGPT_OK or AGPT_ERR_DEVICE / AGPT_ERR_NOMEM / AGPT_ERR_LIMIT with the message recorded.
int build_bvh_device(hipStream_t stream, const float* vertices, int n_vertices, const int32_t* indices, int n_tris,
                     int max_prims_in_node, agpt_bvh_node* nodes_out, int32_t* prim_index_out, int* total_nodes,
                     int* max_depth, int* on_device);

}  // namespace agpt
