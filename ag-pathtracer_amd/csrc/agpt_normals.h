// agpt_normals.h -- smooth vertex normals from positions and topology.  ONE source for agpt_vertex_normals_arrays (host, agpt_obj.cpp),
// for the host path of a mesh in AGPT_NORMALS_SMOOTH mode (agpt_scene_api.hip) and for k_face_normals / k_vertex_normals
// (agpt_update.hip): every unit compiles with -ffp-contract=off and correctly rounded divide and square root, every operation is fp32
// and rounds on its own, so all three produce the same bits.
//
//   a mesh has corners q = 0 .. n_corners-1, each a (vertex, normal, texcoord) triplet as in agpt_scene_add_mesh; triangle t owns the
//   corners 3t, 3t+1, 3t+2.
//   face vector   g_t = cross(p_b - p_a, p_c - p_a), with a, b, c the vertex indices of the corners 3t, 3t+1, 3t+2: area-weighted, not
//                 normalised (face_vector).
//   normal item j the corners in ascending q whose normal index is j: the first sets acc = g_(q/3), every later one acc = acc + g_(q/3)
//                 per component.  A triangle that names j at two corners contributes twice.  The ORDER is part of the definition (fp32
//                 sums do not commute in their roundings): both sides walk the same CSR adjacency (normal_adjacency), which lists an
//                 item's triangles in ascending corner order (vertex_normal).
//   finish        l2 = dot(acc, acc); (+0, +0, +0) if no corner names j, if !(l2 > 0) or if l2 is not finite; otherwise
//                 acc * (1.0f / sqrtf(l2)), normalize's operations (normal_finish).
//
// The zero vector is a defined, harmless value: shade_path reads an interpolated normal of zero as "use the geometric normal"
// (agpt_shade.h).  So a normal item that no corner names, a fan of zero-area triangles, faces that cancel exactly, a sum whose square
// underflows to 0 (|acc| below about 2^-75) or overflows to Inf (|acc| above 2^64) and a NaN or Inf position all give (+0, +0, +0) at
// the items they reach and nothing else anywhere; no fallback array is needed, and non-finite positions are not refused.
//
// Limit: an item of very high valence is walked by one lane (one thread on the host).  Correct and slow; a cooperative reduction
// would need an order-preserving tree and with it a second definition.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "agpt_math.h"

namespace agpt {

AGPT_HD v3 face_vector(v3 pa, v3 pb, v3 pc) { return cross(pb - pa, pc - pa); }

AGPT_HD v3 normal_finish(v3 acc, bool any) {
    const float l2 = dot(acc, acc);
    if (!any || !(l2 > 0.f) || !(l2 <= AGPT_FLT_MAX)) return V3(0.f, 0.f, 0.f);   // (a NaN fails both comparisons)
    const float inv = 1.0f / sqrtf(l2);
    return acc * inv;
}

// normal item j: its incident triangles are corner_tri[offsets[j] .. offsets[j + 1]), g their face vectors (w unused)
AGPT_HD v3 vertex_normal(const int32_t* offsets, const int32_t* corner_tri, const float4* g, size_t j) {
    const int32_t begin = offsets[j], end = offsets[j + 1];
    v3 acc = V3(0.f, 0.f, 0.f);
    for (int32_t k = begin; k < end; k++) {
        const float4 f = g[corner_tri[k]];
        const v3 gt = V3(f.x, f.y, f.z);
        acc = k == begin ? gt : acc + gt;
    }
    return normal_finish(acc, end > begin);
}

// ---- host side: the adjacency and the whole walk ----

// CSR over the normal items: offsets[n_normals + 1], corner_tri[n_corners] = q / 3 of the corners q that name the item, ascending in q
// (a stable counting sort).  `indices` are n_corners checked triplets.
inline void normal_adjacency(const int32_t* indices, size_t n_corners, size_t n_normals, std::vector<int32_t>& offsets,
                             std::vector<int32_t>& corner_tri) {
    offsets.assign(n_normals + 1, 0);
    corner_tri.assign(n_corners, 0);
    for (size_t q = 0; q < n_corners; q++) offsets[(size_t)indices[3 * q + 1] + 1]++;
    for (size_t j = 0; j < n_normals; j++) offsets[j + 1] += offsets[j];
    std::vector<int32_t> next(offsets.begin(), offsets.end() - 1);
    for (size_t q = 0; q < n_corners; q++) corner_tri[(size_t)next[(size_t)indices[3 * q + 1]]++] = (int32_t)(q / 3);
}

// the definition, start to end: 3 * n_normals floats into normals_out (checked arguments; vertices is not normals_out)
inline void vertex_normals_host(const float* vertices, const int32_t* indices, size_t n_corners, size_t n_normals, float* normals_out) {
    std::vector<int32_t> offsets, corner_tri;
    normal_adjacency(indices, n_corners, n_normals, offsets, corner_tri);
    const size_t n_tris = n_corners / 3;
    std::vector<float4> g(n_tris);
    auto at = [&](int32_t v) { return V3(vertices[3 * (size_t)v], vertices[3 * (size_t)v + 1], vertices[3 * (size_t)v + 2]); };
    for (size_t t = 0; t < n_tris; t++) {
        const v3 f = face_vector(at(indices[9 * t]), at(indices[9 * t + 3]), at(indices[9 * t + 6]));
        g[t] = make_float4(f.x, f.y, f.z, 0.f);
    }
    for (size_t j = 0; j < n_normals; j++) {
        const v3 n = vertex_normal(offsets.data(), corner_tri.data(), g.data(), j);
        normals_out[3 * j] = n.x;
        normals_out[3 * j + 1] = n.y;
        normals_out[3 * j + 2] = n.z;
    }
}

}  // namespace agpt
