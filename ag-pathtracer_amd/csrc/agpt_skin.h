// agpt_skin.h -- linear-blend skinning of a mesh's rest arrays by a palette of joint matrices, built on transform_point /
// transform_vector / inverse_transpose of agpt_transform.h.  ONE source for agpt_skin_arrays (host, agpt_obj.cpp) and k_skin_mesh
// (agpt_update.hip, agpt_scene_pose_mesh): both units compile with -ffp-contract=off and a correctly rounded divide, every operation
// is fp32 and rounds on its own, so the two produce the same bits.
//
//   vertex i has K influences (joint[i][k], weight[i][k]), k = 0 .. K-1, flat arrays of stride K; joint j has a row-major 4x4 M_j with
//   the last row (0, 0, 0, 1) and N_j = inverse_transpose(M_j), formed on the host (skin_pack_palette) or, for matrices given in device
//   memory, by k_pack_palette (agpt_update.hip): the same function, the same floats.
//   position   the slots in order; a slot whose weight is exactly 0 (either sign) is skipped; the first used slot sets
//              acc = w * transform_point(M_j, p) per component, every later one acc = acc + w * transform_point(M_j, p); a vertex
//              without a used slot keeps its rest position.  Weights are used as given (not normalised, not reordered).
//   normal     the same walk with transform_vector(N_j, n) and the normal's own influences; not renormalised.
// One used slot of weight 1 therefore gives the bits of agpt_transform_arrays(M_j, ...), and so do two slots of 0.5 with one matrix
// (0.5 * t is exact, and t/2 + t/2 = t).
//
// The palette is what both sides read: per joint `stride` floats -- rows 0..2 of M (12 floats), then, for a mesh with normals, the
// 3x3 of N (9 floats).  The stride is odd (21, or 13 without N): k_skin_mesh keeps the palette in LDS, and an odd stride spreads
// different joints over the banks (agpt_update.hip's header).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "agpt_transform.h"

namespace agpt {

constexpr int kSkinMaxInfluences = 8;
constexpr int kSkinMaxJoints = 65536;

AGPT_HD int skin_palette_stride(bool with_normals) { return with_normals ? 21 : 13; }

// transform_point with the joint's M: the last row is (0, 0, 0, 1) by contract and is evaluated like any other (w is 1 for a finite
// position and NaN for a non-finite one, as in agpt_transform_arrays)
AGPT_HD void skin_joint_point(const float* e, const float p[3], float out[3]) {
    Mat4 M;
    for (int i = 0; i < 12; i++) M.c[i] = e[i];
    M.c[12] = M.c[13] = M.c[14] = 0.f;
    M.c[15] = 1.f;
    transform_point(M, p, out);
}
AGPT_HD void skin_joint_vector(const float* e, const float n[3], float out[3]) {
    Mat4 N;
    for (int i = 0; i < 16; i++) N.c[i] = 0.f;   // (transform_vector reads the 3x3 only)
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) N.c[4 * r + c] = e[12 + 3 * r + c];
    transform_vector(N, n, out);
}

// one vertex (kPoint) or one normal: `joints` / `weights` are its K slots
template <bool kPoint>
AGPT_HD void skin_blend(const float* palette, int stride, const int32_t* joints, const float* weights, int K, const float rest[3], float out[3]) {
    float acc[3] = {rest[0], rest[1], rest[2]};
    bool used = false;
    for (int k = 0; k < K; k++) {
        const float w = weights[k];
        if (w == 0) continue;
        const float* e = palette + (size_t)joints[k] * (size_t)stride;
        float t[3];
        if (kPoint)
            skin_joint_point(e, rest, t);
        else
            skin_joint_vector(e, rest, t);
        if (!used) {
            for (int c = 0; c < 3; c++) acc[c] = w * t[c];
            used = true;
        } else {
            for (int c = 0; c < 3; c++) acc[c] = acc[c] + w * t[c];
        }
    }
    out[0] = acc[0];
    out[1] = acc[1];
    out[2] = acc[2];
}

// ---- host side: the binding, its checks and the palette ----

// A mesh's binding (agpt_scene_set_mesh_skin): influences == 0 is "no skin".  normal_* are empty when the vertex influences serve the
// normals as well (n_normals == n_vertices and none given) or the mesh has no normals.
struct SkinBinding {
    int influences = 0, n_joints = 0;
    std::vector<int32_t> vertex_joints, normal_joints;
    std::vector<float> vertex_weights, normal_weights;
};

// The checks agpt_skin_arrays and agpt_scene_set_mesh_skin share; each returns the message of the refusal, or "" when all is well.
inline std::string skin_check_counts(int influences, int n_joints) {
    if (influences < 1 || influences > kSkinMaxInfluences)
        return "influences is " + std::to_string(influences) + ", outside 1 .. " + std::to_string(kSkinMaxInfluences);
    if (n_joints < 1 || n_joints > kSkinMaxJoints) return "n_joints is " + std::to_string(n_joints) + ", outside 1 .. " + std::to_string(kSkinMaxJoints);
    return "";
}
inline std::string skin_check_influences(const char* what, int influences, int n_joints, size_t n, const int32_t* joints, const float* weights) {
    auto where = [&](size_t i) { return std::string(what) + " " + std::to_string(i / (size_t)influences) + ", slot " + std::to_string(i % (size_t)influences); };
    for (size_t i = 0; i < n * (size_t)influences; i++) {
        if (joints[i] < 0 || joints[i] >= n_joints)
            return "joint index " + std::to_string(joints[i]) + " out of range (" + where(i) + "; " + std::to_string(n_joints) + " joints)";
        if (!std::isfinite(weights[i])) return "non-finite weight (" + where(i) + ")";
        if (weights[i] < 0) return "negative weight (" + where(i) + ")";   // (-0.0 is a zero weight: the slot is skipped)
    }
    return "";
}
inline std::string skin_check_last_rows(const float* joints16, int n_joints) {
    for (int j = 0; j < n_joints; j++) {
        const float* r = joints16 + 16 * (size_t)j + 12;
        if (!(r[0] == 0 && r[1] == 0 && r[2] == 0 && r[3] == 1))
            return "the last row of joint " + std::to_string(j) + " is not (0, 0, 0, 1)";
    }
    return "";
}

// The palette of n_joints row-major 4x4: M's rows 0..2 and, with normals, the 3x3 of inverse_transpose(M) (a determinant of exactly 0
// gives the identity, the reference's rule).  *singular (may be NULL) receives the first joint whose determinant is exactly 0, or -1.
inline std::vector<float> skin_pack_palette(const float* joints16, int n_joints, bool with_normals, int* singular) {
    const int stride = skin_palette_stride(with_normals);
    std::vector<float> palette((size_t)n_joints * (size_t)stride, 0.f);
    if (singular) *singular = -1;
    for (int j = 0; j < n_joints; j++) {
        Mat4 M;
        for (int i = 0; i < 16; i++) M.c[i] = joints16[16 * (size_t)j + i];
        float det = 0;
        const Mat4 N = inverse_transpose(M, &det);
        if (det == 0 && singular && *singular < 0) *singular = j;
        float* e = palette.data() + (size_t)j * (size_t)stride;
        for (int i = 0; i < 12; i++) e[i] = M.c[i];
        if (with_normals)
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) e[12 + 3 * r + c] = N.c[4 * r + c];
    }
    return palette;
}

}  // namespace agpt
