// agpt_transform.h -- the reference's mat4 applied to a mesh's arrays (TriangleMesh::LoadObj, trianglemesh.cpp:208-217): positions
// through mat4::TransformPoint, normals through TransformVector of Inverted().Transposed() (template/precomp.h:940-990, 1020-1040).
// ONE source for agpt_obj.cpp (the OBJ loader's `transform16`), agpt_transform_arrays (host) and k_transform_mesh (agpt_update.hip,
// agpt_scene_transform_mesh): every operation rounded on its own -- all three units compile with -ffp-contract=off and a correctly
// rounded divide --, so the three produce the same bits; pinned to the reference's mat4 by tests/golden/obj_cases.npz.
//
// inverse_transpose() evaluates the 4x4 cofactor expansion of Mesa's gluInvertMatrix (SGI Free Software License B), the form the
// reference's mat4::Inverted uses (template/precomp.h:948-990): the operation order decides the rounded normals.
#pragma once

#include "agpt_math.h"

namespace agpt {

struct Mat4 {
    float c[16];   // row-major
};

AGPT_HD Mat4 mat4_identity() {
    Mat4 m;
    for (int i = 0; i < 16; i++) m.c[i] = (i % 5 == 0) ? 1.f : 0.f;
    return m;
}

// mat4::Inverted (the MESA cofactor expansion) followed by ::Transposed (3x3 part).  *det_out (may be NULL) receives the determinant
// the expansion computes; a matrix whose determinant is exactly 0 inverts to the identity, as in the reference.  Host and device
// (k_pack_palette, agpt_update.hip) evaluate this one text, in this order.
AGPT_HD Mat4 inverse_transpose(const Mat4& M, float* det_out = nullptr) {
    const float* cell = M.c;
    const float inv[16] = {
        cell[5] * cell[10] * cell[15] - cell[5] * cell[11] * cell[14] - cell[9] * cell[6] * cell[15] + cell[9] * cell[7] * cell[14] + cell[13] * cell[6] * cell[11] - cell[13] * cell[7] * cell[10],
        -cell[1] * cell[10] * cell[15] + cell[1] * cell[11] * cell[14] + cell[9] * cell[2] * cell[15] - cell[9] * cell[3] * cell[14] - cell[13] * cell[2] * cell[11] + cell[13] * cell[3] * cell[10],
        cell[1] * cell[6] * cell[15] - cell[1] * cell[7] * cell[14] - cell[5] * cell[2] * cell[15] + cell[5] * cell[3] * cell[14] + cell[13] * cell[2] * cell[7] - cell[13] * cell[3] * cell[6],
        -cell[1] * cell[6] * cell[11] + cell[1] * cell[7] * cell[10] + cell[5] * cell[2] * cell[11] - cell[5] * cell[3] * cell[10] - cell[9] * cell[2] * cell[7] + cell[9] * cell[3] * cell[6],
        -cell[4] * cell[10] * cell[15] + cell[4] * cell[11] * cell[14] + cell[8] * cell[6] * cell[15] - cell[8] * cell[7] * cell[14] - cell[12] * cell[6] * cell[11] + cell[12] * cell[7] * cell[10],
        cell[0] * cell[10] * cell[15] - cell[0] * cell[11] * cell[14] - cell[8] * cell[2] * cell[15] + cell[8] * cell[3] * cell[14] + cell[12] * cell[2] * cell[11] - cell[12] * cell[3] * cell[10],
        -cell[0] * cell[6] * cell[15] + cell[0] * cell[7] * cell[14] + cell[4] * cell[2] * cell[15] - cell[4] * cell[3] * cell[14] - cell[12] * cell[2] * cell[7] + cell[12] * cell[3] * cell[6],
        cell[0] * cell[6] * cell[11] - cell[0] * cell[7] * cell[10] - cell[4] * cell[2] * cell[11] + cell[4] * cell[3] * cell[10] + cell[8] * cell[2] * cell[7] - cell[8] * cell[3] * cell[6],
        cell[4] * cell[9] * cell[15] - cell[4] * cell[11] * cell[13] - cell[8] * cell[5] * cell[15] + cell[8] * cell[7] * cell[13] + cell[12] * cell[5] * cell[11] - cell[12] * cell[7] * cell[9],
        -cell[0] * cell[9] * cell[15] + cell[0] * cell[11] * cell[13] + cell[8] * cell[1] * cell[15] - cell[8] * cell[3] * cell[13] - cell[12] * cell[1] * cell[11] + cell[12] * cell[3] * cell[9],
        cell[0] * cell[5] * cell[15] - cell[0] * cell[7] * cell[13] - cell[4] * cell[1] * cell[15] + cell[4] * cell[3] * cell[13] + cell[12] * cell[1] * cell[7] - cell[12] * cell[3] * cell[5],
        -cell[0] * cell[5] * cell[11] + cell[0] * cell[7] * cell[9] + cell[4] * cell[1] * cell[11] - cell[4] * cell[3] * cell[9] - cell[8] * cell[1] * cell[7] + cell[8] * cell[3] * cell[5],
        -cell[4] * cell[9] * cell[14] + cell[4] * cell[10] * cell[13] + cell[8] * cell[5] * cell[14] - cell[8] * cell[6] * cell[13] - cell[12] * cell[5] * cell[10] + cell[12] * cell[6] * cell[9],
        cell[0] * cell[9] * cell[14] - cell[0] * cell[10] * cell[13] - cell[8] * cell[1] * cell[14] + cell[8] * cell[2] * cell[13] + cell[12] * cell[1] * cell[10] - cell[12] * cell[2] * cell[9],
        -cell[0] * cell[5] * cell[14] + cell[0] * cell[6] * cell[13] + cell[4] * cell[1] * cell[14] - cell[4] * cell[2] * cell[13] - cell[12] * cell[1] * cell[6] + cell[12] * cell[2] * cell[5],
        cell[0] * cell[5] * cell[10] - cell[0] * cell[6] * cell[9] - cell[4] * cell[1] * cell[10] + cell[4] * cell[2] * cell[9] + cell[8] * cell[1] * cell[6] - cell[8] * cell[2] * cell[5]};
    const float det = cell[0] * inv[0] + cell[1] * inv[4] + cell[2] * inv[8] + cell[3] * inv[12];
    if (det_out) *det_out = det;
    Mat4 I = mat4_identity();
    if (det != 0) {
        const float invdet = 1.0f / det;
        for (int i = 0; i < 16; i++) I.c[i] = inv[i] * invdet;
    }
    Mat4 T = mat4_identity();  // Transposed(): 3x3 part only, the rest stays identity (template/precomp.h:940-947)
    T.c[0] = I.c[0]; T.c[1] = I.c[4]; T.c[2] = I.c[8];
    T.c[4] = I.c[1]; T.c[5] = I.c[5]; T.c[6] = I.c[9];
    T.c[8] = I.c[2]; T.c[9] = I.c[6]; T.c[10] = I.c[10];
    return T;
}

AGPT_HD void transform_point(const Mat4& M, const float v[3], float out[3]) {
    const float* c = M.c;
    float rx = c[0] * v[0] + c[1] * v[1] + c[2] * v[2] + c[3];
    float ry = c[4] * v[0] + c[5] * v[1] + c[6] * v[2] + c[7];
    float rz = c[8] * v[0] + c[9] * v[1] + c[10] * v[2] + c[11];
    const float w = c[12] * v[0] + c[13] * v[1] + c[14] * v[2] + c[15];
    if (w == 1) {
        out[0] = rx; out[1] = ry; out[2] = rz;
        return;
    }
    const float iw = 1.f / w;
    out[0] = rx * iw; out[1] = ry * iw; out[2] = rz * iw;
}
AGPT_HD void transform_vector(const Mat4& M, const float v[3], float out[3]) {
    const float* c = M.c;
    out[0] = c[0] * v[0] + c[1] * v[1] + c[2] * v[2];
    out[1] = c[4] * v[0] + c[5] * v[1] + c[6] * v[2];
    out[2] = c[8] * v[0] + c[9] * v[1] + c[10] * v[2];
}

}  // namespace agpt
