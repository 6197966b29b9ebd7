// agpt_records.h -- the writers of the records agpt_scene.h lays out: ONE definition for flatten_scene (agpt_host_scene.cpp, a whole
// scene on the host) and for the kernels of agpt_update.hip (one mesh of a committed scene on the device), so the two write the same
// bytes.  Both units compile with -ffp-contract=off and correctly rounded divide / square root.
#pragma once

#include <vector>

#include "agpt_scene.h"

namespace agpt {

AGPT_HD float bits_as_float(uint32_t u) { return __builtin_bit_cast(float, u); }

// ---- nodes: the 64-B sibling-pair record, as 16 floats ---------------------------------------------------------------------
AGPT_HD void pair_record_set_box(float* rec, size_t side, const float lo[3], const float hi[3]) {
    for (int a = 0; a < 3; a++) {
        rec[2 * a + side] = lo[a];
        rec[6 + 2 * a + side] = hi[a];
    }
}
AGPT_HD void pair_record_set_enc(float* rec, size_t side, uint32_t z, uint32_t w) {
    rec[12 + side] = bits_as_float(z);
    rec[14 + side] = bits_as_float(w);
}
// a mesh's root pair (DevScene::rootpair_base): the root box on both sides (the right one is ignored)
AGPT_HD void rootpair_record_set_box(float* rec, const float lo[3], const float hi[3]) {
    pair_record_set_box(rec, 0, lo, hi);
    pair_record_set_box(rec, 1, lo, hi);
}
// a mesh's prefilter record (DevScene::prefilter), as 8 floats; .w of the first half (the bit index) is the caller's
AGPT_HD void prefilter_record_set_box(float* rec, const float lo[3], const float hi[3]) {
    for (int a = 0; a < 3; a++) {
        rec[a] = lo[a];
        rec[4 + a] = hi[a];
    }
}

// The traversal encoding of a node whose `first` is already global (a triangle slot for a leaf, a node index otherwise); a leaf too
// big for the inline form gets the next entry of `bigleaves`.
inline uint32_t node_encoding(uint32_t first, int count, std::vector<uint32_t>& bigleaves) {
    if (count == 0) return first;
    if (count <= 7 && first < 0x10000000u) return AGPT_ENC_LEAF | ((uint32_t)(count - 1) << 28) | first;
    const uint32_t k = (uint32_t)(bigleaves.size() / 2);
    bigleaves.push_back(first);
    bigleaves.push_back((uint32_t)count);
    return AGPT_ENC_BIGLEAF | k;
}

// ---- triangles -------------------------------------------------------------------------------------------------------------
// the texture coordinates of a mesh without any (trianglemesh.cpp:52-56)
AGPT_HD void default_uv(v2& uv0, v2& uv1, v2& uv2) {
    uv0.x = 0; uv0.y = 0;
    uv1.x = 1; uv1.y = 0;
    uv2.x = 1; uv2.y = 1;
}

// The ray-independent part of TriangleIntersect (trianglemesh.cpp:46-80 + the SurfaceInteraction ctor, intersectable.h:69): uv
// deltas, dpdu / dpdv, the degenerate branches, the geometric normal and ss = normalize(dpdu).  Every operation rounds on its own:
// these fields decide rays.
struct TriFrame {
    v3 ng, ss;
    uint32_t reject;   // AGPT_TRI_FLAG_REJECT for a zero-area triangle (quirk 11)
};
AGPT_HD TriFrame triangle_frame(v3 v0, v3 v1, v3 v2, struct v2 uv0, struct v2 uv1, struct v2 uv2) {
    TriFrame f;
    f.reject = 0;
    const float du02x = uv0.x - uv2.x, du02y = uv0.y - uv2.y;
    const float du12x = uv1.x - uv2.x, du12y = uv1.y - uv2.y;
    const v3 dp02 = v0 - v2, dp12 = v1 - v2;
    const float determinant = du02x * du12y - du02y * du12x;
    const bool degenerate_uv = (double)fabsf(determinant) < 1e-8;
    v3 dpdu = V3s(0), dpdv = V3s(0);
    if (!degenerate_uv) {
        const float invdet = 1 / determinant;
        dpdu = (du12y * dp02 - du02y * dp12) * invdet;
        dpdv = (-du12x * dp02 + du02x * dp12) * invdet;
    }
    if (degenerate_uv || sqrlen(cross(dpdu, dpdv)) == 0) {
        v3 ng = cross(v2 - v0, v1 - v0);
        if (sqrlen(ng) == 0) {
            f.reject = AGPT_TRI_FLAG_REJECT;
            dpdu = V3(1, 0, 0);
            dpdv = V3(0, 1, 0);
        } else {
            coordinate_system(normalize(ng), &dpdu, &dpdv);
        }
    }
    f.ng = normalize(cross(dpdu, dpdv));  // SurfaceInteraction ctor, intersectable.h:69
    f.ss = normalize(dpdu);                // BSDF::ss (reflection.cpp:10) and trianglemesh.cpp:100
    return f;
}

// tri_shade: the four float4 of a global triangle id
AGPT_HD void pack_tri_shade(float4* q, const TriFrame& f, v3 n0, v3 n1, v3 n2, uint32_t prim_id) {
    q[0] = make_float4(f.ng.x, f.ng.y, f.ng.z, f.ss.x);
    q[1] = make_float4(f.ss.y, f.ss.z, n0.x, n0.y);
    q[2] = make_float4(n0.z, n1.x, n1.y, n1.z);
    q[3] = make_float4(n2.x, n2.y, n2.z, bits_as_float(prim_id));
}
// tri_verts: the three float4 of a primitive slot; gid = the triangle's global id, flags = its TriFrame::reject
AGPT_HD void pack_tri_verts(float4* q, v3 v0, v3 v1, v3 v2, uint32_t gid, uint32_t flags) {
    q[0] = make_float4(v0.x, v0.y, v0.z, bits_as_float(gid));
    q[1] = make_float4(v1.x, v1.y, v1.z, bits_as_float(flags));
    q[2] = make_float4(v2.x, v2.y, v2.z, 0.f);
}

}  // namespace agpt
