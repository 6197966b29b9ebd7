// agpt_update.hip -- agpt_scene_update_mesh's device path (agpt_update.h).  Compiled with the flags of the exact units: the
// triangle records decide rays, so every operation rounds on its own and divides / square roots are correctly rounded.
//
//   k_update_tris    one lane per triangle SLOT (BVH leaf order): the three float4 of tri_verts at the slot, the four float4 of
//                    tri_shade at the triangle's global id -- flatten_scene's two per-triangle loops, fused, writing through the
//                    SHARED packers of agpt_records.h.
//   k_refit_nodes    one lane per node of a list: a leaf grows the empty box over its slots' triangle boxes (vertices read back from
//                    tri_verts, which k_update_tris has just written), an interior node takes (left, right) of its child pair -- the
//                    SHARED arithmetic of agpt_bvh_arith.h, stored through the record writers of agpt_records.h.  Launched
//                    once for all leaves, then once per level of interior nodes from the deepest up, on one stream: a launch sees
//                    what the launches before it wrote, and the output does not depend on the launch shape.
//   k_check_finite   one lane per coordinate of the position array: one flag word set if any is Inf or NaN (the rule of the host
//                    path, which looks at every coordinate, referenced by a triangle or not).
//   k_transform_mesh one lane per vertex and one per normal: the mesh's rest arrays through transform_point / transform_vector of
//                    agpt_transform.h into the arrays k_update_tris reads (agpt_scene_transform_mesh).
//   k_skin_mesh      one lane per vertex and one per normal: the rest arrays through skin_blend of agpt_skin.h -- up to 8 (joint,
//                    weight) slots per item, each a gather of the joint's palette entry -- into the arrays k_update_tris reads
//                    (agpt_scene_pose_mesh).
//   k_morph_mesh     one lane per vertex and one per normal: the rest arrays plus the ACTIVE morph targets' deltas (morph_blend of
//                    agpt_morph.h) and, fused (kSkin), straight on through skin_blend (agpt_scene_morph_mesh).
//   k_pack_palette   one lane per joint of a frame's matrices in DEVICE memory (agpt_scene_pose_mesh_device, _morph_mesh_device): four
//                    16-byte loads of M, inverse_transpose of agpt_transform.h -- the host's text -- and the joint's entry of the
//                    palette k_skin_mesh reads, skin_pack_palette's floats; three status words take the lowest joint with a non-finite
//                    entry, a last row that is not (0, 0, 0, 1), a determinant of exactly 0.
//   k_morph_active   one block: a frame's weights in device memory into the (target, weight) list k_morph_mesh walks, morph_active_list's
//                    bytes, its length and the lowest target with a non-finite weight.
//   k_face_normals   one lane per triangle: its three vertex indices (the index array k_update_tris reads) and positions, face_vector of
//                    agpt_normals.h, one float4 g_t (w unused) into a per-mesh scratch of n_tris x 16 B.
//   k_vertex_normals one lane per normal item: offsets[j], offsets[j + 1] of the CSR adjacency, then per incident corner the triangle id
//                    and one 16-byte gather of its g, summed in ascending corner order and finished by vertex_normal / normal_finish of
//                    agpt_normals.h: 12 B of the normals buffer.  Both run only for a mesh in AGPT_NORMALS_SMOOTH mode, between the
//                    front end that leaves positions in `verts` and k_update_tris; no atomics, so the bytes do not depend on the
//                    launch.  An item of very high valence is walked by one lane: correct and slow.
// All are bandwidth kernels (about 72 B read and 112 B written per triangle, 64 B per node pair, 24 B per transformed vertex, 24 + 8 K B
// per skinned vertex, 24 + 12 A B per vertex morphed by A active targets; k_pack_palette and k_morph_active move a few KB and cost their
// launch); all but k_skin_mesh, k_morph_mesh and the one-block k_morph_active run 64-lane blocks, 16-byte accesses of the float4 records,
// no LDS.
//
// k_skin_mesh's palette.  The per-lane gather by joint index is the one access here that is not a stream, and neighbouring vertices
// mostly name the same few joints.  A palette of up to 40 KiB (487 joints with normals, 787 without) is staged in LDS; a larger one is
// read from global memory, and AGPT_SKIN_GLOBAL_PALETTE in the environment, read at every call, forces that route.  Both routes run
// the same arithmetic on the same floats and write the same bytes.  What follows from staging:
//   launch   64-lane blocks, one per 64 items, would stage the palette 16 k times for a 1 M-vertex mesh.  The kernel runs 256-lane
//            blocks on a capped grid, 4 per CU, and strides over the items, so every block stages once and then streams.
//   cap      40 KiB is 160 KiB / 4: all four blocks of a CU stay resident.  Measured with the cap lifted, 1,024 joints with normals
//            (84 KiB, one block per CU) posed the 1 M-triangle heightfield in 0.322 ms against 0.302 ms from global memory: the streams
//            need the waves more than the gather needs the LDS.  At 64 joints the two routes are level.
//   layout   per JOINT, not per component: entry j is `stride` consecutive floats (M's 12, then N's 9; 13 / 21 with the pad).  Lanes
//            that name the same joint read the same address, which the LDS serves as one broadcast -- the common case costs what
//            one lane costs.  Lanes that name DIFFERENT joints read component c at dword stride * j + c, on bank (stride * j + c)
//            mod 32: the natural strides are the bad ones (12 puts joints j and j + 8 on one bank, 16 or 32 every second or every
//            joint), so each entry is padded to an ODD stride and two joints meet on a bank only when j = j' (mod 32).  The
//            entries are read with 4-byte LDS loads (an odd stride has no 16-byte alignment); the kernel is bound by its global
//            streams, not by these.
//   N-less   a mesh without normals stages M only (stride 13): the same kernel, the stride is an argument.
//
// k_morph_mesh<kSkin, kLds>.  Per item (a vertex, or a normal of a mesh whose targets carry normal deltas) with A targets ACTIVE -- weight
// not 0 -- out of the T bound: 12 B of the rest array read, 12 A B of deltas read, 12 B written: 24 + 12 A bytes, independent of T; a
// normal without normal deltas is copied (24 B).  kSkin adds the skin kernel's 8 K B of slots and its palette gather; the morphed value
// stays in registers between morph_blend and skin_blend, so fusing saves the 24 B per item of an intermediate array and a launch.
//   active   the host compacts a frame's weights into the (target, weight) pairs in use, in target order, and uploads only those
//            (8 B each).  The list is a kernel argument of its own, `const ... __restrict__`: index and weight are the same for
//            every lane, the compiler reads them with scalar loads (s_load_dwordx2) and the delta base of a target is formed in SGPRs.
//   deltas   target-major, packed xyz ([t][item][3] floats, positions and normals in buffers of their own): the 64 lanes of a wave
//            read one contiguous 768-B run per active target, one 12-byte load per lane (global_load_dwordx3) like the rest arrays'.
//            Padding to float4 records was NOT measured and not adopted: it would move 16 instead of 12 B per item and active
//            target through a kernel that is bound by exactly those bytes.  Offsets are size_t (T * items * 3 passes 2^31 for a
//            1 M-vertex mesh with 200 targets).
//   launch   256-lane blocks on a capped grid with a stride loop.  Fused: k_skin_mesh's shape and LDS cap (4 blocks per CU, a palette
//            of up to 40 KiB staged, a larger one or AGPT_SKIN_GLOBAL_PALETTE read from global memory).  Morph only: no LDS, 8 blocks
//            per CU (every wave slot of the CU; against 4 it measured 0.301 against 0.305 ms at 16 active).
//            AGPT_MORPH_MAX_BLOCKS in the environment, read at every call, lowers the cap of either: same bytes, it exists so that a
//            test can drive the stride loop on a small mesh.
//   loop     the walk over the active list is left rolled: one scalar load of (target, weight) and one 12-byte delta load per lane and
//            iteration.  Unrolled by four (four delta loads in flight) it was no faster on the 1 M-triangle heightfield and 3 % slower
//            at 64 active targets (0.419 against 0.408 ms per call, three alternating rounds): the CU's other waves already cover
//            the latency.
//   code     from the gfx950 code object of this unit (VGPRs / SGPRs / spilled / scratch bytes):
//              k_morph_mesh<false, false>  33 / 46 / 0 / 0        (morph only)
//              k_morph_mesh<true, false>   50 / 53 / 0 / 0        (fused, palette in global memory)
//              k_morph_mesh<true, true>    52 / 55 / 0 / 0        (fused, palette in LDS)
//            kLds has no meaning without kSkin: <false, true> is not instantiated, so there are three, not four.
//
// k_pack_palette and k_morph_active: the front end of a frame whose matrices and weights are already on the GPU.  What the host did per
// frame -- n_joints inverse transposes, the compaction of the weights, two small uploads -- runs here, and 20 bytes come back
// (DeviceInputStatus): the deform kernels above are launched only when they are clean, k_check_spheres -> synchronise ->
// k_update_spheres' shape (agpt_analytic.hip), and take n_active by value as before.
//   palette  one 64-lane block per 64 joints.  A joint is 64 B read as four float4 (hence the 16-byte alignment asked of the caller) and
//            84 or 52 B written with 4-byte stores (the odd stride has no wider alignment); at 1,024 joints that is 150 KB, a launch
//            and nothing else.  An M-only palette (stride 13) still computes the determinant: the host refuses a singular joint either
//            way.  The pad of an M-only entry is written as 0, as the host's is.
//   status   every lane of a wave arrives at the three ballots; the lowest set bit is the wave's lowest offender (lanes hold consecutive
//            joints) and lane 0 issues one vector atomicMin per word that has one -- aggregated by hand, as everywhere in this library
//            (the atomic optimizer is off).  The words start at 0xFFFFFFFF; a clean call leaves them there, so the memset of the 20
//            bytes is paid by the first call and by the one after a refusal.  They come down into pinned host memory of the cache.
//   active   T <= 4,096 weights, 256 at a time: a pair's place is the pairs of the chunks before, of the waves before (four counts in
//            LDS) and of the lanes before (popcount of the ballot below the lane): no atomic, so the list is in target order whatever
//            the schedule, and its bytes are the host's.  -0.0 is skipped (!(w == 0)).
//   code     from the gfx950 code object of this unit (VGPRs / SGPRs / spilled / scratch bytes):
//              k_pack_palette              50 / 23 / 0 / 0
//              k_morph_active              18 / 28 / 0 / 0        (32 B of LDS)
//            k_skin_mesh and k_morph_mesh keep the figures above.
//
// The host half.  MeshDeviceCache holds the device copies of one mesh; MeshUpdate (agpt_update.h) owns it beside the host copies and
// is the only one to invalidate either.  MeshUpdate::deform is the one launcher of k_transform_mesh, k_skin_mesh and k_morph_mesh: rest
// pose, uploads, argument records, grid and the LDS-or-global route are worked out once.  The bodies of k_skin_mesh and k_morph_mesh
// stay written out: one shared deform_block<kMorph, kSkin, kLds> was tried and grew k_skin_mesh by 12 (LDS) and 20 (global) instructions.
#include <cstdlib>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "agpt_bvh_arith.h"
#include "agpt_internal.h"
#include "agpt_normals.h"

namespace agpt {

namespace {

constexpr int kBlock = 64;

struct TriArgs {
    const float* verts;        // xyz per vertex
    const float* normals;      // xyz per normal, NULL: the mesh has none
    const v2* uv;              // NULL: the mesh has none ((0,0), (1,0), (1,1), trianglemesh.cpp:52-56)
    const int32_t* indices;    // (v, n, t) triplets, 9 per triangle
    const int32_t* prim_index; // 3 * triangle per slot
    float4* tri_verts;
    float4* tri_shade;
    uint32_t tri_base, prim_id;
    int n_tris;
};

__device__ __forceinline__ v3 load3(const float* p, int i) { return V3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]); }

__global__ __launch_bounds__(kBlock) void k_update_tris(TriArgs a) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.n_tris) return;
    const int t = a.prim_index[s] / 3;
    const int32_t* ix = a.indices + 9 * (size_t)t;
    const v3 v0 = load3(a.verts, ix[0]), v1 = load3(a.verts, ix[3]), v2_ = load3(a.verts, ix[6]);
    v2 uv0, uv1, uv2;
    if (a.uv) {
        uv0 = a.uv[ix[2]];
        uv1 = a.uv[ix[5]];
        uv2 = a.uv[ix[8]];
    } else {
        default_uv(uv0, uv1, uv2);
    }
    const TriFrame f = triangle_frame(v0, v1, v2_, uv0, uv1, uv2);
    v3 n0 = V3s(0), n1 = V3s(0), n2 = V3s(0);
    if (a.normals) {
        n0 = load3(a.normals, ix[1]);
        n1 = load3(a.normals, ix[4]);
        n2 = load3(a.normals, ix[7]);
    }
    const uint32_t gid = a.tri_base + (uint32_t)t;
    pack_tri_shade(a.tri_shade + 4 * (size_t)gid, f, n0, n1, n2, a.prim_id);
    pack_tri_verts(a.tri_verts + 3 * (size_t)(a.tri_base + (uint32_t)s), v0, v1, v2_, gid, f.reject);
}

struct RefitArgs {
    const int2* topo;          // (first, count) per node, mesh-local
    const int32_t* list;       // the nodes of this launch
    int n;
    const float4* tri_verts;
    float4* bounds;            // reference layout: (bmin, -), (bmax, -) per node, mesh-local
    float* nodes;              // the scene's pair records, as floats
    uint32_t node_base, tri_base;
    // the copies of the root box (node 0)
    DevPrim* prim;
    float* rootpair;
    float* prefilter;
};

__global__ __launch_bounds__(kBlock) void k_refit_nodes(RefitArgs a) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= a.n) return;
    const int i = a.list[k];
    const int2 fc = a.topo[i];
    Box bounds;
    if (fc.y > 0) {
        // Builder::choose_split's `bounds`: the box of every primitive of the leaf, in slot order
        const float4* tv = a.tri_verts + 3 * (size_t)(a.tri_base + (uint32_t)fc.x);
        for (int s = 0; s < fc.y; s++) {
            const float4 q0 = tv[3 * (size_t)s], q1 = tv[3 * (size_t)s + 1], q2 = tv[3 * (size_t)s + 2];
            bounds.grow(tri_box(V3(q0.x, q0.y, q0.z), V3(q1.x, q1.y, q1.z), V3(q2.x, q2.y, q2.z)));
        }
    } else {
        const float4 llo = a.bounds[2 * (size_t)fc.x], lhi = a.bounds[2 * (size_t)fc.x + 1];
        const float4 rlo = a.bounds[2 * (size_t)fc.x + 2], rhi = a.bounds[2 * (size_t)fc.x + 3];
        pair_union(&llo.x, &lhi.x, &rlo.x, &rhi.x, bounds.lo, bounds.hi);
    }
    const float *lo = bounds.lo, *hi = bounds.hi;
    a.bounds[2 * (size_t)i] = make_float4(lo[0], lo[1], lo[2], 0.f);
    a.bounds[2 * (size_t)i + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    const size_t g = (size_t)a.node_base + (size_t)i;
    pair_record_set_box(a.nodes + 16 * (g >> 1), g & 1, lo, hi);   // (the encodings of the record stay)
    if (i == 0) {   // the copies of the root box
        for (int c = 0; c < 3; c++) {
            a.prim->root_bmin[c] = lo[c];
            a.prim->root_bmax[c] = hi[c];
        }
        if (a.rootpair) rootpair_record_set_box(a.rootpair, lo, hi);
        if (a.prefilter) prefilter_record_set_box(a.prefilter, lo, hi);
    }
}

__global__ __launch_bounds__(kBlock) void k_check_finite(const float* x, size_t n, uint32_t* flag) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool bad = i < n && (__float_as_uint(x[i]) & 0x7f800000u) == 0x7f800000u;
    if (__any(bad) && (threadIdx.x & 63) == 0) *flag = 1u;   // (every wave that sees one stores the same word)
}

__global__ __launch_bounds__(kBlock) void k_face_normals(const float* verts, const int32_t* indices, float4* face, int n_tris) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tris) return;
    const int32_t* ix = indices + 9 * (size_t)t;
    const v3 g = face_vector(load3(verts, ix[0]), load3(verts, ix[3]), load3(verts, ix[6]));
    face[t] = make_float4(g.x, g.y, g.z, 0.f);
}

__global__ __launch_bounds__(kBlock) void k_vertex_normals(const int32_t* offsets, const int32_t* corner_tri, const float4* face, float* normals,
                                                           int n_normals) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n_normals) return;
    const v3 n = vertex_normal(offsets, corner_tri, face, (size_t)j);
    normals[3 * (size_t)j] = n.x;
    normals[3 * (size_t)j + 1] = n.y;
    normals[3 * (size_t)j + 2] = n.z;
}

struct TransformArgs {
    Mat4 M, N;                 // N = inverse_transpose(M), formed on the host
    const float* rest_verts;
    const float* rest_normals;
    float* verts;
    float* normals;
    int n_vertices, n_normals;
};

__global__ __launch_bounds__(kBlock) void k_transform_mesh(TransformArgs a) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < (size_t)a.n_vertices) {
        const float v[3] = {a.rest_verts[3 * i], a.rest_verts[3 * i + 1], a.rest_verts[3 * i + 2]};
        float out[3];
        transform_point(a.M, v, out);
        a.verts[3 * i] = out[0];
        a.verts[3 * i + 1] = out[1];
        a.verts[3 * i + 2] = out[2];
    } else if (i < (size_t)a.n_vertices + (size_t)a.n_normals) {
        const size_t j = i - (size_t)a.n_vertices;
        const float v[3] = {a.rest_normals[3 * j], a.rest_normals[3 * j + 1], a.rest_normals[3 * j + 2]};
        float out[3];
        transform_vector(a.N, v, out);
        a.normals[3 * j] = out[0];
        a.normals[3 * j + 1] = out[1];
        a.normals[3 * j + 2] = out[2];
    }
}

struct SkinArgs {
    const float* palette;      // n_joints entries of `stride` floats (agpt_skin.h)
    int stride, n_joints, influences;
    const float* rest_verts;
    const float* rest_normals;
    const int32_t* vertex_joints;
    const float* vertex_weights;
    const int32_t* normal_joints;   // (the vertex arrays again when they serve both)
    const float* normal_weights;
    float* verts;
    float* normals;
    int n_vertices, n_normals;
};

constexpr int kSkinBlock = 256;
constexpr int kSkinBlocksPerCU = 4;
constexpr size_t kLdsPerCU = 160 * 1024;
constexpr size_t kSkinLdsBytes = kLdsPerCU / kSkinBlocksPerCU;   // the largest staged palette, 40 KiB: all four blocks stay resident

template <bool kLds>
__global__ __launch_bounds__(kSkinBlock) void k_skin_mesh(SkinArgs a) {
    extern __shared__ __attribute__((aligned(16))) float skin_lds[];
    if (kLds) {
        const int n = a.n_joints * a.stride;
        for (int i = threadIdx.x; i < n; i += kSkinBlock) skin_lds[i] = a.palette[i];
        __syncthreads();
    }
    const size_t nv = (size_t)a.n_vertices, total = nv + (size_t)a.n_normals, K = (size_t)a.influences;
    for (size_t i = (size_t)blockIdx.x * kSkinBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kSkinBlock) {
        const bool point = i < nv;
        const size_t j = point ? i : i - nv;
        const float* rest = (point ? a.rest_verts : a.rest_normals) + 3 * j;
        const int32_t* joints = (point ? a.vertex_joints : a.normal_joints) + K * j;
        const float* weights = (point ? a.vertex_weights : a.normal_weights) + K * j;
        const float r[3] = {rest[0], rest[1], rest[2]};
        float out[3];
        if (point) {
            if (kLds)
                skin_blend<true>(skin_lds, a.stride, joints, weights, a.influences, r, out);
            else
                skin_blend<true>(a.palette, a.stride, joints, weights, a.influences, r, out);
        } else {
            if (kLds)
                skin_blend<false>(skin_lds, a.stride, joints, weights, a.influences, r, out);
            else
                skin_blend<false>(a.palette, a.stride, joints, weights, a.influences, r, out);
        }
        float* dst = (point ? a.verts : a.normals) + 3 * j;
        dst[0] = out[0];
        dst[1] = out[1];
        dst[2] = out[2];
    }
}

struct MorphArgs {
    const float* position_deltas;   // [t][vertex][3]
    const float* normal_deltas;     // [t][normal][3]; NULL: the normals keep their rest values
    SkinArgs s;                     // rest arrays, outputs and counts; with kSkin the binding and the palette as well
};

constexpr int kMorphBlocksPerCU = 8;   // morph only (no LDS): 8 x 256 lanes are the 32 wave slots of a CU

// `active` is an argument of its own so that it can be `__restrict__`: uniform, never written here -> scalar loads
template <bool kSkin, bool kLds>
__global__ __launch_bounds__(kSkinBlock) void k_morph_mesh(const MorphActive* __restrict__ active, int n_active, MorphArgs m) {
    extern __shared__ __attribute__((aligned(16))) float skin_lds[];
    const SkinArgs& a = m.s;
    if (kSkin && kLds) {
        const int n = a.n_joints * a.stride;
        for (int i = threadIdx.x; i < n; i += kSkinBlock) skin_lds[i] = a.palette[i];
        __syncthreads();
    }
    const size_t nv = (size_t)a.n_vertices, nn = (size_t)a.n_normals, total = nv + nn, K = (size_t)a.influences;
    for (size_t i = (size_t)blockIdx.x * kSkinBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kSkinBlock) {
        const bool point = i < nv;
        const size_t j = point ? i : i - nv;
        const float* rest = (point ? a.rest_verts : a.rest_normals) + 3 * j;
        const float* deltas = point ? m.position_deltas : m.normal_deltas;
        const float r[3] = {rest[0], rest[1], rest[2]};
        float morphed[3] = {r[0], r[1], r[2]}, out[3];
        if (deltas) morph_blend(active, n_active, deltas, point ? nv : nn, j, r, morphed);
        if (kSkin) {
            const int32_t* joints = (point ? a.vertex_joints : a.normal_joints) + K * j;
            const float* weights = (point ? a.vertex_weights : a.normal_weights) + K * j;
            const float* palette = kLds ? skin_lds : a.palette;
            if (point)
                skin_blend<true>(palette, a.stride, joints, weights, a.influences, morphed, out);
            else
                skin_blend<false>(palette, a.stride, joints, weights, a.influences, morphed, out);
        } else {
            out[0] = morphed[0];
            out[1] = morphed[1];
            out[2] = morphed[2];
        }
        float* dst = (point ? a.verts : a.normals) + 3 * j;
        dst[0] = out[0];
        dst[1] = out[1];
        dst[2] = out[2];
    }
}

__device__ __forceinline__ bool non_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// The lowest item of a wave whose lane has `bad` set, into *word: the lanes of a wave hold consecutive items, so it is the lowest set
// bit of the ballot, and lane 0 issues the one vector atomicMin.  Every lane of the wave must arrive.
__device__ __forceinline__ void wave_lowest(bool bad, uint32_t wave_first_item, uint32_t* word) {
    const unsigned long long b = __ballot(bad);
    if (b != 0 && (threadIdx.x & 63) == 0) atomicMin(word, wave_first_item + (uint32_t)(__ffsll(b) - 1));
}

struct PaletteArgs {
    const float4* joints;      // four float4 per joint: the rows of M
    int n_joints, stride;
    float* palette;
    uint32_t* status;          // DeviceInputStatus' first three words, kNoItem on entry
};

__global__ __launch_bounds__(kBlock) void k_pack_palette(PaletteArgs a) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    bool nonfinite = false, bad_row = false, singular = false;
    if (j < a.n_joints) {
        Mat4 M;
        for (int r = 0; r < 4; r++) {
            const float4 q = a.joints[4 * (size_t)j + r];
            M.c[4 * r] = q.x; M.c[4 * r + 1] = q.y; M.c[4 * r + 2] = q.z; M.c[4 * r + 3] = q.w;
        }
        for (int i = 0; i < 16; i++) nonfinite |= non_finite(M.c[i]);
        bad_row = !(M.c[12] == 0 && M.c[13] == 0 && M.c[14] == 0 && M.c[15] == 1);   // skin_check_last_rows' test
        float det = 0;
        const Mat4 N = inverse_transpose(M, &det);   // (computed for an M-only palette as well: the host refuses a singular joint either way)
        singular = det == 0;
        float* e = a.palette + (size_t)j * (size_t)a.stride;   // skin_pack_palette's entry
        for (int i = 0; i < 12; i++) e[i] = M.c[i];
        if (a.stride == skin_palette_stride(true)) {
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) e[12 + 3 * r + c] = N.c[4 * r + c];
        } else {
            e[12] = 0.f;   // the pad of the M-only entry
        }
    }
    const uint32_t first = (uint32_t)(blockIdx.x * kBlock);   // (kBlock is one wave)
    wave_lowest(nonfinite, first, a.status);
    wave_lowest(bad_row, first, a.status + 1);
    wave_lowest(singular, first, a.status + 2);
}

constexpr int kActiveBlock = 256, kActiveWaves = kActiveBlock / 64;

// One block.  The targets are taken kActiveBlock at a time, in order; the place of a pair is the pairs of the chunks before (`base`, the
// same in every lane), of the waves before in this chunk, and of the lanes before in this wave -- ballots and popcounts, no atomic, so
// the list is in target order whatever the schedule.
__global__ __launch_bounds__(kActiveBlock) void k_morph_active(const float* __restrict__ weights, int n_targets, MorphActive* __restrict__ active,
                                                               uint32_t* __restrict__ status) {
    __shared__ uint32_t wave_count[kActiveWaves], wave_bad[kActiveWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t base = 0, bad = kNoItem;
    for (int first = 0; first < n_targets; first += kActiveBlock) {
        const int t = first + (int)threadIdx.x;
        const float w = t < n_targets ? weights[t] : 0.f;
        const bool use = !(w == 0);   // morph_active_list's test: -0.0 is skipped
        if (bad == kNoItem && non_finite(w)) bad = (uint32_t)t;   // (a lane's targets ascend: its first is its lowest)
        const unsigned long long b = __ballot(use);
        if (lane == 0) wave_count[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int k = 0; k < kActiveWaves; k++) {
            const uint32_t c = wave_count[k];
            before += k < wave ? c : 0u;
            all += c;
        }
        if (use) active[base + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = MorphActive{t, w};
        base += all;
        __syncthreads();   // (the next chunk rewrites wave_count)
    }
    for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, o));
    if (lane == 0) wave_bad[wave] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kActiveWaves; k++) bad = min(bad, wave_bad[k]);
        status[0] = base;
        status[1] = bad;
    }
}

}  // namespace

int launch_pack_palette(hipStream_t stream, const float* joints16_dev, int n_joints, bool with_normals, float* palette_dev, uint32_t* status3_dev) {
    if (!joints16_dev || !palette_dev || !status3_dev || n_joints < 1 || n_joints > kSkinMaxJoints || ((uintptr_t)joints16_dev & 15) != 0)
        return fail(AGPT_ERR_INVALID, "k_pack_palette: NULL or misaligned pointer, or n_joints outside 1 .. " + std::to_string(kSkinMaxJoints));
    PaletteArgs a;
    a.joints = reinterpret_cast<const float4*>(joints16_dev);
    a.n_joints = n_joints;
    a.stride = skin_palette_stride(with_normals);
    a.palette = palette_dev;
    a.status = status3_dev;
    hipLaunchKernelGGL(k_pack_palette, dim3((unsigned)((n_joints + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return AGPT_OK;
}

int launch_morph_active(hipStream_t stream, const float* weights_dev, int n_targets, MorphActive* active_dev, uint32_t* status2_dev) {
    if (!weights_dev || !active_dev || !status2_dev || n_targets < 1 || n_targets > kMorphMaxTargets)
        return fail(AGPT_ERR_INVALID, "k_morph_active: NULL pointer, or n_targets outside 1 .. " + std::to_string(kMorphMaxTargets));
    hipLaunchKernelGGL(k_morph_active, dim3(1), dim3(kActiveBlock), 0, stream, weights_dev, n_targets, active_dev, status2_dev);
    HIP_TRY(hipGetLastError());
    return AGPT_OK;
}

struct MeshDeviceCache {
    DevBuf<float> verts, normals;
    // the rest pose k_transform_mesh, k_skin_mesh and k_morph_mesh read (uploaded by the first deform after the arrays were given)
    DevBuf<float> rest_verts, rest_normals;
    bool has_rest = false;
    // the binding (uploaded by the first pose after it was set) and the palette of the last pose
    DevBuf<int32_t> skin_vertex_joints, skin_normal_joints;
    DevBuf<float> skin_vertex_weights, skin_normal_weights, skin_palette;
    bool has_skin = false;
    // the targets' deltas (uploaded by the first morph after they were set) and the active list of the last morph
    DevBuf<float> morph_position_deltas, morph_normal_deltas;
    DevBuf<MorphActive> morph_active;
    bool has_morph = false;
    // AGPT_NORMALS_SMOOTH: the CSR adjacency of the normal items (built and uploaded by the first smooth update of this cache) and the
    // face vectors of the last one
    DevBuf<int32_t> normal_offsets, normal_corner_tri;
    DevBuf<float4> face_normals;
    bool has_adjacency = false;
    DevBuf<uint32_t> flag;        // k_check_finite's word
    // DeviceInputStatus' five words (k_pack_palette, k_morph_active) and the pinned host words they are downloaded into.  joint_words_clean:
    // the three atomicMin words hold kNoItem -- a clean call leaves them so, and only a refused one (or a new allocation) costs a memset
    DevBuf<uint32_t> input_status;
    uint32_t* input_status_host = nullptr;
    bool joint_words_clean = false;
    ~MeshDeviceCache() {
        if (input_status_host) (void)hipHostFree(input_status_host);
    }
    DevBuf<v2> uv;
    DevBuf<int32_t> indices, prim_index, lists;
    DevBuf<int2> topo;
    DevBuf<float4> bounds;
    // lists: all leaves first, then the interior nodes level by level from the deepest up; launch l covers [begin[l], begin[l + 1])
    std::vector<int> begin;
    int total_nodes = 0;
};

MeshUpdate::MeshUpdate() = default;
MeshUpdate::MeshUpdate(MeshUpdate&&) noexcept = default;
MeshUpdate::~MeshUpdate() = default;

void MeshUpdate::arrays_given() {
    rest_valid_ = false;
    rest_vertices_ = rest_normals_ = std::vector<v3>();
    if (dev_) dev_->has_rest = false;
}

void MeshUpdate::rest_taken(const std::vector<v3>& vertices, const std::vector<v3>& normals) {
    rest_vertices_ = vertices;
    rest_normals_ = normals;
    rest_valid_ = true;
    if (dev_) dev_->has_rest = false;
}

void MeshUpdate::skin_changed(SkinBinding&& skin) {
    skin_ = std::move(skin);
    if (!dev_) return;   // (nothing goes up here: the next pose uploads the new binding)
    for (DevBuf<int32_t>* b : {&dev_->skin_vertex_joints, &dev_->skin_normal_joints}) b->release();
    for (DevBuf<float>* b : {&dev_->skin_vertex_weights, &dev_->skin_normal_weights, &dev_->skin_palette}) b->release();
    dev_->has_skin = false;
}

void MeshUpdate::morph_changed(MorphTargets&& morph) {
    morph_ = std::move(morph);
    if (!dev_) return;   // (nothing goes up here: the next morph uploads the new targets)
    dev_->morph_position_deltas.release();
    dev_->morph_normal_deltas.release();
    dev_->morph_active.release();
    dev_->has_morph = false;
}

void MeshUpdate::topology_changed() {
    dev_.reset();
    bounds_stale = arrays_stale = false;
}

// the topology and the per-level node lists of a tree of build_bvh's, checked against the sizes the kernels index with
static int prepare(hipStream_t stream, MeshDeviceCache& u, const HostMesh& mesh) {
    const int total = mesh.total_nodes, n_tris = (int)mesh.prim_index.size();
    std::vector<int2> topo((size_t)total + 1, make_int2(0, 0));
    std::vector<int> depth((size_t)total + 1, -1);
    std::vector<std::vector<int32_t>> interior;
    std::vector<int32_t> lists;
    depth[0] = 0;
    for (int i = 0; i <= total; i++) {   // a parent has a lower slot than its children: its depth is known when it is reached
        if (i == 1) continue;
        const agpt_bvh_node& nd = mesh.nodes[i];
        topo[i] = make_int2(nd.first, nd.count);
        if (depth[i] < 0) return fail(AGPT_ERR_INVALID, "agpt_scene_update_mesh: the mesh's BVH has an unreachable node");
        if (nd.count > 0) {
            if (nd.first < 0 || nd.count > n_tris - nd.first) return fail(AGPT_ERR_INVALID, "agpt_scene_update_mesh: leaf range outside the mesh");
            lists.push_back(i);
        } else {
            if (nd.count < 0 || nd.first <= i || nd.first < 2 || nd.first >= total)
                return fail(AGPT_ERR_INVALID, "agpt_scene_update_mesh: child pair outside the tree");
            depth[nd.first] = depth[nd.first + 1] = depth[i] + 1;
            if ((int)interior.size() <= depth[i]) interior.resize((size_t)depth[i] + 1);
            interior[depth[i]].push_back(i);
        }
    }
    u.begin.assign(1, 0);
    u.begin.push_back((int)lists.size());
    for (int d = (int)interior.size() - 1; d >= 0; d--) {
        lists.insert(lists.end(), interior[d].begin(), interior[d].end());
        u.begin.push_back((int)lists.size());
    }
    for (int32_t p : mesh.prim_index)
        if (p < 0 || p % 3 != 0 || p / 3 >= n_tris) return fail(AGPT_ERR_INVALID, "agpt_scene_update_mesh: bad prim_index");
    u.total_nodes = total;
    if (const int rc = upload(u.topo, topo, stream)) return rc;
    if (const int rc = upload(u.lists, lists, stream)) return rc;
    if (const int rc = upload(u.indices, mesh.indices, stream)) return rc;
    if (const int rc = upload(u.prim_index, mesh.prim_index, stream)) return rc;
    if (!mesh.texcoords.empty())
        if (const int rc = upload(u.uv, mesh.texcoords, stream)) return rc;
    if (const int rc = u.bounds.ensure(2 * ((size_t)total + 1))) return rc;
    HIP_TRY(hipMemsetAsync(u.bounds.p, 0, 2 * ((size_t)total + 1) * sizeof(float4), stream));
    HIP_TRY(hipStreamSynchronize(stream));   // the staging vectors above go out of scope
    return AGPT_OK;
}

int MeshUpdate::ensure_cache(hipStream_t stream, const HostMesh& mesh) {
    if (dev_) return AGPT_OK;
    std::unique_ptr<MeshDeviceCache> u(new MeshDeviceCache());
    if (const int rc = prepare(stream, *u, mesh)) return rc;
    dev_ = std::move(u);
    return AGPT_OK;
}

// The records of the mesh from the cache's verts / normals, then the root box; with `finite`, k_check_finite runs ahead of the rest and
// its flag comes back beside the box.  A non-finite position harms nothing here (every index comes from the topology): the caller
// replaces what this wrote through the host path.
int MeshUpdate::refit(hipStream_t stream, const HostMesh& mesh, const UpdateTarget& tg, float root6[6], bool* finite) {
    MeshDeviceCache& u = *dev_;
    const int n_tris = (int)mesh.prim_index.size();
    if (finite) {
        const size_t n = 3 * mesh.vertices.size();
        if (const int rc = u.flag.ensure(1)) return rc;
        HIP_TRY(hipMemsetAsync(u.flag.p, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL(k_check_finite, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, u.verts.p, n, u.flag.p);
    }
    TriArgs ta;
    ta.verts = u.verts.p;
    ta.normals = mesh.normals.empty() ? nullptr : u.normals.p;
    ta.uv = mesh.texcoords.empty() ? nullptr : u.uv.p;
    ta.indices = u.indices.p;
    ta.prim_index = u.prim_index.p;
    ta.tri_verts = tg.tri_verts;
    ta.tri_shade = tg.tri_shade;
    ta.tri_base = tg.tri_base;
    ta.prim_id = tg.prim_id;
    ta.n_tris = n_tris;
    hipLaunchKernelGGL(k_update_tris, dim3((n_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, ta);

    RefitArgs ra;
    ra.topo = u.topo.p;
    ra.tri_verts = tg.tri_verts;
    ra.bounds = u.bounds.p;
    ra.nodes = reinterpret_cast<float*>(tg.nodes);
    ra.node_base = tg.node_base;
    ra.tri_base = tg.tri_base;
    ra.prim = tg.prim;
    ra.rootpair = reinterpret_cast<float*>(tg.rootpair);
    ra.prefilter = reinterpret_cast<float*>(tg.prefilter);
    for (size_t l = 0; l + 1 < u.begin.size(); l++) {
        ra.list = u.lists.p + u.begin[l];
        ra.n = u.begin[l + 1] - u.begin[l];
        if (ra.n > 0) hipLaunchKernelGGL(k_refit_nodes, dim3((ra.n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, ra);
    }
    HIP_TRY(hipGetLastError());
    float4 root[2];
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(root, u.bounds.p, sizeof(root), hipMemcpyDeviceToHost, stream));
    if (finite) HIP_TRY(hipMemcpyAsync(&flag, u.flag.p, sizeof(flag), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (finite) *finite = flag == 0;
    root6[0] = root[0].x; root6[1] = root[0].y; root6[2] = root[0].z;
    root6[3] = root[1].x; root6[4] = root[1].y; root6[5] = root[1].z;
    return AGPT_OK;
}

int MeshUpdate::update(hipStream_t stream, const HostMesh& mesh, const float* vertices, const float* normals, const UpdateTarget& tg,
                       float root6[6]) {
    if (const int rc = ensure_cache(stream, mesh)) return rc;
    if (const int rc = upload(dev_->verts, vertices, 3 * mesh.vertices.size(), stream)) return rc;
    if (!mesh.normals.empty())
        if (const int rc = upload(dev_->normals, normals, 3 * mesh.normals.size(), stream)) return rc;
    return refit(stream, mesh, tg, root6, nullptr);
}

int MeshUpdate::copy_arrays(hipStream_t stream, const HostMesh& mesh, const float* vertices_dev, const float* normals_dev) {
    if (const int rc = ensure_cache(stream, mesh)) return rc;
    MeshDeviceCache& u = *dev_;
    const size_t nv = 3 * mesh.vertices.size(), nn = 3 * mesh.normals.size();
    if (const int rc = u.verts.ensure(nv)) return rc;
    HIP_TRY(hipMemcpyAsync(u.verts.p, vertices_dev, nv * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (nn) {
        if (const int rc = u.normals.ensure(nn)) return rc;
        if (normals_dev) HIP_TRY(hipMemcpyAsync(u.normals.p, normals_dev, nn * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    return AGPT_OK;
}

int MeshUpdate::upload_positions(hipStream_t stream, const HostMesh& mesh, const float* vertices) {
    if (const int rc = ensure_cache(stream, mesh)) return rc;
    if (const int rc = upload(dev_->verts, vertices, 3 * mesh.vertices.size(), stream)) return rc;
    return dev_->normals.ensure(3 * mesh.normals.size());
}

int MeshUpdate::smooth_normals(hipStream_t stream, const HostMesh& mesh) {
    MeshDeviceCache& u = *dev_;
    const size_t nn = mesh.normals.size(), n_corners = mesh.indices.size() / 3, n_tris = n_corners / 3;
    // what the kernels index with, against what they index (the indices were checked by agpt_scene_add_mesh)
    if (nn == 0 || n_tris == 0 || n_tris != mesh.prim_index.size() || n_corners > (size_t)INT32_MAX || !u.verts.p || !u.normals.p)
        return fail(AGPT_ERR_INVALID, "smooth normals: the mesh has no normals, or the cache does not hold its arrays");
    if (!u.has_adjacency) {
        std::vector<int32_t> offsets, corner_tri;
        normal_adjacency(mesh.indices.data(), n_corners, nn, offsets, corner_tri);
        if (const int rc = upload(u.normal_offsets, offsets, stream)) return rc;
        if (const int rc = upload(u.normal_corner_tri, corner_tri, stream)) return rc;
        if (const int rc = u.face_normals.ensure(n_tris)) return rc;
        HIP_TRY(hipStreamSynchronize(stream));   // the staging vectors go out of scope
        u.has_adjacency = true;
    }
    hipLaunchKernelGGL(k_face_normals, dim3((unsigned)((n_tris + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, u.verts.p, u.indices.p,
                       u.face_normals.p, (int)n_tris);
    hipLaunchKernelGGL(k_vertex_normals, dim3((unsigned)((nn + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, u.normal_offsets.p,
                       u.normal_corner_tri.p, u.face_normals.p, u.normals.p, (int)nn);
    HIP_TRY(hipGetLastError());
    return AGPT_OK;
}

// the cache, the rest pose on the device (uploaded when the cache holds none) and room for the deformed arrays
int MeshUpdate::ensure_rest(const char* fn, hipStream_t stream, const HostMesh& mesh) {
    if (const int rc = ensure_cache(stream, mesh)) return rc;
    MeshDeviceCache& u = *dev_;
    const size_t nv = mesh.vertices.size(), nn = mesh.normals.size();
    if (rest_vertices_.size() != nv || rest_normals_.size() != nn)
        return fail(AGPT_ERR_INVALID, std::string(fn) + ": the rest pose does not have the mesh's counts");
    if (!u.has_rest) {
        if (const int rc = upload(u.rest_verts, &rest_vertices_.data()->x, 3 * nv, stream)) return rc;
        if (nn)
            if (const int rc = upload(u.rest_normals, &rest_normals_.data()->x, 3 * nn, stream)) return rc;
        HIP_TRY(hipStreamSynchronize(stream));   // (the rest vectors may change behind this call)
        u.has_rest = true;
    }
    if (const int rc = u.verts.ensure(3 * nv)) return rc;
    return nn ? u.normals.ensure(3 * nn) : AGPT_OK;
}

// the arrays of the rest pose and of the result (ensure_rest has made them): the six fields the three argument records share
template <class Args>
static void rest_args(const MeshDeviceCache& u, const HostMesh& mesh, bool with_normals, Args& a) {
    const size_t nv = mesh.vertices.size(), nn = with_normals ? mesh.normals.size() : 0;
    a.rest_verts = u.rest_verts.p;
    a.rest_normals = nn ? u.rest_normals.p : nullptr;
    a.verts = u.verts.p;
    a.normals = nn ? u.normals.p : nullptr;
    a.n_vertices = (int)nv;
    a.n_normals = (int)nn;
}

// the binding on the device (uploaded when the cache holds none), this call's palette -- `palette` == NULL: k_pack_palette has written
// it from `n_joints` matrices in device memory --, and the skin's share of the kernel arguments
static int skin_on_device(const char* fn, hipStream_t stream, MeshDeviceCache& u, const HostMesh& mesh, const SkinBinding& skin,
                          const std::vector<float>* palette, int n_joints, bool with_normals, SkinArgs& a) {
    const size_t nv = mesh.vertices.size(), nn = mesh.normals.size(), K = (size_t)skin.influences;
    const int stride = skin_palette_stride(nn != 0 && with_normals);   // (without: M only, as for a mesh that has no normals)
    const bool own_normal_slots = nn && !skin.normal_joints.empty();
    // what the kernel indexes with, against what it indexes (the joint indices were checked against n_joints when the skin was set)
    if (K < 1 || K > (size_t)kSkinMaxInfluences || skin.vertex_joints.size() != nv * K || skin.vertex_weights.size() != nv * K ||
        (own_normal_slots ? skin.normal_joints.size() != nn * K || skin.normal_weights.size() != nn * K : nn && nn != nv) ||
        (palette ? palette->size() != (size_t)skin.n_joints * (size_t)stride : n_joints != skin.n_joints || !u.skin_palette.p))
        return fail(AGPT_ERR_INVALID, std::string(fn) + ": the binding does not have the mesh's counts");
    if (!u.has_skin) {
        if (const int rc = upload(u.skin_vertex_joints, skin.vertex_joints, stream)) return rc;
        if (const int rc = upload(u.skin_vertex_weights, skin.vertex_weights, stream)) return rc;
        if (own_normal_slots) {
            if (const int rc = upload(u.skin_normal_joints, skin.normal_joints, stream)) return rc;
            if (const int rc = upload(u.skin_normal_weights, skin.normal_weights, stream)) return rc;
        }
        HIP_TRY(hipStreamSynchronize(stream));   // (the binding may be replaced behind this call)
        u.has_skin = true;
    }
    // room for either stride (ensure only grows: the narrow palette of a later call lands in the same allocation)
    if (const int rc = u.skin_palette.ensure((size_t)skin.n_joints * (size_t)skin_palette_stride(true))) return rc;
    if (palette)
        if (const int rc = upload(u.skin_palette, *palette, stream)) return rc;
    a.palette = u.skin_palette.p;
    a.stride = stride;
    a.n_joints = skin.n_joints;
    a.influences = skin.influences;
    a.vertex_joints = u.skin_vertex_joints.p;
    a.vertex_weights = u.skin_vertex_weights.p;
    a.normal_joints = own_normal_slots ? u.skin_normal_joints.p : u.skin_vertex_joints.p;
    a.normal_weights = own_normal_slots ? u.skin_normal_weights.p : u.skin_vertex_weights.p;
    return AGPT_OK;
}

// the targets' deltas on the device (uploaded when the cache holds none), this call's active list -- `active` == NULL: k_morph_active has
// written its n_active pairs from `n_targets` weights in device memory, every target below n_targets by construction --, and the morph's
// share of the arguments
static int morph_on_device(const char* fn, hipStream_t stream, MeshDeviceCache& u, const HostMesh& mesh, const MorphTargets& morph,
                           const std::vector<MorphActive>* active, int n_targets, size_t n_active, MorphArgs& m) {
    const size_t nv = mesh.vertices.size(), nn = mesh.normals.size(), T = (size_t)morph.n_targets;
    const bool normal_deltas = nn && !morph.normal_deltas.empty();
    // what the kernel indexes with, against what it indexes
    if (T < 1 || T > (size_t)kMorphMaxTargets || morph.position_deltas.size() != T * nv * 3 ||
        (normal_deltas && morph.normal_deltas.size() != T * nn * 3) || n_active > T ||
        (!active && ((size_t)n_targets != T || !u.morph_active.p)))
        return fail(AGPT_ERR_INVALID, std::string(fn) + ": the targets do not have the mesh's counts");
    for (size_t k = 0; active && k < active->size(); k++)
        if ((*active)[k].target < 0 || (size_t)(*active)[k].target >= T)
            return fail(AGPT_ERR_INVALID, std::string(fn) + ": an active target outside the targets");
    if (!u.has_morph) {
        if (const int rc = upload(u.morph_position_deltas, morph.position_deltas, stream)) return rc;
        if (normal_deltas)
            if (const int rc = upload(u.morph_normal_deltas, morph.normal_deltas, stream)) return rc;
        HIP_TRY(hipStreamSynchronize(stream));   // (the targets may be replaced behind this call)
        u.has_morph = true;
    }
    if (const int rc = u.morph_active.ensure(T)) return rc;   // (room for every target: the list of a later frame may be longer)
    if (active)
        if (const int rc = upload(u.morph_active, *active, stream)) return rc;
    m.position_deltas = u.morph_position_deltas.p;
    m.normal_deltas = normal_deltas ? u.morph_normal_deltas.p : nullptr;
    return AGPT_OK;
}

int MeshUpdate::device_inputs(hipStream_t stream, const HostMesh& mesh, const DeformRequest& rq) {
    const std::string f = std::string(rq.fn) + ": ";
    if (!rq.status || (!rq.joints16_dev && !rq.weights_dev)) return fail(AGPT_ERR_INVALID, f + "no device inputs, or nowhere to put their status");
    if ((rq.joints16_dev && rq.n_joints != skin_.n_joints) || (rq.weights_dev && rq.n_targets != morph_.n_targets))
        return fail(AGPT_ERR_INVALID, f + "the device inputs do not have the binding's or the targets' counts");
    if (const int rc = ensure_cache(stream, mesh)) return rc;
    MeshDeviceCache& u = *dev_;
    static_assert(sizeof(DeviceInputStatus) == 5 * sizeof(uint32_t), "DeviceInputStatus is the five words of the download");
    if (!u.input_status.p) u.joint_words_clean = false;
    if (const int rc = u.input_status.ensure(5)) return rc;
    if (!u.input_status_host) HIP_TRY(hipHostMalloc((void**)&u.input_status_host, sizeof(DeviceInputStatus), hipHostMallocDefault));
    if (!u.joint_words_clean) HIP_TRY(hipMemsetAsync(u.input_status.p, 0xFF, sizeof(DeviceInputStatus), stream));   // kNoItem everywhere
    u.joint_words_clean = false;   // until they have come back clean
    if (rq.joints16_dev) {
        // room for either stride, as skin_on_device makes it (which then finds the allocation as it is)
        if (const int rc = u.skin_palette.ensure((size_t)rq.n_joints * (size_t)skin_palette_stride(true))) return rc;
        if (const int rc = launch_pack_palette(stream, rq.joints16_dev, rq.n_joints, !mesh.normals.empty() && rq.with_normals, u.skin_palette.p,
                                               u.input_status.p))
            return rc;
    }
    if (rq.weights_dev) {
        if (const int rc = u.morph_active.ensure((size_t)rq.n_targets)) return rc;
        if (const int rc = launch_morph_active(stream, rq.weights_dev, rq.n_targets, u.morph_active.p, u.input_status.p + 3)) return rc;
    }
    HIP_TRY(hipMemcpyAsync(u.input_status_host, u.input_status.p, sizeof(DeviceInputStatus), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::memcpy(rq.status, u.input_status_host, sizeof(DeviceInputStatus));
    u.joint_words_clean = rq.status->nonfinite_joint == kNoItem && rq.status->bad_row_joint == kNoItem && rq.status->singular_joint == kNoItem;
    if (!rq.weights_dev) {   // (k_morph_active did not run: its two words are those of an earlier call)
        rq.status->n_active = 0;
        rq.status->nonfinite_weight = kNoItem;
    }
    return AGPT_OK;
}

// The one launcher of the three deforming kernels.  A pose is a morph without targets as far as the host is concerned: the same rest
// arrays, uploads and grid, k_skin_mesh in place of k_morph_mesh.
int MeshUpdate::deform(hipStream_t stream, const HostMesh& mesh, const DeformRequest& rq) {
    if (const int rc = ensure_rest(rq.fn, stream, mesh)) return rc;
    MeshDeviceCache& u = *dev_;
    if (rq.M) {
        TransformArgs a;
        a.M = *rq.M;
        a.N = *rq.N;
        rest_args(u, mesh, rq.with_normals, a);
        const size_t items = (size_t)a.n_vertices + (size_t)a.n_normals;
        hipLaunchKernelGGL(k_transform_mesh, dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, a);
        HIP_TRY(hipGetLastError());
        return AGPT_OK;
    }
    const bool morph = rq.active || rq.weights_dev, skin = rq.palette || rq.joints16_dev;
    if (!morph && !skin) return fail(AGPT_ERR_INVALID, std::string(rq.fn) + ": neither a matrix, a palette nor an active list");
    // device pointers: device_inputs has left the palette and the active list in the cache, and nothing is launched on a status that is not clean
    if ((rq.weights_dev || rq.joints16_dev) && (!rq.status || !rq.status->clean()))
        return fail(AGPT_ERR_INVALID, std::string(rq.fn) + ": device inputs without a clean status");
    const int n_active = rq.active ? (int)rq.active->size() : rq.weights_dev ? (int)rq.status->n_active : 0;
    MorphArgs m;
    m.position_deltas = m.normal_deltas = nullptr;
    m.s = SkinArgs();
    if (morph)
        if (const int rc = morph_on_device(rq.fn, stream, u, mesh, morph_, rq.active, rq.n_targets, (size_t)n_active, m)) return rc;
    if (skin)
        if (const int rc = skin_on_device(rq.fn, stream, u, mesh, skin_, rq.palette, rq.n_joints, rq.with_normals, m.s)) return rc;
    rest_args(u, mesh, rq.with_normals, m.s);
    // 256-lane blocks on a capped grid: 4 per CU with a skin (its LDS cap), 8 for the morph alone
    const size_t cus = (size_t)(rq.num_cus > 0 ? rq.num_cus : 1);
    size_t blocks = std::min(((size_t)m.s.n_vertices + (size_t)m.s.n_normals + kSkinBlock - 1) / kSkinBlock, cus * (skin ? kSkinBlocksPerCU : kMorphBlocksPerCU));
    if (morph) {   // AGPT_MORPH_MAX_BLOCKS is k_morph_mesh's alone
        if (const char* cap = getenv("AGPT_MORPH_MAX_BLOCKS")) {
            const long c = std::strtol(cap, nullptr, 10);
            if (c >= 1) blocks = std::min(blocks, (size_t)c);
        }
        blocks = std::max(blocks, (size_t)1);
    }
    const dim3 grid((unsigned)blocks), block(kSkinBlock);
    const size_t lds = skin ? (size_t)m.s.n_joints * (size_t)m.s.stride * sizeof(float) : 0;   // the palette's bytes, host- or device-made
    const bool staged = skin && lds <= kSkinLdsBytes && !getenv("AGPT_SKIN_GLOBAL_PALETTE");
    if (!morph) {
        if (staged) hipLaunchKernelGGL(k_skin_mesh<true>, grid, block, lds, stream, m.s);
        else hipLaunchKernelGGL(k_skin_mesh<false>, grid, block, 0, stream, m.s);
    } else if (!skin) {
        hipLaunchKernelGGL((k_morph_mesh<false, false>), grid, block, 0, stream, u.morph_active.p, n_active, m);
    } else if (staged) {
        hipLaunchKernelGGL((k_morph_mesh<true, true>), grid, block, lds, stream, u.morph_active.p, n_active, m);
    } else {
        hipLaunchKernelGGL((k_morph_mesh<true, false>), grid, block, 0, stream, u.morph_active.p, n_active, m);
    }
    HIP_TRY(hipGetLastError());
    return AGPT_OK;
}

int MeshUpdate::download_arrays(hipStream_t stream, std::vector<v3>& vertices, std::vector<v3>& normals) const {
    static_assert(sizeof(v3) == 3 * sizeof(float), "v3 is three packed floats");
    if (!vertices.empty()) HIP_TRY(hipMemcpyAsync(vertices.data(), dev_->verts.p, vertices.size() * sizeof(v3), hipMemcpyDeviceToHost, stream));
    if (!normals.empty()) HIP_TRY(hipMemcpyAsync(normals.data(), dev_->normals.p, normals.size() * sizeof(v3), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return AGPT_OK;
}

int MeshUpdate::download_bounds(hipStream_t stream, HostMesh& mesh) const {
    const int total = dev_->total_nodes;
    std::vector<float4> b(2 * ((size_t)total + 1));
    HIP_TRY(hipMemcpyAsync(b.data(), dev_->bounds.p, b.size() * sizeof(float4), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int i = 0; i <= total; i++) {
        if (i == 1) continue;
        agpt_bvh_node& nd = mesh.nodes[i];
        nd.bmin[0] = b[2 * (size_t)i].x; nd.bmin[1] = b[2 * (size_t)i].y; nd.bmin[2] = b[2 * (size_t)i].z;
        nd.bmax[0] = b[2 * (size_t)i + 1].x; nd.bmax[1] = b[2 * (size_t)i + 1].y; nd.bmax[2] = b[2 * (size_t)i + 1].z;
    }
    return AGPT_OK;
}

}  // namespace agpt
