// agpt_scene.h -- flat, HBM-resident scene representation shared by the host builder and the kernels.
//
// Layout (all arrays 64-B aligned, replicated per GPU):
//   nodes      float4[2*N]  the reference's 32-B BVHNode content (bvhtrimesh.h:126-130: bounds, first, count), stored per
//                           SIBLING PAIR: nodes 2k and 2k+1 (always fetched together, bvhtrimesh.h:350-351) share one
//                           64-B line with their boxes interleaved component-wise --
//                             [4k+0] lx0 rx0 ly0 ry0  [4k+1] lz0 rz0 lx1 rx1  [4k+2] ly1 ry1 lz1 rz1  [4k+3] zL zR wL wR
//                           z = the node's precomputed traversal encoding (interior: child-pair index; leaf:
//                           AGPT_ENC_LEAF|count-1|first slot; leaf with > 7 primitives: AGPT_ENC_BIGLEAF|k, with
//                           (first, count) in bigleaves[2k..]), w = count; all meshes concatenated, indices rebased
//                           to global node / triangle-slot indices
//   tri_verts  float4[3*T]  per REORDERED primitive slot (BVH leaf order): v0,v1,v2; v0.w = global triangle id,
//                           v1.w = flags (bit0: degenerate-reject, quirk 11), v2.w unused.  Replaces the reference's
//                           primitives[] -> indices[] -> vertices[] double indirection (88 B/test -> 48 B/test)
//   tri_shade  float4[4*T]  per global triangle id, ray-independent parts of the SurfaceInteraction the reference
//                           rebuilds on every accepted hit (trianglemesh.cpp:46-111): geometric normal ng,
//                           ss = normalize(dpdu), the three vertex normals, owning primitive
//   tri_uv     float4[2*T]  per global triangle id, ONLY in scenes with a textured material: (u0, v0, u1, v1), (u2, v2, -, -) --
//                           the triangle's texture coordinates (trianglemesh.cpp:46-56; (0,0), (1,0), (1,1) for a mesh without),
//                           two aligned 16-B loads per shaded hit
//   textures   DevTexture[X], material_texture int32[M] (texture id of a material, -1 = none): kept beside DevMaterial so that the
//                           material table the untextured kernels stage in LDS stays what it was.  In a scene with roughness /
//                           metallic maps the table has a second half, material_texture[M + m] = the packed parameter slots of
//                           material m (param_slots_pack below), which only the MAPPED kernel variants read (a SAMPLED scene
//                           -- see DevTexture -- always has it: its kernels are the MAPPED ones with a filtering lookup)
//                           In a scene with a normal map (agpt_scene_set_material_normal_texture) the table is followed, at the next
//                           16-byte boundary, by one DevNormalSlot per material, which only the NORMAL kernel variants read -- straight
//                           from global memory: the halves above are all the LDS a block of k_shade has left
//   prims      DevPrim[P]   Scene::primitives in insertion order (scene.h:5-19 walks them linearly)
//   materials  DevMaterial[M], lights DevLight[L]
// The node, root-pair, prefilter, tri_verts and tri_shade records are written by the functions of agpt_records.h alone, on the host
// (flatten_scene) and on the device (agpt_update.hip).
#pragma once

#include "agpt_math.h"

#define AGPT_PRIM_MESH 0
#define AGPT_PRIM_SPHERE 1
#define AGPT_PRIM_PLANE 2   // intersectable.h:119-157: cx,cy,cz = O, r = HalfSize.x, r2 = HalfSize.y
#define AGPT_LIGHT_AREA 0
#define AGPT_LIGHT_UNIFORM_INFINITE 1
#define AGPT_LIGHT_INFINITE_AREA 2

#define AGPT_HIT_MISS 0xFFFFFFFFu
#define AGPT_HIT_SPHERE 0x80000000u   // analytic primitive (sphere or plane): low bits = primitive index

#define AGPT_TRI_FLAG_REJECT 1u     // degenerate triangle: TriangleIntersect returns false after the t test
#ifndef AGPT_STACK_DEPTH
#define AGPT_STACK_DEPTH 32         // per-lane traversal stack entries staged in LDS (production kernel)
#endif
#define AGPT_MAX_CHUNKS 32          // the production trace kernels walk lists of up to 32 x 64 primitives (beyond: the reference-order kernel)
#define AGPT_STACK_DEPTH_MAX 64     // deepest BVH the generic kernel's 64-entry variant can walk

// traversal-stack / node encoding: bit31 = leaf.  leaf with count<=7: bits 28..30 = count-1, bits 0..27 = first slot.
// leaf with more prims (identical centroids, bvhtrimesh.h:235-238): 0xF0000000 | node index (node is re-fetched).
#define AGPT_ENC_LEAF 0x80000000u
#define AGPT_ENC_BIGLEAF 0xF0000000u

// bound on |coordinate| of ray origins and mesh boxes under which the trace kernels' Markstein divide equals the division (agpt_trace.h)
#define AGPT_MDIV_COORD_LIMIT 0x1p86f

struct DevPrim {
    int32_t type;
    int32_t material;   // -1 = nullptr (emitter spheres)
    int32_t arealight;  // index into lights, -1 = none
    int32_t root;       // mesh: global index of the root node
    int32_t tri_base;   // mesh: global id of its first triangle
    int32_t has_normals;
    int32_t n_tris;
    int32_t mesh_ordinal;  // number of non-empty meshes before this primitive in Scene::primitives
    float cx, cy, cz, r;  // sphere (intersectable.h:161-162)
    float r2;
    float root_bmin[3];   // mesh root bounds (bvhtrimesh.h:185-198 tests them before descending)
    float root_bmax[3];
    uint32_t root_enc;    // encoded root node
};

struct DevMaterial {
    int32_t type;
    int32_t has_diffuse, has_retro, has_microfacet, has_specular;
    float diffuse_R[3];  // diffuseWeight * color
    float roughness;
    float alphax, alphay;
    float R0[3];         // Cspec0
    float metallic, eta;
    float mirror_R[3];
};

// The colour-dependent part of a material (DisneyMaterial / MirrorMaterial ctor, material.h:14-49,72-77), for a material whose
// colour-independent fields are set: make_material runs it once with the material's constant colour, the textured shading
// kernels once per hit with the texel -- the same fp32 operations in the same order.
AGPT_HD void material_set_color(DevMaterial& m, v3 c) {
    if (m.has_microfacet) {   // Disney
        const float eta = 1.5f;
        const float strans = 0.f;
        const float diffuse_weight = (1 - m.metallic) * (1 - strans);
        if (diffuse_weight > 0) {
            v3 d = diffuse_weight * c;
            m.diffuse_R[0] = d.x;
            m.diffuse_R[1] = d.y;
            m.diffuse_R[2] = d.z;
        }
        const float spec_tint = 0.f;
        const v3 ctint = V3s(1.f);
        const float r0 = ((eta - 1) * (eta - 1)) / ((eta + 1) * (eta + 1));  // SchlickR0FromEta, disney.h:23
        v3 cspec0 = lerp3(m.metallic, r0 * lerp3(spec_tint, V3s(1.f), ctint), c);
        m.R0[0] = cspec0.x;
        m.R0[1] = cspec0.y;
        m.R0[2] = cspec0.z;
    } else if (m.has_specular) {   // mirror
        m.mirror_R[0] = c.x;
        m.mirror_R[1] = c.y;
        m.mirror_R[2] = c.z;
    } else {   // diffuse only
        m.diffuse_R[0] = c.x;
        m.diffuse_R[1] = c.y;
        m.diffuse_R[2] = c.z;
    }
}

// The whole DisneyMaterial constructor (material.h:14-49) on a material whose type is set: every field that depends on the colour,
// the roughness or the metallic weight -- the lobe set (has_diffuse / has_retro: diffuseWeight > 0), roughness (DisneyRetro),
// alphax / alphay with both .001 clamps, metallic, eta, diffuse_R (zero without a diffuse lobe), R0.  make_material runs it once with
// the material's constants, the MAPPED shading kernels once per hit with the texels -- the same fp32 operations in the same order.
AGPT_HD void material_set_disney(DevMaterial& m, v3 c, float roughness, float metallic) {
    const float strans = 0.f;
    const float diffuse_weight = (1 - metallic) * (1 - strans);
    m.has_diffuse = m.has_retro = diffuse_weight > 0 ? 1 : 0;
    m.roughness = roughness;
    const float aspect = 1.f;
    float ax = smaxf(.001f, (roughness * roughness) / aspect);
    float ay = smaxf(.001f, (roughness * roughness) * aspect);
    m.alphax = smaxf(0.001f, ax);  // TrowbridgeReitzDistribution ctor, microfacet.h:120-122
    m.alphay = smaxf(0.001f, ay);
    m.metallic = metallic;
    m.eta = 1.5f;
    m.has_microfacet = 1;
    m.diffuse_R[0] = m.diffuse_R[1] = m.diffuse_R[2] = 0.f;
    material_set_color(m, c);   // diffuse_R (with a diffuse lobe), R0
}

// Roughness / metallic maps (agpt_scene_set_material_param_texture): a slot is 0 = the material's constant, or
// (texture id + 1) << 2 | channel in 16 bits; a material's two slots share one word -- parameter p (agpt.h: AGPT_PARAM_ROUGHNESS 0,
// AGPT_PARAM_METALLIC 1) in bits 16p .. 16p + 15 -- so that the table costs the MAPPED kernels one word per material of LDS.  A
// texture with an id above AGPT_PARAM_MAX_TEXTURE cannot be named.
#define AGPT_PARAM_MAX_TEXTURE 16382
AGPT_HD uint32_t param_slots_pack(int rough_texture, int rough_channel, int metal_texture, int metal_channel) {
    const uint32_t r = rough_texture < 0 ? 0u : ((uint32_t)(rough_texture + 1) << 2 | (uint32_t)rough_channel);
    const uint32_t m = metal_texture < 0 ? 0u : ((uint32_t)(metal_texture + 1) << 2 | (uint32_t)metal_channel);
    return r | m << 16;
}
AGPT_HD int param_slot_texture(uint32_t slots, int param) { return (int)((slots >> (16 * param) & 0xFFFFu) >> 2) - 1; }   // -1 = none
AGPT_HD int param_slot_channel(uint32_t slots, int param) { return (int)(slots >> (16 * param) & 3u); }

// An image texture (HDRTexture, texture.h:41-84): texels row-major, row 0 = top, one float4 (rgb, -) each so that a lookup is
// one 16-byte gather.  In a SAMPLED scene (a texture that a material names has a sampler other than nearest / repeat / repeat,
// agpt_scene_set_texture_sampler) the two size words also carry the sampler: width * height <= 2^28 leaves bits 29..31 of both
// free, so the record stays one 16-B load and costs the shading kernels no LDS -- width: bit 31 filter, bits 29..30 wrap_u;
// height: bits 29..30 wrap_v.  Every other scene has the plain sizes there, which is what the TEXTURED and MAPPED kernels read.
struct DevTexture {
    const float4* texels;
    int32_t width, height;
};
#define AGPT_TEXTURE_SIZE_MASK 0x1FFFFFFFu
#define AGPT_TEXTURE_WRAP_REPEAT 0u   // (agpt.h: AGPT_WRAP_*, AGPT_FILTER_*)
#define AGPT_TEXTURE_WRAP_CLAMP 1u
#define AGPT_TEXTURE_WRAP_MIRROR 2u
AGPT_HD int32_t texture_size_pack(int size, int wrap, int filter) {
    return (int32_t)((uint32_t)size | (uint32_t)wrap << 29 | (uint32_t)filter << 31);
}
AGPT_HD int texture_size(int32_t word) { return (int)((uint32_t)word & AGPT_TEXTURE_SIZE_MASK); }
AGPT_HD uint32_t texture_wrap_mode(int32_t word) { return (uint32_t)word >> 29 & 3u; }
AGPT_HD bool texture_bilinear(const DevTexture& t) { return t.width < 0; }

// The normal-map slot of a material (agpt_scene_set_material_normal_texture), in a scene that has one: a copy of the texture's
// record, so that the lookup costs no load behind the table's (its address depends on the material alone, like the records of the
// other slots), the scale, and the texture's id (-1: the material has no normal map; `tex` is then some valid record), by which a slot
// that names the same image shares its taps.  Two 16-byte loads.
struct DevNormalSlot {
    DevTexture tex;
    float scale;
    int32_t texture;
    int32_t pad[2];
};
// where the slots begin in a material_texture table of n_materials materials (in int32 words; a NORMAL scene's table has both halves)
AGPT_HD int normal_slots_offset(int n_materials) { return (2 * n_materials + 3) & ~3; }

struct DevLight {
    int32_t type;
    int32_t shape;  // primitive index of the emitting sphere
    float L[3];
    int32_t env;    // AGPT_LIGHT_INFINITE_AREA: index into DevScene::envs
};

// InfiniteAreaLight's HDRTexture + Distribution1D (lights.cpp:31-48, texture.h:41-84, sampling.h:19-69) in HBM
struct DevEnv {
    const float4* pixels;  // [height*width] rgb
    const float* func;     // [n] max(rgb) * sin(theta_row)
    const float* cdf;      // [n+1]
    int32_t width, height, n;
    float funcInt;
};

struct DevCamera {
    v3 origin, u, v, w, lower_left_corner, horizontal, vertical;
    float lens_radius;
};

struct DevScene {
    const float4* nodes;
    const uint32_t* bigleaves;  // (first, count) pairs, see above
    const float4* tri_verts;
    const float4* tri_shade;
    const DevPrim* prims;
    const DevMaterial* materials;
    const DevLight* lights;
    const DevEnv* envs;
    int32_t n_prims, n_lights, n_materials;
    int32_t n_infinite;        // number of IsInfinite() lights
    int32_t n_meshes;          // non-empty mesh primitives
    int32_t max_depth;         // deepest BVH of the scene (selects the traversal-stack size)
    // Root pairs: for each of the first 64 * AGPT_MAX_CHUNKS primitives that is a non-empty mesh, nodes[] holds one extra pair record at
    // node index rootpair_base + 2k whose LEFT box is the mesh's root box and whose encoding is the mesh's root -- the
    // reference's root-box test at BVHTriMesh::Intersect (bvhtrimesh.h:187,195) then runs as an ordinary interior step
    // of the traversal kernel (the right half of the record is ignored).  mesh_masks: bit k of word c set for primitive
    // 64c + k if it is such a mesh.
    uint32_t rootpair_base;
    unsigned long long mesh_masks[AGPT_MAX_CHUNKS];   // per chunk of 64 primitives
    unsigned long long analytic_masks[AGPT_MAX_CHUNKS];   // spheres and planes, same layout
    // Prefilter table: per non-empty mesh in list order two float4 -- (root bmin.xyz, bit index in its chunk), (root
    // bmax.xyz, -) -- read through scalar loads by the trace kernel's conservative per-primitive filter; chunk c owns the
    // records [pf_begin[c], pf_begin[c + 1]).
    const float4* prefilter;
    int32_t pf_begin[AGPT_MAX_CHUNKS + 1];
    // Top-level tree (primitive lists longer than 64 entries; agpt_host_scene.cpp: build_skip_tree, pack_skip_tree16): a binary
    // tree over the root boxes of all non-empty meshes in depth-first order with skip links, one 16-byte node each: the box
    // as six IEEE halves rounded OUTWARD (x: bmin.x | bmin.y << 16, y: bmin.z | bmax.x << 16, z: bmax.y | bmax.z << 16) and
    // w: index of the node after this node's subtree | (leaf: list index of the primitive / interior: 0xFFFF) << 16.
    // k_candidates walks it once per ray (one 16-byte load per visit: the walk is bound by the vector L1's rate for divergent
    // loads) and leaves one 64-bit candidate word per chunk of 64 primitives; k_trace_fast<LIST> walks the candidates in
    // list order and tests the exact fp32 root boxes.
    const uint4* toplevel;   // 16-byte nodes, see below
    int32_t n_toplevel;
    const unsigned long long* chunk_mesh_masks;   // mesh_masks[] again, in global memory (per-lane chunk index)
    DevCamera cam;
    // image textures: all three NULL unless a material of the scene has one (only the TEXTURED kernel variants read them)
    const float4* tri_uv;
    const DevTexture* textures;
    const int32_t* material_texture;   // [n_materials], or [2 * n_materials] in a scene with roughness / metallic maps (see above)
                                       // (+ DevNormalSlot[n_materials] at normal_slots_offset in a scene with a normal map)
    // 1 iff every finite coordinate of every mesh root box (hence of every node box) is below AGPT_MDIV_COORD_LIMIT in magnitude: the
    // condition on the scene under which the trace kernels' Markstein divide equals the division (agpt_trace.h).  Set by
    // agpt_scene_commit and again after every refit.
    int32_t mdiv_coords_ok;
};

// 16-B hit record written by the trace kernel
struct DevHit {
    float t;
    uint32_t id;  // AGPT_HIT_MISS | AGPT_HIT_SPHERE|prim | global triangle id
    float b1, b2;
};
