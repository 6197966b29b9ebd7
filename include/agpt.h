/* include/agpt.h -- C ABI of libagpt_hip.so, the MI355X (gfx950) path-tracing hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  The reference has no
 * FFI -- its seam is three in-process C++ abstract classes:
 *     Intersectable  intersectable.h:17-61      Scene  scene.h:3-30      Integrator  integrator.h:28-31
 * and the caller is the per-pixel loop of MyApp::Tick (myapp.cpp:163-175).  Each entry point below
 * names the reference interface it replaces (paths relative to the reference checkout); the C++
 * adapter classes that keep reference-style host code unchanged are in include/agpt_host.hpp and the
 * binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions: every function returns AGPT_OK (0) or a negative agpt_status and records a message
 * retrievable with agpt_last_error().  The caller owns host buffers; the library owns device memory
 * except where a parameter is documented as a DEVICE pointer.  One context per GPU/process; calls on
 * one context are serialised by the caller.  All arithmetic is fp32, indices int32.
 */
#ifndef AGPT_H
#define AGPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    AGPT_OK = 0,
    AGPT_ERR_INVALID = -1,   /* bad argument / call order */
    AGPT_ERR_DEVICE = -2,    /* HIP runtime error, no device */
    AGPT_ERR_NOMEM = -3,
    AGPT_ERR_LIMIT = -4,     /* scene exceeds a kernel limit (e.g. BVH deeper than the traversal stack) */
    AGPT_ERR_IO = -5         /* file could not be opened / written (image writers) */
} agpt_status;

typedef struct agpt_ctx agpt_ctx;
typedef struct agpt_scene agpt_scene;

/* material kinds: material.h:11-58 DisneyMaterial, material.h:60-81 MirrorMaterial; DIFFUSE_ONLY is a
 * Material whose SetupBSDF adds a single DisneyDiffuse lobe (disney.h:25-38) -- BASELINE config 2's
 * "Lambertian" (the reference has no Lambertian material). */
enum { AGPT_MAT_DISNEY = 0, AGPT_MAT_MIRROR = 1, AGPT_MAT_DIFFUSE_ONLY = 2 };

/* 32-byte BVH node, identical to the reference's BVHNode (bvhtrimesh.h:126-130) */
typedef struct {
    float bmin[3];
    float bmax[3];
    int32_t first; /* interior: index of the first child (pair first, first+1); leaf: first primitive */
    int32_t count; /* 0 = interior */
} agpt_bvh_node;

/* Ray (camera.h:3-15); d need not be normalised, the library normalises it like Ray's ctor */
typedef struct { float o[3]; float d[3]; float tmax; } agpt_ray;

/* result of Scene::Intersect (scene.h:5-13) reduced to what identifies the hit */
typedef struct {
    int32_t hit;   /* 0/1 */
    int32_t prim;  /* index into Scene::primitives (insertion order); -1 on miss / any-hit queries */
    int32_t tri;   /* triangle meshes: index of the triangle's first index_type (= 3*triangle); else -1 */
    float t, b1, b2;
} agpt_hit;

/* CameraDesc (camera.h:17-25) */
typedef struct {
    float lookfrom[3];
    float lookat[3];
    float vup[3];
    float aspect_ratio;
    float vfov;       /* degrees; reference default 45 */
    float aperture;   /* reference default 0 */
} agpt_camera_desc;

typedef struct {
    uint64_t closest_rays;    /* Scene::Intersect-equivalents: primary + continuation + MIS + emitter pass-through */
    uint64_t anyhit_rays;     /* Scene::IntersectP-equivalents: shadow rays */
    uint64_t interior_visits; /* interior nodes whose child pair was fetched (only if counters enabled) */
    uint64_t tri_tests;       /* triangle tests (only if counters enabled) */
    uint64_t shaded_vertices;
    uint64_t samples;
    uint64_t outliers;        /* NaN/inf samples zeroed (myapp.cpp:169-172) */
    uint64_t iterations;      /* wavefront iterations executed */
    double   trace_ms;        /* HIP-event time of the trace kernels over the call (stream the kernels ran on) */
    double   total_ms;        /* HIP-event time of the whole call */
    uint64_t trace_launches;
    uint64_t root_tests;      /* mesh root-box tests, bvhtrimesh.h:187,195 (only if counters enabled) */
    double   ext_ms, mis_ms, shadow_ms; /* trace_ms split: continuation / MIS closest-hit launches, any-hit launches
                                           (only if agpt_render_params::enable_timing) */
    uint64_t answered_rays;   /* of closest_rays: Scene::Intersect calls of the reference that the production path settles without
                                 a traversal, with the same result for the image -- MIS queries (integrator.h:76-88) towards a
                                 sphere light whose ray misses the light's sphere, and the ray after the last bounce of a path
                                 whose hit nothing reads (integrator.h:139-150).  0 with enable_counters = 1 (reference order). */
} agpt_stats;

/* parameters of one agpt_render call = MyApp::Tick's per-pixel loop (myapp.cpp:163-175) for a tile */
typedef struct {
    int32_t width, height;        /* film size W x H (Accumulator width/height, myapp.h:10) */
    int32_t x0, y0, w, h;         /* tile to render, in film pixels */
    int32_t spp_begin, spp_count; /* samples [spp_begin, spp_begin+spp_count) of every pixel */
    uint32_t seed_base;           /* per-(pixel,sample) stream: WangHash((pixel + W*H*sample + 1)*17 + seed_base) */
    int32_t max_depth;            /* PathTracer::MaxDepth (integrator.h:122), reference default 5 */
    int32_t accum_pitch;          /* row pitch of accum in float4 pixels */
    int32_t accum_row0;           /* film row (after the y flip) that accum's row 0 holds; tile rows map to
                                     accum row (H-1-y) - accum_row0 */
    int32_t samples_per_batch;    /* 0 = library default */
    int32_t enable_counters;      /* 1 = also count interior visits / triangle tests in the reference's order (the instrumented
                                   * reference-order kernel, slower); 2 = the production trace kernel counts the work it
                                   * does itself (child-pair / root-pair records fetched, triangle tests) */
    int32_t enable_timing;        /* 1 = bracket every trace launch with HIP events on the launch stream */
    /* multi-GPU row interleave (0 = off): of the film rows, cut into blocks of interleave_block rows, render only the
     * blocks k with k % interleave_world == interleave_rank (the tile must then be the whole film: x0=y0=0, w=W, h=H).
     * accum is the rank's COMPACT buffer: block j of this rank occupies rows [j*block, j*block+h_j), flipped inside the
     * block like Accumulator::AddSample; accum_row0 is ignored. */
    int32_t interleave_block, interleave_world, interleave_rank;
    int32_t trace_all_rays;       /* 1 = send every Scene::Intersect call of the reference through the BVH.  By default (0) the
                                   * production path only COUNTS the two kinds of call whose answer cannot reach the image (MIS
                                   * queries whose ray misses the sampled sphere light, the ray after a path's last bounce; see
                                   * agpt_stats::answered_rays): same image bit for bit, same ray totals, less work */
} agpt_render_params;

const char* agpt_last_error(void);
int agpt_version(void);

/* context: picks the GPU.  stream = hipStream_t to launch on, or NULL for the null stream.
 * agpt_set_stream: every later call on the context enqueues on `hip_stream` and is ordered with the caller's other work there, a
 *   stream created with hipStreamNonBlocking included.  The context's scratch memory, queues, counters and events are one set shared
 *   by all its calls, and some calls return with work still queued (agpt_render without stats, the tile calls): the call therefore
 *   SYNCHRONISES THE STREAM IT LEAVES before it stores the new one, so that work in flight on the old stream never shares that state
 *   with a call on the new one.  Setting the handle the context already has does nothing.  The handle must belong to the HIP runtime
 *   instance this library is linked to (a process can hold more than one copy of libamdhip64; a handle of another copy is
 *   meaningless here). */
int agpt_init(int device, agpt_ctx** out);
int agpt_set_stream(agpt_ctx*, void* hip_stream);
void agpt_destroy(agpt_ctx*);

/* ---- scene building: mirrors the reference's scene-construction calls (myapp.cpp:13-114) ---------- */
int agpt_scene_create(agpt_ctx*, agpt_scene** out);
void agpt_scene_destroy(agpt_scene*);
/* DisneyMaterial::Make / MirrorMaterial::Make (material.h:60-62,83-85): returns material id >= 0 */
int agpt_scene_add_material(agpt_scene*, int type, const float color[3], float roughness, float metallic);
/* scene->primitives.push_back(make_shared<BVHTriMesh>(TriangleMesh(indices, vertices, normals, texcoords), mat,
 * maxPrimsInNode)) (bvhtrimesh.h:154-178): builds the binned-SAH BVH on the host.  indices are
 * (vertex, normal, texcoord) triplets = index_type (trianglemesh.h:5-12); n_normals / n_texcoords may be 0.
 * returns the primitive index (position in Scene::primitives) */
int agpt_scene_add_mesh(agpt_scene*, const float* vertices, int n_vertices, const float* normals, int n_normals,
                        const float* texcoords, int n_texcoords, const int32_t* indices, int n_indices,
                        int material, int max_prims_in_node);
/* scene->primitives.push_back(make_shared<Sphere>(center, r, material)); material -1 = nullptr */
int agpt_scene_add_sphere(agpt_scene*, const float center[3], float radius, int material);
/* scene->primitives.push_back(make_shared<Plane>(o, size, material)) (intersectable.h:119-157): XZ rectangle, +Y normal */
int agpt_scene_add_plane(agpt_scene*, const float o[3], const float size[2], int material);
/* Scene::addAreaLight(make_shared<Sphere>(center, r, nullptr), L) (scene.h:21-25): returns primitive index */
int agpt_scene_add_area_light(agpt_scene*, const float center[3], float radius, const float L[3]);
/* scene->lights.push_back(make_shared<UniformInfiniteLight>(L)) (lights.h:37-51): returns light index */
int agpt_scene_add_uniform_infinite_light(agpt_scene*, const float L[3]);
/* scene->lights.push_back(make_shared<InfiniteAreaLight>(texmap)) (lights.cpp:31-112 with ILS): the HDR environment map is
 * passed as width*height RGB floats (row-major, row 0 = top), i.e. what stbi_loadf returns in the reference (texture.h:43-53);
 * builds the max(rgb)*sin(theta) Distribution1D (sampling.h:19-69) on the host.  returns light index */
int agpt_scene_add_infinite_area_light(agpt_scene*, const float* rgb, int width, int height);
/* ---- image textures for the base colour of materials --------------------------------------------------------
 * An RGB image for materials: width*height RGB floats, row-major, row 0 = top, LINEAR values -- the same form
 * agpt_scene_add_infinite_area_light takes (an sRGB image is linearised by the host first).  Copied.  Returns the texture
 * id >= 0.  Before agpt_scene_commit. */
int agpt_scene_add_texture(agpt_scene*, const float* rgb, int width, int height);
/* From now on `material`'s colour at a mesh hit is value(u, v) of `texture` instead of the constant it was created with;
 * texture = -1 restores the constant.  Before agpt_scene_commit.  All fp32, every operation rounded on its own:
 *   uv of the hit   TriangleIntersect's (trianglemesh.cpp:46-57): uv = uv0 * b0 + uv1 * b1 + uv2 * b2, summed left to right, with
 *                   b0 = 1 - b1 - b2; a mesh without texture coordinates has (0,0), (1,0), (1,1) at every triangle.
 *   value(u, v)     HDRTexture::value (texture.h:59-79): s = (int)floorf(u * width - .5f), t = (int)floorf(v * height - .5f), both
 *                   wrapped with Mod (a - (a / b) * b, + b if negative), the nearest texel (s, t), no filtering.  A non-finite u
 *                   or v reads texel (0, 0).
 *   what it feeds   exactly what agpt_scene_add_material derives from `color`, recomputed per hit with the same operations in
 *                   the same order (Disney: diffuseWeight * c and Cspec0 = lerp(metallic, R0(eta), c); mirror: R = c; diffuse-only:
 *                   R = c).  The lobe set, roughness and metallic stay per material.  A texture whose texels all equal the
 *                   material's colour therefore renders bit-identical to the untextured scene.
 * Every path that shades sees the texture -- agpt_render, agpt_render_adaptive, agpt_li_batch, in both shading arithmetics (the
 * uv interpolation and the texel choice decide what is read and stay exact under AGPT_SHADING_FAST) -- and agpt_render_features
 * writes the texel as the albedo.  Triangle meshes only: agpt_scene_commit returns AGPT_ERR_INVALID if a sphere or a plane carries a
 * textured material.  Scenes without a textured material run the kernels they ran before textures existed.
 * Both calls return AGPT_ERR_INVALID (+ agpt_last_error) for a NULL argument, a non-positive size, an unknown material or texture
 * id, or a scene that is already committed. */
int agpt_scene_set_material_texture(agpt_scene*, int material, int texture);
/* ---- image textures for the roughness and the metallic weight of Disney materials ------------------------------
 * From now on `material`'s roughness / metallic at a mesh hit is channel `channel` (0 = r, 1 = g, 2 = b) of value(u, v) of
 * `texture` instead of the constant it was created with; texture = -1 restores the constant (channel is then ignored).  Before
 * agpt_scene_commit.  Textures are those of agpt_scene_add_texture: one image may serve several slots of several materials (glTF
 * keeps roughness in g and metallic in b of one image), and the colour slot (agpt_scene_set_material_texture) is independent of
 * these two.
 *   uv, value(u, v)  exactly the colour texture's, above: nearest texel, Mod wrap, texel (0, 0) for a non-finite uv; exact under
 *                    AGPT_SHADING_FAST.
 *   the value        the channel as stored, no clamp: it is treated exactly as if it had been passed to agpt_scene_add_material
 *                    (the host owns the range).
 *   what it feeds    at the hit the material is what agpt_scene_add_material(AGPT_MAT_DISNEY, c, r, m) would have built, with c, r
 *                    and m each the texel or the constant -- the DisneyMaterial constructor (material.h:14-49) per hit, same fp32
 *                    operations in the same order: diffuseWeight = (1 - m) * (1 - 0); the diffuse and the retro lobe exist iff
 *                    diffuseWeight > 0 (metallic 1 drops both); roughness; alphax = alphay = max(.001, max(.001, r * r)); metallic;
 *                    diffuseWeight * c; Cspec0.  A map whose texels equal the constant therefore renders bit-identical to no map, and
 *                    a texel per mesh bit-identical to a material per mesh.
 * Every path that shades sees the maps -- agpt_render, agpt_render_adaptive, agpt_li_batch, in both shading arithmetics.
 * agpt_render_features does not: its albedo stays the colour (or the colour texel), whatever the maps say.  agpt_kat_bsdf_eval /
 * _sample have no hit and keep the constants.  Triangle meshes only: agpt_scene_commit returns AGPT_ERR_INVALID if a sphere or a
 * plane carries a material with a map.  Scenes without a map run the kernels they ran before maps existed.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error) for a NULL scene, an unknown material, param, texture or channel, a material that is
 * not AGPT_MAT_DISNEY (mirror and diffuse-only materials ignore both parameters) or a scene that is already committed, and
 * AGPT_ERR_LIMIT for a texture id above 16382 (a material's two slots are packed into one 32-bit word). */
enum { AGPT_PARAM_ROUGHNESS = 0, AGPT_PARAM_METALLIC = 1 };
int agpt_scene_set_material_param_texture(agpt_scene*, int material, int param, int texture, int channel);
/* ---- filtering and wrap modes of image textures ------------------------------------------------------------------
 * The sampler of `texture`: how value(u, v) above is formed from its texels.  It belongs to the texture (as in glTF) and holds for
 * every slot that names it -- the colour slot, AGPT_PARAM_ROUGHNESS and AGPT_PARAM_METALLIC.  The default, (AGPT_FILTER_NEAREST,
 * AGPT_WRAP_REPEAT, AGPT_WRAP_REPEAT), is value(u, v) as described above.  Before agpt_scene_commit.  All fp32, every operation rounded
 * on its own, nothing contracted into an fma:
 *   position        s = u * width - .5f, t = v * height - .5f (the expressions above).
 *   wrap(x, n)      of an integer coordinate x on an axis of n texels -- REPEAT: Mod(x, n); CLAMP: min(max(x, 0), n - 1); MIRROR:
 *                   m = Mod(x, 2n), then m < n ? m : 2n - 1 - m.  wrap_u holds for x, wrap_v for y.
 *   NEAREST         the texel (wrap_u((int)floorf(s)), wrap_v((int)floorf(t))).
 *   BILINEAR        x0 = (int)floorf(s), fx = s - floorf(s) (exact); y0, fy likewise.  The four taps are c00 = (wrap_u(x0), wrap_v(y0)),
 *                   c10 = (wrap_u(x0 + 1), wrap_v(y0)), c01 = (wrap_u(x0), wrap_v(y0 + 1)), c11 = (wrap_u(x0 + 1), wrap_v(y0 + 1)); x0 + 1
 *                   is formed without integer overflow, and where the float-to-int conversion saturated (|floorf(s)| >= 2^31 or s not
 *                   finite) fx is 0.  Per channel top = c00 + fx * (c10 - c00), bot = c01 + fx * (c11 - c01), c = top + fy * (bot - top)
 *                   -- this form, not (1 - f) * a + f * b: equal taps return the tap exactly, whatever the weights.
 *   non-finite uv   a non-finite u or v reads texel (0, 0), as above.
 *   what it feeds   exactly what the nearest texel feeds above: the colour goes through what agpt_scene_add_material derives from
 *                   `color`; with a map, colour, roughness and metallic go through the DisneyMaterial constructor.  A map's channel is
 *                   taken after the blend.
 * The texel choice and the blend decide what is read and stay exact under AGPT_SHADING_FAST, like the uv interpolation.
 * agpt_render_features writes the filtered colour as the albedo; agpt_kat_bsdf_eval / _sample keep the constants.  Scenes in which no
 * material names a texture with a non-default sampler run the kernels they ran before samplers existed.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error) for a NULL scene, an unknown texture id, an unknown filter or wrap value, or a scene
 * that is already committed. */
enum { AGPT_FILTER_NEAREST = 0, AGPT_FILTER_BILINEAR = 1 };
enum { AGPT_WRAP_REPEAT = 0, AGPT_WRAP_CLAMP = 1, AGPT_WRAP_MIRROR = 2 };
int agpt_scene_set_texture_sampler(agpt_scene*, int texture, int filter, int wrap_u, int wrap_v);
/* ---- tangent-space normal maps ------------------------------------------------------------------------------------
 * From now on `material`'s shading normal at a mesh hit is perturbed by `texture`; texture = -1 removes it (scale ignored).  Before
 * agpt_scene_commit.  Any material type (Disney, mirror, diffuse-only); the texture is one of agpt_scene_add_texture's, read through its
 * own sampler (agpt_scene_set_texture_sampler) like every other slot, and the slot is independent of the colour, roughness and
 * metallic slots.  All fp32, every operation rounded on its own, nothing contracted into an fma:
 *   uv, texel       the hit's uv as above; (r, g, b) = value(u, v) through the texture's sampler, exactly as for the colour slot; a
 *                   non-finite uv reads texel (0, 0).
 *   decode          tx = (2 * r - 1) * scale, ty = (2 * g - 1) * scale, tz = 2 * b - 1.
 *   no-op rule      the hit is left exactly as it was, with no arithmetic on it, if tx == 0 && ty == 0 && tz > 0 (a texel along the
 *                   normal), if m below has a non-finite component, or if sqrlen(m) == 0.  A map of (.5, .5, 1) texels therefore
 *                   renders bit-identical to no map, whatever the scale and the filter.
 *   frame           the one the BSDF uses at that hit, non-orthogonal for an interpolated normal: ns = the shading normal, ss =
 *                   normalize(dpdu) of the triangle (the tangent the BSDF's frame is built on), ts = cross(ns, ss).
 *   perturbed ns    m = (ss.c * tx + ts.c * ty + ns.c * tz per component c, summed left to right); ns' = m * (1 / sqrtf(dot(m, m))).
 *   what stays      the geometric normal (already face-forwarded against the unperturbed ns) and ss; the BSDF then forms its
 *                   ts = cross(ns', ss) as it always does.  A mesh without vertex normals has ns = ng and is perturbed the same way.
 *   conventions     +x of the texel is along normalize(dpdu), +y along cross(ns, ss), rows top-first as everywhere in this ABI; a host
 *                   whose images use the other green convention flips g itself.  A perturbed normal that ends up below the geometric
 *                   surface is not corrected: the host owns the map.
 * Every path that shades sees it -- agpt_render, agpt_render_adaptive, agpt_li_batch.  The perturbation decides ray directions and
 * stays exact under AGPT_SHADING_FAST, like the uv interpolation and the texel blend.  agpt_render_features writes the perturbed
 * normal into normal_depth.xyz (the denoiser's normal edge-stop sees the detail); its albedo is unaffected.  agpt_kat_bsdf_eval /
 * _sample have no hit and are unaffected.  Triangle meshes only: agpt_scene_commit returns AGPT_ERR_INVALID if a sphere or a plane
 * carries such a material.  Scenes without a normal map run the kernels they ran before normal maps existed.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error) for a NULL scene, an unknown material or texture id, a non-finite scale, or a scene
 * that is already committed -- checked in this order, the first that applies is the one reported; the scale is looked at only for
 * texture >= 0. */
int agpt_scene_set_material_normal_texture(agpt_scene*, int material, int texture, float scale);
/* scene->camera = desc; Camera(desc) (camera.h:29-56,77-90) */
int agpt_scene_set_camera(agpt_scene*, const agpt_camera_desc*);
/* flatten + upload to HBM; must be called after the last add_* and before render/intersect */
int agpt_scene_commit(agpt_scene*);

/* BVH inspection (host copy, reference layout): nodes_out has agpt_mesh_num_nodes()+1 entries (slot 1 unused),
 * prim_index_out the reordered Primitive::index list (bvhtrimesh.h:132-145,208) */
int agpt_mesh_num_nodes(const agpt_scene*, int prim);
int agpt_mesh_num_prims(const agpt_scene*, int prim);
int agpt_mesh_get_bvh(const agpt_scene*, int prim, agpt_bvh_node* nodes_out, int32_t* prim_index_out);
/* BVHTriMesh's constructor alone (bvhtrimesh.h:154-178,213-330), host-only -- needs no GPU and no context.
 * indices as in agpt_scene_add_mesh.  nodes_out needs 2*(n_indices/3)+2 entries of capacity (total_nodes+1 are
 * written, slot 1 unused); prim_index_out n_indices/3 entries.  Either output may be NULL. */
int agpt_bvh_build(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, int max_prims_in_node,
                   agpt_bvh_node* nodes_out, int32_t* prim_index_out, int* total_nodes_out, int* max_depth_out);
/* The bounds of an existing tree recomputed for new vertex positions, host-only like agpt_bvh_build: the topology (first and count
 * of every node, prim_index) stays, every box is rebuilt bottom-up with the builder's own comparisons in the builder's order -- a
 * leaf is the +-1e34 box grown over its primitives' vertices in slot order, an interior node (left, right) of its child pair.  With
 * the vertices the tree was built from it returns the builder's bytes.  nodes_inout has total_nodes + 1 entries (slot 1 unused).
 * AGPT_ERR_INVALID for a NULL argument, an index out of range or a tree that is not one of agpt_bvh_build's. */
int agpt_bvh_refit(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, const int32_t* prim_index,
                   agpt_bvh_node* nodes_inout, int total_nodes);
/* New vertex positions (and vertex normals, if the mesh has any) for mesh primitive `prim` of a COMMITTED scene; indices, texture
 * coordinates, material and max_prims_in_node stay.  vertices / normals are host arrays of the mesh's own counts.  Synchronises
 * with the context's stream and leaves the scene committed: every call that reads the scene -- agpt_render*, agpt_intersect_*,
 * agpt_li_batch, agpt_render_features, agpt_dbg_li_batch, agpt_mesh_get_bvh -- sees the new geometry from then on.
 *   REBUILD: a new BVH from the scene's builder (agpt_scene_set_bvh_builder), then the full flatten and upload of agpt_scene_commit:
 *            the scene is what creating it from scratch with the new arrays gives.
 *   REFIT:   the tree keeps its topology and gets agpt_bvh_refit's bounds; the triangle records and the bounds are rewritten on the
 *            GPU (the same bytes as the host flatten's), so the cost is that of the one mesh.  A non-finite position takes the host
 *            refit and the full upload instead.  A tree refitted far from the pose it was built for is still correct but slower to
 *            traverse (its boxes overlap more): the host decides when to REBUILD.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error), checked in this order, for a NULL scene or NULL vertices; a scene that is not
 * committed; a prim that is out of range or not a mesh; an n_vertices or n_normals that differs from the mesh's own count (normals
 * may be NULL only if the mesh has none); an unknown mode.  A refused call changes nothing. */
enum { AGPT_UPDATE_REFIT = 0, AGPT_UPDATE_REBUILD = 1 };
int agpt_scene_update_mesh(agpt_scene*, int prim, const float* vertices, int n_vertices, const float* normals, int n_normals, int mode);
/* agpt_scene_update_mesh with the two arrays in DEVICE memory of the context's GPU (packed xyz floats, the mesh's own counts): the
 * call behaves as agpt_scene_update_mesh would with host copies of them, and leaves the same bytes everywhere.
 *   ordering   the library does not know the stream that produced the arrays: they must be complete when the call is made, or have
 *              been produced on the context's stream (agpt_set_stream).  The call enqueues on the context's stream and synchronises
 *              with it.
 *   ownership  REFIT copies the arrays device-to-device into buffers of its own, REBUILD downloads them, before the call returns;
 *              the caller may reuse them afterwards.
 *   REFIT      one kernel looks at all 3 * n_vertices coordinates (referenced by a triangle or not, the host call's rule) and
 *              reduces "is any Inf or NaN" to one flag; the triangle records and the bounds are rewritten on the GPU as for
 *              agpt_scene_update_mesh.  The flag and the 24-byte root box are all that comes back.  With the flag set the arrays
 *              are downloaded and the host call's path is taken: the host refit and the full upload.
 *   REBUILD    the arrays are downloaded and the scene's builder runs as for agpt_scene_update_mesh.
 * The scene's host copy of the mesh is brought up to date -- by a download -- when something next reads it: a later full upload
 * (agpt_scene_commit, a REBUILD or a non-finite update of any mesh) or the first agpt_scene_transform_mesh of this mesh.
 * agpt_mesh_get_bvh downloads the bounds only.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error) for the same conditions in the same order as agpt_scene_update_mesh (NULL scene or
 * NULL vertices_dev; not committed; not a mesh; counts; unknown mode); a refused call changes nothing.  A pointer that is not
 * device memory is not detected: the copy fails with AGPT_ERR_DEVICE or faults.
 * Not covered: index or texture-coordinate changes, spheres, planes and lights, fewer launches per tree level.  (Temporal history
 * follows the moved meshes through agpt_scene_snapshot_positions and agpt_temporal_accumulate_motion.) */
int agpt_scene_update_mesh_device(agpt_scene*, int prim, const float* vertices_dev, int n_vertices, const float* normals_dev, int n_normals,
                                  int mode);
/* The reference's mat4 applied to a mesh's arrays, host-only like agpt_bvh_build (no GPU, no context).  transform16 is a row-major
 * 4x4 as in agpt_obj_load, and the arithmetic is that loader's (TriangleMesh::LoadObj), fp32, every operation rounded on its own,
 * nothing contracted into an fma, sums left to right:
 *   position   r = (m[4i] * x + m[4i+1] * y + m[4i+2] * z + m[4i+3]) for rows i = 0, 1, 2; w the same with row 3; the result is r
 *              if w == 1, else r * (1 / w) per component.
 *   normal     (n[4i] * x + n[4i+1] * y + n[4i+2] * z) for rows i = 0, 1, 2 of n = the 3x3 transpose of the inverse of m; the inverse
 *              is the cofactor expansion (the 16 cofactors, det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12], each
 *              cofactor times 1 / det).  A matrix whose det is exactly 0 leaves the normals as they are (the reference's rule).
 *              Normals are not renormalised.
 * n_normals may be 0 (normals and normals_out are then ignored).  An output may be its own input.  AGPT_ERR_INVALID for a NULL
 * transform16, vertices or vertices_out, a negative count, or n_normals > 0 with NULL normals or normals_out. */
int agpt_transform_arrays(const float* transform16, const float* vertices, int n_vertices, const float* normals, int n_normals,
                          float* vertices_out, float* normals_out);
/* Mesh primitive `prim` of a COMMITTED scene placed by a matrix, on the GPU: afterwards the scene is byte for byte what
 * agpt_scene_update_mesh(scene, prim, V, n_vertices, N, n_normals, mode) leaves, with V and N = agpt_transform_arrays(transform16,
 * the mesh's rest pose).  The rest pose is the arrays the mesh last received explicitly -- agpt_scene_add_mesh,
 * agpt_scene_update_mesh or agpt_scene_update_mesh_device --, so the transform is absolute, not cumulative: repeated calls do not
 * drift, the same matrix gives the same bytes, and the identity gives the rest pose back.  One lane per vertex and per normal runs
 * agpt_transform_arrays' arithmetic (one source for host and device); the inverse transpose is formed once on the host.  The rest
 * arrays go to the GPU with the mesh's first transform and stay there; per call only the matrix goes up, and under REFIT the
 * finiteness flag and the root box come down (a non-finite transformed position takes the host path, as above).  REBUILD downloads
 * the transformed arrays and rebuilds.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error), checked in this order: the conditions of agpt_scene_update_mesh that apply (NULL
 * scene; not committed; not a mesh; unknown mode); a NULL matrix; a non-finite entry; a determinant (the value above) of exactly 0.
 * A refused call changes nothing.  Not covered: as for agpt_scene_update_mesh_device. */
int agpt_scene_transform_mesh(agpt_scene*, int prim, const float* transform16, int mode);
/* Linear-blend skinning of a mesh's arrays by a palette of joint matrices, host-only like agpt_transform_arrays (no GPU, no context)
 * and built on its arithmetic: fp32, every operation rounded on its own, nothing contracted into an fma.
 *   inputs     joints16: n_joints (1 .. 65536) row-major 4x4 M_j, each with the last row exactly (0, 0, 0, 1).  Every vertex has
 *              `influences` = K (1 .. 8) slots (joint, weight): vertex_joints / vertex_weights are flat, stride K.  Normals have
 *              slots of their own (normal_joints / normal_weights, n_normals * K); both may be NULL only when n_normals == n_vertices,
 *              and the vertex slots then serve both.  n_normals may be 0.
 *   position   the slots in order k = 0 .. K-1; a slot whose weight is exactly 0 (either sign) is skipped; the first used slot sets
 *              acc = w * P per component, every later one acc = acc + w * P, with P = agpt_transform_arrays' position through M_j;
 *              a vertex whose every weight is 0 keeps its rest position.  Weights are used as given: neither normalised nor
 *              reordered.
 *   normal     the same walk over the normal's slots with agpt_transform_arrays' normal through n_j = the 3x3 transpose of the
 *              inverse of M_j (a determinant of exactly 0 gives the identity, the reference's rule).  Not renormalised.
 * One used slot of weight 1 gives the bits of agpt_transform_arrays(M_j, ...); so do two slots of 0.5 with the same joint.
 * An output may be its own input.  AGPT_ERR_INVALID (+ agpt_last_error) for a NULL argument or a bad count, influences outside
 * 1 .. 8, n_joints outside 1 .. 65536, a joint index out of range, a weight that is negative or not finite, a last row that is not
 * exactly (0, 0, 0, 1); a refused call writes nothing. */
int agpt_skin_arrays(const float* joints16, int n_joints, int influences,
                     const float* vertices, int n_vertices, const int32_t* vertex_joints, const float* vertex_weights,
                     const float* normals, int n_normals, const int32_t* normal_joints, const float* normal_weights,
                     float* vertices_out, float* normals_out);
/* The binding of mesh primitive `prim` for agpt_scene_pose_mesh: its vertices' (and normals') influences as in agpt_skin_arrays, with
 * the mesh's own counts, and the number of joints every later pose must bring.  May be called any time after agpt_scene_add_mesh, on
 * a committed scene or not.  The scene keeps a host copy and uploads nothing; the first pose takes the binding to the GPU, where it
 * stays.  Setting it again replaces the binding (the device copies are dropped); influences == 0 removes it (the other arguments are
 * then ignored).  agpt_scene_update_mesh / _device keep the binding: the counts cannot change, and the new arrays become the rest pose.
 * AGPT_ERR_INVALID (+ agpt_last_error) for a NULL scene, a prim that is not a mesh of the scene, and agpt_skin_arrays' conditions on
 * influences, n_joints, the four arrays and their contents; a refused call changes nothing. */
int agpt_scene_set_mesh_skin(agpt_scene*, int prim, int influences, int n_joints, const int32_t* vertex_joints, const float* vertex_weights,
                             const int32_t* normal_joints, const float* normal_weights);
/* Mesh primitive `prim` of a COMMITTED scene posed by its skin, on the GPU: afterwards the scene is byte for byte what
 * agpt_scene_update_mesh(scene, prim, V, n_vertices, N, n_normals, mode) leaves, with V and N = agpt_skin_arrays(joints16, the mesh's
 * rest pose, the binding).  The rest pose is agpt_scene_transform_mesh's -- the arrays the mesh last received explicitly --, so a pose
 * is absolute, not cumulative; pose and transform calls may alternate, and the last one wins.  One lane per vertex and per normal runs
 * agpt_skin_arrays' arithmetic (one source for host and device) on a palette of M_j and n_j formed on the host: per call
 * n_joints * (12 + 9) floats go up (12 for a mesh without normals), and under REFIT the finiteness flag and the root box come down (a
 * non-finite posed position takes the host path, as for the other update calls).  REBUILD downloads the posed arrays and rebuilds;
 * the binding goes up again with the next pose.  A palette of up to 40 KiB is staged in LDS; AGPT_SKIN_GLOBAL_PALETTE in the
 * environment (read at every call) makes the kernel read it from global memory instead, as a larger one is.  Same bytes either way.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error), checked in this order: the conditions of agpt_scene_update_mesh that apply (NULL
 * scene; not committed; not a mesh; unknown mode); a mesh without a skin; NULL joints16; an n_joints that is not the binding's; a
 * non-finite entry; a last row that is not exactly (0, 0, 0, 1); a joint whose determinant (agpt_transform_arrays' value) is exactly
 * 0, named in the message.  A refused call changes nothing.
 * Out of scope: sparse morph targets, tangent deltas, dual-quaternion blending (and what agpt_scene_update_mesh_device does not
 * cover).  Morph targets: agpt_scene_morph_mesh.  Joint matrices in device memory: agpt_scene_pose_mesh_device.  Normals recomputed
 * from the posed positions: agpt_scene_set_mesh_normals_mode. */
int agpt_scene_pose_mesh(agpt_scene*, int prim, const float* joints16, int n_joints, int mode);
/* The palette agpt_scene_pose_mesh forms from a frame's joint matrices, host-only like agpt_skin_arrays (no GPU, no context): per joint
 * rows 0 .. 2 of M_j (12 floats) and, with_normals != 0, the 3x3 of n_j (9 floats, agpt_skin_arrays' arithmetic) -- palette_out
 * receives n_joints * 21 floats, or n_joints * 13 without (the odd strides of the GPU's staging; the thirteenth float is a pad
 * of 0).  *singular_out (may be NULL) receives the first joint whose determinant is exactly 0, or -1: such a joint is reported, not
 * refused, and its n_j is the identity.  AGPT_ERR_INVALID (+ agpt_last_error) for NULL joints16 or palette_out, n_joints outside
 * 1 .. 65536, a non-finite entry, a last row that is not exactly (0, 0, 0, 1), in that order and in agpt_scene_pose_mesh's words;
 * a refused call writes nothing. */
int agpt_skin_palette(const float* joints16, int n_joints, int with_normals, float* palette_out, int* singular_out);
/* agpt_scene_pose_mesh with the matrices in DEVICE memory of the context's GPU (n_joints row-major 4x4, packed): the call leaves the
 * scene byte for byte what agpt_scene_pose_mesh leaves with a host copy of them -- REFIT, REBUILD and the non-finite-position path,
 * either normals mode, either palette route.  Nothing of the matrices crosses the bus: k_pack_palette, one lane per joint, runs
 * agpt_skin_palette's arithmetic (one source for host and device) into the palette k_skin_mesh reads and reduces the three checks of
 * the matrices to three words, each the lowest offending joint; those come back in one 20-byte download, and the pose is launched
 * only when they are clean.  That is one stream round trip more than agpt_scene_pose_mesh makes.
 *   ordering   as for agpt_scene_update_mesh_device: the matrices must be complete when the call is made, or have been produced on
 *              the context's stream (agpt_set_stream).  The call enqueues on that stream and synchronises with it.
 *   ownership  the caller may reuse the array when the call returns.
 *   alignment  joints16_dev must be 16-byte aligned (the kernel reads a matrix as four 16-byte rows).
 * Returns AGPT_ERR_INVALID (+ agpt_last_error) for agpt_scene_pose_mesh's conditions in its order, with its messages behind this
 * call's name -- they name the same joint: the lowest with a non-finite entry; if there is none, the lowest with a bad last row; if
 * there is none, the lowest with a determinant of exactly 0 -- and, after the n_joints check, for a joints16_dev that is not 16-byte
 * aligned.  A refused call changes nothing in the scene.  A pointer that is not device memory is not detected.
 * Out of scope: a binding given in device memory; a variant without the extra round trip (the pose predicated on the status words). */
int agpt_scene_pose_mesh_device(agpt_scene*, int prim, const float* joints16_dev, int n_joints, int mode);
/* Morph targets (blend shapes) applied to a mesh's arrays, host-only like agpt_skin_arrays (no GPU, no context): fp32, every operation
 * rounded on its own, nothing contracted into an fma.
 *   inputs     n_targets = T (1 .. 4096) targets and T weights.  Target t has one position delta per vertex and, optionally, one normal
 *              delta per NORMAL (a mesh may have other counts of normals than vertices): position_deltas is T * n_vertices * 3 floats,
 *              normal_deltas T * n_normals * 3 or NULL, both target-major ([t][item][xyz]).  n_normals may be 0.
 *   position   acc = the vertex; the targets in order t = 0 .. T-1; a target whose weight is exactly 0 (either sign) is skipped; every
 *              other one adds acc = acc + w[t] * delta[t][i] per component, the product rounded, then the sum.  Weights are used as
 *              given: any finite value, negative and above 1 included, neither normalised nor reordered.
 *   normal     the same walk with the normal deltas; with normal_deltas == NULL the normals are copied through.  Not renormalised.
 * All weights zero gives the input arrays bit for bit.  The skip is by weight, not by delta: a target of weight 1 with an all-zero
 * delta turns a coordinate of -0.0 into +0.0.
 * An output may be its own input.  AGPT_ERR_INVALID (+ agpt_last_error) for a NULL argument or a bad count, n_targets outside
 * 1 .. 4096, a weight that is not finite, a delta that is not finite (the message names target and item); a refused call writes
 * nothing. */
int agpt_morph_arrays(const float* weights, int n_targets,
                      const float* vertices, int n_vertices, const float* position_deltas,
                      const float* normals, int n_normals, const float* normal_deltas,
                      float* vertices_out, float* normals_out);
/* The morph targets of mesh primitive `prim` for agpt_scene_morph_mesh: deltas as in agpt_morph_arrays, with the mesh's own counts
 * (normal_deltas NULL: the targets leave the normals alone; ignored for a mesh without normals), and the number of weights every later
 * morph must bring.  May be called any time after agpt_scene_add_mesh, on a committed scene or not.  The scene keeps a host copy and
 * uploads nothing; the first morph takes the deltas to the GPU, where they stay.  Setting them again replaces the targets (the device
 * copies are dropped); n_targets == 0 removes them (the other arguments are then ignored).  agpt_scene_update_mesh / _device keep the
 * targets: the counts cannot change, and the new arrays become the rest pose.  A REBUILD -- by any update call of this mesh --
 * destroys the mesh's device cache, so the next morph uploads the deltas again: for a large target set that re-upload
 * (n_targets * (n_vertices + n_normals) * 12 bytes) is the cost of REBUILD.
 * AGPT_ERR_INVALID (+ agpt_last_error) for a NULL scene, a prim that is not a mesh of the scene, n_targets outside 0 .. 4096, NULL
 * position_deltas, a delta that is not finite; a refused call changes nothing. */
int agpt_scene_set_mesh_morph_targets(agpt_scene*, int prim, int n_targets, const float* position_deltas, const float* normal_deltas);
/* Mesh primitive `prim` of a COMMITTED scene morphed by its targets and, with joints16 != NULL, then posed by its skin (glTF's order),
 * on the GPU: afterwards the scene is byte for byte what agpt_scene_update_mesh(scene, prim, V, n_vertices, N, n_normals, mode) leaves,
 * with (V, N) = agpt_morph_arrays(weights, the mesh's rest pose, the targets) when joints16 is NULL (n_joints is then ignored), and
 * agpt_skin_arrays(joints16, the binding, that (V, N)) otherwise -- so a vertex without a used slot keeps its MORPHED position.  The
 * rest pose is the one of agpt_scene_transform_mesh and agpt_scene_pose_mesh: the call is absolute, not cumulative; the three may
 * alternate, and the last one wins.  One lane per vertex and per normal runs the twins' arithmetic (one source for host and device);
 * the morphed value goes to the skin in registers: one kernel, no intermediate array.  Per call only the ACTIVE targets go up -- 8 bytes
 * (index, weight) for every weight that is not 0 -- and, with a skin, agpt_scene_pose_mesh's palette; the kernel walks the active list, so
 * a frame costs by the targets in use, not by the targets bound.  Under REFIT the finiteness flag and the root box come down (a
 * non-finite morphed position takes the host path, as for the other update calls); REBUILD downloads the arrays and rebuilds, and the
 * deltas (and the binding) go up again with the next morph.  The palette is staged as for agpt_scene_pose_mesh
 * (AGPT_SKIN_GLOBAL_PALETTE applies).  AGPT_MORPH_MAX_BLOCKS in the environment (a positive integer, read at every call) lowers the
 * number of blocks the kernel is launched with; same bytes whatever its value -- it exists so that a test can drive the kernel's stride
 * loop on a small mesh.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error), checked in this order: the conditions of agpt_scene_update_mesh that apply (NULL
 * scene; not committed; not a mesh; unknown mode); a mesh without morph targets; NULL weights; an n_targets that is not the one the
 * targets were set with; a weight that is not finite; then, with joints16, agpt_scene_pose_mesh's remaining checks in its order (a mesh
 * without a skin; n_joints; a non-finite entry; a last row; a singular joint).  A refused call changes nothing.
 * Out of scope: sparse targets (a delta for every item of every target is stored), tangent deltas (and what
 * agpt_scene_update_mesh_device does not cover).  Weights and joint matrices in device memory: agpt_scene_morph_mesh_device.  Normals
 * recomputed from the morphed positions (glTF's advice for targets without normal deltas): agpt_scene_set_mesh_normals_mode. */
int agpt_scene_morph_mesh(agpt_scene*, int prim, const float* weights, int n_targets, const float* joints16, int n_joints, int mode);
/* The active list agpt_scene_morph_mesh forms from a frame's weights, host-only like agpt_morph_arrays (no GPU, no context): the
 * (target, weight) pairs of the weights that are not 0 (either sign of zero is skipped), in ascending target order.  targets_out and
 * weights_out have room for n_targets entries; *n_active_out receives the number written.  AGPT_ERR_INVALID (+ agpt_last_error) for a
 * NULL argument, n_targets outside 1 .. 4096, a weight that is not finite (agpt_morph_arrays' message); a refused call writes nothing. */
int agpt_morph_active(const float* weights, int n_targets, int32_t* targets_out, float* weights_out, int* n_active_out);
/* agpt_scene_morph_mesh with the weights and, for the fused call, the joint matrices in DEVICE memory of the context's GPU (joints16_dev
 * may be NULL: no skin stage, n_joints is ignored): the call leaves the scene byte for byte what agpt_scene_morph_mesh leaves with
 * host copies of them, in every mode, either normals mode, either palette route and whatever AGPT_MORPH_MAX_BLOCKS says.  k_morph_active,
 * one block, compacts the weights into agpt_morph_active's list -- a pair's place comes from ballots and popcounts, never from an
 * atomic, so the list is in target order -- and counts it; with joints16_dev, agpt_scene_pose_mesh_device's k_pack_palette runs beside
 * it.  The count and the status words come back in one 20-byte download, and the morph is launched only when they are clean: one
 * stream round trip more than agpt_scene_morph_mesh makes, and nothing goes up per frame.
 * Ordering, ownership and the alignment of joints16_dev: as for agpt_scene_pose_mesh_device; weights_dev needs the 4 bytes of a float.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error) for agpt_scene_morph_mesh's conditions in its order, with its messages behind this
 * call's name: they name the lowest target with a non-finite weight, then agpt_scene_pose_mesh_device's joint.  A refused call
 * changes nothing in the scene.  Out of scope: targets' deltas given in device memory; as for agpt_scene_pose_mesh_device. */
int agpt_scene_morph_mesh_device(agpt_scene*, int prim, const float* weights_dev, int n_targets, const float* joints16_dev, int n_joints,
                                 int mode);
/* Smooth vertex normals from positions and topology, host-only like agpt_morph_arrays (no GPU, no context): fp32, every operation
 * rounded on its own, nothing contracted into an fma.  indices are n_indices (vertex, normal, texcoord) triplets -- corners -- as in
 * agpt_scene_add_mesh; triangle t owns the corners 3t, 3t+1, 3t+2.
 *   face vector   g_t = cross(p_b - p_a, p_c - p_a), a, b, c the vertex indices of the corners 3t, 3t+1, 3t+2: area-weighted, not normalised.
 *   normal item j the corners in ascending order whose normal index is j: the first sets acc = g of its triangle, every later one
 *                 acc = acc + g per component.  A triangle that names j at two corners contributes twice.  The order is part of the
 *                 definition.
 *   finish        l2 = dot(acc, acc); the result is (+0, +0, +0) if no corner names j, if !(l2 > 0) or if l2 is not finite; otherwise
 *                 acc * (1.0f / sqrtf(l2)).
 * Shading reads a zero normal as "use the geometric normal", so an unreferenced item, zero-area or exactly cancelling faces, a sum whose
 * square underflows (|acc| below about 2^-75) or overflows (above 2^64) and NaN or Inf positions -- which are NOT refused -- all have a
 * defined, harmless value.  Writes 3 * n_normals floats; also serves a host that loads an OBJ without normals.
 * AGPT_ERR_INVALID (+ agpt_last_error) for a NULL pointer, n_vertices <= 0 or n_normals <= 0, n_indices < 3 or not a multiple of 3, a
 * vertex or normal index out of range (agpt_scene_add_mesh's rules); a refused call writes nothing.
 * Limit: an item of very high valence is summed by one thread (on the GPU: one lane).  Out of scope: angle-weighted or crease-angle
 * normals, tangents. */
int agpt_vertex_normals_arrays(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, int n_normals,
                               float* normals_out);
/* Where the normals of mesh primitive `prim` come from at an update.  GIVEN (the default): from the caller, or from the transform, skin
 * or morph of the rest normals, as documented at each call.  SMOOTH: EVERY update call of the mesh -- agpt_scene_update_mesh, _device,
 * agpt_scene_transform_mesh, agpt_scene_pose_mesh, agpt_scene_morph_mesh, fused morph + skin included -- leaves the scene byte for byte
 * what the same call's positions V would leave through agpt_scene_update_mesh(scene, prim, V, n_vertices, N, n_normals, mode) in GIVEN
 * mode with N = agpt_vertex_normals_arrays(V, the mesh's indices).
 *   update_mesh / _device   normals (normals_dev) may be NULL and is never read; n_normals is still checked against the mesh's count,
 *              and every other refusal and their order are unchanged.
 *   transform / pose / morph   the normal halves of their kernels get an item count of zero, and the palette goes up without its
 *              normal part; normal deltas and normal slots are kept but not read.
 *   REFIT      after the front end has left the positions on the GPU, k_face_normals (one lane per triangle, 16 bytes each into a
 *              per-mesh scratch) and k_vertex_normals (one lane per normal item, walking a CSR adjacency in ascending corner order)
 *              write the normals there, and the refit runs as before: no normals cross the bus, no atomics, the same bytes every run.
 *              The adjacency (4 * (n_normals + 1 + n_indices) bytes) is built on the host and uploaded by the mesh's first SMOOTH
 *              device update, and kept.  A REBUILD -- by any update call of this mesh -- destroys the mesh's device cache, so the next
 *              REFIT uploads it again.
 *   REBUILD and a non-finite position   the positions come down as for GIVEN, agpt_vertex_normals_arrays' function fills the normals
 *              on the host, and the host path continues.
 *   rest pose  stays "the arrays the mesh last received explicitly": an explicit update in SMOOTH mode makes (V, the recomputed N) the
 *              rest pose.  Switching back to GIVEN changes nothing until the next call, which then uses the rest normals as before.
 * May be called any time after agpt_scene_add_mesh, on a committed scene or not; it stores the mode and changes nothing else (no
 * record, no buffer: the scene reads the same before and after).  A mesh in GIVEN mode runs what it ran before, with no new launch.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error), checked in this order: NULL scene; a prim that is not a mesh of the scene; an unknown
 * mode; SMOOTH for a mesh without normals (the counts cannot change, so there is nothing to write into).
 * Limit: a normal item of very high valence is summed by one lane.  Out of scope: angle-weighted or crease-angle normals, adding
 * normals to a mesh that has none, tangents, spheres, planes and lights. */
enum { AGPT_NORMALS_GIVEN = 0, AGPT_NORMALS_SMOOTH = 1 };
int agpt_scene_set_mesh_normals_mode(agpt_scene*, int prim, int mode);
/* Which builder agpt_scene_add_mesh uses for the BVH of later meshes on this scene (default HOST).  Both produce the same
 * bytes; DEVICE runs agpt_bvh_build_device on the scene's context. */
enum { AGPT_BVH_BUILDER_HOST = 0, AGPT_BVH_BUILDER_DEVICE = 1 };
int agpt_scene_set_bvh_builder(agpt_scene*, int builder);
/* The arithmetic of the scene's shading kernels (default EXACT).  Scene state, valid before or after agpt_scene_commit; it takes
 * effect at the next agpt_render, agpt_li_batch, agpt_kat_bsdf_eval or agpt_kat_bsdf_sample call on the scene (no recommit).
 *   EXACT: correctly rounded fp32 divides and square roots, sin / cos / acos / atan2 correctly rounded through fp64 -- renders
 *          bit-identical to the oracle.
 *   FAST:  the path weights -- BSDF f and pdf (lobe evaluation, Fresnel, microfacet D and G), light pdfs, MIS weights, the
 *          contributions and the throughput -- use the hardware reciprocal (a * rcp(b) for a / b), square root and reciprocal
 *          square root (the half vector of the microfacet lobe alone keeps its exact bits: a smooth lobe turns its last bit
 *          into a tenth of D).  What decides a ray stays exact: sampled directions and their trigonometry, surface frames, the
 *          environment map's texel choices, ray origins / directions / tmax, traversal and intersection (the MIS pre-test
 *          included), camera rays, the RNG streams, accumulation and the queue logic.  A FAST render therefore traces the same
 *          rays as an EXACT one and is deterministic: bit-identical across repeated calls, samples_per_batch splits and rank
 *          shares.  Tested at BSDF f / pdf within rel 1e-4 (sampled wi within abs 1e-5), >= 99 % of pixels within rel 1e-3 of
 *          the oracle with the same seeds at 1-2 spp, per-channel image means within rel 1e-3 at 16 spp.
 * A NULL scene or an unknown mode returns AGPT_ERR_INVALID. */
enum { AGPT_SHADING_EXACT = 0, AGPT_SHADING_FAST = 1 };
int agpt_scene_set_shading_arith(agpt_scene*, int mode);
/* Which of the library's shading kernels the next agpt_render / agpt_render_adaptive / agpt_li_batch on a committed scene launches,
 * host-only (no GPU work): out4 = { texturing level 0 .. 4 (plain, colour textures, parameter maps, non-default samplers, normal
 * maps), arithmetic (AGPT_SHADING_EXACT / _FAST), scene tables in LDS (1) or read from global memory (0: more than 256 primitives,
 * 128 materials or 64 lights, or AGPT_SHADE_GLOBAL_TABLES set in the environment), an InfiniteAreaLight is present }.  Computed
 * by the code those calls use, the environment read included.  All instantiations compute the same values; the query is for tests
 * and profiling.  A NULL argument or an uncommitted scene returns AGPT_ERR_INVALID. */
int agpt_scene_shade_variant(const agpt_scene*, int32_t out4[4]);
/* agpt_bvh_build on the context's GPU: same arguments, same outputs byte for byte; synchronises with the context's stream.
 * *on_device_out (may be NULL) is 0 when a referenced coordinate is non-finite or the mesh's extent overflows: then the host
 * builder ran (the device folds are exact only on finite input).  HIP errors return AGPT_ERR_DEVICE / AGPT_ERR_NOMEM. */
int agpt_bvh_build_device(agpt_ctx*, const float* vertices, int n_vertices, const int32_t* indices, int n_indices,
                          int max_prims_in_node, agpt_bvh_node* nodes_out, int32_t* prim_index_out, int* total_nodes_out,
                          int* max_depth_out, int* on_device_out);
/* Work tiers of the device builder: nodes of up to LANE_MAX primitives are built whole by one lane; larger ones level by level,
 * one 64-lane block per CHUNK primitives. */
enum { AGPT_BVH_DEVICE_LANE_MAX = 64, AGPT_BVH_DEVICE_CHUNK = 2048 };
/* The top-level structure the library builds over Scene::primitives (scene.h:5-19) when the list is longer than 64 entries,
 * host-only (no GPU, no context): a binary tree over n boxes (6 floats each: bmin.xyz, bmax.xyz) in depth-first order with
 * skip links.  Writes 2n-1 nodes of 8 floats -- (bmin.xyz, uint32 index of the node after this node's subtree), (bmax.xyz,
 * uint32 leaf: index of the box / interior: 0xFFFFFFFF) -- and returns the node count.  A ray collects its candidate
 * primitives with "hit -> next node, miss -> skip link"; the walk over the candidates stays in list order. */
int agpt_toplevel_build(const float* boxes6, int n, float* nodes8_out);
/* The 16-byte node form the GPU reads: per node 4 words -- bmin.x | bmin.y << 16, bmin.z | bmax.x << 16, bmax.y | bmax.z << 16
 * as IEEE halves rounded OUTWARD (bmin down, bmax up; no half denormals; beyond +-65504 -> +-inf), skip | leaf << 16 as
 * 16-bit indices (leaf 0xFFFF = interior).  nodes8 = agpt_toplevel_build's output.  Host-only. */
int agpt_toplevel_pack16(const float* nodes8, int n_nodes, uint32_t* packed4_out);
/* TriangleMesh::CreateBackdrop (trianglemesh.cpp:232-318), host-side scene prep.
 * capacities: vertices/normals 3*2*(steps+5) floats, texcoords 2*2*(steps+5), indices 3*6*(steps+4) ints */
int agpt_create_backdrop(const float origin[3], const float size[3], float radius, int steps, float* vertices,
                         float* normals, float* texcoords, int32_t* indices, int* n_vertices, int* n_indices);

/* TriangleMesh::LoadObj (trianglemesh.cpp:157-230): OBJ text -> the four arrays agpt_scene_add_mesh takes.  Host-only.
 * transform16 = row-major mat4 (template/precomp.h:845-1030) applied to points (TransformPoint) and, as inverse
 * transpose, to normals; NULL = identity.  Polygons are triangulated like the tinyobjloader 2.0.0 the reference vendors.
 * Errors (unreadable file, malformed / zero face index, face referencing a missing normal or texcoord) return
 * AGPT_ERR_INVALID with agpt_obj_last_error() -- the reference calls exit(1) / reads out of bounds instead. */
typedef struct agpt_obj_mesh agpt_obj_mesh;
int agpt_obj_load(const char* path, const float* transform16, int ignore_normals, agpt_obj_mesh** out);
int agpt_obj_parse(const char* text, size_t length, const float* transform16, int ignore_normals, agpt_obj_mesh** out);
int agpt_obj_counts(const agpt_obj_mesh*, int* n_vertices, int* n_normals, int* n_texcoords, int* n_indices);
int agpt_obj_get(const agpt_obj_mesh*, float* vertices, float* normals, float* texcoords, int32_t* indices);
void agpt_obj_free(agpt_obj_mesh*);
const char* agpt_obj_last_error(void);

/* ---- hot path -------------------------------------------------------------------------------------- */
/* Scene::Intersect (any_hit=0, scene.h:5-13) / Scene::IntersectP (any_hit=1, scene.h:15-19) for n rays.
 * rays/out are HOST arrays (copied in/out); BVHTriMesh::RecursiveHit/RecursiveHitP (bvhtrimesh.h:332-413),
 * TriangleIntersect/P (trianglemesh.cpp:7-155), Sphere::Intersect/P (intersectable.h:164-226) run on the GPU. */
int agpt_intersect_batch(agpt_scene*, const agpt_ray* rays, int n, agpt_hit* out, int any_hit, agpt_stats* stats);
/* Same, with rays_dev / out_dev DEVICE arrays (e.g. from agpt_device_alloc or the host application's own HIP
 * allocations): nothing crosses PCIe; enqueued on the context's stream and synchronised before returning. */
int agpt_intersect_device(agpt_scene*, const agpt_ray* rays_dev, int n, agpt_hit* out_dev, int any_hit, agpt_stats* stats);

/* MyApp::Tick's loop body for every pixel of the tile and every sample in the range:
 *   jitter -> Camera::GetRay -> PathTracer::Li -> NaN/inf reject -> Accumulator::AddSample  (myapp.cpp:165-173)
 * accum_dev is a DEVICE pointer to float4 pixels (rgb + unused w); samples are ADDED in sample order, so
 * successive calls continue a progressive render (Accumulator, myapp.h:17-32).  Returns after the work
 * has been enqueued and, if stats != NULL, synchronised. */
int agpt_render(agpt_scene*, const agpt_render_params*, float* accum_dev, agpt_stats* stats);

/* ---- adaptive sampling -------------------------------------------------------------------------------------
 * agpt_render_adaptive works in rounds.  A tile pixel holding n samples (samples [0, n) of its agpt_render streams, already in
 * accum.rgb; n = accum.w) is ACTIVE when n < max_spp and either n < min_spp or the stop test fails:
 *     mu = luminance(accum.rgb) / n,  var = max(0, moment2 / n - mu*mu) * n / (n - 1)
 *     stop <=> sqrt(var / n) <= rel_error * max(mu, abs_floor)          (rel_error <= 0: never -- every pixel to max_spp)
 * The test is fp32, every operation rounded on its own, the divisions and the square root IEEE; every max(a, b) is fmaxf: a NaN
 * operand yields the other one, so a NaN moment2 is a variance of 0 (the pixel stops), as in agpt_denoise below.
 * An active pixel takes samples [n, n + step_spp) in sample order: accum.rgb += clr exactly as agpt_render, moment2 += Y*Y
 * (Y = luminance(clr) after the NaN / inf reject, fp32), accum.w = n + step_spp.  Rounds repeat until no pixel is active.  The
 * decision reads only the pixel's own buffers, so the result is independent of batching, tiles, rank shares and how calls are
 * split, and every pixel is bit-identical to agpt_render's pixel at spp = its own count. */
typedef struct {
    int32_t min_spp;    /* every pixel reaches at least this; multiple of step_spp, >= 2 */
    int32_t max_spp;    /* no pixel goes beyond; multiple of step_spp, <= 1 << 24 (w holds the count exactly) */
    int32_t step_spp;   /* samples an active pixel gets per round, >= 1 */
    float   rel_error;  /* stop test threshold; <= 0: off, every pixel to max_spp */
    float   abs_floor;  /* luminance floor of the test's denominator (dark pixels), >= 0 */
} agpt_adaptive_params;

typedef struct {
    int32_t  rounds;            /* rounds this call ran (a full-tile warm-up to min_spp counts as one) */
    int32_t  active_last;       /* pixels that took samples in the last round */
    uint64_t samples;           /* samples this call added */
    uint64_t pixels_stopped;    /* tile pixels left with min_spp <= n < max_spp (stopped by the test) */
} agpt_adaptive_stats;

/* rp as for agpt_render (film, tile, seed_base, max_depth, accum_pitch / accum_row0, interleave, samples_per_batch as a batch cap,
 * trace_all_rays, counters, timing) except that spp_begin and spp_count must be 0: the counts come from accum.w.  moment2_dev:
 * DEVICE, one float per pixel indexed like accum (same pitch, row flip and compact interleave layout), not NULL; the caller keeps
 * it with accum between calls -- a later call with a larger max_spp or a smaller rel_error continues the frame.  A fresh frame
 * starts with accum and moment2 zeroed.  A tile pixel whose count is not an integer multiple of step_spp in [0, 2^24] returns
 * AGPT_ERR_INVALID before any sample is added.  stats (may be NULL) covers the whole call; astats may be NULL.  Synchronises
 * with the context's stream (one read-back per round). */
int agpt_render_adaptive(agpt_scene*, const agpt_render_params* rp, const agpt_adaptive_params* ap, float* accum_dev,
                         float* moment2_dev, agpt_stats* stats, agpt_adaptive_stats* astats);

/* ---- first-hit feature buffers and the denoiser -----------------------------------------------------------------
 * agpt_render_features casts ONE ray per tile pixel through the pixel centre -- film position ((x + 0.5) / W, (y + 0.5) / H) through
 * Camera::GetRay's arithmetic (camera.h:58-64) with the lens offset zero whatever the aperture; no RNG is drawn, so the buffers do
 * not depend on a seed -- and runs one Scene::Intersect (scene.h:5-13) on it (the launch path of agpt_intersect_device).  Per pixel:
 *     albedo       = (color.rgb, flag)   flag 1: a primitive with a material (Disney, mirror or diffuse-only), color = what
 *                                                agpt_scene_add_material was given, bit for bit -- or, for a material with a
 *                                                texture (agpt_scene_set_material_texture) on a mesh, the texel at the hit
 *                                        flag 2: an emitter (a primitive with the null material), color = (1, 1, 1)
 *                                        flag 0: a miss, color = (1, 1, 1)
 *     normal_depth = (ns.xyz, t)         ns = the shading normal the path tracer shades that hit with (shading.n: the interpolated
 *                                        normal of a mesh with normals, else the geometric one; +y for a plane), except that a
 *                                        sphere's is written as (p - c) / r, p = o + t d: the value Sphere::Intersect's dpdu x dpdv
 *                                        expression has for a p exactly on the sphere, without that expression's loss of accuracy
 *                                        near the poles (up to 2e-4 in fp32).  t = the hit distance; 0 on a miss
 * rp: film, tile, accum_pitch and accum_row0 as for agpt_render -- both outputs are DEVICE float4 buffers indexed like accum (same
 * pitch and row flip); spp_begin, spp_count and the interleave_* fields must be 0 (AGPT_ERR_INVALID otherwise); seed_base, max_depth
 * and the remaining fields are ignored.  Synchronises with the context's stream. */
int agpt_render_features(agpt_scene*, const agpt_render_params* rp, float* albedo_dev, float* normal_depth_dev);

/* agpt_denoise: a variance-guided edge-avoiding a-trous filter over an adaptive render's buffers and its feature buffers.
 * accum_dev / moment2_dev are agpt_render_adaptive's (the count in accum.w); a UNIFORM render for denoising is agpt_render_adaptive
 * with rel_error <= 0 and min_spp = max_spp.  All buffers cover the full film, pitch = width, Accumulator::pixels order.
 * Everything is fp32, every operation rounded on its own, divisions and square roots IEEE; luminance(c) = 0.212671 r + 0.715160 g +
 * 0.072169 b summed left to right; expc(x) = (float)exp((double)x), the correctly rounded value through fp64; every max(a, b) is
 * fmaxf: a NaN operand yields the other one.  Subnormal values are kept, not flushed.
 *   Prepare, per pixel:  n = accum.w.  Unless n > 0 (0, -0, a negative or a NaN count) the pixel is EXCLUDED (weight 0 as a tap,
 *       output rgb 0).  Otherwise (n need not be an integer: agpt_temporal_accumulate hands over effective counts)
 *       c = accum.rgb / n;   v = 0 for n < 2, else with mu = luminance(accum.rgb) / n:
 *       v = max(0, moment2 / n - mu * mu) * n / (n - 1) / n        (the variance of the mean luminance, agpt_render_adaptive's estimate)
 *       with demodulate:  a = max(albedo.rgb, 1e-3) per channel,  c = c / a,  v = v / (luminance(a) * luminance(a))
 *   Pass i = 0 .. iterations - 1 (spacing s = 1 << i), for pixel p, from the state (c, v) the previous pass left:
 *       over the taps q = p + s * (dx, dy), dy = -2 .. 2 outermost, dx = -2 .. 2, that lie inside the film:
 *           h = k[dx] * k[dy],  k = (1/16, 1/4, 3/8, 1/4, 1/16)
 *           a tap with flag_q != flag_p or an excluded q is skipped (w = 0); otherwise
 *           ez = |t_p - t_q| / (sigma_z * s * max(t_p, 1e-3))                        (0 when flag_p == 0: sky)
 *           en = ((ns_p - ns_q) . (ns_p - ns_q)) / (sigma_n * sigma_n)               (0 when flag_p == 0)
 *           el = |Y_p - Y_q| / (sigma_l * sqrt(v_p) + 1e-6),  Y = luminance(c)
 *           w = h * expc(-((ez + en) + el))
 *           sw += w;  sc += w * c_q (per channel);  sv += (w * w) * v_q             (in tap order; the centre tap has w = h)
 *       c' = sc / sw,  v' = sv / (sw * sw)
 *   Finish (in the last pass): rgb = c' * a with demodulate, else c';  out.w = 1.
 * Non-finite inputs: a NaN albedo channel is the floor 1e-3 and a NaN moment2 a variance of 0 (fmaxf).  A NaN t_p also floors ez's
 * denominator, but ez's numerator is NaN with it.  The filter does not contain non-finite radiance: an Inf or NaN accum.rgb, or a NaN
 * t, makes w * c_q NaN (0 * Inf included) for every pixel of the same flag that taps the pixel, and each pass carries that on, so after
 * k iterations the pixels within 2 * (2^k - 1) of it in x and in y may be NaN, and none farther.  Hosts clamp or drop non-finite
 * samples before denoising.
 * out_dev: DEVICE float4, rgb = the denoised MEAN radiance, w = 1 -- agpt_resolve(out, n, 1) and agpt_resolve_counts(out, n) both
 * display it.  It must not alias an input; the inputs are not written.  The one ping-pong scratch buffer is the context's
 * (allocated on first use, released by agpt_destroy).  No atomics and a fixed order: repeated calls are bit-identical.  Enqueued
 * on the context's stream and synchronised before returning. */
typedef struct {
    int32_t width, height;   /* all buffers: full film, pitch = width, Accumulator::pixels order */
    int32_t iterations;      /* passes with tap spacing 1, 2, 4, ...; 1..8 */
    int32_t demodulate;      /* 1: filter radiance / albedo, multiply back at the end; 0: filter radiance */
    float sigma_z, sigma_n, sigma_l;   /* > 0; AGPT_DENOISE_SIGMA_* are the defaults the tools use */
} agpt_denoise_params;
#define AGPT_DENOISE_SIGMA_Z 1.0f
#define AGPT_DENOISE_SIGMA_N 0.25f
#define AGPT_DENOISE_SIGMA_L 4.0f
int agpt_denoise(agpt_ctx*, const agpt_denoise_params*, const float* accum_dev, const float* moment2_dev, const float* albedo_dev,
                 const float* normal_depth_dev, float* out_dev);

/* ---- temporal reprojection of render history -----------------------------------------------------------------------
 * Camera(desc) (camera.h:29-56) as the library derives it: out22 = origin, u, v, w, lower_left_corner, horizontal, vertical
 * (3 floats each) and lens_radius -- the values agpt_scene_set_camera stores.  Host-only, needs no context: for hosts that project
 * points themselves.  AGPT_ERR_INVALID for a NULL argument. */
int agpt_camera_vectors(const agpt_camera_desc*, float out22[22]);

/* agpt_temporal_accumulate: the temporal half of the SVGF-style filter agpt_denoise is the spatial half of.  Per frame the host
 * renders a few samples (agpt_render_adaptive -> accum_cur, moment2_cur, fresh buffers) and the feature buffers (agpt_render_features
 * -> albedo_cur, normal_depth_cur) with cam_cur; this call finds for every pixel where the surface it sees was on the previous
 * film, fetches the history accumulated there and adds it to the frame's sums:
 *     agpt_temporal_accumulate -> agpt_denoise(ctx, ..., hist_accum_out, hist_moment2_out, albedo_cur, normal_depth_cur, out)
 * The host keeps hist_accum_out, hist_moment2_out, albedo_cur and normal_depth_cur for the next frame, where they are
 * hist_accum_prev, hist_moment2_prev, albedo_prev and normal_depth_prev (all four NULL on the first frame, else all non-NULL).
 * The outputs have the form of agpt_render_adaptive's buffers -- sums with the count in w, and the luminance second moment --, so
 * agpt_denoise and agpt_resolve_counts take them as they are; but their w is an EFFECTIVE count that need not be an integer: they
 * must NOT be handed back to agpt_render_adaptive.
 * Everything is fp32, every operation rounded on its own (no fma), divisions and square roots IEEE; dot (summed left to right),
 * length = sqrt(dot) and normalize = v * (1 / sqrt(dot)).  For film pixel (x, y), buffer index i = (H-1-y) * W + x:
 *   1. a = accum_cur[i] (rgb sums, n_c = a.w), m_c = moment2_cur[i], flag = albedo_cur[i].w, g = normal_depth_cur[i].
 *   2. First frame (prev NULL): the outputs are the current values, bit for bit.
 *   3. The position on the previous film.  If the bytes of cam_prev equal the bytes of cam_cur (decided once per call):
 *      x0 = x, y0 = y, fx = fy = 0, te = g.w, without arithmetic.  Otherwise, with C = Camera(cam_cur), P = Camera(cam_prev):
 *        D = the direction agpt_render_features' ray through (x, y) has with C
 *        Q = flag != 0 ? (C.origin + g.w * D) - P.origin : D        (a miss is a point at infinity: the sky reprojects under rotation)
 *        te = length(Q);  L = P.lower_left_corner - P.origin;  dw = dot(Q, P.w);  !(dw < 0): NO HISTORY (not in front of P)
 *        k = dot(L, P.w) / dw;  R = Q * k - L
 *        s = dot(R, P.horizontal) / dot(P.horizontal, P.horizontal);  t likewise with P.vertical
 *        sx = s * W - .5f,  sy = t * H - .5f;  !(sx > -1 && sx < W && sy > -1 && sy < H): NO HISTORY (also for NaN)
 *        x0 = (int)floorf(sx), fx = sx - floorf(sx);  y0, fy likewise
 *   4. The taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) in this order, b = (1-fx)*(1-fy), fx*(1-fy), (1-fx)*fy, fx*fy.
 *      A tap q (buffer index by its own row flip) is used iff it lies inside the film, b > 0, n_q = hist_accum_prev[q].w > 0,
 *      albedo_prev[q].w == flag and, if flag != 0, fabsf(te - normal_depth_prev[q].w) <= depth_tol * fmaxf(te, 1e-3f) and
 *      dot(g.xyz, normal_depth_prev[q].xyz) >= normal_cos.  In tap order:
 *        sb += b;  sn += b * n_q;  sc += b * (hist_accum_prev[q].rgb / n_q) per channel;  sm += b * (hist_moment2_prev[q] / n_q)
 *   5. !(sb >= AGPT_TEMPORAL_MIN_WEIGHT): NO HISTORY.  Otherwise n_h = fminf(sn / sb, max_history), c_h = sc / sb, m_h = sm / sb,
 *        out.rgb = a.rgb + c_h * n_h,  out.w = n_c + n_h,  moment2_out = m_c + m_h * n_h
 *      (a current pixel with n_c == 0 takes the history alone).
 *   6. NO HISTORY (disocclusion): the outputs are the current values, bit for bit.
 * One thread computes one pixel in this fixed order, without atomics: repeated calls are bit-identical.  The outputs alias no
 * input and not each other; the inputs are not written.  Enqueued on the context's stream and synchronised before returning.
 * Returns AGPT_ERR_INVALID (+ agpt_last_error), checked in this order, for: NULL params; a bad film size (as agpt_denoise);
 * max_history not positive and finite; depth_tol negative or not finite; normal_cos outside [-1, 1] or NaN; a NULL context or a
 * NULL current or output pointer; prev pointers that are partly NULL; an output that aliases an input or the other output.
 * Not covered: moving geometry -- here it is handled only by the depth, normal and flag tests rejecting stale history;
 * agpt_temporal_accumulate_motion (below) follows meshes that the update calls moved --; history behind specular bounces (a mirror
 * image is reprojected as the mirror's surface); more than one GPU or buffers that are not the full film; variance clamping --
 * agpt_temporal_accumulate_clamped (below) clamps the history to the current frame's neighbourhood --; sub-pixel jitter. */
typedef struct {
    int32_t width, height;            /* all buffers: full film, pitch = width, Accumulator::pixels order (row H-1-y) */
    agpt_camera_desc cam_cur, cam_prev;
    float max_history;                /* cap on the reprojected sample count, > 0, finite */
    float depth_tol;                  /* relative depth tolerance, >= 0, finite   (default 0.05) */
    float normal_cos;                 /* minimum dot(ns_cur, ns_prev), in [-1, 1] (default 0.9)  */
} agpt_temporal_params;
#define AGPT_TEMPORAL_DEPTH_TOL 0.05f
#define AGPT_TEMPORAL_NORMAL_COS 0.9f
#define AGPT_TEMPORAL_MIN_WEIGHT 1e-2f
int agpt_temporal_accumulate(agpt_ctx*, const agpt_temporal_params*,
        const float* accum_cur_dev, const float* moment2_cur_dev, const float* albedo_cur_dev, const float* normal_depth_cur_dev,
        const float* hist_accum_prev_dev, const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
        float* hist_accum_out_dev, float* hist_moment2_out_dev);

/* ---- spheres, planes and lights of a COMMITTED scene, moved in place ---------------------------------------------------
 * A sphere or a plane is five floats of one device record, a light's radiance three; nothing else on the device is derived from them.
 * The calls below rewrite those bytes and the host's copy, enqueue on the context's stream, synchronise with it and leave the scene
 * committed.  Afterwards the scene is, byte for byte, what agpt_scene_commit uploads for a scene built with the new values, so every
 * render, agpt_li_batch, agpt_intersect_*, agpt_render_features and agpt_dbg_li_batch result is that scene's.  The values are
 * absolute, not cumulative.  The host applies the result like a camera move (clear the accumulator).
 *   agpt_scene_update_sphere     prim: a sphere (agpt_scene_add_sphere) or a light's sphere (what agpt_scene_add_area_light returned);
 *                                the record of agpt_scene_add_sphere: the centre, the radius and radius * radius.
 *   agpt_scene_update_plane      prim: a plane; the record of agpt_scene_add_plane: o and size / 2 per axis.
 *   agpt_scene_set_area_light_radiance      prim: what agpt_scene_add_area_light returned.
 *   agpt_scene_set_infinite_light_radiance  light: what agpt_scene_add_uniform_infinite_light returned.
 * AGPT_ERR_INVALID (+ agpt_last_error), checked in this order, scene untouched: a NULL argument; a scene that is not committed; a prim
 * (a light) out of range or of another type; for the area-light call a sphere without a light; any non-finite value, radius <= 0, a
 * plane size <= 0.  The last rule is stricter than the add calls' on purpose: a NaN primitive can make an emitter re-cast a path for
 * ever, and that must not be reachable from a per-frame call.  L may be any finite value, zero and negative included. */
int agpt_scene_update_sphere(agpt_scene*, int prim, const float center[3], float radius);
int agpt_scene_update_plane(agpt_scene*, int prim, const float o[3], const float size[2]);
int agpt_scene_set_area_light_radiance(agpt_scene*, int prim, const float L[3]);
int agpt_scene_set_infinite_light_radiance(agpt_scene*, int light, const float L[3]);
/* agpt_scene_update_sphere for n spheres at once with the new values in DEVICE memory of the context's GPU (a particle or rigid-body
 * step that never visits the host): prims is a HOST array of n distinct sphere primitive ids (lights' spheres among them),
 * center_radius_dev n records (cx, cy, cz, radius) of 16 bytes each, 16-byte aligned.  Ordering as for agpt_scene_update_mesh_device:
 * the records must be complete when the call is made, or have been produced on the context's stream.
 * One kernel reduces "any value Inf or NaN, or a radius <= 0" over the n records to one flag word, the only thing that comes back;
 * with the flag set the call returns AGPT_ERR_INVALID and nothing has been written.  Otherwise one lane per record writes the five
 * floats of its primitive: the same bytes as n agpt_scene_update_sphere calls.
 * AGPT_ERR_INVALID before any launch, in this order: a NULL argument; a scene that is not committed; n < 0; a pointer that is not
 * 16-byte aligned; walking the list, an id out of range or not a sphere, or an id listed twice.  n == 0 is AGPT_OK and launches
 * nothing.  A pointer that is not device memory is not detected.
 * The scene's host copy of the spheres is brought up to date -- by a download -- when something next reads it: agpt_scene_commit, an
 * AGPT_UPDATE_REBUILD of any mesh, agpt_dbg_li_batch. */
int agpt_scene_update_spheres_device(agpt_scene*, const int32_t* prims, int n, const float* center_radius_dev);

/* ---- motion vectors: temporal history that follows moved meshes, spheres and planes ------------------------------------
 * Step 3 above reprojects the point the pixel sees NOW; for a mesh that agpt_scene_update_mesh / _device, agpt_scene_transform_mesh,
 * agpt_scene_pose_mesh or agpt_scene_morph_mesh moved since the previous frame that is the wrong place on the previous film.  The three
 * calls below reproject where that surface point WAS instead.  Per frame:
 *     update calls -> agpt_scene_snapshot_positions -> agpt_render_adaptive -> agpt_render_features_motion
 *                  -> agpt_temporal_accumulate_motion -> agpt_denoise
 *
 * agpt_scene_snapshot_positions: once per frame, after that frame's mesh updates and before its feature pass.  The scene owns two
 * generations of world-space triangle positions, float4[3 * T] each (T = the scene's triangles), indexed by the GLOBAL triangle id
 * (meshes in the order they were added, each mesh's triangles in index-array order) and not by BVH slot, so an AGPT_UPDATE_REBUILD
 * between two snapshots changes nothing.  The call makes the newer generation the older one and fills the newer one from the positions
 * the update calls left on the device (every route: no updater knows about snapshots); the w lanes are 0.  The first call allocates
 * both generations and leaves the same bytes in both: nothing has moved yet.  A scene that never calls this allocates and launches
 * nothing.  A scene with a sphere or a plane also keeps two generations of analytic records by PRIMITIVE index -- (cx, cy, cz, r) and r2,
 * for a plane o and the two half-sizes --, filled by one more small launch from the device's primitive records (so agpt_scene_update_sphere,
 * _plane and _spheres_device are all seen) under the same rules.  T == 0 skips the triangle part only; a scene with neither triangles
 * nor spheres nor planes succeeds without a launch.  agpt_scene_commit drops both generations of both kinds; an AGPT_UPDATE_REBUILD,
 * which re-commits with every id unchanged, keeps them.
 * AGPT_ERR_INVALID for a NULL or an uncommitted scene.  Enqueued on the context's stream behind the updates and synchronised. */
int agpt_scene_snapshot_positions(agpt_scene*);

/* agpt_render_features_motion: agpt_render_features -- the same ray, the same one trace launch, albedo and normal_depth byte for
 * byte -- plus, from the same hit, prev_point_dev (DEVICE float4, indexed like the other two) = (p.xyz, w):
 *     a miss                        (0, 0, 0, 0)
 *     a sphere or a plane k         if its 20 record bytes are the same in the two generations: p = O + t * D, w = 2 (O, D: the pixel's
 *                                   ray).  Otherwise w = 1 and, with c the centre (a plane's o), _old / _new the generation and
 *                                   s = (q, q, q), q = r_old / r_new for a sphere, s = (r_old / r_new, 1, r2_old / r2_new) for a plane:
 *                                   p = c_old + ((O + t * D) - c_new) * s per component -- the same point of the surface before the move
 *                                   (spheres do not rotate).  If a component of s or of that p is not finite: w = 2, p = O + t * D.
 *     a triangle with global id g   if its 36 position bytes are the same in the two generations: p = O + t * D, w = 2 (not moved);
 *                                   otherwise w = 1 and, with v0, v1, v2 its positions in the OLDER generation and (b1, b2) the hit's
 *                                   barycentrics, b0 = (1 - b1) - b2,  p = (v0 * b0 + v1 * b1) + v2 * b2 per component
 * fp32, every operation rounded on its own, no fma.  The comparison is on bytes: -0 against +0 counts as moved (harmless: the point is
 * the same).  rp and the argument checks as for agpt_render_features; then AGPT_ERR_INVALID for a NULL prev_point_dev, for
 * prev_point_dev aliasing another output, and for a scene without a snapshot.  Synchronises with the context's stream. */
int agpt_render_features_motion(agpt_scene*, const agpt_render_params* rp, float* albedo_dev, float* normal_depth_dev, float* prev_point_dev);

/* agpt_temporal_accumulate_motion: agpt_temporal_accumulate's contract with step 3 decided per pixel by m = prev_point_cur[i]
 * (agpt_render_features_motion's output for this frame, full film):
 *     m.w != 1 (a miss, static geometry, any other value, NaN): step 3 exactly as above, the same-camera-bytes shortcut included.
 *     m.w == 1: no shortcut, even if the camera bytes are equal.  Q = m.xyz - P.origin, and from te = length(Q) on step 3 continues
 *               as written (dw, k, R, s, t, sx, sy and the NO HISTORY exits); steps 4-6 unchanged.
 * On the first frame (prev NULL) the outputs are the current values bit for bit and prev_point_cur is not read.  Where every w != 1
 * the outputs are agpt_temporal_accumulate's, bit for bit.  Checks: agpt_temporal_accumulate's in their order, then a NULL
 * prev_point_cur_dev, then an output aliasing it (AGPT_ERR_INVALID).
 * Limits: the normal test compares the current normal with the previous tap's, so a surface that turns by more than
 * acos(normal_cos) within one frame is rejected -- agpt_temporal_accumulate_surface_motion (below) compares the normal the surface
 * point had a frame ago instead; no motion vectors behind specular bounces; a moved light's sphere carries its own
 * history, but what it lights is followed by agpt_temporal_accumulate_clamped only; one GPU, full film. */
int agpt_temporal_accumulate_motion(agpt_ctx*, const agpt_temporal_params*,
        const float* accum_cur_dev, const float* moment2_cur_dev, const float* albedo_cur_dev, const float* normal_depth_cur_dev,
        const float* hist_accum_prev_dev, const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
        float* hist_accum_out_dev, float* hist_moment2_out_dev, const float* prev_point_cur_dev);

/* ---- neighbourhood clamping of temporal history against stale lighting ------------------------------------------------
 * The two calls above accept history by geometry alone (flag, depth, normal).  A static receiver whose LIGHTING changed -- the floor
 * a moved mesh's shadow left -- passes all three, and its history of up to max_history samples keeps saying "in shadow": the shadow
 * trails behind the object.  agpt_temporal_accumulate_clamped clamps the reprojected history mean to a box mu +- gamma * sigma built
 * from the CURRENT frame's neighbourhood, and cuts a clamped pixel's history count so that what is left of it fades.
 * prev_point_cur_dev == NULL: steps 1-4 and 6 are agpt_temporal_accumulate's; otherwise agpt_temporal_accumulate_motion's.  The first
 * frame (prev NULL) returns the current values bit for bit and reads nothing else.  Only step 5 changes.
 *   Neighbourhood statistics of pixel p = (x, y), from the current frame only: taps q = (x + dx, y + dy) in film coordinates,
 *   dy = -r .. r outermost, dx = -r .. r.  A tap is used iff it lies inside the film, n_q = accum_cur[q].w > 0 and
 *   albedo_cur[q].w == albedo_cur[p].w.  x_q = accum_cur[q].rgb / n_q; with demodulate, x_q = x_q / fmaxf(albedo_cur[q].rgb, 1e-3f)
 *   per channel.  In tap order, starting from +0:  k += 1.f;  s1 += x_q;  s2 += x_q * x_q  (per channel).  Then per channel
 *       mu = s1 / k,  var = fmaxf(s2 / k - mu * mu, 0),  sd = sqrtf(var),  lo = mu - gamma * sd,  hi = mu + gamma * sd.
 *   5'. !(sb >= AGPT_TEMPORAL_MIN_WEIGHT): NO HISTORY (and the window is not read).  Otherwise
 *       n_raw = fminf(sn / sb, max_history), c_h = sc / sb, m_h = sm / sb.  If k > 0, per channel j, with
 *       a_j = fmaxf(albedo_cur[p].j, 1e-3f):   d = demodulate ? c_h.j / a_j : c_h.j;   e = fminf(fmaxf(d, lo_j), hi_j);
 *       if !(e == d) the channel is CLAMPED: c_h.j = demodulate ? e * a_j : e.  (The == is deliberate: an unclamped channel keeps its
 *       bits -- no demodulation round trip --, and signed zeros do not count.)  If any channel was clamped, with Y = agpt_denoise's
 *       luminance, c_old the three channels before and c_new after the clamp:
 *           m_h = fmaxf(m_h - Y(c_old) * Y(c_old), 0) + Y(c_new) * Y(c_new)       (the history keeps its variance around the new mean)
 *           n_h = fminf(n_raw, clamped_max_history)
 *       otherwise n_h = n_raw.  Then, as in step 5:  out.rgb = a.rgb + c_h * n_h,  out.w = n_c + n_h,  moment2_out = m_c + m_h * n_h.
 * Every fmaxf / fminf returns the other operand for a NaN, as in agpt_denoise: NaN bounds (a NaN neighbour, or Inf * 0 from
 * gamma = +Inf and sd = 0) clamp nothing; a NaN history channel is replaced by a bound.  With gamma = +Inf and finite buffers the
 * outputs are the unclamped call's, bit for bit.  fp32, every operation rounded on its own (no fma), divide and square root IEEE; one
 * thread produces one pixel, without atomics: repeated calls are bit-identical.
 * Checks (AGPT_ERR_INVALID): agpt_temporal_accumulate's in their order, then a NULL clamp struct; radius outside 1..3; demodulate
 * not 0 or 1; gamma negative or NaN; clamped_max_history not positive and finite; an output aliasing prev_point_cur_dev.
 * Not covered: clamping in another colour space or to a min/max box; what the other two calls do not cover. */
typedef struct {
    int32_t radius;               /* window half-width r: (2r+1)^2 taps of the CURRENT frame; 1..3 */
    int32_t demodulate;           /* 0 / 1: statistics and clamp on radiance / max(albedo, 1e-3), as agpt_denoise demodulates */
    float   gamma;                /* box half-width in standard deviations; >= 0, not NaN; +Inf never clamps */
    float   clamped_max_history;  /* cap on the history count of a pixel whose history was clamped; > 0, finite */
} agpt_temporal_clamp_params;
int agpt_temporal_accumulate_clamped(agpt_ctx*, const agpt_temporal_params*, const agpt_temporal_clamp_params*,
        const float* accum_cur_dev, const float* moment2_cur_dev, const float* albedo_cur_dev, const float* normal_depth_cur_dev,
        const float* hist_accum_prev_dev, const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
        float* hist_accum_out_dev, float* hist_moment2_out_dev, const float* prev_point_cur_dev /* may be NULL */);

/* ---- previous-frame normals: temporal history that follows turning surfaces --------------------------------------------
 * agpt_temporal_accumulate_motion finds the previous pixel of a moved surface point and then tests the normal it has NOW against the
 * normal the previous frame stored there: a surface that turned by more than acos(normal_cos) loses its history.  The three calls
 * below carry the shading normal the point had a frame ago.  Per frame:
 *     update calls -> agpt_scene_snapshot_surfaces -> agpt_render_adaptive -> agpt_render_features_surface_motion
 *                  -> agpt_temporal_accumulate_surface_motion -> agpt_denoise
 *
 * agpt_scene_snapshot_surfaces: agpt_scene_snapshot_positions -- the same rules, the same generation flip, the same analytic records --
 * and two generations of the per-triangle shading records (64 B per global triangle id: geometric normal, tangent, the three vertex
 * normals, primitive id; float4[4 * T] each, 128 B per triangle for the two).  The newer one is filled by one device-to-device copy of the
 * records every update route leaves on the device, on the context's stream behind the updates.  The first call allocates both and
 * leaves the same bytes in both.  If the scene's last snapshot was made by agpt_scene_snapshot_positions, or there was none, the shading
 * generations count as absent and the call behaves like a first call for them; agpt_scene_snapshot_positions after this call frees them.
 * agpt_scene_commit drops them, an AGPT_UPDATE_REBUILD keeps them.  T == 0 skips the shading part.  Errors as agpt_scene_snapshot_positions. */
int agpt_scene_snapshot_surfaces(agpt_scene*);

/* agpt_render_features_surface_motion: agpt_render_features_motion -- albedo, normal_depth and prev_point byte for byte -- plus
 * prev_normal_dev (DEVICE float4, indexed like the others) = (n.xyz, w), w = prev_point's w:
 *     a miss                           (0, 0, 0, 0)
 *     w == 2                           n = the bits of normal_depth.xyz
 *     w == 1, a sphere or a plane      n = the bits of normal_depth.xyz (spheres do not rotate; a plane's normal is +y)
 *     w == 1, a triangle g             n = what normal_depth.xyz would be for this hit if g's shading record were the OLDER generation's:
 *                                      the same reconstruction at this hit's barycentrics (the interpolated-normal frame and its
 *                                      fallbacks included) and, for a material with a normal map, the same texel and scale
 *                                      (texture coordinates and images do not move)
 * Checks: agpt_render_features_motion's in their order, then AGPT_ERR_INVALID for a NULL prev_normal_dev, for prev_normal_dev aliasing
 * another output, and for a scene whose shading generations are absent.
 * Limits: a triangle whose normals changed while its 36 position bytes did not stays w == 2 and is not followed. */
int agpt_render_features_surface_motion(agpt_scene*, const agpt_render_params* rp, float* albedo_dev, float* normal_depth_dev,
                                        float* prev_point_dev, float* prev_normal_dev);

/* agpt_temporal_accumulate_surface_motion: with clamp == NULL agpt_temporal_accumulate_motion's contract, otherwise
 * agpt_temporal_accumulate_clamped's with a non-NULL prev_point_cur_dev, and one change in step 4: for a pixel with prev_point_cur.w == 1
 * the normal compared with each tap's is prev_normal_cur[i].xyz (agpt_render_features_surface_motion's output for this frame, full
 * film) instead of normal_depth_cur[i].xyz.  A NaN there fails the >=: the tap is rejected.  The depth test, the first-frame rule and
 * everything else are unchanged; prev_normal_cur is read for w == 1 pixels only.  One launch.  Where every prev_normal_cur.xyz has the
 * bits of normal_depth_cur.xyz the outputs are the other two calls', bit for bit.
 * Checks (AGPT_ERR_INVALID): those of the call it extends in their order (with clamp, a NULL prev_point_cur_dev after the clamp
 * parameters), then a NULL prev_normal_cur_dev, then an output aliasing it. */
int agpt_temporal_accumulate_surface_motion(agpt_ctx*, const agpt_temporal_params*, const agpt_temporal_clamp_params* clamp /* may be NULL */,
        const float* accum_cur_dev, const float* moment2_cur_dev, const float* albedo_cur_dev, const float* normal_depth_cur_dev,
        const float* hist_accum_prev_dev, const float* hist_moment2_prev_dev, const float* albedo_prev_dev, const float* normal_depth_prev_dev,
        float* hist_accum_out_dev, float* hist_moment2_out_dev, const float* prev_point_cur_dev, const float* prev_normal_cur_dev);

/* Integrator::Li(const Ray&, const Scene&) (integrator.h:28-31) of PathTracer (integrator.h:120-191) for n rays of the caller --
 * the single-ray entry the reference's split-screen compare (myapp.cpp:168) and mouse picking (myapp.cpp:197-201) use, batched.
 * rays / rng_states / radiance3_out are HOST arrays.  rng_states[i] is the xorshift32 state the path's RandomFloat() calls start
 * from (template/template.cpp:667-675; the reference has one global state -- a host that wants one stream per ray derives them
 * as agpt_render does: WangHash((pixel + W*H*sample + 1)*17 + seed_base)); rng_states_out (may be NULL) receives the state after
 * the path.  radiance3_out[3i..3i+2] is Li's return value unfiltered (the NaN / inf reject belongs to the caller's loop,
 * myapp.cpp:169-172).  Ray::t = rays[i].tmax; the direction is normalised like Ray's ctor. */
int agpt_li_batch(agpt_scene*, const agpt_ray* rays, const uint32_t* rng_states, int n, int max_depth, float* radiance3_out,
                  uint32_t* rng_states_out, agpt_stats* stats);

/* DbgIntegrator::Li (integrator.h:107-118), the reference's debug view: (u, v, 0) / 5 of the closest hit's texture coordinates, red
 * where u or v is exactly 0, black on a miss.  Scene::Intersect runs on the GPU; the uv comes from the host copy of the scene
 * (the device keeps no texture coordinates).  rays / radiance3_out: HOST arrays of n rays and 3n floats. */
int agpt_dbg_li_batch(agpt_scene*, const agpt_ray* rays, int n, float* radiance3_out);

/* ---- multi-GPU (one process / context per GPU) -----------------------------------------------------------
 * The reference is single-process (myapp.cpp:163-175 is its whole frame loop); a multi-GPU host splits the film into
 * row blocks dealt round-robin to the ranks (agpt_render_params::interleave_*), every rank accumulates its blocks for
 * the whole sample budget into its compact buffer, and ONE exchange at resolve time brings the buffers to rank 0.
 * agpt_comm_unique_id: rank 0 fills a 128-byte id (ncclUniqueId) that the host passes to the other ranks by its own
 * means (MPI_Bcast, a file, an environment variable); agpt_comm_init: every rank, collectively (world == 1 needs no id
 * and never loads RCCL).  agpt_gather_tiles: every rank, collectively, enqueued on the context's stream -- grouped
 * RCCL send/recv of the compact buffers to rank 0 (each peer over its own direct xGMI link) followed, on rank 0, by the
 * de-interleave into the full accumulator full_accum_dev[height][width] float4 in Accumulator::pixels order (row
 * H-1-y, myapp.h:17-19); full_accum_dev is ignored on the other ranks. */
typedef struct agpt_comm agpt_comm;
int agpt_comm_unique_id(void* id128);
int agpt_comm_init(agpt_ctx*, const void* id128, int world, int rank, agpt_comm** out);
void agpt_comm_destroy(agpt_comm*);
int agpt_gather_tiles(agpt_comm*, const float* local_accum_dev, int width, int height, int block_rows, float* full_accum_dev);
/* The de-interleave step alone (no communication; enqueued on the context's stream): writes the rows of `rank`'s compact
 * buffer to their places in the full accumulator.  For hosts that move the buffers themselves (MPI, hipMemcpyPeer). */
int agpt_deinterleave_tiles(agpt_ctx*, const float* compact_dev, int width, int height, int block_rows, int world, int rank,
                            float* full_accum_dev);

/* Accumulator::CopyToSurface (myapp.h:34-41): lin2rgb(sum/samples) -> 0x00RRGGBB.  accum_dev DEVICE float4,
 * out_rgb HOST uint32[w*h] */
int agpt_resolve(agpt_ctx*, const float* accum_dev, int n_pixels, int samples, uint32_t* out_rgb);
/* CopyToSurface with the per-pixel count in accum.w (agpt_render_adaptive's buffers); a pixel with w == 0 resolves to 0 */
int agpt_resolve_counts(agpt_ctx*, const float* accum_dev, int n_pixels, uint32_t* out_rgb);

/* Host-only image writers (no GPU work) for headless use; the reference only blits to an OpenGL window
 * (myapp.cpp:177).  agpt_write_png: rgb = width*height 0x00RRGGBB words as agpt_resolve returns them, top row first
 * (Accumulator::CopyToSurface order).  agpt_write_pfm: accum_host = a HOST copy of the float4 accumulator (row 0 =
 * top image row, myapp.h:24); writes sum/samples as little-endian RGB float32, bottom row first. */
int agpt_write_png(const char* path, const uint32_t* rgb, int width, int height);
int agpt_write_pfm(const char* path, const float* accum_host, int width, int height, int samples);

/* Radiance RGBE (.hdr) reader, host only: what HDRTexture's constructor gets from stbi_loadf(filename, &w, &h, &n, 0)
 * (texture.h:41-52; the vendored stb_image v2.27, lib/stb_image.h:7005-7215) -- *rgb_out = width*height RGB float32, top row
 * first, malloc'ed, released with agpt_hdr_free; pass it to agpt_scene_add_infinite_area_light.  Anything that is not a
 * well-formed Radiance file fails with AGPT_ERR_INVALID (the reference goes on to stb's LDR decoders, or reads past the end). */
int agpt_hdr_load(const char* path, int* width_out, int* height_out, float** rgb_out);
int agpt_hdr_parse(const void* bytes, size_t length, int* width_out, int* height_out, float** rgb_out);
void agpt_hdr_free(float* rgb);

/* device memory helpers for hosts that do not bring their own allocator (tests, the C++ adapter) */
int agpt_device_alloc(agpt_ctx*, size_t bytes, void** out_dev);
int agpt_device_free(agpt_ctx*, void* dev);
int agpt_device_memset(agpt_ctx*, void* dev, int value, size_t bytes);
int agpt_device_download(agpt_ctx*, void* host_dst, const void* dev_src, size_t bytes);
int agpt_device_upload(agpt_ctx*, void* dev_dst, const void* host_src, size_t bytes);

/* known-answer entry points (each runs the device implementation of one hot-path function on one lane) */
/* BSDF::f + BSDF::Pdf (reflection.h:114-123,174-188) on the canonical frame ng = ns = +z, ss = +x.  There is no hit here: both
 * known-answer calls use the material's constant colour, whether or not it has a texture. */
int agpt_kat_bsdf_eval(agpt_scene*, int material, int n, const float* wo3, const float* wi3, float* f3_out, float* pdf_out);
/* BSDF::Sample_f (reflection.h:124-172) */
int agpt_kat_bsdf_sample(agpt_scene*, int material, int n, const float* wo3, const float* u2, float* wi3_out,
                         float* f3_out, float* pdf_out, int32_t* specular_out);
/* known-answer: the perturbation of agpt_scene_set_material_normal_texture alone, one lane per item (n items: ns3, ss3, rgb3 in,
 * ns_out3 out; HOST arrays) */
int agpt_kat_normal_map(agpt_ctx*, int n, const float* ns3, const float* ss3, const float* rgb3, float scale, float* ns_out3);
/* known-answer: the surface reconstruction of a mesh hit alone -- shading normal (ns3_out) and tangent (ss3_out) -- for n global
 * triangle ids and barycentrics (HOST arrays), from the scene's live shading records (generation -1) or from the newer (0) or the
 * older (1) generation of agpt_scene_snapshot_surfaces.  AGPT_ERR_INVALID for an id out of range or an absent generation. */
int agpt_kat_surface(agpt_scene*, int generation, int n, const uint32_t* tri_ids, const float* b1, const float* b2, float* ns3_out,
                     float* ss3_out);
/* RNG stream of a (pixel, sample): first n floats (template.cpp:667-675 + cl/tools.cl:1-2) */
int agpt_kat_rng(agpt_ctx*, uint32_t pixel, uint32_t wh, uint32_t sample, uint32_t seed_base, int n, float* out,
                 uint32_t* seed_out);
/* Distribution1D (sampling.h:19-69), the importance table of InfiniteAreaLight (lights.cpp:31-48): the ctor on the host
 * (cdf_out[n + 1], *func_int_out; either may be NULL) and SampleContinuous (:37-52, with FindInterval :4-17) on the device
 * for k draws u[k] -> x_out[k], pdf_out[k] */
int agpt_kat_distribution1d(agpt_ctx*, const float* func, int n, const float* u, int k, float* cdf_out, float* func_int_out,
                            float* x_out, float* pdf_out);
/* known-answer: the environment light's three device functions -- InfiniteAreaLight::Le, Pdf_Li and Sample_Li (lights.cpp:50-112), the
 * very functions the shading kernels call -- on the map of light `light` (an index into the scene's light list), one lane per item, in
 * the scene's shading arithmetic (agpt_scene_set_shading_arith).  HOST arrays.  n_dirs directions d3, taken as given (not normalized
 * first; finite and not of zero length): le3_out = Le, pdf_li_out = Pdf_Li.  n_draws draws u, each the one value Sample_Li takes from the
 * stream: wi3_out, pdf_out, sample_le3_out = the radiance it returns (Le of the normalized wi) and ok_out = 1, or zeros and ok_out = 0
 * where it samples nothing (a texel of weight zero).  Either count may be 0, with its arrays NULL.  AGPT_ERR_INVALID for a light that is
 * not an infinite-area light. */
int agpt_kat_env_light(agpt_scene*, int light, int n_dirs, const float* d3, float* le3_out, float* pdf_li_out, int n_draws, const float* u,
                       float* wi3_out, float* pdf_out, float* sample_le3_out, int32_t* ok_out);
/* known-answer: k_pack_palette, the kernel agpt_scene_pose_mesh_device runs, on n_joints (1 .. 65536) HOST matrices: uploads them, runs
 * it, downloads palette_out (agpt_skin_palette's floats) and status_out = the lowest joint with a non-finite entry, with a last row
 * that is not (0, 0, 0, 1), with a determinant of exactly 0 (0xFFFFFFFF: none).  Nothing is refused for its contents: the palette is
 * written whatever the status says. */
int agpt_kat_skin_palette(agpt_ctx*, const float* joints16, int n_joints, int with_normals, float* palette_out, uint32_t status_out[3]);
/* known-answer: k_morph_active, the kernel agpt_scene_morph_mesh_device runs, on n_targets (1 .. 4096) HOST weights: status_out =
 * (the number of pairs, the lowest target with a non-finite weight or 0xFFFFFFFF), targets_out / weights_out (room for n_targets) the
 * pairs -- agpt_morph_active's for finite weights. */
int agpt_kat_morph_active(agpt_ctx*, const float* weights, int n_targets, int32_t* targets_out, float* weights_out, uint32_t status_out[2]);

#ifdef __cplusplus
}
#endif
#endif
