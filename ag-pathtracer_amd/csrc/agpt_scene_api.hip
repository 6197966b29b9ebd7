// agpt_scene_api.hip -- the scene side of include/agpt.h: building a scene and committing it to the device (agpt_scene_commit), the
// host BVH and top-level entry points, the mesh-update state machine (agpt_scene_update_mesh and its two device-resident front ends)
// and agpt_dbg_li_batch, which is host arithmetic over agpt_intersect_batch.  Host code only: the kernels this unit's calls run are
// launched by agpt_bvh_device.hip and agpt_update.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "agpt_analytic.h"
#include "agpt_bvh_device.h"
#include "agpt_internal.h"
#include "agpt_normals.h"

using agpt::fail;

extern "C" {

// ---- scene building -----------------------------------------------------------------------------------------
int agpt_scene_create(agpt_ctx* c, agpt_scene** out) {
    if (!c || !out) return fail(AGPT_ERR_INVALID, "agpt_scene_create: NULL argument");
    agpt_scene* s = new agpt_scene();
    s->ctx = c;
    *out = s;
    return AGPT_OK;
}

void agpt_scene_destroy(agpt_scene* s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipDeviceSynchronize();
    delete s;
}

int agpt_scene_add_material(agpt_scene* s, int type, const float color[3], float roughness, float metallic) {
    if (!s || !color) return fail(AGPT_ERR_INVALID, "agpt_scene_add_material: NULL argument");
    if (type < AGPT_MAT_DISNEY || type > AGPT_MAT_DIFFUSE_ONLY) return fail(AGPT_ERR_INVALID, "unknown material type");
    s->materials.push_back(agpt::make_material(type, color, roughness, metallic));
    s->colors.push_back(make_float4(color[0], color[1], color[2], 0.f));
    s->material_texture.push_back(-1);
    s->material_param_slots.push_back(0u);
    s->material_normal_texture.push_back(-1);
    s->material_normal_scale.push_back(0.f);
    s->committed = false;
    return (int)s->materials.size() - 1;
}

// n packed xyz triples as v3
static void set_v3(std::vector<v3>& out, const float* xyz, int n) {
    out.resize(n);
    for (int i = 0; i < n; i++) out[i] = V3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}

// the Scene::primitives record of a mesh / sphere / plane just added; returns its primitive id
static int add_prim(agpt_scene* s, int type, int index, int material) {
    agpt::HostPrim p;
    p.type = type;
    p.index = index;
    p.material = material;
    p.arealight = -1;
    s->prims.push_back(p);
    s->committed = false;
    return (int)s->prims.size() - 1;
}

int agpt_scene_add_mesh(agpt_scene* s, const float* vertices, int n_vertices, const float* normals, int n_normals,
                        const float* texcoords, int n_texcoords, const int32_t* indices, int n_indices, int material,
                        int max_prims_in_node) {
    if (!s || !vertices || !indices) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: NULL argument");
    if (n_indices < 3 || n_indices % 3 != 0 || n_vertices <= 0)
        return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: need at least one triangle (the reference's BVH build does not terminate on an empty mesh)");
    if (material < -1 || material >= (int)s->materials.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: bad material id");
    for (int i = 0; i < n_indices; i++) {
        const int32_t* ix = indices + 3 * i;
        if (ix[0] < 0 || ix[0] >= n_vertices) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: vertex index out of range");
        if (n_normals > 0 && (ix[1] < 0 || ix[1] >= n_normals)) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: normal index out of range");
        if (n_texcoords > 0 && (ix[2] < 0 || ix[2] >= n_texcoords)) return fail(AGPT_ERR_INVALID, "agpt_scene_add_mesh: texcoord index out of range");
    }
    agpt::HostMesh m;
    set_v3(m.vertices, vertices, n_vertices);
    if (normals && n_normals > 0) set_v3(m.normals, normals, n_normals);
    if (texcoords && n_texcoords > 0) {
        m.texcoords.resize(n_texcoords);
        for (int i = 0; i < n_texcoords; i++) {
            m.texcoords[i].x = texcoords[2 * i];
            m.texcoords[i].y = texcoords[2 * i + 1];
        }
    }
    m.indices.assign(indices, indices + (size_t)3 * n_indices);
    m.material = material;
    if (s->bvh_builder == AGPT_BVH_BUILDER_DEVICE) {
        // same bytes as build_bvh (agpt_bvh_device.hip)
        HIP_TRY(hipSetDevice(s->ctx->device));
        const int n_tris = n_indices / 3;
        m.nodes.resize((size_t)2 * n_tris + 2);
        m.prim_index.resize(n_tris);
        int on_device = 0;
        const int rc = agpt::build_bvh_device(s->ctx->stream, vertices, n_vertices, indices, n_tris, max_prims_in_node, m.nodes.data(),
                                              m.prim_index.data(), &m.total_nodes, &m.max_depth, &on_device);
        if (rc != AGPT_OK) return rc;
        m.nodes.resize((size_t)m.total_nodes + 1);
        m.max_prims_in_node = max_prims_in_node;
    } else {
        agpt::build_bvh(m, max_prims_in_node);
    }
    s->meshes.push_back(std::move(m));
    s->updates.emplace_back();
    return add_prim(s, AGPT_PRIM_MESH, (int)s->meshes.size() - 1, material);
}

int agpt_scene_add_sphere(agpt_scene* s, const float center[3], float radius, int material) {
    if (!s || !center) return fail(AGPT_ERR_INVALID, "agpt_scene_add_sphere: NULL argument");
    if (material < -1 || material >= (int)s->materials.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_add_sphere: bad material id");
    const AnalyticRecord a = sphere_record(center[0], center[1], center[2], radius);
    agpt::HostSphere sp;
    sp.center = V3(a.cx, a.cy, a.cz);
    sp.r = a.r;
    sp.r2 = a.r2;
    s->spheres.push_back(sp);
    return add_prim(s, AGPT_PRIM_SPHERE, (int)s->spheres.size() - 1, material);
}

int agpt_scene_add_plane(agpt_scene* s, const float o[3], const float size[2], int material) {
    if (!s || !o || !size) return fail(AGPT_ERR_INVALID, "agpt_scene_add_plane: NULL argument");
    if (material < -1 || material >= (int)s->materials.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_add_plane: bad material id");
    agpt::HostSphere sp;  // reused record: center = O, r = HalfSize.x, r2 = HalfSize.y
    sp.center = V3(o[0], o[1], o[2]);
    sp.r = size[0] / 2;
    sp.r2 = size[1] / 2;
    s->spheres.push_back(sp);
    return add_prim(s, AGPT_PRIM_PLANE, (int)s->spheres.size() - 1, material);
}

int agpt_scene_add_area_light(agpt_scene* s, const float center[3], float radius, const float L[3]) {
    if (!s || !center || !L) return fail(AGPT_ERR_INVALID, "agpt_scene_add_area_light: NULL argument");
    int prim = agpt_scene_add_sphere(s, center, radius, -1);
    if (prim < 0) return prim;
    agpt::HostLight l;
    l.type = AGPT_LIGHT_AREA;
    l.shape = prim;
    l.L = V3(L[0], L[1], L[2]);
    s->lights.push_back(l);
    s->prims[prim].arealight = (int)s->lights.size() - 1;
    return prim;
}

int agpt_scene_add_uniform_infinite_light(agpt_scene* s, const float L[3]) {
    if (!s || !L) return fail(AGPT_ERR_INVALID, "agpt_scene_add_uniform_infinite_light: NULL argument");
    agpt::HostLight l;
    l.type = AGPT_LIGHT_UNIFORM_INFINITE;
    l.shape = -1;
    l.L = V3(L[0], L[1], L[2]);
    s->lights.push_back(l);
    s->committed = false;
    return (int)s->lights.size() - 1;
}

int agpt_scene_add_infinite_area_light(agpt_scene* s, const float* rgb, int width, int height) {
    if (!s || !rgb || width <= 0 || height <= 0 || (long long)width * height > (1ll << 28))
        return fail(AGPT_ERR_INVALID, "agpt_scene_add_infinite_area_light: bad argument");
    s->envs.push_back(agpt::make_env(rgb, width, height));
    agpt::HostLight l;
    l.type = AGPT_LIGHT_INFINITE_AREA;
    l.shape = -1;
    l.L = V3s(0.f);
    l.env = (int)s->envs.size() - 1;
    s->lights.push_back(l);
    s->committed = false;
    return (int)s->lights.size() - 1;
}

int agpt_scene_add_texture(agpt_scene* s, const float* rgb, int width, int height) {
    if (!s || !rgb) return fail(AGPT_ERR_INVALID, "agpt_scene_add_texture: NULL argument");
    if (width <= 0 || height <= 0 || (long long)width * height > (1ll << 28))
        return fail(AGPT_ERR_INVALID, "agpt_scene_add_texture: width and height must be positive (at most 2^28 texels)");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_add_texture: the scene is already committed");
    agpt_scene::HostTexture t;
    t.width = width;
    t.height = height;
    t.texels.resize((size_t)width * height);
    for (size_t i = 0; i < t.texels.size(); i++) t.texels[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.f);
    s->textures.push_back(std::move(t));
    return (int)s->textures.size() - 1;
}

int agpt_scene_set_material_texture(agpt_scene* s, int material, int texture) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_texture: scene is NULL");
    if (material < 0 || material >= (int)s->materials.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_texture: bad material id");
    if (texture < -1 || texture >= (int)s->textures.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_texture: bad texture id");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_texture: the scene is already committed");
    s->material_texture[material] = texture;
    return AGPT_OK;
}

static_assert(AGPT_PARAM_ROUGHNESS == 0 && AGPT_PARAM_METALLIC == 1, "param_slots_pack (agpt_scene.h) numbers the parameters like agpt.h");

int agpt_scene_set_material_param_texture(agpt_scene* s, int material, int param, int texture, int channel) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: scene is NULL");
    if (material < 0 || material >= (int)s->materials.size())
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: bad material id");
    if (param != AGPT_PARAM_ROUGHNESS && param != AGPT_PARAM_METALLIC)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: param is neither AGPT_PARAM_ROUGHNESS nor AGPT_PARAM_METALLIC");
    if (texture < -1 || texture >= (int)s->textures.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: bad texture id");
    if (texture >= 0 && (channel < 0 || channel > 2))
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: channel must be 0 (r), 1 (g) or 2 (b)");
    if (s->materials[material].type != AGPT_MAT_DISNEY)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: only AGPT_MAT_DISNEY materials have a roughness and a metallic weight");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_param_texture: the scene is already committed");
    if (texture > AGPT_PARAM_MAX_TEXTURE)
        return fail(AGPT_ERR_LIMIT, "agpt_scene_set_material_param_texture: a parameter map must be one of the scene's first " +
                                        std::to_string(AGPT_PARAM_MAX_TEXTURE + 1) + " textures");
    const uint32_t old = s->material_param_slots[material];
    int tex[2] = {param_slot_texture(old, 0), param_slot_texture(old, 1)};
    int ch[2] = {param_slot_channel(old, 0), param_slot_channel(old, 1)};
    tex[param] = texture;
    ch[param] = texture >= 0 ? channel : 0;
    s->material_param_slots[material] = param_slots_pack(tex[0], ch[0], tex[1], ch[1]);
    return AGPT_OK;
}

int agpt_scene_set_material_normal_texture(agpt_scene* s, int material, int texture, float scale) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: scene is NULL");
    if (material < 0 || material >= (int)s->materials.size())
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: bad material id");
    if (texture < -1 || texture >= (int)s->textures.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: bad texture id");
    if (texture >= 0 && !std::isfinite(scale)) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: scale is not finite");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_set_material_normal_texture: the scene is already committed");
    s->material_normal_texture[material] = texture;
    s->material_normal_scale[material] = texture >= 0 ? scale : 0.f;
    return AGPT_OK;
}

static_assert(AGPT_WRAP_REPEAT == (int)AGPT_TEXTURE_WRAP_REPEAT && AGPT_WRAP_CLAMP == (int)AGPT_TEXTURE_WRAP_CLAMP &&
                  AGPT_WRAP_MIRROR == (int)AGPT_TEXTURE_WRAP_MIRROR && AGPT_FILTER_NEAREST == 0 && AGPT_FILTER_BILINEAR == 1,
              "texture_size_pack (agpt_scene.h) numbers filters and wrap modes like agpt.h");

int agpt_scene_set_texture_sampler(agpt_scene* s, int texture, int filter, int wrap_u, int wrap_v) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: scene is NULL");
    if (texture < 0 || texture >= (int)s->textures.size()) return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: bad texture id");
    if (filter != AGPT_FILTER_NEAREST && filter != AGPT_FILTER_BILINEAR)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: filter is neither AGPT_FILTER_NEAREST nor AGPT_FILTER_BILINEAR");
    for (int wrap : {wrap_u, wrap_v})
        if (wrap != AGPT_WRAP_REPEAT && wrap != AGPT_WRAP_CLAMP && wrap != AGPT_WRAP_MIRROR)
            return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: a wrap mode is none of AGPT_WRAP_REPEAT, AGPT_WRAP_CLAMP, AGPT_WRAP_MIRROR");
    if (s->committed) return fail(AGPT_ERR_INVALID, "agpt_scene_set_texture_sampler: the scene is already committed");
    agpt_scene::HostTexture& t = s->textures[texture];
    t.filter = filter;
    t.wrap_u = wrap_u;
    t.wrap_v = wrap_v;
    return AGPT_OK;
}

int agpt_scene_set_camera(agpt_scene* s, const agpt_camera_desc* d) {
    if (!s || !d) return fail(AGPT_ERR_INVALID, "agpt_scene_set_camera: NULL argument");
    s->cam = agpt::make_camera(*d);
    s->has_camera = true;
    s->dev.cam = s->cam;
    return AGPT_OK;
}

// the bounds of the host copies of meshes that were refitted on the device (agpt_scene_update_mesh) and, with `arrays`, the positions
// and normals of those whose new arrays never existed on the host (agpt_scene_update_mesh_device, agpt_scene_transform_mesh); the
// spheres that agpt_scene_update_spheres_device moved
static int sync_mirror(agpt_scene* s, bool arrays) {
    if (const int rc = agpt::download_spheres(s)) return rc;
    for (size_t m = 0; m < s->updates.size(); m++) {
        agpt::MeshUpdate& up = s->updates[m];
        if (up.bounds_stale) {
            HIP_TRY(hipSetDevice(s->ctx->device));
            if (const int rc = up.download_bounds(s->ctx->stream, s->meshes[m])) return rc;
            up.bounds_stale = false;
        }
        if (arrays && up.arrays_stale) {
            HIP_TRY(hipSetDevice(s->ctx->device));
            if (const int rc = up.download_arrays(s->ctx->stream, s->meshes[m].vertices, s->meshes[m].normals)) return rc;
            up.arrays_stale = false;
        }
    }
    return AGPT_OK;
}

// DevScene::mdiv_coords_ok from the host's copies of the root boxes (kept current by commit and by refit_done).  A non-finite
// coordinate does not clear it: such a mesh is traced as before (the reference's own answer to a NaN vertex is a hit at t = NaN and,
// behind it, a path that an emitter re-casts for ever).
static int32_t mdiv_coords_ok(const agpt_scene* s) {
    auto outside = [](float x) { return std::isfinite(x) && !(std::fabs(x) < AGPT_MDIV_COORD_LIMIT); };
    for (const agpt::HostMesh& m : s->meshes) {
        if (m.nodes.empty()) continue;
        for (int a = 0; a < 3; a++)
            if (outside(m.nodes[0].bmin[a]) || outside(m.nodes[0].bmax[a])) return 0;
    }
    return 1;
}

int agpt_scene_commit(agpt_scene* s) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_commit: scene is NULL");
    if (const int rc = sync_mirror(s, true)) return rc;   // flatten_scene reads every mesh's arrays and boxes
    // The scene's texturing level: the highest one a material needs.  Every level's kernels are those of the level below plus one
    // thing (same uv records, same texture table), so the conditions below compare against it.
    bool has_texture = false, has_map = false, has_sampler = false, has_normal_map = false;
    for (size_t m = 0; m < s->material_texture.size(); m++) {
        has_texture = has_texture || s->material_texture[m] >= 0;
        has_map = has_map || s->material_param_slots[m] != 0;
        has_normal_map = has_normal_map || s->material_normal_texture[m] >= 0;
        // a texture that the material names -- in its colour slot or in a parameter slot -- has a sampler of its own
        for (int t : {(int)s->material_texture[m], param_slot_texture(s->material_param_slots[m], 0), param_slot_texture(s->material_param_slots[m], 1)})
            has_sampler = has_sampler || (t >= 0 && !s->textures[t].default_sampler());
    }
    const agpt::ShadeLevel level = has_normal_map ? agpt::SHADE_NORMAL : has_sampler ? agpt::SHADE_SAMPLED : has_map ? agpt::SHADE_MAPPED
                                   : has_texture  ? agpt::SHADE_TEXTURED : agpt::SHADE_PLAIN;
    const bool textured = level >= agpt::SHADE_TEXTURED;
    if (textured)
        for (const agpt::HostPrim& hp : s->prims)
            if (hp.type != AGPT_PRIM_MESH && hp.material >= 0 &&
                (s->material_texture[hp.material] >= 0 || s->material_param_slots[hp.material] != 0 || s->material_normal_texture[hp.material] >= 0))
                return fail(AGPT_ERR_INVALID, "agpt_scene_commit: a sphere or a plane has a material with a colour texture, a roughness / metallic map or a normal map "
                                              "(textures apply to triangle meshes only)");
    HIP_TRY(hipSetDevice(s->ctx->device));
    s->snapshots.drop();   // agpt_scene_snapshot_positions: the triangle ids may change meaning (update_on_host puts them back)
    agpt::FlatScene flat;
    flat.want_tri_uv = textured;
    agpt::flatten_scene(s->meshes, s->spheres, s->prims, flat);
    s->max_depth = flat.max_depth;
    if (flat.max_depth > AGPT_STACK_DEPTH_MAX)
        return fail(AGPT_ERR_LIMIT, "agpt_scene_commit: BVH depth " + std::to_string(flat.max_depth) +
                                        " exceeds the deepest traversal stack (" + std::to_string(AGPT_STACK_DEPTH_MAX) + ")");
    std::vector<DevLight> lights(s->lights.size());
    int n_inf = 0;
    for (size_t i = 0; i < lights.size(); i++) {
        lights[i].type = s->lights[i].type;
        lights[i].shape = s->lights[i].shape;
        lights[i].L[0] = s->lights[i].L.x;
        lights[i].L[1] = s->lights[i].L.y;
        lights[i].L[2] = s->lights[i].L.z;
        lights[i].env = s->lights[i].env;
        if (lights[i].type != AGPT_LIGHT_AREA) n_inf++;
    }
    hipStream_t st = s->ctx->stream;
    int rc;
    if ((rc = upload(s->d_nodes, flat.nodes, st))) return rc;
    if (flat.bigleaves.empty()) flat.bigleaves.assign(2, 0u);
    if ((rc = upload(s->d_bigleaves, flat.bigleaves, st))) return rc;
    if ((rc = upload(s->d_tri_verts, flat.tri_verts, st))) return rc;
    if ((rc = upload(s->d_tri_shade, flat.tri_shade, st))) return rc;
    if ((rc = upload(s->d_prefilter, flat.prefilter, st))) return rc;
    if ((rc = upload(s->d_toplevel, flat.toplevel16, st))) return rc;
    {
        std::vector<unsigned long long> mm(flat.mesh_masks, flat.mesh_masks + AGPT_MAX_CHUNKS);
        if ((rc = upload(s->d_chunk_mesh_masks, mm, st))) return rc;
    }
    if ((rc = upload(s->d_prims, flat.prims, st))) return rc;
    if ((rc = upload(s->d_materials, s->materials, st))) return rc;
    if ((rc = upload(s->d_colors, s->colors, st))) return rc;
    if ((rc = upload(s->d_lights, lights, st))) return rc;
    std::vector<DevEnv> envs(s->envs.size());
    s->d_env_pixels.resize(envs.size());
    s->d_env_func.resize(envs.size());
    s->d_env_cdf.resize(envs.size());
    for (size_t i = 0; i < envs.size(); i++) {
        const agpt::HostEnv& he = s->envs[i];
        if ((rc = upload(s->d_env_pixels[i], he.pixels, st))) return rc;
        if ((rc = upload(s->d_env_func[i], he.func, st))) return rc;
        if ((rc = upload(s->d_env_cdf[i], he.cdf, st))) return rc;
        envs[i].pixels = s->d_env_pixels[i].p;
        envs[i].func = s->d_env_func[i].p;
        envs[i].cdf = s->d_env_cdf[i].p;
        envs[i].width = he.width;
        envs[i].height = he.height;
        envs[i].n = he.width * he.height;
        envs[i].funcInt = he.funcInt;
    }
    if ((rc = upload(s->d_envs, envs, st))) return rc;
    // texture coordinates, texels and the tables are uploaded only for a scene that has a textured material
    std::vector<DevTexture> textures(textured ? s->textures.size() : 0);
    std::vector<std::vector<float4>> own_texels;   // (kept until the copies below have completed)
    if (textured) {
        // The device's material_texture table.  A material with a roughness / metallic map or a normal map and no colour texture gets a 1x1 texture of
        // its constant colour here (any uv reads that texel, and the texel has the constant's bits), so the MAPPED kernels have
        // one source for the colour; with maps the table's second half holds the packed slots (agpt_scene.h).
        std::vector<int32_t> table = s->material_texture;
        for (size_t m = 0; m < table.size(); m++)
            if ((s->material_param_slots[m] != 0 || s->material_normal_texture[m] >= 0) && table[m] < 0) {
                table[m] = (int32_t)(s->textures.size() + own_texels.size());
                own_texels.push_back(std::vector<float4>(1, s->colors[m]));
            }
        if (level >= agpt::SHADE_MAPPED)   // (the kernels above MAPPED read the slots too: all 0 in a scene without maps)
            table.insert(table.end(), s->material_param_slots.begin(), s->material_param_slots.end());
        textures.resize(s->textures.size() + own_texels.size());
        s->d_texels.resize(textures.size());
        for (size_t i = 0; i < textures.size(); i++) {
            const bool own = i >= s->textures.size();
            if ((rc = upload(s->d_texels[i], own ? own_texels[i - s->textures.size()] : s->textures[i].texels, st))) return rc;
            textures[i].texels = s->d_texels[i].p;
            textures[i].width = own ? 1 : s->textures[i].width;
            textures[i].height = own ? 1 : s->textures[i].height;
            if (level >= agpt::SHADE_SAMPLED && !own) {   // (only the kernels from SAMPLED up decode the size words, agpt_scene.h: DevTexture)
                textures[i].width = texture_size_pack(s->textures[i].width, s->textures[i].wrap_u, s->textures[i].filter);
                textures[i].height = texture_size_pack(s->textures[i].height, s->textures[i].wrap_v, 0);
            }
        }
        if (level == agpt::SHADE_NORMAL) {   // one DevNormalSlot per material behind the two halves (agpt_scene.h)
            static_assert(sizeof(DevNormalSlot) == 8 * sizeof(int32_t), "a normal slot is two 16-byte loads");
            const size_t off = (size_t)normal_slots_offset((int)s->materials.size());
            table.resize(off + 8 * s->materials.size(), 0);
            for (size_t m = 0; m < s->materials.size(); m++) {
                const int t = s->material_normal_texture[m];
                DevNormalSlot slot{};
                slot.tex = textures[t >= 0 ? t : 0];
                slot.scale = s->material_normal_scale[m];
                slot.texture = t;
                memcpy(&table[off + 8 * m], &slot, sizeof(slot));
            }
        }
        if ((rc = upload(s->d_tri_uv, flat.tri_uv, st))) return rc;
        if ((rc = upload(s->d_textures, textures, st))) return rc;
        if ((rc = upload(s->d_material_texture, table, st))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    s->shade_level = level;
    s->dev.tri_uv = textured ? s->d_tri_uv.p : nullptr;
    s->dev.textures = textured ? s->d_textures.p : nullptr;
    s->dev.material_texture = textured ? s->d_material_texture.p : nullptr;
    s->dev.envs = s->d_envs.p;
    s->dev.nodes = s->d_nodes.p;
    s->dev.bigleaves = s->d_bigleaves.p;
    s->dev.tri_verts = s->d_tri_verts.p;
    s->dev.tri_shade = s->d_tri_shade.p;
    s->dev.prims = s->d_prims.p;
    s->dev.materials = s->d_materials.p;
    s->dev.lights = s->d_lights.p;
    s->dev.n_prims = (int)flat.prims.size();
    s->dev.n_lights = (int)lights.size();
    s->dev.n_materials = (int)s->materials.size();
    s->dev.n_infinite = n_inf;
    s->dev.max_depth = flat.max_depth;
    s->dev.rootpair_base = flat.rootpair_base;
    for (int ch = 0; ch < AGPT_MAX_CHUNKS; ch++) s->dev.mesh_masks[ch] = flat.mesh_masks[ch];
    for (int ch = 0; ch < AGPT_MAX_CHUNKS; ch++) s->dev.analytic_masks[ch] = flat.analytic_masks[ch];
    for (int ch = 0; ch <= AGPT_MAX_CHUNKS; ch++) s->dev.pf_begin[ch] = flat.pf_begin[ch];
    s->dev.prefilter = s->d_prefilter.p;
    s->dev.toplevel = reinterpret_cast<const uint4*>(s->d_toplevel.p);
    s->dev.n_toplevel = flat.n_toplevel;
    s->dev.chunk_mesh_masks = s->d_chunk_mesh_masks.p;
    s->dev.n_meshes = 0;
    for (const DevPrim& dp : flat.prims)
        if (dp.type == AGPT_PRIM_MESH && dp.n_tris > 0) s->dev.n_meshes++;
    s->dev.cam = s->cam;
    s->dev.mdiv_coords_ok = mdiv_coords_ok(s);
    s->committed = true;
    return AGPT_OK;
}

static const agpt::HostMesh* mesh_of(const agpt_scene* s, int prim) {
    if (!s || prim < 0 || prim >= (int)s->prims.size() || s->prims[prim].type != AGPT_PRIM_MESH) return nullptr;
    return &s->meshes[s->prims[prim].index];
}
int agpt_mesh_num_nodes(const agpt_scene* s, int prim) {
    const agpt::HostMesh* m = mesh_of(s, prim);
    return m ? m->total_nodes : fail(AGPT_ERR_INVALID, "agpt_mesh_num_nodes: not a mesh primitive");
}
int agpt_mesh_num_prims(const agpt_scene* s, int prim) {
    const agpt::HostMesh* m = mesh_of(s, prim);
    return m ? (int)m->prim_index.size() : fail(AGPT_ERR_INVALID, "agpt_mesh_num_prims: not a mesh primitive");
}
int agpt_mesh_get_bvh(const agpt_scene* s, int prim, agpt_bvh_node* nodes_out, int32_t* prim_index_out) {
    const agpt::HostMesh* m = mesh_of(s, prim);
    if (!m) return fail(AGPT_ERR_INVALID, "agpt_mesh_get_bvh: not a mesh primitive");
    if (const int rc = sync_mirror(const_cast<agpt_scene*>(s), false)) return rc;   // (the boxes only)
    if (nodes_out) std::memcpy(nodes_out, m->nodes.data(), m->nodes.size() * sizeof(agpt_bvh_node));
    if (prim_index_out) std::memcpy(prim_index_out, m->prim_index.data(), m->prim_index.size() * sizeof(int32_t));
    return AGPT_OK;
}

// the mesh arguments of agpt_bvh_build / agpt_bvh_build_device (n_indices index triplets, as agpt_scene_add_mesh)
static int check_bvh_input(const char* fn, const float* vertices, int n_vertices, const int32_t* indices, int n_indices) {
    if (!vertices || !indices || n_vertices <= 0 || n_indices < 3 || n_indices % 3 != 0)
        return fail(AGPT_ERR_INVALID, std::string(fn) + ": need at least one triangle");
    for (int i = 0; i < n_indices; i++)
        if (indices[3 * i] < 0 || indices[3 * i] >= n_vertices) return fail(AGPT_ERR_INVALID, std::string(fn) + ": vertex index out of range");
    return AGPT_OK;
}

int agpt_bvh_build(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, int max_prims_in_node,
                   agpt_bvh_node* nodes_out, int32_t* prim_index_out, int* total_nodes_out, int* max_depth_out) {
    if (const int rc = check_bvh_input("agpt_bvh_build", vertices, n_vertices, indices, n_indices)) return rc;
    agpt::HostMesh m;
    set_v3(m.vertices, vertices, n_vertices);
    m.indices.assign(indices, indices + (size_t)3 * n_indices);
    agpt::build_bvh(m, max_prims_in_node);
    if (nodes_out) std::memcpy(nodes_out, m.nodes.data(), m.nodes.size() * sizeof(agpt_bvh_node));
    if (prim_index_out) std::memcpy(prim_index_out, m.prim_index.data(), m.prim_index.size() * sizeof(int32_t));
    if (total_nodes_out) *total_nodes_out = m.total_nodes;
    if (max_depth_out) *max_depth_out = m.max_depth;
    return AGPT_OK;
}

int agpt_bvh_refit(const float* vertices, int n_vertices, const int32_t* indices, int n_indices, const int32_t* prim_index,
                   agpt_bvh_node* nodes_inout, int total_nodes) {
    if (const int rc = check_bvh_input("agpt_bvh_refit", vertices, n_vertices, indices, n_indices)) return rc;
    const int n_tris = n_indices / 3;
    if (!prim_index || !nodes_inout || total_nodes < 1 || total_nodes > 2 * n_tris)
        return fail(AGPT_ERR_INVALID, "agpt_bvh_refit: NULL tree or a node count outside [1, 2 * triangles]");
    for (int t = 0; t < n_tris; t++)
        if (prim_index[t] < 0 || prim_index[t] % 3 != 0 || prim_index[t] / 3 >= n_tris) return fail(AGPT_ERR_INVALID, "agpt_bvh_refit: bad prim_index");
    std::vector<v3> v;
    set_v3(v, vertices, n_vertices);
    const std::vector<int32_t> ix(indices, indices + (size_t)3 * n_indices), order(prim_index, prim_index + n_tris);
    std::vector<agpt_bvh_node> nodes(nodes_inout, nodes_inout + total_nodes + 1);   // (a refused call changes nothing)
    if (!agpt::refit_bvh(v, ix, order, nodes.data(), total_nodes)) return fail(AGPT_ERR_INVALID, "agpt_bvh_refit: not a tree of agpt_bvh_build's");
    std::memcpy(nodes_inout, nodes.data(), nodes.size() * sizeof(agpt_bvh_node));
    return AGPT_OK;
}

// the top-level tree again (lists longer than 64 primitives): its topology depends on the root boxes (flatten_scene)
static int upload_toplevel(agpt_scene* s) {
    std::vector<float> boxes;
    std::vector<uint32_t> index;
    for (size_t pi = 0; pi < std::min<size_t>(s->prims.size(), 64 * (size_t)AGPT_MAX_CHUNKS); pi++)
        if (s->prims[pi].type == AGPT_PRIM_MESH) {
            const agpt_bvh_node& r = s->meshes[s->prims[pi].index].nodes[0];
            boxes.insert(boxes.end(), {r.bmin[0], r.bmin[1], r.bmin[2], r.bmax[0], r.bmax[1], r.bmax[2]});
            index.push_back((uint32_t)pi);
        }
    std::vector<float4> tree;
    std::vector<uint32_t> packed;
    agpt::build_skip_tree(boxes.data(), index.data(), (int)index.size(), tree);
    agpt::pack_skip_tree16(tree, packed);
    if (packed.size() > s->d_toplevel.n || (int32_t)(tree.size() / 2) != s->dev.n_toplevel)
        return fail(AGPT_ERR_DEVICE, "agpt_scene_update_mesh: the top-level tree changed size");
    HIP_TRY(hipMemcpyAsync(s->d_toplevel.p, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return AGPT_OK;
}

// the arrays an update call brings; the calls that bring none (transform, pose, morph) keep the mesh's own counts by construction
struct GivenArrays {
    const void* vertices;
    int n_vertices;
    const void* normals;
    int n_normals;
};

static bool smooth_normals(const agpt_scene* s, size_t mi) { return s->updates[mi].normals_mode == AGPT_NORMALS_SMOOTH; }

// the argument checks every update call shares, in agpt_scene_update_mesh's order (`fn` names the call in the message)
static int check_update(const char* fn, const agpt_scene* s, int prim, const GivenArrays* given, int mode) {
    const std::string f(fn);
    if (!s || (given && !given->vertices)) return fail(AGPT_ERR_INVALID, f + ": NULL scene or vertices");
    if (!s->committed) return fail(AGPT_ERR_INVALID, f + ": the scene is not committed");
    if (prim < 0 || prim >= (int)s->prims.size() || s->prims[prim].type != AGPT_PRIM_MESH)
        return fail(AGPT_ERR_INVALID, f + ": primitive " + std::to_string(prim) + " is not a mesh of this scene");
    const size_t mi = (size_t)s->prims[prim].index;
    const agpt::HostMesh& mesh = s->meshes[mi];
    if (given && (given->n_vertices != (int)mesh.vertices.size() || given->n_normals != (int)mesh.normals.size() ||
                  (!given->normals && !mesh.normals.empty() && !smooth_normals(s, mi))))   // (SMOOTH: its normals are never read)
        return fail(AGPT_ERR_INVALID, f + ": the mesh has " + std::to_string(mesh.vertices.size()) + " vertices and " +
                                          std::to_string(mesh.normals.size()) + " normals; both counts stay (normals may be NULL only without any)");
    if (mode != AGPT_UPDATE_REFIT && mode != AGPT_UPDATE_REBUILD) return fail(AGPT_ERR_INVALID, f + ": unknown mode " + std::to_string(mode));
    return AGPT_OK;
}

// Host orchestration of what exists, from host arrays: a new tree (REBUILD) or the host refit (a non-finite position under REFIT),
// then the full commit.  normals == NULL for a mesh in AGPT_NORMALS_SMOOTH mode: they are the twin's (agpt_normals.h), from the new
// positions.
static int update_on_host(agpt_scene* s, size_t mi, const float* vertices, const float* normals, int mode) {
    agpt::HostMesh& mesh = s->meshes[mi];
    const int n_vertices = (int)mesh.vertices.size(), n_normals = (int)mesh.normals.size();
    std::vector<float> twin;
    if (!normals && smooth_normals(s, mi)) {
        twin.resize(3 * mesh.normals.size());
        agpt::vertex_normals_host(vertices, mesh.indices.data(), mesh.indices.size() / 3, mesh.normals.size(), twin.data());
        normals = twin.data();
    }
    auto set_arrays = [&]() {
        set_v3(mesh.vertices, vertices, n_vertices);
        set_v3(mesh.normals, normals, n_normals);
    };
    if (mode == AGPT_UPDATE_REBUILD && s->bvh_builder == AGPT_BVH_BUILDER_DEVICE) {
        const int n_tris = (int)mesh.prim_index.size();
        std::vector<agpt_bvh_node> nodes((size_t)2 * n_tris + 2);
        std::vector<int32_t> order(n_tris);
        int total = 0, depth = 0, on_device = 0;
        const int rc = agpt::build_bvh_device(s->ctx->stream, vertices, n_vertices, mesh.indices.data(), n_tris, mesh.max_prims_in_node,
                                              nodes.data(), order.data(), &total, &depth, &on_device);
        if (rc != AGPT_OK) return rc;
        nodes.resize((size_t)total + 1);
        set_arrays();
        mesh.nodes.swap(nodes);
        mesh.prim_index.swap(order);
        mesh.total_nodes = total;
        mesh.max_depth = depth;
    } else if (mode == AGPT_UPDATE_REBUILD) {
        set_arrays();
        agpt::build_bvh(mesh, mesh.max_prims_in_node);
    } else {
        set_arrays();
        agpt::refit_bvh(mesh.vertices, mesh.indices, mesh.prim_index, mesh.nodes.data(), mesh.total_nodes);
    }
    agpt::MeshUpdate& up = s->updates[mi];
    up.bounds_stale = false;   // every box of this mesh has just been computed on the host,
    up.arrays_stale = false;   // from arrays that are now the mirror's
    if (mode == AGPT_UPDATE_REBUILD) up.topology_changed();   // the cache holds the old topology
    // the commit below leaves every triangle its global id (same meshes, same index arrays): the position snapshots stay valid
    agpt_scene::PositionSnapshots kept = std::move(s->snapshots);
    s->snapshots = agpt_scene::PositionSnapshots();
    const int rc = agpt_scene_commit(s);
    if (rc == AGPT_OK) s->snapshots = std::move(kept);
    return rc;
}

static int update_from_updater(agpt_scene* s, int prim, size_t mi, int mode);

// REFIT on the device: where flatten_scene put this mesh
static agpt::UpdateTarget update_target(const agpt_scene* s, int prim, size_t mi) {
    size_t node_base = 0, tri_base = 0;
    for (size_t m = 0; m < mi; m++) {
        node_base += (s->meshes[m].nodes.size() + 1) & ~size_t(1);
        tri_base += s->meshes[m].prim_index.size();
    }
    int ordinal = 0;   // its prefilter record: non-empty meshes before it in the list (every mesh has a triangle)
    for (int pi = 0; pi < prim; pi++) ordinal += s->prims[pi].type == AGPT_PRIM_MESH;
    const bool listed = prim < 64 * AGPT_MAX_CHUNKS;   // root pairs and prefilter records exist for these only
    agpt::UpdateTarget tg;
    tg.nodes = s->d_nodes.p;
    tg.tri_verts = s->d_tri_verts.p;
    tg.tri_shade = s->d_tri_shade.p;
    tg.prim = s->d_prims.p + prim;
    tg.rootpair = listed ? s->d_nodes.p + 4 * (((size_t)s->dev.rootpair_base + 2 * (size_t)prim) >> 1) : nullptr;
    tg.prefilter = listed ? s->d_prefilter.p + 2 * (size_t)ordinal : nullptr;
    tg.node_base = (uint32_t)node_base;
    tg.tri_base = (uint32_t)tri_base;
    tg.prim_id = (uint32_t)prim;
    return tg;
}

// the host's share of a device REFIT: the root box (the top-level tree is built from it) and what the mirror now lacks
static int refit_done(agpt_scene* s, size_t mi, const float root[6], bool arrays_on_device_only) {
    agpt::HostMesh& mesh = s->meshes[mi];
    std::memcpy(mesh.nodes[0].bmin, root, 12);
    std::memcpy(mesh.nodes[0].bmax, root + 3, 12);
    s->updates[mi].bounds_stale = true;
    s->updates[mi].arrays_stale = arrays_on_device_only;
    s->dev.mdiv_coords_ok = mdiv_coords_ok(s);
    if (s->prims.size() > 64) return upload_toplevel(s);
    return AGPT_OK;
}

int agpt_scene_update_mesh(agpt_scene* s, int prim, const float* vertices, int n_vertices, const float* normals, int n_normals, int mode) {
    const GivenArrays given{vertices, n_vertices, normals, n_normals};
    if (const int rc = check_update("agpt_scene_update_mesh", s, prim, &given, mode)) return rc;
    const size_t mi = (size_t)s->prims[prim].index;
    agpt::HostMesh& mesh = s->meshes[mi];
    agpt::MeshUpdate& up = s->updates[mi];
    HIP_TRY(hipSetDevice(s->ctx->device));
    up.arrays_given();
    bool finite = true;
    for (int i = 0; i < 3 * n_vertices && finite; i++) finite = std::isfinite(vertices[i]);
    const bool smooth = smooth_normals(s, mi);   // `normals` is not read
    if (mode == AGPT_UPDATE_REBUILD || !finite) return update_on_host(s, mi, vertices, smooth ? nullptr : normals, mode);
    if (smooth) {
        if (const int rc = up.upload_positions(s->ctx->stream, mesh, vertices)) return rc;
        return update_from_updater(s, prim, mi, mode);   // (synchronises with the stream: `vertices` lives until then)
    }
    float root[6];
    if (const int rc = up.update(s->ctx->stream, mesh, vertices, normals, update_target(s, prim, mi), root)) return rc;
    set_v3(mesh.vertices, vertices, n_vertices);
    set_v3(mesh.normals, normals, n_normals);
    return refit_done(s, mi, root, false);
}

// the new arrays are in the mesh's device cache (copied or deformed there): REFIT from them, or -- REBUILD, a non-finite position --
// bring them to the host and do what agpt_scene_update_mesh does with host arrays
static int update_from_updater(agpt_scene* s, int prim, size_t mi, int mode) {
    agpt::HostMesh& mesh = s->meshes[mi];
    agpt::MeshUpdate& up = s->updates[mi];
    const bool smooth = smooth_normals(s, mi);   // the front end left positions only: the normals are recomputed from them
    if (mode == AGPT_UPDATE_REFIT) {
        float root[6];
        bool finite = true;
        if (smooth)
            if (const int rc = up.smooth_normals(s->ctx->stream, mesh)) return rc;
        if (const int rc = up.refit(s->ctx->stream, mesh, update_target(s, prim, mi), root, &finite)) return rc;
        if (finite) return refit_done(s, mi, root, true);
    }
    std::vector<v3> v(mesh.vertices.size()), n(smooth ? 0 : mesh.normals.size());   // (smooth: not fetched, the host twin fills them)
    if (const int rc = up.download_arrays(s->ctx->stream, v, n)) return rc;
    return update_on_host(s, mi, &v.data()->x, n.empty() ? nullptr : &n.data()->x, mode);
}

int agpt_scene_update_mesh_device(agpt_scene* s, int prim, const float* vertices_dev, int n_vertices, const float* normals_dev, int n_normals,
                                  int mode) {
    const GivenArrays given{vertices_dev, n_vertices, normals_dev, n_normals};
    if (const int rc = check_update("agpt_scene_update_mesh_device", s, prim, &given, mode)) return rc;
    const size_t mi = (size_t)s->prims[prim].index;
    agpt::MeshUpdate& up = s->updates[mi];
    const bool smooth = smooth_normals(s, mi);   // `normals_dev` is not read
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (mode == AGPT_UPDATE_REBUILD) {   // the builders take host arrays
        std::vector<float> v((size_t)3 * n_vertices), n(smooth ? 0 : (size_t)3 * n_normals);
        HIP_TRY(hipMemcpyAsync(v.data(), vertices_dev, v.size() * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream));
        if (!n.empty()) HIP_TRY(hipMemcpyAsync(n.data(), normals_dev, n.size() * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream));
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        up.arrays_given();
        return update_on_host(s, mi, v.data(), n.empty() ? nullptr : n.data(), mode);
    }
    if (const int rc = up.copy_arrays(s->ctx->stream, s->meshes[mi], vertices_dev, smooth ? nullptr : normals_dev)) return rc;
    up.arrays_given();
    return update_from_updater(s, prim, mi, mode);
}

// What the status words of a device-pointer call refuse, in the host calls' order and words -- the weights first, then the joints: a
// non-finite entry, a last row, a determinant of 0, each naming the lowest offender -- or "" when they are clean.
static std::string device_refusal(const agpt::DeviceInputStatus& st) {
    if (st.nonfinite_weight != agpt::kNoItem) return "non-finite weight (target " + std::to_string(st.nonfinite_weight) + ")";
    if (st.nonfinite_joint != agpt::kNoItem) return "joint " + std::to_string(st.nonfinite_joint) + " has a non-finite entry";
    if (st.bad_row_joint != agpt::kNoItem) return "the last row of joint " + std::to_string(st.bad_row_joint) + " is not (0, 0, 0, 1)";
    if (st.singular_joint != agpt::kNoItem) return "joint " + std::to_string(st.singular_joint) + " is singular (its determinant is exactly 0)";
    return "";
}

// The tail the transform, the pose and the morph share.  The rest pose: the arrays the mesh last received explicitly -- the mirror,
// brought up to date if they came as device pointers.  Then the one launcher and the refit.  Synchronises with the stream: what the
// request points to lives until then.
// A request with device pointers (rq.status) starts with the front-end kernels and their status words, ahead of anything that touches
// the mesh: a refused call changes nothing.
static int deform_mesh(agpt_scene* s, int prim, int mode, agpt::DeformRequest rq) {
    const size_t mi = (size_t)s->prims[prim].index;
    agpt::MeshUpdate& up = s->updates[mi];
    HIP_TRY(hipSetDevice(s->ctx->device));
    rq.with_normals = !smooth_normals(s, mi);
    rq.num_cus = s->ctx->num_cus;
    if (rq.status) {
        if (const int rc = up.device_inputs(s->ctx->stream, s->meshes[mi], rq)) return rc;
        const std::string bad = device_refusal(*rq.status);
        if (!bad.empty()) return fail(AGPT_ERR_INVALID, std::string(rq.fn) + ": " + bad);
    }
    if (!up.has_rest()) {
        if (const int rc = sync_mirror(s, true)) return rc;
        up.rest_taken(s->meshes[mi].vertices, s->meshes[mi].normals);
    }
    if (const int rc = up.deform(s->ctx->stream, s->meshes[mi], rq)) return rc;
    return update_from_updater(s, prim, mi, mode);
}

int agpt_scene_transform_mesh(agpt_scene* s, int prim, const float* transform16, int mode) {
    if (const int rc = check_update("agpt_scene_transform_mesh", s, prim, nullptr, mode)) return rc;
    if (!transform16) return fail(AGPT_ERR_INVALID, "agpt_scene_transform_mesh: NULL matrix");
    agpt::Mat4 M;
    std::memcpy(M.c, transform16, sizeof(M.c));
    for (float c : M.c)
        if (!std::isfinite(c)) return fail(AGPT_ERR_INVALID, "agpt_scene_transform_mesh: the matrix has a non-finite entry");
    float det = 0;
    const agpt::Mat4 N = agpt::inverse_transpose(M, &det);
    if (det == 0) return fail(AGPT_ERR_INVALID, "agpt_scene_transform_mesh: the matrix is singular (its determinant is exactly 0)");
    agpt::DeformRequest rq{"agpt_scene_transform_mesh"};
    rq.M = &M;
    rq.N = &N;
    return deform_mesh(s, prim, mode, rq);
}

// the scene and the mesh primitive of a setter (`f` is the call's name and ": "): the mesh and its update state
static int setter_mesh(const std::string& f, agpt_scene* s, int prim, const agpt::HostMesh** m, agpt::MeshUpdate** up) {
    if (!s) return fail(AGPT_ERR_INVALID, f + "NULL scene");
    *m = mesh_of(s, prim);
    if (!*m) return fail(AGPT_ERR_INVALID, f + "primitive " + std::to_string(prim) + " is not a mesh of this scene");
    *up = &s->updates[(size_t)s->prims[prim].index];
    return AGPT_OK;
}

int agpt_scene_set_mesh_skin(agpt_scene* s, int prim, int influences, int n_joints, const int32_t* vertex_joints, const float* vertex_weights,
                             const int32_t* normal_joints, const float* normal_weights) {
    const std::string f = "agpt_scene_set_mesh_skin: ";
    const agpt::HostMesh* m;
    agpt::MeshUpdate* up;
    if (const int rc = setter_mesh(f, s, prim, &m, &up)) return rc;
    agpt::SkinBinding skin;
    if (influences != 0) {   // the twin's rules, with the mesh's own counts
        const size_t nv = m->vertices.size(), nn = m->normals.size();
        std::string bad = agpt::skin_check_counts(influences, n_joints);
        if (!bad.empty()) return fail(AGPT_ERR_INVALID, f + bad);
        if (!vertex_joints || !vertex_weights) return fail(AGPT_ERR_INVALID, f + "NULL vertex_joints or vertex_weights");
        const bool own = nn && normal_joints && normal_weights;
        if (nn && !own && ((normal_joints || normal_weights) || nn != nv))
            return fail(AGPT_ERR_INVALID, f + "normal_joints and normal_weights may be NULL (both) only when the mesh has as many normals as vertices; it has " +
                                              std::to_string(nv) + " vertices and " + std::to_string(nn) + " normals");
        bad = agpt::skin_check_influences("vertex", influences, n_joints, nv, vertex_joints, vertex_weights);
        if (bad.empty() && own) bad = agpt::skin_check_influences("normal", influences, n_joints, nn, normal_joints, normal_weights);
        if (!bad.empty()) return fail(AGPT_ERR_INVALID, f + bad);
        skin.influences = influences;
        skin.n_joints = n_joints;
        skin.vertex_joints.assign(vertex_joints, vertex_joints + nv * (size_t)influences);
        skin.vertex_weights.assign(vertex_weights, vertex_weights + nv * (size_t)influences);
        if (own) {
            skin.normal_joints.assign(normal_joints, normal_joints + nn * (size_t)influences);
            skin.normal_weights.assign(normal_weights, normal_weights + nn * (size_t)influences);
        }
    }
    if (up->on_device()) HIP_TRY(hipSetDevice(s->ctx->device));
    up->skin_changed(std::move(skin));
    return AGPT_OK;
}

// the checks of a frame's joint matrices that need no look at them, shared by the host and the device-pointer calls: the refusal's
// message, or ""
static std::string pose_args(const agpt_scene* s, int prim, const float* joints16, int n_joints) {
    const agpt::SkinBinding& skin = s->updates[(size_t)s->prims[prim].index].skin();
    if (skin.influences == 0) return "primitive " + std::to_string(prim) + " has no skin (agpt_scene_set_mesh_skin)";
    if (!joints16) return "NULL joints16";
    if (n_joints != skin.n_joints) return "n_joints is " + std::to_string(n_joints) + ", the skin was set with " + std::to_string(skin.n_joints);
    return "";
}

// the checks of a frame's joint matrices that agpt_scene_pose_mesh and agpt_scene_morph_mesh share, in their order, then the palette
// (`f` is the call's name and ": "; for a mesh in AGPT_NORMALS_SMOOTH mode, as for one without normals, the palette carries M only)
static int pose_palette(const std::string& f, const agpt_scene* s, int prim, const float* joints16, int n_joints, std::vector<float>& palette) {
    const size_t mi = (size_t)s->prims[prim].index;
    const std::string args = pose_args(s, prim, joints16, n_joints);
    if (!args.empty()) return fail(AGPT_ERR_INVALID, f + args);
    for (size_t i = 0; i < 16 * (size_t)n_joints; i++)
        if (!std::isfinite(joints16[i])) return fail(AGPT_ERR_INVALID, f + "joint " + std::to_string(i / 16) + " has a non-finite entry");
    const std::string bad = agpt::skin_check_last_rows(joints16, n_joints);
    if (!bad.empty()) return fail(AGPT_ERR_INVALID, f + bad);
    int singular = -1;
    palette = agpt::skin_pack_palette(joints16, n_joints, !s->meshes[mi].normals.empty() && !smooth_normals(s, mi), &singular);
    if (singular >= 0) return fail(AGPT_ERR_INVALID, f + "joint " + std::to_string(singular) + " is singular (its determinant is exactly 0)");
    return AGPT_OK;
}

int agpt_scene_pose_mesh(agpt_scene* s, int prim, const float* joints16, int n_joints, int mode) {
    if (const int rc = check_update("agpt_scene_pose_mesh", s, prim, nullptr, mode)) return rc;
    std::vector<float> palette;
    if (const int rc = pose_palette("agpt_scene_pose_mesh: ", s, prim, joints16, n_joints, palette)) return rc;
    agpt::DeformRequest rq{"agpt_scene_pose_mesh"};
    rq.palette = &palette;
    return deform_mesh(s, prim, mode, rq);
}

int agpt_scene_pose_mesh_device(agpt_scene* s, int prim, const float* joints16_dev, int n_joints, int mode) {
    const std::string f = "agpt_scene_pose_mesh_device: ";
    if (const int rc = check_update("agpt_scene_pose_mesh_device", s, prim, nullptr, mode)) return rc;
    const std::string args = pose_args(s, prim, joints16_dev, n_joints);
    if (!args.empty()) return fail(AGPT_ERR_INVALID, f + args);
    if (((uintptr_t)joints16_dev & 15) != 0) return fail(AGPT_ERR_INVALID, f + "joints16_dev is not 16-byte aligned");
    agpt::DeviceInputStatus status;
    agpt::DeformRequest rq{"agpt_scene_pose_mesh_device"};
    rq.joints16_dev = joints16_dev;
    rq.n_joints = n_joints;
    rq.status = &status;
    return deform_mesh(s, prim, mode, rq);   // (the matrices' own checks are k_pack_palette's)
}

int agpt_scene_set_mesh_morph_targets(agpt_scene* s, int prim, int n_targets, const float* position_deltas, const float* normal_deltas) {
    const std::string f = "agpt_scene_set_mesh_morph_targets: ";
    const agpt::HostMesh* m;
    agpt::MeshUpdate* up;
    if (const int rc = setter_mesh(f, s, prim, &m, &up)) return rc;
    agpt::MorphTargets morph;
    if (n_targets != 0) {   // the twin's rules, with the mesh's own counts
        const size_t nv = m->vertices.size(), nn = m->normals.size(), T = (size_t)n_targets;
        std::string bad = agpt::morph_check_count(n_targets);
        if (!bad.empty()) return fail(AGPT_ERR_INVALID, f + bad);
        if (!position_deltas) return fail(AGPT_ERR_INVALID, f + "NULL position_deltas");
        bad = agpt::morph_check_deltas("position", "vertex", n_targets, nv, position_deltas);
        if (bad.empty() && normal_deltas) bad = agpt::morph_check_deltas("normal", "normal", n_targets, nn, normal_deltas);
        if (!bad.empty()) return fail(AGPT_ERR_INVALID, f + bad);
        morph.n_targets = n_targets;
        morph.position_deltas.assign(position_deltas, position_deltas + T * nv * 3);
        if (normal_deltas) morph.normal_deltas.assign(normal_deltas, normal_deltas + T * nn * 3);   // (nothing for a mesh without normals)
    }
    if (up->on_device()) HIP_TRY(hipSetDevice(s->ctx->device));
    up->morph_changed(std::move(morph));
    return AGPT_OK;
}

int agpt_scene_morph_mesh(agpt_scene* s, int prim, const float* weights, int n_targets, const float* joints16, int n_joints, int mode) {
    const std::string f = "agpt_scene_morph_mesh: ";
    if (const int rc = check_update("agpt_scene_morph_mesh", s, prim, nullptr, mode)) return rc;
    const int bound = s->updates[(size_t)s->prims[prim].index].morph().n_targets;
    if (bound == 0) return fail(AGPT_ERR_INVALID, f + "primitive " + std::to_string(prim) + " has no morph targets (agpt_scene_set_mesh_morph_targets)");
    if (!weights) return fail(AGPT_ERR_INVALID, f + "NULL weights");
    if (n_targets != bound)
        return fail(AGPT_ERR_INVALID, f + "n_targets is " + std::to_string(n_targets) + ", the targets were set with " + std::to_string(bound));
    const std::string bad = agpt::morph_check_weights(weights, n_targets);
    if (!bad.empty()) return fail(AGPT_ERR_INVALID, f + bad);
    std::vector<float> palette;
    if (joints16)   // morph, then skin: agpt_scene_pose_mesh's checks
        if (const int rc = pose_palette(f, s, prim, joints16, n_joints, palette)) return rc;
    const std::vector<agpt::MorphActive> active = agpt::morph_active_list(weights, n_targets);
    agpt::DeformRequest rq{"agpt_scene_morph_mesh"};
    rq.active = &active;
    if (joints16) rq.palette = &palette;
    return deform_mesh(s, prim, mode, rq);
}

int agpt_scene_morph_mesh_device(agpt_scene* s, int prim, const float* weights_dev, int n_targets, const float* joints16_dev, int n_joints, int mode) {
    const std::string f = "agpt_scene_morph_mesh_device: ";
    if (const int rc = check_update("agpt_scene_morph_mesh_device", s, prim, nullptr, mode)) return rc;
    const size_t mi = (size_t)s->prims[prim].index;
    const int bound = s->updates[mi].morph().n_targets;
    if (bound == 0) return fail(AGPT_ERR_INVALID, f + "primitive " + std::to_string(prim) + " has no morph targets (agpt_scene_set_mesh_morph_targets)");
    if (!weights_dev) return fail(AGPT_ERR_INVALID, f + "NULL weights");
    if (n_targets != bound)
        return fail(AGPT_ERR_INVALID, f + "n_targets is " + std::to_string(n_targets) + ", the targets were set with " + std::to_string(bound));
    if (((uintptr_t)weights_dev & 3) != 0) return fail(AGPT_ERR_INVALID, f + "weights_dev is not 4-byte aligned");
    agpt::DeviceInputStatus status;
    agpt::DeformRequest rq{"agpt_scene_morph_mesh_device"};
    rq.weights_dev = weights_dev;
    rq.n_targets = n_targets;
    rq.status = &status;
    std::string args = joints16_dev ? pose_args(s, prim, joints16_dev, n_joints) : "";
    if (args.empty() && joints16_dev && ((uintptr_t)joints16_dev & 15) != 0) args = "joints16_dev is not 16-byte aligned";
    if (!args.empty()) {   // the host call looks at the weights before it looks at the skin: k_morph_active alone, then this refusal
        HIP_TRY(hipSetDevice(s->ctx->device));
        if (const int rc = s->updates[mi].device_inputs(s->ctx->stream, s->meshes[mi], rq)) return rc;
        const std::string weights = device_refusal(status);
        return fail(AGPT_ERR_INVALID, f + (weights.empty() ? args : weights));
    }
    if (joints16_dev) {
        rq.joints16_dev = joints16_dev;
        rq.n_joints = n_joints;
    }
    return deform_mesh(s, prim, mode, rq);
}

int agpt_scene_set_mesh_normals_mode(agpt_scene* s, int prim, int mode) {
    const std::string f = "agpt_scene_set_mesh_normals_mode: ";
    const agpt::HostMesh* m;
    agpt::MeshUpdate* up;
    if (const int rc = setter_mesh(f, s, prim, &m, &up)) return rc;
    if (mode != AGPT_NORMALS_GIVEN && mode != AGPT_NORMALS_SMOOTH) return fail(AGPT_ERR_INVALID, f + "unknown mode " + std::to_string(mode));
    if (mode == AGPT_NORMALS_SMOOTH && m->normals.empty())
        return fail(AGPT_ERR_INVALID, f + "primitive " + std::to_string(prim) + " has no normals (the counts of a mesh cannot change)");
    up->normals_mode = mode;
    return AGPT_OK;
}

int agpt_scene_set_bvh_builder(agpt_scene* s, int builder) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_bvh_builder: NULL scene");
    if (builder != AGPT_BVH_BUILDER_HOST && builder != AGPT_BVH_BUILDER_DEVICE)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_bvh_builder: unknown builder " + std::to_string(builder));
    s->bvh_builder = builder;
    return AGPT_OK;
}

int agpt_scene_set_shading_arith(agpt_scene* s, int mode) {
    if (!s) return fail(AGPT_ERR_INVALID, "agpt_scene_set_shading_arith: NULL scene");
    if (mode != AGPT_SHADING_EXACT && mode != AGPT_SHADING_FAST)
        return fail(AGPT_ERR_INVALID, "agpt_scene_set_shading_arith: unknown mode " + std::to_string(mode));
    s->shading_arith = mode;
    return AGPT_OK;
}

int agpt_bvh_build_device(agpt_ctx* c, const float* vertices, int n_vertices, const int32_t* indices, int n_indices,
                          int max_prims_in_node, agpt_bvh_node* nodes_out, int32_t* prim_index_out, int* total_nodes_out,
                          int* max_depth_out, int* on_device_out) {
    if (!c) return fail(AGPT_ERR_INVALID, "agpt_bvh_build_device: NULL context");
    if (const int rc = check_bvh_input("agpt_bvh_build_device", vertices, n_vertices, indices, n_indices)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int total = 0, depth = 0, on_device = 0;
    const int rc = agpt::build_bvh_device(c->stream, vertices, n_vertices, indices, n_indices / 3, max_prims_in_node, nodes_out,
                                          prim_index_out, &total, &depth, &on_device);
    if (rc != AGPT_OK) return rc;
    if (total_nodes_out) *total_nodes_out = total;
    if (max_depth_out) *max_depth_out = depth;
    if (on_device_out) *on_device_out = on_device;
    return AGPT_OK;
}

int agpt_toplevel_build(const float* boxes6, int n, float* nodes8_out) {
    if (!boxes6 || !nodes8_out || n < 1) return fail(AGPT_ERR_INVALID, "agpt_toplevel_build: need at least one box");
    std::vector<uint32_t> payload((size_t)n);
    for (int k = 0; k < n; k++) payload[k] = (uint32_t)k;
    std::vector<float4> nodes;
    agpt::build_skip_tree(boxes6, payload.data(), n, nodes);
    std::memcpy(nodes8_out, nodes.data(), nodes.size() * sizeof(float4));
    return (int)(nodes.size() / 2);
}

int agpt_toplevel_pack16(const float* nodes8, int n_nodes, uint32_t* packed4_out) {
    if (!nodes8 || !packed4_out || n_nodes < 1) return fail(AGPT_ERR_INVALID, "agpt_toplevel_pack16: need at least one node");
    std::vector<float4> nodes((size_t)2 * n_nodes);
    std::memcpy(nodes.data(), nodes8, nodes.size() * sizeof(float4));
    std::vector<uint32_t> packed;
    agpt::pack_skip_tree16(nodes, packed);
    std::memcpy(packed4_out, packed.data(), packed.size() * sizeof(uint32_t));
    return n_nodes;
}

int agpt_create_backdrop(const float origin[3], const float size[3], float radius, int steps, float* vertices, float* normals,
                         float* texcoords, int32_t* indices, int* n_vertices, int* n_indices) {
    if (!origin || !size || !vertices || !normals || !texcoords || !indices || steps < 1)
        return fail(AGPT_ERR_INVALID, "agpt_create_backdrop: bad argument");
    std::vector<v3> v, n;
    std::vector<v2> t;
    std::vector<int32_t> ix;
    agpt::create_backdrop(V3(origin[0], origin[1], origin[2]), V3(size[0], size[1], size[2]), radius, steps, v, n, t, ix);
    for (size_t i = 0; i < v.size(); i++) {
        vertices[3 * i] = v[i].x; vertices[3 * i + 1] = v[i].y; vertices[3 * i + 2] = v[i].z;
        normals[3 * i] = n[i].x; normals[3 * i + 1] = n[i].y; normals[3 * i + 2] = n[i].z;
        texcoords[2 * i] = t[i].x; texcoords[2 * i + 1] = t[i].y;
    }
    std::memcpy(indices, ix.data(), ix.size() * sizeof(int32_t));
    if (n_vertices) *n_vertices = (int)v.size();
    if (n_indices) *n_indices = (int)ix.size() / 3;
    return AGPT_OK;
}

// DbgIntegrator::Li (integrator.h:107-118): Scene::Intersect on the GPU, then the hit's uv -- which only this debug view reads, so
// the device keeps no texture coordinates -- from the host copy of the scene in the arithmetic of trianglemesh.cpp:46-57,
// intersectable.h:133 and :187-201.
int agpt_dbg_li_batch(agpt_scene* s, const agpt_ray* rays, int n, float* radiance3_out) {
    if (!s || !rays || !radiance3_out || n < 0) return fail(AGPT_ERR_INVALID, "agpt_dbg_li_batch: bad argument");
    if (n == 0) return AGPT_OK;
    std::vector<agpt_hit> hits((size_t)n);
    int rc = agpt_intersect_batch(s, rays, n, hits.data(), 0, nullptr);
    if (rc) return rc;
    if ((rc = sync_mirror(s, false))) return rc;   // (the spheres: the uv below is computed from the host copy)
    for (int i = 0; i < n; ++i) {
        float* L = radiance3_out + 3 * (size_t)i;
        L[0] = L[1] = L[2] = 0.f;
        const agpt_hit& h = hits[i];
        if (!h.hit) continue;
        const agpt::HostPrim& hp = s->prims[h.prim];
        float u, v;
        if (hp.type == AGPT_PRIM_MESH) {
            const agpt::HostMesh& m = s->meshes[hp.index];
            float uv[3][2] = {{0, 0}, {1, 0}, {1, 1}};   // a mesh without texture coordinates (trianglemesh.cpp:52-56)
            if (!m.texcoords.empty())
                for (int k = 0; k < 3; ++k) {
                    const v2 t = m.texcoords[m.indices[3 * (h.tri + k) + 2]];
                    uv[k][0] = t.x;
                    uv[k][1] = t.y;
                }
            const float b0 = 1.f - h.b1 - h.b2;
            u = uv[0][0] * b0 + uv[1][0] * h.b1 + uv[2][0] * h.b2;
            v = uv[0][1] * b0 + uv[1][1] * h.b1 + uv[2][1] * h.b2;
        } else {
            const agpt::HostSphere& sp = s->spheres[hp.index];
            const v3 D = normalize(V3(rays[i].d[0], rays[i].d[1], rays[i].d[2]));   // the Ray ctor's (camera.h:6), as k_prepare_rays
            const v3 P = V3(rays[i].o[0], rays[i].o[1], rays[i].o[2]) + h.t * D;
            if (hp.type == AGPT_PRIM_PLANE) {   // centre = O, r / r2 = HalfSize.x / .y
                u = ((P.x - sp.center.x) / sp.r + 1) * .5f;
                v = ((P.z - sp.center.z) / sp.r2 + 1) * .5f;
            } else {
                v3 pHit = P - sp.center;
                if (pHit.x == 0 && pHit.y == 0) pHit.x = AGPT_EPSILON * sp.r;
                float phi = cr_atan2f(pHit.y, pHit.x);
                if (phi < 0) phi += AGPT_TWOPI;
                u = phi * AGPT_INV2PI;
                v = cr_acosf(tclampf(pHit.z / sp.r, -1.f, 1.f)) * AGPT_INVPI;
            }
        }
        if (u == 0 || v == 0) {
            L[0] = 1.f;
        } else {
            L[0] = u / 5;
            L[1] = v / 5;
        }
    }
    return AGPT_OK;
}

int agpt_camera_vectors(const agpt_camera_desc* d, float out22[22]) {
    if (!d || !out22) return fail(AGPT_ERR_INVALID, "agpt_camera_vectors: NULL argument");
    const DevCamera cam = agpt::make_camera(*d);
    static_assert(sizeof(DevCamera) == 22 * sizeof(float), "origin, u, v, w, lower_left_corner, horizontal, vertical, lens_radius");
    std::memcpy(out22, &cam, sizeof(cam));
    return AGPT_OK;
}

}  // extern "C"
