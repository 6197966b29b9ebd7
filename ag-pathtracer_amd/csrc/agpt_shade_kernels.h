// agpt_shade_kernels.h -- the shading kernels of the wavefront path tracer (see agpt_kernels.h for the iteration they are part
// of): k_shade = PathTracer::Li's loop body (integrator.h:132-188) for every live path, and the kernels that consume a finished batch
// (k_accumulate, k_export_li; k_resolve_pending for the one consumer that lives elsewhere), which add an ended path's last light sample
// in this unit's arithmetic.
// Compiled as their own translation unit (agpt_shade_kernels.hip) with MachineLICM off: the pass hoists the materialisation of
// every fp64 polynomial coefficient of the trigonometry (two v_mov each) out of the path loop and keeps the pairs in registers
// for the whole kernel -- 168 registers and 7-14 spilled, against 134 and none without it, which is what lets the kernel be
// held to four waves per SIMD (128 registers, 2 spilled).
#pragma once

#include "agpt_shade.h"
#include "agpt_trace.h"   // TraceRay + sphere_test_c: MIS queries answered without a traversal
#include "agpt_wavefront.h"

// The texturing levels (AGPT_SHADE_LEVEL here, agpt::ShadeLevel on the host).  Each level is the one below plus one thing, and is
// compiled as a unit of its own per arithmetic (agpt_shade_kernels<suffix>.hip, agpt_shade_kernels<suffix>_fast.hip), so adding a level
// leaves the code of the units below it alone.  agpt_scene_commit gives a scene the highest level that one of its materials needs.
//   level       adds, at a mesh hit                                                     kernel              selected by
//   0 PLAIN     --                                                                      k_shade             (a scene without textures)
//   1 TEXTURED  the material's colour comes from its image texture                      k_shade_textured    agpt_scene_set_material_texture
//               (agpt_scene.h: tri_uv, textures, material_texture)
//   2 MAPPED    roughness and metallic come from image textures too (param_slots_pack), k_shade_mapped      agpt_scene_set_material_param_texture
//               so the whole Disney constructor runs per hit
//   3 SAMPLED   the lookups honour each texture's sampler (DevTexture: bilinear         k_shade_sampled     agpt_scene_set_texture_sampler, non-default,
//               filtering, clamp and mirror wrap), colour slot and both maps alike                          on a texture that a material names
//   4 NORMAL    the normal-map slot (DevNormalSlot; agpt_shade.h:                       k_shade_normal      agpt_scene_set_material_normal_texture
//               surface_apply_normal_map), its taps in the other slots' round trip
// One row per level: (level, suffix of the unit's file, kernels and launcher).
#define AGPT_SHADE_LEVEL_LIST(X) X(0, ) X(1, _textured) X(2, _mapped) X(3, _sampled) X(4, _normal)
#ifndef AGPT_SHADE_LEVEL
#define AGPT_SHADE_LEVEL 0
#endif
// A unit's kernels and launchers are named name + its level's suffix + _fast for a unit compiled with AGPT_SHADE_FAST 1
// (agpt_shade_arith.h): the host-side stubs of two units would otherwise collide at link time.
#if AGPT_SHADE_FAST
#define AGPT_SHADE_FAST_SUFFIX _fast
#else
#define AGPT_SHADE_FAST_SUFFIX
#endif
#define AGPT_SHADE_NTH_0(s0, ...) s0
#define AGPT_SHADE_NTH_1(s0, s1, ...) s1
#define AGPT_SHADE_NTH_2(s0, s1, s2, ...) s2
#define AGPT_SHADE_NTH_3(s0, s1, s2, s3, ...) s3
#define AGPT_SHADE_NTH_4(s0, s1, s2, s3, s4, ...) s4
#define AGPT_SHADE_SUFFIX_ARG(level, suffix) suffix,
#define AGPT_SHADE_CAT_(a, b, c) a##b##c
#define AGPT_SHADE_CAT(a, b, c) AGPT_SHADE_CAT_(a, b, c)
#define AGPT_SHADE_NTH(n, list) AGPT_SHADE_CAT(AGPT_SHADE_NTH_, n, )(list)   // (the list's commas separate arguments only on this rescan)
#define AGPT_SHADE_KNAME(n) AGPT_SHADE_CAT(n, AGPT_SHADE_NTH(AGPT_SHADE_LEVEL, AGPT_SHADE_LEVEL_LIST(AGPT_SHADE_SUFFIX_ARG)), AGPT_SHADE_FAST_SUFFIX)

// ---------------------------------------------------------------------------------------------------------
// PathTracer::Li's loop body (integrator.h:132-188) in wavefront form, for one path.  Returns which of the next
// iteration's queues the path goes to.
#define SB_EXT 1u
#define SB_MIS 2u
#define SB_SHADOW 4u          // (bits 0..2 = the queue the path is appended to, in Queues order)
#define SB_SHADED 32u
#define SB_MIS_ANSWERED 64u   // a MIS query answered in k_shade (counted as the Scene::Intersect call it replaces, not enqueued)
#define SB_RAY_ANSWERED 128u  // a continuation ray whose hit nothing reads (same bookkeeping)

// The light sample a vertex left pending (EstimateDirect's two terms, integrator.h:38-105), now that its shadow ray and its
// MIS query have been traced: c1 if the shadow ray got through, c2 if the MIS query's answer is yes.
__device__ __forceinline__ v3 pending_light_sample(const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t pid,
                                                   uint32_t flags, uint32_t was_occluded, uint32_t was_mis_ok, float4 c1_4, float4 c2_4,
                                                   float4 f4) {
    v3 Ld = V3s(0.f);
    if (flags & PF_PEND_C1) {
        if (!was_occluded) {  // VisibilityTester::Unoccluded, lights.cpp:10-12
            Ld = Ld + V3(c1_4.x, c1_4.y, c1_4.z);
        }
    }
    if (flags & PF_PEND_C2) {
        uint32_t light = __float_as_uint(f4.w);
        bool add;
        if (rc.mis_mode) {
            add = was_mis_ok != 0;
        } else if (uint32_t hid = pb.mis_hit[pid].id; hid != AGPT_HIT_MISS) {  // integrator.h:82-85: hit shape's area light must be the sampled light
            int hp = (hid & AGPT_HIT_SPHERE) ? (int)(hid & 0x7FFFFFFFu)
                                             : (int)__float_as_uint(sc.tri_shade[4 * (size_t)hid + 3].w);
            add = sc.prims[hp].arealight == (int)light;
        } else {  // :86-87 light.Le(ray): non-zero only for an IsInfinite() light
            add = sc.lights[light].type != AGPT_LIGHT_AREA;
        }
        if (add) Ld = Ld + V3(c2_4.x, c2_4.y, c2_4.z);
    }
    return Ld;
}

// developer build -DAGPT_SHADE_CLOCK: s_memtime stamps at the phase boundaries of shade_path, summed over waves into
// counters->dbg[56..63] (phase k ends at SCK(k); the stamp waits for outstanding memory so a phase owns its own latency)
#ifdef AGPT_SHADE_CLOCK
#define SCK_PARAMS , unsigned long long* sck_acc, unsigned long long& sck_last
#define SCK_ARGS , sck_acc, sck_last
#define SCK(k) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long sck_now = __builtin_amdgcn_s_memtime(); \
                    sck_acc[k] += sck_now - sck_last; sck_last = sck_now; } while (0)
#else
#define SCK_PARAMS
#define SCK_ARGS
#define SCK(k)
#endif
// ENV: the scene has an InfiniteAreaLight (lights.cpp:31-112).  Its sampling / pdf / Le helpers are out-of-line calls whose mere
// presence costs the register allocation of every path (values live across a call site go to callee-saved registers); scenes
// without an environment map -- every BASELINE configuration -- run the instantiation that does not contain them.
// TEXTURED (level 1 above): the hit triangle's two uv records are fetched beside its tri_shade record (one more
// pair of 16-B loads in the same round trip); the texel gather follows the material lookup, and material_set_color puts what
// make_material derives from a colour -- diffuse_R, R0, mirror_R -- into a register copy of the material, which is what
// bsdf_setup, lobe_eval, disney_fresnel and lobe_sample then read.
// MAPPED (level 2): up to three texels per vertex (colour, roughness, metallic), one gather per DISTINCT
// texture -- slots that name the same image, as glTF's metallic-roughness image does, share its texel -- all issued before
// material_set_disney rebuilds the register copy, lobe set included.
// SAMPLED (level 3): MAPPED with texture_address / texture_load / texture_blend (agpt_shade.h) in texture_value's place: one tap of a NEAREST
// texture, four of a BILINEAR one, the taps of every distinct texture issued before the first blend (up to twelve 16-B gathers in
// flight behind the material lookup instead of three round trips of four).
// NORMAL (level 4): SAMPLED with a fourth lookup: the material's DevNormalSlot is read from the global-memory table
// (`normal_table`: sc.material_texture before the LDS copy took its place; nullptr in every other variant) beside the other slots' texture
// records, its address and its taps are formed and issued with theirs -- up to sixteen gathers in one round trip; an image that another
// slot names shares that slot's taps -- and surface_apply_normal_map perturbs the shading normal before bsdf_setup.
template <bool ENV, bool TEXTURED = (AGPT_SHADE_LEVEL >= 1), bool MAPPED = (AGPT_SHADE_LEVEL >= 2), bool SAMPLED = (AGPT_SHADE_LEVEL >= 3),
          bool NORMAL = (AGPT_SHADE_LEVEL == 4)>
__device__ __forceinline__ uint32_t shade_path(const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t pid,
                                               const int32_t* normal_table SCK_PARAMS) {
    uint32_t bits = 0;
    // Every per-path record is fetched up front, unconditionally: the loads then overlap in one memory round trip instead
    // of forming a chain of dependent ones behind the flag tests (a record that turns out not to be needed is a coalesced
    // 16-B read of a valid slot -- every path id owns a slot in every array).
    float4 b4 = pb.beta4[pid];
    float4 l4 = pb.L4[pid];
    const float4 f4 = pb.fac4[pid];
    const uint32_t was_occluded = pb.occluded[pid];
    const uint32_t was_mis_ok = pb.mis_ok[pid];
    const float4 c1_4 = pb.c1[pid], c2_4 = pb.c2[pid];
    const DevHit h = pb.hit[pid];
    const float4 o4 = pb.ext_o[pid], d4 = pb.ext_d[pid];
    v3 beta = V3(b4.x, b4.y, b4.z);
    v3 L = V3(l4.x, l4.y, l4.z);
    uint32_t flags = __float_as_uint(b4.w);
    uint32_t rng = __float_as_uint(l4.w);

    SCK(0);   // records arrived
    // From here on the path id is a fresh value for the compiler: the addresses of the stores below are then formed where they
    // are used (one 64-bit add each) instead of being kept from the loads above across the whole body -- seven address pairs
    // lived in registers and five more went to scratch, reloaded on every path.
    asm volatile("" : "+v"(pid));
    // ---- resolve the previous vertex' UniformSampleOneLight (integrator.h:38-105) ------------------
    if (flags & PF_PENDING) {
        const v3 Ld = pending_light_sample(sc, rc, pb, pid, flags, was_occluded, was_mis_ok, c1_4, c2_4, f4);
        float lightPdf = sh_rcp(sc.n_lights);         // integrator.h:100,104
        L = L + beta * sh_div3(Ld, lightPdf);         // integrator.h:166
        if (!(flags & PF_DEAD)) beta = beta * V3(f4.x, f4.y, f4.z);  // integrator.h:176
        flags &= ~(PF_PENDING | PF_PEND_C1 | PF_PEND_C2);
    }

    SCK(1);   // pending light sample resolved
    if (!(flags & PF_DEAD)) {
        uint32_t bounces = flags & PF_BOUNCE_MASK;
        v3 O = V3(o4.x, o4.y, o4.z), D = V3(d4.x, d4.y, d4.z);
        const bool found = h.id != AGPT_HIT_MISS;
        Surface s;
        float4 uv01 = {0.f, 0.f, 0.f, 0.f}, uv2 = {0.f, 0.f, 0.f, 0.f};   // (TEXTURED only)
        if (found) {
            if (h.id & AGPT_HIT_SPHERE)
                surface_from_sphere(sc, (int)(h.id & 0x7FFFFFFFu), O, D, h.t, s);
            else {
                if constexpr (TEXTURED) {
                    uv01 = sc.tri_uv[2 * (size_t)h.id];
                    uv2 = sc.tri_uv[2 * (size_t)h.id + 1];
                }
                surface_from_triangle(sc, h.id, h.b1, h.b2, O, D, h.t, s);
            }
        }
        SCK(2);   // surface record (tri_shade fetch + interpolation)
        // integrator.h:139-147
        if (bounces == 0 || (flags & PF_SPECULAR)) {
            if (found) {
                int al = sc.prims[s.prim].arealight;
                v3 Le = al >= 0 ? mat_v3(sc.lights[al].L) : V3s(0.f);
                L = L + beta * Le;
            } else {
                for (int li = 0; li < sc.n_lights; li++) {
                    if (sc.lights[li].type == AGPT_LIGHT_UNIFORM_INFINITE)
                        L = L + beta * mat_v3(sc.lights[li].L);
                    else if (ENV && sc.lights[li].type == AGPT_LIGHT_INFINITE_AREA)
                        L = L + beta * env_Le(&sc.envs[sc.lights[li].env], D);
                }
            }
        }
        if (!found || (int)bounces >= rc.max_depth) {  // :150
            flags |= PF_DEAD;
        } else if (sc.prims[s.prim].material < 0) {
            // :152-161 null material: skip the surface, re-cast without counting a bounce
            v3 nO = s.p + AGPT_EPSILON * D;
            v3 nD = normalize(D);
            float4 no4, nd4;
            no4.x = nO.x; no4.y = nO.y; no4.z = nO.z; no4.w = AGPT_FLT_MAX;
            nd4.x = nD.x; nd4.y = nD.y; nd4.z = nD.z;
            nd4.w = bounces == 0 ? 2.f : ((flags & PF_SPECULAR) ? 0.f : 1.f);   // (see below: the trace kernel may re-cast again itself)
            pb.ext_o[pid] = no4;
            pb.ext_d[pid] = nd4;
            bits |= SB_EXT;
        } else {
            SCK(3);   // emission, termination
            bits |= SB_SHADED;
            const DevMaterial& mc = sc.materials[sc.prims[s.prim].material];
            DevMaterial mt;   // TEXTURED: the material with the colour of the texel at the hit (MAPPED: and its roughness / metallic)
            if constexpr (MAPPED) {
                mt = mc;
                const int mat = sc.prims[s.prim].material;
                // (a material with a parameter map always has a colour texture: agpt_scene_commit gives it a 1x1 one of its constant
                // colour if the host set none, so the constructor's third input needs no table of its own)
                const int tex = sc.material_texture[mat];
                const uint32_t slots = (uint32_t)sc.material_texture[sc.n_materials + mat];
                if (tex >= 0 && !(h.id & AGPT_HIT_SPHERE)) {
                    const int rtex = param_slot_texture(slots, 0), mtex = param_slot_texture(slots, 1);   // (0 = roughness, 1 = metallic)
                    // the texture records first (valid for any slot: record 0 stands in for "none"), then the gathers, then their uses
                    const DevTexture ct = sc.textures[tex], rt = sc.textures[rtex >= 0 ? rtex : 0], mx = sc.textures[mtex >= 0 ? mtex : 0];
                    DevNormalSlot nslot;
                    if constexpr (NORMAL) nslot = normal_slot(normal_table, sc.n_materials, mat);
                    float tu, tv;
                    triangle_uv(uv01, uv2, h.b1, h.b2, &tu, &tv);
                    v3 c, rv, mv;
                    if constexpr (SAMPLED) {
                        const bool r_own = rtex >= 0 && rtex != tex, m_own = mtex >= 0 && mtex != tex && mtex != rtex;
                        // all the arithmetic (a texture that is not fetched gets the colour's record: no branch around a division), then
                        // all the gathers, then the blends
                        TextureAddress ca, ra, ma;
                        TextureTaps ck, rk, mk;
                        texture_address(ct, tu, tv, ca);
                        texture_address(r_own ? rt : ct, tu, tv, ra);
                        texture_address(m_own ? mx : ct, tu, tv, ma);
                        int ntex = -1;
                        bool n_own = false;
                        TextureAddress na;
                        TextureTaps nk;
                        if constexpr (NORMAL) {
                            ntex = nslot.texture;
                            n_own = ntex >= 0 && ntex != tex && ntex != rtex && ntex != mtex;
                            texture_address(n_own ? nslot.tex : ct, tu, tv, na);
                        }
                        texture_load(ca, ck);
                        if (r_own) texture_load(ra, rk);
                        if (m_own) texture_load(ma, mk);
                        if constexpr (NORMAL)
                            if (n_own) texture_load(na, nk);
                        c = texture_blend(ca, ck);
                        rv = r_own ? texture_blend(ra, rk) : c;
                        mv = m_own ? texture_blend(ma, mk) : (mtex == rtex ? rv : c);
                        if constexpr (NORMAL)
                            if (ntex >= 0)
                                surface_apply_normal_map(s, n_own ? texture_blend(na, nk) : (ntex == tex ? c : (ntex == rtex ? rv : mv)), nslot.scale);
                    } else {
                        c = texture_value(ct, tu, tv);
                        rv = c, mv = c;
                        if (rtex >= 0 && rtex != tex) rv = texture_value(rt, tu, tv);
                        if (mtex >= 0 && mtex != tex) mv = mtex == rtex ? rv : texture_value(mx, tu, tv);
                    }
                    if (slots)   // (Disney: the only type agpt_scene_set_material_param_texture accepts)
                        material_set_disney(mt, c, rtex >= 0 ? comp(rv, param_slot_channel(slots, 0)) : mc.roughness,
                                            mtex >= 0 ? comp(mv, param_slot_channel(slots, 1)) : mc.metallic);
                    else
                        material_set_color(mt, c);
                }
            } else if constexpr (TEXTURED) {
                mt = mc;
                const int tex = sc.material_texture[sc.prims[s.prim].material];
                if (tex >= 0 && !(h.id & AGPT_HIT_SPHERE)) {
                    float tu, tv;
                    triangle_uv(uv01, uv2, h.b1, h.b2, &tu, &tv);
                    material_set_color(mt, texture_value(sc.textures[tex], tu, tv));
                }
            }
            const DevMaterial& m = TEXTURED ? mt : mc;
            Bsdf bsdf;
            bsdf_setup(bsdf, m, s.n, s.ns, s.ss_bsdf);
            const WoCache wc = bsdf_wo_cache(bsdf, m, s.wo);
            // ---- UniformSampleOneLight / EstimateDirect (integrator.h:38-105) -------------------
            const bool do_nee = !bsdf_is_perfectly_specular(bsdf) && sc.n_lights > 0;
            int numLight = 0;
            float uS0 = 0.f, uS1 = 0.f;
            float scatteringPdf = 0;
            v3 wi = V3s(0.f);
            bool light_ok = false;
            float nee_lightPdf = 0;
            v3 nee_Li = V3s(0.f);
            if (do_nee) {
                int nLights = sc.n_lights;
                numLight = (int)(rng_float(rng) * nLights);
                if (nLights - 1 < numLight) numLight = nLights - 1;
                float uL0 = rng_float(rng), uL1 = rng_float(rng);
                uS0 = rng_float(rng);
                uS1 = rng_float(rng);
                const DevLight& light = sc.lights[numLight];
                flags |= PF_PENDING;
                float lightPdf = 0;
                v3 Li;
                v3 visO = V3s(0.f), visD = V3(0, 0, 1);
                float visT = 0;
                if (light.type == AGPT_LIGHT_UNIFORM_INFINITE) {  // lights.cpp:15-24 (quirk 3)
                    wi = random_in_hemisphere(rng, s.ns);
                    lightPdf = AGPT_INV2PI;
                    visO = s.p + AGPT_EPSILON * wi;
                    visD = normalize(wi);
                    visT = AGPT_FLT_MAX;
                    Li = mat_v3(light.L);
                } else if (ENV && light.type == AGPT_LIGHT_INFINITE_AREA) {  // lights.cpp:50-90: 1 extra draw, offset along n
                    const DevEnv& env = sc.envs[light.env];
                    Li = V3s(0.f);
                    if (env_sample_li(&env, rng_float(rng), &wi, &lightPdf)) {
                        visO = s.p + AGPT_EPSILON * s.n;
                        visD = normalize(wi);
                        visT = AGPT_FLT_MAX;
                        Li = env_Le(&env, visD);
                    }
                } else {  // AreaLight::Sample_Li lights.cpp:115-126
                    v3 pS;
                    sphere_sample_ref(sc.prims[light.shape], s.p, uL0, uL1, &pS, &lightPdf);
                    if (lightPdf == 0 || sqrlen(pS - s.p) == 0) {
                        lightPdf = 0;
                        Li = V3s(0.f);
                    } else {
                        wi = pS - s.p;
                        float dist = length(wi);
                        wi = wi / dist;
                        visO = s.p + AGPT_EPSILON * wi;
                        visD = normalize(wi);
                        visT = dist - 10 * AGPT_EPSILON;
                        Li = mat_v3(light.L);
                    }
                }
                light_ok = lightPdf > 0 && !isblack(Li);   // integrator.h:44
                nee_lightPdf = lightPdf;
                nee_Li = Li;
                // the shadow ray is written where it is known (it only counts if the path joins the shadow queue below): seven
                // registers fewer across the three evaluations
                if (light_ok) {
                    float4 so4, sd4;
                    so4.x = visO.x; so4.y = visO.y; so4.z = visO.z; so4.w = visT;
                    sd4.x = visD.x; sd4.y = visD.y; sd4.z = visD.z; sd4.w = 0.f;
                    pb.sh_o[pid] = so4;
                    pb.sh_d[pid] = sd4;
                }
            }
            SCK(4);   // BSDF set-up + light sampling
            // ---- the three BSDF evaluations of a vertex run through ONE loop with one evaluator call site:
            //   it 0: BSDF::f + BSDF::Pdf for the light sample          (integrator.h:46-47, reflection.h:114-123,174-188)
            //   it 1: EstimateDirect's BSDF-sampling leg, uScattering   (integrator.h:63-90,  BSDF::Sample_f reflection.h:124-172)
            //   it 2: the continuation                                   (integrator.h:170-187, BSDF::Sample_f)
            v3 fac = V3s(1.f);
            const v3 wo_l = w2l(bsdf, s.wo);
            const float woDotNg = dot(s.wo, bsdf.ng);
#pragma unroll 1
            for (int it = do_nee ? (light_ok ? 0 : 1) : 2; it < 3; ++it) {
                const uint32_t lmask = lobes_matching(bsdf, it < 2);   // skipSpecular for both EstimateDirect evaluations
                const int matching = __popc(lmask);
                float pdf = it == 1 ? scatteringPdf : 0.f;   // EstimateDirect reuses its scatteringPdf variable (quirk 9)
                v3 f = V3s(0.f), wi_l = V3s(0.f);
                int skip_lobe = -1;
                bool eval = false, sampledSpecular = false;
                if (it == 0) {   // bsdf_f_pdf's prologue
                    if (bsdf.lobes != 0 && wo_l.z != 0) {
                        wi_l = w2l(bsdf, wi);
                        eval = true;
                    }
                } else {         // bsdf_sample_f's prologue
                    float u0, u1;
                    if (it == 1) {
                        u0 = uS0;
                        u1 = uS1;
                    } else {
                        wi = V3s(0.f);
                        u0 = rng_float(rng);
                        u1 = rng_float(rng);
                    }
                    if (matching == 0) {
                        pdf = 0;
                    } else {
                        int comp = (int)floorf(u0 * matching);
                        if (matching - 1 < comp) comp = matching - 1;
                        uint32_t mm = lmask;   // the comp-th matching lobe in list order
                        for (int i = 0; i < comp; ++i) mm &= mm - 1;
                        const int lobe = __ffs((int)mm) - 1;
                        const float ur0 = sminf(u0 * matching - comp, AGPT_ONE_MINUS_EPS);
                        if (wo_l.z != 0) {   // (wo.z == 0: returns 0 with the caller's pdf untouched, quirk 9)
                            pdf = 0;
                            sampledSpecular = lobe == LOBE_SPECULAR;
                            const v3 fs = lobe_sample(m, lobe, wo_l, &wi_l, ur0, u1, &pdf, wc);
                            if (pdf != 0) {
                                wi = l2w(bsdf, wi_l);
                                if (lobe == LOBE_SPECULAR) {
                                    if (matching > 1) pdf = sh_div(pdf, matching);
                                    f = fs;
                                } else {
                                    eval = true;   // pdf += the other lobes' Pdf (list order), f = sum of all matching lobes' f
                                    skip_lobe = matching > 1 ? lobe : -2;
                                }
                            }
                        }
                    }
                }
                if (eval) {
                    const bool reflect = dot(wi, bsdf.ng) * woDotNg > 0;
                    const LobeEval e = bsdf_eval_lobes_inl(m, lmask, wo_l, wi_l, skip_lobe, pdf, reflect, wc);
                    if (it == 0)
                        pdf = matching > 0 ? sh_div(e.pdf, matching) : 0.f;
                    else if (matching > 1)
                        pdf = sh_div(e.pdf, matching);
                    if (reflect) f = e.f;
                }
                if (it == 0) {   // integrator.h:46-60
                    scatteringPdf = pdf;
                    f = f * absdot(wi, s.ns);
                    if (!isblack(f)) {
                        float weight = power_heuristic(1, nee_lightPdf, 1, scatteringPdf);
                        v3 c1 = sh_div3(f * nee_Li * weight, nee_lightPdf);
                        float4 c4;
                        c4.x = c1.x; c4.y = c1.y; c4.z = c1.z; c4.w = 0.f;
                        pb.c1[pid] = c4;
                        flags |= PF_PEND_C1;
                        bits |= SB_SHADOW;
                    }
                } else if (it == 1) {   // integrator.h:63-90
                    const DevLight& light = sc.lights[numLight];
                    f = f * absdot(wi, s.ns);
                    if (!isblack(f) && pdf > 0) {
                        float lp;
                        if (light.type == AGPT_LIGHT_UNIFORM_INFINITE)
                            lp = dot(s.n, wi) > 0 ? AGPT_INV2PI : 0.f;  // lights.cpp:26-28 (geometric n)
                        else if (ENV && light.type == AGPT_LIGHT_INFINITE_AREA)
                            lp = env_pdf_li(&sc.envs[light.env], wi);
                        else
                            lp = sphere_pdf(sc.prims[light.shape], s.p);
                        if (lp != 0) {
                            float weight = power_heuristic(1, pdf, 1, lp);
                            // Le(-wi) of the light's shape, or light.Le(ray) on a miss (ray.D = normalize(wi))
                            v3 Li2 = ENV && light.type == AGPT_LIGHT_INFINITE_AREA ? env_Le(&sc.envs[light.env], normalize(wi))
                                                                            : mat_v3(light.L);
                            // the reference traces this ray before it looks at Li (integrator.h:77-88); a black Li only
                            // means nothing is added afterwards
                            v3 c2 = isblack(Li2) ? V3s(0.f) : sh_div3(f * Li2 * weight, pdf);
                            v3 mO = s.p + AGPT_EPSILON * wi;
                            v3 mD = normalize(wi);
                            // The query's answer for an area light is "the closest hit is the light's sphere" (integrator.h:82-85):
                            // a ray that misses that sphere altogether cannot say yes, whatever else it meets, so it is answered
                            // here -- by the very test the MIS-query kernel starts a ray with (k_trace_fast: mis_reach) -- and
                            // never enters the queue.  BSDF-sampled directions rarely point at a small light: on C3 this
                            // settles most of the queries of the two sphere lights.  (The ray still counts as the
                            // Scene::Intersect call the reference makes.)
                            bool reach = true;
                            if (rc.answer_rays && light.type == AGPT_LIGHT_AREA) {
                                const DevPrim& LS = sc.prims[light.shape];
                                TraceRay qr;
                                qr.O = mO;
                                qr.D = mD;
                                float ts;
                                reach = sphere_test_c(V3(LS.cx, LS.cy, LS.cz), LS.r2, qr, AGPT_FLT_MAX, ts);
                            }
                            if (!reach) {
                                bits |= SB_MIS_ANSWERED;
                            } else {
                            float4 c4, mo4, md4;
                            c4.x = c2.x; c4.y = c2.y; c4.z = c2.z; c4.w = 0.f;
                            // tmax = FLT_MAX; the MIS-query kernel (mis_mode 1) is told the sampled light's sphere in its place
                            mo4.x = mO.x; mo4.y = mO.y; mo4.z = mO.z;
                            mo4.w = rc.mis_mode ? __uint_as_float(light.type == AGPT_LIGHT_AREA ? (uint32_t)light.shape : 0xFFFFFFFFu)
                                                : AGPT_FLT_MAX;
                            md4.x = mD.x; md4.y = mD.y; md4.z = mD.z; md4.w = __uint_as_float((uint32_t)numLight);
                            pb.c2[pid] = c4;
                            pb.mis_o[pid] = mo4;
                            pb.mis_d[pid] = md4;
                            flags |= PF_PEND_C2;
                            bits |= SB_MIS;
                            }
                        }
                    }
                } else if (isblack(f) || pdf == 0) {   // integrator.h:175
                    flags |= PF_DEAD;
                } else {
                    fac = sh_div3(f * absdot(wi, s.ns), pdf);
                    if (!(flags & PF_PENDING)) beta = beta * fac;
                    flags = (flags & ~PF_SPECULAR) | (sampledSpecular ? PF_SPECULAR : 0u);
                    flags = (flags & ~PF_BOUNCE_MASK) | ((bounces + 1) & PF_BOUNCE_MASK);
                    if (rc.answer_rays && (int)(bounces + 1) >= rc.max_depth && !sampledSpecular) {
                        // The ray that would follow ends the path whatever it hits: at the next vertex the loop adds emission
                        // only after a specular bounce (integrator.h:139-147) and breaks on `bounces >= maxDepth` (:150) before
                        // anything else looks at the intersection.  The reference still makes that Scene::Intersect call; its
                        // answer cannot reach the image, so the production path counts the ray and does not trace it.  (This
                        // vertex' light sample, if one is pending, is added when the batch is consumed: finished_radiance.)
                        flags |= PF_DEAD;
                        bits |= SB_RAY_ANSWERED;
                    } else {
                        v3 nO = s.p + AGPT_EPSILON * wi;
                        v3 nD = normalize(wi);
                        float4 no4, nd4;
                        no4.x = nO.x; no4.y = nO.y; no4.z = nO.z; no4.w = AGPT_FLT_MAX;
                        nd4.x = nD.x; nd4.y = nD.y; nd4.z = nD.z;
                        // d.w = 1: should this ray's closest hit be a primitive without a material (an emitter sphere), the next
                        // vertex does nothing but re-cast it (no emission after a non-specular bounce, :139-147; below maxDepth,
                        // :150; no bounce counted, :152-161) -- k_trace_fast may then do that re-cast itself instead of sending the
                        // path through a whole iteration for it
                        nd4.w = (!sampledSpecular && (int)(bounces + 1) < rc.max_depth) ? 1.f : 0.f;
                        pb.ext_o[pid] = no4;
                        pb.ext_d[pid] = nd4;
                        bits |= SB_EXT;
                    }
                }
            }
            SCK(5);   // the three evaluations incl. their ray / contribution stores
            if (flags & PF_PENDING) {  // the continuation factor and the chosen light wait for the resolve
                float4 f4;
                f4.x = fac.x; f4.y = fac.y; f4.z = fac.z; f4.w = __uint_as_float((uint32_t)numLight);
                pb.fac4[pid] = f4;
            }
        }
    }
    // a path that goes on has a continuation ray (SB_EXT: the queue k_shade reads next).  One that has ended but still owes its
    // last light sample (which waits for the next iteration's shadow ray / MIS query) joins no queue and keeps PF_PENDING: the
    // sample is added where the path's radiance is consumed (finished_radiance below)
    b4.x = beta.x; b4.y = beta.y; b4.z = beta.z; b4.w = __uint_as_float(flags);
    pb.beta4[pid] = b4;
    l4.x = L.x; l4.y = L.y; l4.z = L.z; l4.w = __uint_as_float(rng);
    pb.L4[pid] = l4;
    SCK(6);   // final stores
    return bits;
}

// Every wave handles tiles of 64 * SHADE_U queue entries and aggregates its queue appends per tile: ballots give the per-queue
// counts, ONE atomic per queue reserves the tile's slots, then every lane writes its path id at its (order-preserving) offset
// -- same-line atomics serialise at ~11 ns each and were the kernel's bottleneck with one append per 64 paths.
#ifndef SHADE_GRAB
#define SHADE_GRAB 2   // wave tiles a wave takes per atomic
#endif
#ifndef SHADE_U
#define SHADE_U 4
#endif

// Waves per SIMD the register allocation is held to.  build.py compiles this unit with -DAGPT_SHADE_WAVES=4 and MachineLICM off:
// 128 VGPRs, 2 spilled (134 and none uncapped).  With the pass on the same source needs 168 + 7-14 spilled at three waves and
// ~90 spilled at four.  C3 step, non-trace time: 3 waves / LICM on 77.8 ms, 3 waves / off 77.2, 4 waves / off 73.9.
#ifndef AGPT_SHADE_WAVES
#define AGPT_SHADE_WAVES 3
#endif
// LDS_TABLES: the scene's small tables -- Scene::primitives records, materials, lights -- are copied into LDS at kernel
// start and every lookup of the shading code goes there.  As per-lane global loads they were ~50 separate load -> wait -> use
// points inside one long dependent chain (their addresses depend on the hit), each paying an L1/L2 round trip with only
// three to four waves per SIMD to cover it, and every store to the path state forced the compiler to re-load fields it already
// had (it cannot prove that the tables and the path buffers do not alias).  Scenes whose tables exceed the limits below
// use the global-memory instantiation.
#define AGPT_SHADE_LDS_PRIMS 256
#define AGPT_SHADE_LDS_MATERIALS 128
#define AGPT_SHADE_LDS_LIGHTS 64
template <bool LDS_TABLES, bool ENV>
__global__ void __launch_bounds__(AGPT_BLOCK, AGPT_SHADE_WAVES)
AGPT_SHADE_KNAME(k_shade)(DevScene sc_in, RenderConsts rc, PathBuffers pb, Queues qin, Queues qout, DevCounters* __restrict__ counters,
        uint32_t* __restrict__ tile_heads) {
    __shared__ DevPrim s_tab_prims[LDS_TABLES ? AGPT_SHADE_LDS_PRIMS : 1];
    __shared__ DevMaterial s_tab_materials[LDS_TABLES ? AGPT_SHADE_LDS_MATERIALS : 1];
    __shared__ DevLight s_tab_lights[LDS_TABLES ? AGPT_SHADE_LDS_LIGHTS : 1];
#if AGPT_SHADE_LEVEL
    // 512 B beside the 9.5 KB of materials; MAPPED, SAMPLED: both halves of the table, 1 KB (40,960 B per block in all: still four blocks
    // per CU; the sampler state rides in the texture records, agpt_scene.h).  NORMAL: the same 1 KB -- a fifth block-wide kilobyte would
    // cost the fourth block of the CU, so the normal slots stay in global memory
    constexpr int n_tab_halves = AGPT_SHADE_LEVEL >= 2 ? 2 : 1;
    __shared__ int32_t s_tab_material_texture[LDS_TABLES ? n_tab_halves * AGPT_SHADE_LDS_MATERIALS : 1];
#endif
    // (a launch over a short queue: one wave per 256-path tile is all it can use -- the rest of the grid leaves before setting up)
    if (blockIdx.x * (AGPT_BLOCK / 64) * 64u * SHADE_U >= QCOUNT(qin, 0) && blockIdx.x > 0) return;
    DevScene sc = sc_in;
    if (LDS_TABLES) {
        auto copy_words = [&](void* dst, const void* src, int n_bytes) {
            uint32_t* d = (uint32_t*)dst;
            const uint32_t* g = (const uint32_t*)src;
            for (int i = threadIdx.x; i < n_bytes / 4; i += AGPT_BLOCK) d[i] = g[i];
        };
        copy_words(s_tab_prims, sc_in.prims, sc_in.n_prims * (int)sizeof(DevPrim));
        copy_words(s_tab_materials, sc_in.materials, sc_in.n_materials * (int)sizeof(DevMaterial));
        copy_words(s_tab_lights, sc_in.lights, sc_in.n_lights * (int)sizeof(DevLight));
        sc.prims = s_tab_prims;
        sc.materials = s_tab_materials;
        sc.lights = s_tab_lights;
#if AGPT_SHADE_LEVEL
        copy_words(s_tab_material_texture, sc_in.material_texture, n_tab_halves * sc_in.n_materials * (int)sizeof(int32_t));
        sc.material_texture = s_tab_material_texture;
#endif
        __syncthreads();
    }
    __shared__ uint32_t s_pid[SHADE_U][AGPT_BLOCK];
    __shared__ uint32_t s_bits[SHADE_U][AGPT_BLOCK];
    const uint32_t n_active = QCOUNT(qin, 0);
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    uint32_t shaded = 0, mis_answered = 0;
#ifdef AGPT_SHADE_CLOCK
    unsigned long long sck_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long sck_last = __builtin_amdgcn_s_memtime();
    const unsigned long long sck_begin = sck_last;
#endif
    // Wave-private tiles of 64 * SHADE_U queue entries: the wave shades them, counts its appends per queue with ballots and
    // reserves the slots with one atomic per queue (lanes 0..2, one queue each).  No block barrier: with block-wide tiles
    // the three __syncthreads per tile made every wave wait for the slowest of its block -- 10 % of the kernel's wave
    // time (s_memtime phase clocks) -- while 4x the atomics (one per queue per 256 paths) stay far below the ~11 ns per
    // same-line atomic that had made per-wave-per-64-paths appends the bottleneck.
    const uint32_t wtile = 64u * SHADE_U;
    const uint32_t n_wtiles = (n_active + wtile - 1) / wtile;
    // Tiles are handed out dynamically, SHADE_GRAB at a time, from AGPT_FRONTIERS segment heads (one per XCD, AGPT_QSTRIDE words
    // apart: same-line atomics serialise).  Tiles differ a lot in cost (a tile of misses against a tile of surface hits); with a
    // static stride the slowest wave of a CU ran alone at the end of every launch (83.6 -> 77.7 ms of non-trace time per C3 step).
    uint32_t seg = blockIdx.x & (AGPT_FRONTIERS - 1u), segs_left = AGPT_FRONTIERS;
    const uint32_t seg_tiles = (n_wtiles + AGPT_FRONTIERS - 1u) / AGPT_FRONTIERS;
    uint32_t t_next = 0, t_end = 0;
    auto next_tile = [&](uint32_t& t) -> bool {
        if (t_next < t_end) {
            t = t_next++;
            return true;
        }
        while (segs_left) {
            uint32_t off = 0;
            if (lane == 0) off = atomicAdd(tile_heads + seg * AGPT_QSTRIDE, (uint32_t)SHADE_GRAB);
            off = (uint32_t)__builtin_amdgcn_readfirstlane((int)off);
            const uint32_t seg_begin = seg * seg_tiles;
            const uint32_t seg_end = min(seg_begin + seg_tiles, n_wtiles);
            if (seg_begin < seg_end && off < seg_end - seg_begin) {
                t = seg_begin + off;
                t_next = t + 1u;
                t_end = min(t + (uint32_t)SHADE_GRAB, seg_end);
                return true;
            }
            seg = (seg + 1u) & (AGPT_FRONTIERS - 1u);
            --segs_left;
            // segments that other waves have drained meanwhile are skipped after one look at all the heads (lane k reads head k,
            // past the L1) instead of one failing atomic each: without it every wave of the grid ends with a walk through all
            // eight -- 8,192 x 8 same-line atomics at ~11 ns, ~90 us in which the launch only drains.  A head only grows: a stale
            // value costs an atomic, never a tile.
            if (segs_left) {
                uint32_t head = 0;
                if (lane < (int)AGPT_FRONTIERS) head = __hip_atomic_load(tile_heads + lane * AGPT_QSTRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t fb = (uint32_t)lane * seg_tiles;
                const bool live = lane < (int)AGPT_FRONTIERS && fb < n_wtiles && head < min(seg_tiles, n_wtiles - fb);
                const uint32_t live_mask = (uint32_t)__ballot(live);
                while (segs_left && !((live_mask >> seg) & 1u)) {
                    seg = (seg + 1u) & (AGPT_FRONTIERS - 1u);
                    --segs_left;
                }
            }
        }
        return false;
    };
    for (uint32_t t = 0; next_tile(t);) {
        uint32_t total[AGPT_NQUEUES] = {0, 0, 0};
#pragma unroll 1
        for (int u = 0; u < SHADE_U; ++u) {
#ifdef AGPT_SHADE_CLOCK
            { const unsigned long long n0 = __builtin_amdgcn_s_memtime(); sck_acc[7] += n0 - sck_last; sck_last = n0; }   // queue appends
#endif
            const uint32_t qi = t * wtile + (uint32_t)u * 64u + (uint32_t)lane;
            uint32_t pid = 0, bits = 0;
            if (qi < n_active) {
                pid = qin.ext[qi];
                bits = shade_path<ENV>(sc, rc, pb, pid, AGPT_SHADE_LEVEL == 4 ? sc_in.material_texture : nullptr SCK_ARGS);
            }
            s_pid[u][tid] = pid;     // (slots private to the thread: no synchronisation)
            s_bits[u][tid] = bits;
            shaded += (bits & SB_SHADED) ? 1u : 0u;
            mis_answered += ((bits & SB_MIS_ANSWERED) ? 1u : 0u) + ((bits & SB_RAY_ANSWERED) ? 1u : 0u);
            for (int q = 0; q < AGPT_NQUEUES; ++q) total[q] += (uint32_t)__popcll(__ballot((bits >> q) & 1u));
        }
        uint32_t my_total = total[0];
        for (int q = 1; q < AGPT_NQUEUES; ++q) my_total = lane == q ? total[q] : my_total;
        uint32_t base = 0;
        if (lane < AGPT_NQUEUES && my_total) base = atomicAdd(&QCOUNT(qout, lane), my_total);
        uint32_t run[AGPT_NQUEUES];
        for (int q = 0; q < AGPT_NQUEUES; ++q) run[q] = (uint32_t)__shfl((int)base, q);
        for (int u = 0; u < SHADE_U; ++u) {
            const uint32_t bits = s_bits[u][tid];
            const uint32_t pid = s_pid[u][tid];
            for (int q = 0; q < AGPT_NQUEUES; ++q) {
                const bool pred = (bits >> q) & 1u;
                const unsigned long long m = __ballot(pred);
                if (pred) {
                    uint32_t* qq = q == 0 ? qout.ext : (q == 1 ? qout.mis : qout.shadow);
                    qq[run[q] + (uint32_t)__popcll(m & lt_mask)] = pid;
                }
                run[q] += (uint32_t)__popcll(m);
            }
        }
    }
#ifdef AGPT_SHADE_CLOCK
    if (lane == 0) {
        for (int k = 0; k < 8; ++k) atomicAdd(&counters->dbg[56 + k], sck_acc[k]);
        atomicAdd(&counters->dbg[55], __builtin_amdgcn_s_memtime() - sck_begin);
    }
#endif
    // one atomic per wave, not per lane
    for (int off = 32; off > 0; off >>= 1) {
        shaded += __shfl_down(shaded, off);
        mis_answered += __shfl_down(mis_answered, off);
    }
    if (lane == 0 && shaded) atomicAdd(&counters->shaded, (unsigned long long)shaded);
    if (lane == 0 && mis_answered) {
        atomicAdd(&counters->closest_rays, (unsigned long long)mis_answered);   // MIS queries are Scene::Intersect calls
        atomicAdd(&counters->answered, (unsigned long long)mis_answered);
    }
}

// ---------------------------------------------------------------------------------------------------------
// The radiance of a finished path.  A path that has ended (MaxDepth reached, miss, black sample) while its last vertex' light
// sample was still waiting for its shadow ray / MIS query keeps PF_PENDING: the rays have been traced by the time the batch is
// finished, the operands are where k_shade left them (an ended path issues no more rays and owns its slots), and the sample is
// added (integrator.h:166) here, where L4 is consumed -- the expressions and their order are those of k_shade's own resolve of a
// live path's pending sample.  (Ended paths used to leave through a fifth queue and a kernel of their own, which re-read all of
// this and wrote L4 back for the accumulate pass to read again: after the last bounce that is every path of the batch.)
// The operands are fetched only for a pending path, fac4 (the chosen light) only where the closest-hit form of the MIS query needs it.
__device__ __forceinline__ v3 finished_radiance(const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t pid, float4 b4,
                                                float4 l4) {
    const v3 L = V3(l4.x, l4.y, l4.z);
    const uint32_t flags = __float_as_uint(b4.w);
    if (!(flags & PF_PENDING)) return L;
    const uint32_t was_occluded = pb.occluded[pid], was_mis_ok = pb.mis_ok[pid];
    const float4 c1_4 = pb.c1[pid], c2_4 = pb.c2[pid];
    float4 f4 = {0.f, 0.f, 0.f, 0.f};
    if (!rc.mis_mode) f4 = pb.fac4[pid];
    const v3 Ld = pending_light_sample(sc, rc, pb, pid, flags, was_occluded, was_mis_ok, c1_4, c2_4, f4);
    const float lightPdf = sh_rcp(sc.n_lights);         // integrator.h:100,104
    return L + V3(b4.x, b4.y, b4.z) * sh_div3(Ld, lightPdf);   // integrator.h:166
}

#if !AGPT_SHADE_LEVEL   // (no BSDF, no material: every scene runs the plain unit's kernels of its arithmetic)
// film_sample (agpt_wavefront.h: the NaN / inf reject) + Accumulator::AddSample (myapp.h:17-19): samples are added in sample order.
// A block owns AGPT_BLOCK / G pixels (G = sample_group: a pixel's samples lie in runs of G consecutive path ids, so the block's runs
// of one sample group are AGPT_BLOCK consecutive ids).  Per sample group every thread finishes ONE path -- the reads of L4, beta4 and
// a pending path's operands are coalesced, 64 lanes on 64 neighbouring records -- and parks the sample in LDS; then the first
// AGPT_BLOCK / G threads add their pixel's G samples in sample order, ((a + s0) + s1) + ..., continuing over the sample groups.
// (One thread per pixel walking its own samples kept the additions and the loads in one lane: with the operands of a pending path
// to fetch behind each flag test that was 10 ms per C3 step against the 0.45 ms of adding up L4 alone.)
__global__ void __launch_bounds__(AGPT_BLOCK)
AGPT_SHADE_KNAME(k_accumulate)(DevScene sc, RenderConsts rc, PathBuffers pb, float4* __restrict__ accum, DevCounters* __restrict__ counters) {
    __shared__ float4 s_clr[AGPT_BLOCK];
    const uint32_t G = sample_group(rc.S), per_block = AGPT_BLOCK / G;
    const uint32_t tid = threadIdx.x;
    const uint32_t p0 = blockIdx.x * per_block;
    const uint32_t pf = p0 + tid / G;                 // the pixel whose sample this thread finishes
    const bool owner = tid < per_block && p0 + tid < rc.NP;   // ... and the one it adds up
    float4 a = {0.f, 0.f, 0.f, 0.f};
    size_t ai = 0;
    if (owner) {
        int x, y;
        pixel_of(rc, p0 + tid, x, y, ai);
        a = accum[ai];
    }
    uint32_t bad = 0;
    for (uint32_t sg = 0; sg < (uint32_t)rc.S / G; ++sg) {
        if (pf < rc.NP) {
            const uint32_t i = (sg * rc.NP + p0) * G + tid;   // = (sg * NP + pf) * G + tid % G (path ids fit 31 bits: agpt_render's batch limit)
            const FilmSample fs = film_sample(finished_radiance(sc, rc, pb, i, pb.beta4[i], pb.L4[i]), bad);
            const v3 clr = fs.clr;
            bad = fs.bad;
            float4 c4;
            c4.x = clr.x; c4.y = clr.y; c4.z = clr.z; c4.w = 0.f;
            s_clr[tid] = c4;
        }
        __syncthreads();
        if (owner) {
#pragma unroll 4
            for (uint32_t j = 0; j < G; ++j) {   // (the order of the additions is the sample order)
                const float4 c4 = s_clr[tid * G + j];
                a.x += c4.x;
                a.y += c4.y;
                a.z += c4.z;
            }
        }
        __syncthreads();
    }
    if (owner) accum[ai] = a;
    if (bad) atomicAdd(&counters->outliers, (unsigned long long)bad);  // outliers are rare
}

// agpt_li_batch's consumer: Li's return value as it is (the NaN / inf filter belongs to MyApp::Tick, myapp.cpp:169-172, not to the
// integrator) and the stream's state after the path, so that a host can go on drawing from it
__global__ void __launch_bounds__(AGPT_BLOCK)
AGPT_SHADE_KNAME(k_export_li)(DevScene sc, RenderConsts rc, PathBuffers pb, uint32_t n, float* __restrict__ radiance3, uint32_t* __restrict__ rng_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 l4 = pb.L4[i];
    const v3 L = finished_radiance(sc, rc, pb, i, pb.beta4[i], l4);
    radiance3[3 * i] = L.x;
    radiance3[3 * i + 1] = L.y;
    radiance3[3 * i + 2] = L.z;
    if (rng_out) rng_out[i] = __float_as_uint(l4.w);
}

// agpt_render_adaptive's consumer, k_accumulate_list, belongs to agpt_adaptive.hip, a unit with other code-generation options: for it
// ONE pass over the batch's n paths, after its last iteration, puts a pending path's radiance into L4 and clears the flags
// (idempotent).  No queue, no launch per iteration: it keeps the name of the per-iteration kernel it replaces, the one kernel of
// these units that does nothing but add pending light samples.
__global__ void __launch_bounds__(AGPT_BLOCK)
AGPT_SHADE_KNAME(k_resolve_pending)(DevScene sc, RenderConsts rc, PathBuffers pb, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 b4 = pb.beta4[i];
    const uint32_t flags = __float_as_uint(b4.w);
    if (!(flags & PF_PENDING)) return;
    float4 l4 = pb.L4[i];
    const v3 L = finished_radiance(sc, rc, pb, i, b4, l4);
    l4.x = L.x; l4.y = L.y; l4.z = L.z;
    pb.L4[i] = l4;
    b4.w = __uint_as_float(flags & ~(PF_PENDING | PF_PEND_C1 | PF_PEND_C2));
    pb.beta4[i] = b4;
}
#endif

// ---------------------------------------------------------------------------------------------------------
// The host-side launchers of a unit, named like its kernels (launch_shade_fast, ...).  agpt::launch_shading (agpt_shade_kernels.hip)
// picks among the units.
namespace agpt {
using ShadeLaunch = void(hipStream_t stream, int grid, bool lds_tables, bool env, const DevScene& sc, const RenderConsts& rc,
                         const PathBuffers& pb, const Queues& qin, const Queues& qout, DevCounters* counters, uint32_t* tile_heads);
using AccumulateLaunch = void(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, float4* accum,
                               DevCounters* counters);
using FinishPathsLaunch = void(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t n);
#define X(level, suffix) ShadeLaunch launch_shade##suffix, launch_shade##suffix##_fast;
AGPT_SHADE_LEVEL_LIST(X)
#undef X
// (only the two level-0 units have these, see k_accumulate)
AccumulateLaunch finish_accumulate, finish_accumulate_fast;
FinishPathsLaunch finish_paths, finish_paths_fast;
using ExportLiLaunch = void(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t n, float* radiance3,
                            uint32_t* rng_out);
ExportLiLaunch finish_export_li, finish_export_li_fast;

void AGPT_SHADE_KNAME(launch_shade)(hipStream_t stream, int grid, bool lds_tables, bool env, const DevScene& sc, const RenderConsts& rc,
                                    const PathBuffers& pb, const Queues& qin, const Queues& qout, DevCounters* counters,
                                    uint32_t* tile_heads) {
    const dim3 g(grid), b(AGPT_BLOCK);
    if (lds_tables && env)
        hipLaunchKernelGGL((AGPT_SHADE_KNAME(k_shade)<true, true>), g, b, 0, stream, sc, rc, pb, qin, qout, counters, tile_heads);
    else if (lds_tables)
        hipLaunchKernelGGL((AGPT_SHADE_KNAME(k_shade)<true, false>), g, b, 0, stream, sc, rc, pb, qin, qout, counters, tile_heads);
    else if (env)
        hipLaunchKernelGGL((AGPT_SHADE_KNAME(k_shade)<false, true>), g, b, 0, stream, sc, rc, pb, qin, qout, counters, tile_heads);
    else
        hipLaunchKernelGGL((AGPT_SHADE_KNAME(k_shade)<false, false>), g, b, 0, stream, sc, rc, pb, qin, qout, counters, tile_heads);
}
#if !AGPT_SHADE_LEVEL
void AGPT_SHADE_KNAME(finish_accumulate)(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, float4* accum,
                                         DevCounters* counters) {
    hipLaunchKernelGGL(AGPT_SHADE_KNAME(k_accumulate), agpt_blocks((uint64_t)rc.NP * sample_group(rc.S))   /* blocks own AGPT_BLOCK / G pixels each */, dim3(AGPT_BLOCK), 0, stream, sc, rc, pb, accum, counters);
}
void AGPT_SHADE_KNAME(finish_paths)(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t n) {
    hipLaunchKernelGGL(AGPT_SHADE_KNAME(k_resolve_pending), agpt_blocks(n), dim3(AGPT_BLOCK), 0, stream, sc, rc, pb, n);
}
void AGPT_SHADE_KNAME(finish_export_li)(hipStream_t stream, const DevScene& sc, const RenderConsts& rc, const PathBuffers& pb, uint32_t n,
                                        float* radiance3, uint32_t* rng_out) {
    hipLaunchKernelGGL(AGPT_SHADE_KNAME(k_export_li), agpt_blocks(n), dim3(AGPT_BLOCK), 0, stream, sc, rc, pb, n, radiance3, rng_out);
}
#endif
}  // namespace agpt
