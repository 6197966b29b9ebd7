// agpt_trace_kernels.h -- the trace kernels of the wavefront path tracer: k_trace (instrumented variant and fallback), k_trace_fast
// (the production kernel) and k_candidates (top-level walk of lists longer than 64 primitives).  The iteration they are part of is
// described at the top of agpt_kernels.h.  Compiled by agpt_trace_kernels.hip alone, whose launch_trace picks the instantiation.
//
// Still written out more than once here, each copy with a note that names the other: the MIS-query decoding (3), the analytic loop (2),
// the primitive record (2), pop-or-pick_next (2) in k_trace_fast / k_candidates; the counter flush (k_trace, k_trace_fast).
#pragma once

#include <type_traits>

#include "agpt_shade.h"
#include "agpt_trace.h"

#include "agpt_wavefront.h"

// ---------------------------------------------------------------------------------------------------------
// DEPTH: per-lane stack entries (32, or 64 for BVHs deeper than AGPT_STACK_DEPTH: 64 KiB of LDS per block)
template <bool ANY, bool COUNT, int DEPTH>
__global__ void __launch_bounds__(AGPT_BLOCK)
k_trace(DevScene sc, const uint32_t* __restrict__ queue, const uint32_t* __restrict__ count_ptr, uint32_t count_imm,
        uint32_t* __restrict__ work_head, const float4* __restrict__ ray_o, const float4* __restrict__ ray_d,
        DevHit* __restrict__ hits, uint32_t* __restrict__ occluded, DevCounters* __restrict__ counters) {
    __shared__ uint32_t s_stack[DEPTH * AGPT_BLOCK];
    uint32_t* stack = s_stack + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t count = count_ptr ? *count_ptr : count_imm;
    TraceCounters cnt;
    cnt.interior = 0;
    cnt.tris = 0;
    cnt.roots = 0;
    cnt.last_mesh = 0;
    for (;;) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(work_head, (uint32_t)AGPT_CHUNK);
        base = __shfl(base, 0);
        if (base >= count) break;
        uint32_t i = base + lane;
        if (i < count) {
            uint32_t pid = queue ? queue[i] : i;
            float4 o = ray_o[pid], d = ray_d[pid];
            DevHit h;
            bool hit = trace_scene<ANY, COUNT>(sc, V3(o.x, o.y, o.z), V3(d.x, d.y, d.z), o.w, h, stack, AGPT_BLOCK, cnt);
            if (ANY)
                occluded[pid] = hit ? 1u : 0u;
            else
                hits[pid] = h;
        }
    }
    // (k_trace_fast ends with the same flush, the second copy: its counters go in the order interior, roots, tris, here interior,
    // tris, roots.  One by-value function for both changed the code of every counting k_trace_fast instantiation, and of this kernel.)
    if (COUNT) {
        for (int off = 32; off > 0; off >>= 1) {
            cnt.interior += __shfl_down(cnt.interior, off);
            cnt.tris += __shfl_down(cnt.tris, off);
            cnt.roots += __shfl_down(cnt.roots, off);
        }
        if (lane == 0) {
            atomicAdd(&counters->interior, (unsigned long long)cnt.interior);
            atomicAdd(&counters->tris, (unsigned long long)cnt.tris);
            atomicAdd(&counters->roots, (unsigned long long)cnt.roots);
        }
    }
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (ANY)
            atomicAdd(&counters->anyhit_rays, (unsigned long long)count);
        else
            atomicAdd(&counters->closest_rays, (unsigned long long)count);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Production trace kernel (the generic k_trace above stays as the instrumented variant and the fallback for more than
// 2048 primitives; both are checked against the oracle and against each other).  Same decisions as trace_scene(),
// restructured for wave efficiency on 64-wide CDNA4 wavefronts:
//   * persistent waves with IN-FLIGHT REFILL: when at least AGPT_REFILL lanes (agpt_internal.h) have retired their rays the wave hands
//     them new rays from a wave-private LDS ring instead of idling until all 64 are done;
//   * PREFILTER RING: rays enter the ring 64 at a time (one atomic on the frontier counter of the wave's queue segment)
//     with a per-primitive candidate mask from a cheap conservative slab test, all 64 lanes busy; the exact
//     Bounds::Intersect is re-run per lane where the reference runs it;
//   * VOTE-SCHEDULED traversal: a lane is between primitives (A), at an interior node (B) or at a leaf (C); each step
//     the wave executes the body most lanes wait for.  A mesh's root-box test is an interior step on its root pair, which a
//     fast ray skips on short lists (pick_next: ROOT ENTRY).
#define AGPT_RING 128  // entries of the per-wave ring of pre-filtered rays (power of two, >= 64 + 63)
// per-primitive root record staged in LDS: [2k] = (bmin.xyz | sphere centre.xyz, kind), [2k+1] = (bmax.xyz, root_enc) |
// (r2, -, -, -) | (half x, half z, -, -); kind 0 = mesh, 1 = sphere, 2 = empty mesh (never hit), 3 = plane

// MODE 0: Scene::Intersect (closest hit).  MODE 1: Scene::IntersectP (any hit, shadow rays).
// MODE 2: the MIS query of EstimateDirect's BSDF-sampling leg (integrator.h:76-88).  The reference runs a full
// Scene::Intersect there but only uses "is the closest hit the sampled light's shape" (area light) or "did the ray
// escape" (infinite light).  That boolean is answered exactly by an early-exit traversal:
//   * infinite light: ok iff nothing is hit (any-hit);
//   * area light with sphere S (primitive index kS): let t_s be S's accepted root for this ray.  If S is missed the
//     answer is no; else ok iff no other primitive yields a hit the reference would have kept in front of S:
//     triangles and planes need t < t_s (their tests are strict on both list sides), another sphere P blocks iff
//     root_P < t_s when P precedes S in Scene::primitives and root_P <= t_s when it follows (Sphere::Intersect accepts
//     root <= ray.t, so a tie goes to the later primitive); degenerate triangles never block (quirk 11).
// Every MIS ray is still traced through the BVH; it stops at the first blocker instead of finishing a closest-hit search.
// LIST: scenes with more than 64 primitives.  k_candidates (below) has walked the top-level tree over the meshes' root
// boxes once per ray and left one 64-bit candidate word per chunk of 64 primitives plus a word saying which chunks have
// any (cand_mask[chunk * cand_stride + path], cand_chunks[path]); the lane walks its candidates chunk by chunk in list
// order -- exactly Scene::Intersect's sequential walk with a shared ray.t (scene.h:5-19), minus the primitives the ray
// cannot touch.  The prefilter and the LDS copy of the primitive records belong to the short-list instantiation only.
// COUNT: the same kernel also counts the work it does -- pair records fetched (interior), the first record fetched of each mesh
// (roots: the mesh entries that survive the prefilter -- the root pair, or the root's child pair where pick_next enters there)
// and triangle tests -- for bench.py's roofline; the counts are per-lane sums, deterministic for a given queue (every lane's own
// operation sequence is fixed).
// DEPTH = per-lane stack entries kept in LDS.  SPILL: the scene's BVHs are deeper than that -- entries DEPTH and up live
// in a per-thread column of an HBM buffer (spill[(k - DEPTH) * threads_in_grid + thread]); near-first descent rarely needs
// them.  Occupancy is LDS-bound (DEPTH KiB of stack + 8 KiB per block): 23 entries -> 5 blocks = 20 waves per CU, which
// is worth 9 % over the 4 blocks of a 32-entry stack (measured; the round-1 test of a fifth block used an exact 32-KiB fit
// that never became resident).
#ifndef AGPT_TRACE_WAVES
#define AGPT_TRACE_WAVES 1   // minimum waves per SIMD the register allocation of k_trace_fast is held to
#endif
// The rays of a launch.  The short-list closest-hit instantiations re-cast a ray in place (CUR_RECAST below): they read and write
// the rays through one plain pointer each; every other instantiation only reads them, and says so.
template <int MODE, bool LIST>
using TraceRays = std::conditional_t<MODE == 0 && !LIST, float4*, const float4* __restrict__>;
// recast_on (MODE 0, short lists): the rays carry d.w and may be re-cast; path_beta4 / path_L4 are then the paths' state
// COH (MODE 0, short lists, no counting): the launch over the camera rays of a 64-sample group.  A wave takes one pixel's 64 rays
// at a time (the host passes refill = 64), and where every lane that is about to run an interior or a leaf step stands at the SAME
// node, the wave fetches that record once, through scalar loads, instead of 64 times through the vector L1: the box and triangle
// coordinates are then SGPR operands of the very same per-lane arithmetic.  Lanes that stand at different nodes run the vector
// step of every other instantiation.  Only loads go through the scalar unit.
template <int MODE, int DEPTH, bool LIST, bool COUNT, bool SPILL, bool PEEK, bool COH = false>
__global__ void __launch_bounds__(AGPT_BLOCK, COH ? 5 : AGPT_TRACE_WAVES)
k_trace_fast(DevScene sc, const uint32_t* __restrict__ queue, const uint32_t* __restrict__ count_ptr, uint32_t count_imm,
             uint32_t* __restrict__ work_head, TraceRays<MODE, LIST> ray_o, TraceRays<MODE, LIST> ray_d,
             DevHit* __restrict__ hits, uint32_t* __restrict__ occluded, DevCounters* __restrict__ counters, int refill,
             uint32_t cand_stride, uint32_t* __restrict__ spill, const unsigned long long* __restrict__ cand_mask,
             const uint32_t* __restrict__ cand_chunks, bool recast_on, const float4* path_beta4, float4* path_L4, bool root_entry) {
    constexpr bool ANY = MODE != 0;
    constexpr bool MIS = MODE == 2;
    static_assert(!COH || (MODE == 0 && !LIST && !COUNT), "the coherent instantiation is a plain short-list closest-hit launch");
    constexpr int BLOCK = AGPT_BLOCK;
    if constexpr (COH) refill = 64;    // (what the host passes: a wave takes a whole 64-ray chunk, and only when it is empty)
    constexpr bool PRIM_LDS = !LIST;   // short lists: the primitive records live in LDS
    __shared__ uint32_t s_stack[DEPTH * BLOCK];
    __shared__ float4 s_prim[PRIM_LDS ? 2 * 64 : 2];
    uint32_t* stack = s_stack + threadIdx.x;
    uint32_t* spill_col = SPILL ? spill + (size_t)blockIdx.x * BLOCK + threadIdx.x : nullptr;
    const size_t spill_stride = (size_t)gridDim.x * BLOCK;
    auto stack_push = [&](int k, uint32_t v) {
        if (!SPILL || k < DEPTH)
            stack[k * BLOCK] = v;
        else
            spill_col[(size_t)(k - DEPTH) * spill_stride] = v;
    };
    auto stack_at = [&](int k) -> uint32_t {
        if (!SPILL || k < DEPTH) return stack[k * BLOCK];
        return spill_col[(size_t)(k - DEPTH) * spill_stride];
    };
    const int lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    // (a value loaded through a pointer counts as divergent for the compiler: readfirstlane keeps the bookkeeping scalar)
    const uint32_t count = (uint32_t)__builtin_amdgcn_readfirstlane((int)(count_ptr ? *count_ptr : count_imm));
    // (the late iterations' queues are short or empty: a launch can use one wave per 64 rays -- the rest of the grid leaves
    // before setting up, with nothing to drain)
    if (blockIdx.x * (uint32_t)BLOCK >= count) return;
    const int n_prims = LIST ? 0 : sc.n_prims;   // (short lists: the primitive records live in LDS)
    if (PRIM_LDS && (int)threadIdx.x < n_prims) {
        const DevPrim& P = sc.prims[threadIdx.x];
        float4 a, b;   // (the record; its kind and operands are formed once more in the !PRIM_LDS branch of state A, which says why)
        if (P.type == AGPT_PRIM_SPHERE) {
            a.x = P.cx; a.y = P.cy; a.z = P.cz; a.w = 1.f;
            b.x = P.r2; b.y = 0.f; b.z = P.material < 0 ? 1.f : 0.f; b.w = 0.f;   // b.z: no material (an emitter's sphere)
        } else if (P.type == AGPT_PRIM_PLANE) {
            a.x = P.cx; a.y = P.cy; a.z = P.cz; a.w = 3.f;
            b.x = P.r; b.y = P.r2; b.z = P.material < 0 ? 1.f : 0.f; b.w = 0.f;
        } else {
            a.x = P.root_bmin[0]; a.y = P.root_bmin[1]; a.z = P.root_bmin[2]; a.w = P.n_tris > 0 ? 0.f : 2.f;
            b.x = P.root_bmax[0]; b.y = P.root_bmax[1]; b.z = P.root_bmax[2]; b.w = __uint_as_float(P.root_enc);
        }
        s_prim[2 * threadIdx.x] = a;
        s_prim[2 * threadIdx.x + 1] = b;
    }
    __syncthreads();
    const unsigned long long all_prims = n_prims >= 64 ? ~0ull : ((1ull << n_prims) - 1ull);

    // Work distribution: rays are taken 64 at a time from the frontier of one of AGPT_FRONTIERS queue segments (see the
    // refill code below); within a segment the frontier moves monotonically, so at any moment an XCD traces rays that are
    // neighbours in the queue (neighbouring pixels / path ids), which keeps their BVH nodes hot in its L2.  Reserving large
    // private ranges per wave instead measured 8 % slower (A/B on MI355X, same process).
    // A lane's scheduling state is carried by `cur` itself: CUR_IDLE = no ray, CUR_PICK = between meshes (state A),
    // anything below = an interior child-pair index (state B), sign bit set = a leaf encoding (state C).  One v_cmp per
    // state gives the wave's vote masks.  LIST adds CUR_FETCH (voted with state A): the current chunk's candidates are used
    // up and the next chunk's word has to be fetched.
    uint32_t pid = 0;
    unsigned long long mask = 0;
    // CUR_RECAST (closest-hit launches of the wavefront loop): the ray has retired on a primitive without a material and waits for
    // the top of the outer loop to be re-cast (see there); it takes part in no vote.
    constexpr uint32_t CUR_IDLE = 0x7FFFFFFFu, CUR_RECAST = 0x7FFFFFFEu, CUR_PICK = 0x7FFFFFFDu, CUR_FETCH = 0x7FFFFFFCu;
    constexpr uint32_t CUR_B_END = LIST ? CUR_FETCH : CUR_PICK;   // state B: cur < CUR_B_END
    const uint32_t rootpair_base = sc.rootpair_base;
    const bool coords_ok = sc.mdiv_coords_ok != 0;   // agpt_trace.h: the scene's boxes lie in the Markstein divide's domain
    const unsigned long long mesh_mask0 = sc.mesh_masks[0];
    // LIST lane state: the mesh bits of the current chunk
    unsigned long long mmask = 0;
    TraceRay r;   // the lane's ray: set before every pick_next() call, which looks at r.fast
    r.O = V3s(0.f);
    r.D = V3(0.f, 0.f, 1.f);
    r.R = V3s(1.f);
    r.fast = true;
    bool at_entry = false;   // COUNT: the record the lane fetches next is the first of a mesh (counted as a root test)
    uint32_t cvisit = 0, cchunk = 0;   // LIST: chunks of the ray's candidates still to visit (one bit each), the current chunk
    // the sphere of an area light as (centre, r2), wherever it sits in the primitive list
    auto light_sphere = [&](int shape, v3& c, float& r2) {
        if (PRIM_LDS) {
            const float4 sa = s_prim[2 * shape], sb = s_prim[2 * shape + 1];
            c = V3(sa.x, sa.y, sa.z);
            r2 = sb.x;
        } else {
            const DevPrim& P = sc.prims[shape];
            c = V3(P.cx, P.cy, P.cz);
            r2 = P.r2;
        }
    };
    // Scene::Intersect's walk to the next primitive of the list (scene.h:8-17).  A mesh is entered through its root
    // pair -- the root-box test becomes the lane's next interior step (state B); spheres, planes and the end of the
    // list go through state A.
    // ROOT ENTRY (short lists, root_entry: off with the developer knob AGPT_ROOT_STEP=1): a fast ray enters a mesh whose root is
    // interior at the root's CHILD pair (the root_enc staged in s_prim[2k+1].w) and never runs the root-box step.  box_test_fast is
    // monotone under box containment (a box inside a rejected box is rejected), and a root box is the exact
    // union of its children's: where the reference rejects the root, both children are rejected at the same rayt and the lane
    // moves on after the same one step; where it accepts the root, its next step is this very pair at an unchanged rayt.  Slow
    // rays (NaN / inf quotients: not monotone) and meshes whose root is a leaf keep the root pair.
    auto pick_next = [&](unsigned long long& m) -> uint32_t {
        const unsigned long long low = m & (0ull - m);
        if (LIST) {
            if (m == 0) return cvisit ? CUR_FETCH : CUR_PICK;
            if (low & mmask) {
                m ^= low;
                if (COUNT) at_entry = true;
                return rootpair_base + 2u * (64u * cchunk + (uint32_t)(__ffsll((long long)low) - 1));
            }
            return CUR_PICK;
        }
        if (low & mesh_mask0) {
            m ^= low;
            const uint32_t k = (uint32_t)(__ffsll((long long)low) - 1);
            if (COUNT) at_entry = true;
            uint32_t entry = rootpair_base + 2u * k;
            if (root_entry) {   // (wave-uniform)
                const uint32_t enc = __float_as_uint(s_prim[2 * k + 1].w);
                entry = (r.fast && (int32_t)enc >= 0) ? enc : entry;
            }
            return entry;
        }
        return CUR_PICK;
    };
    // LIST: start on chunk c of the lane's ray (issues the loads of its candidate word and of the chunk's mesh bits)
    auto enter_chunk = [&](uint32_t c) {
        cvisit &= ~(1u << c);
        cchunk = c;
        mask = cand_mask[(size_t)c * cand_stride + pid];
        mmask = sc.chunk_mesh_masks[c];
    };
    // Work distribution and the refill pipeline.  The queue is cut into AGPT_FRONTIERS contiguous segments, each with its own
    // frontier counter on its own 128-B line; a wave starts in the segment of its XCD (workgroups are dealt round-robin to
    // the 8 XCDs) and moves on to the next segment when its own is drained.  (One shared counter was the limit of the
    // any-hit launches: same-address atomics complete one per ~11 ns chip-wide.)  Getting 64 new rays is a chain of four
    // dependent memory operations -- frontier atomic -> queue[] -> ray_o/ray_d[] -> (prefilter) -> ring -- that took
    // 10-20 k cycles per top-up when run back to back (13 % of the closest-hit launches' wave time, 30 % of the MIS
    // launches', measured with s_memtime stamps).  It is therefore software-pipelined over successive top-ups:
    // pump_consume() prefilters the rays whose loads were issued one top-up earlier into the ring; pump_issue() -- called
    // AFTER the idle lanes have been handed their rays, because vector-memory results return in issue order and anything
    // loaded after it would wait for it -- issues the ray loads for the path ids fetched by the previous pump_issue, the
    // queue load for the offset returned by the previous atomic, and the next atomic.  The traversal steps between two
    // top-ups hide all of it; only a cold pipeline (kernel start, segment change) runs the chain synchronously.
    uint32_t seg = blockIdx.x & (AGPT_FRONTIERS - 1u), segs_left = AGPT_FRONTIERS;   // wave-uniform
    const uint32_t seg_len = ((count + AGPT_FRONTIERS - 1u) / AGPT_FRONTIERS + 63u) & ~63u;
    uint32_t cur = CUR_IDLE, hid = AGPT_HIT_MISS;
    int sp = 0;
    float rayt = 0.f, hb1 = 0.f, hb2 = 0.f;

    // wave-private ring of pre-filtered rays (path id + primitive mask), filled 64 rays at a time
    __shared__ uint32_t s_ring_pid[BLOCK / 64][AGPT_RING];
    __shared__ unsigned long long s_ring_mask[BLOCK / 64][AGPT_RING];
    uint32_t* ring_pid = s_ring_pid[threadIdx.x >> 6];
    unsigned long long* ring_mask = s_ring_mask[threadIdx.x >> 6];
    uint32_t ring_head = 0, ring_tail = 0;  // wave-uniform, monotonically increasing
    bool mis_area = false;    // MODE 2: the sampled light is an area light
    int mis_skip = -1;        // MODE 2: primitive index of the sampled area light's sphere (never a blocker itself)
    bool mis_reach = true;    // MODE 2: infinite light, or the ray reaches the light's sphere
    bool any_slow = false;                  // wave-uniform: some active lane's ray needs the true-division slab test
    uint32_t c_int = 0, c_root = 0, c_tri = 0;   // COUNT
    TS(unsigned long long ts_steps[3] = {0, 0, 0}; unsigned long long ts_lanes[3] = {0, 0, 0}; unsigned long long ts_act = 0;
       unsigned long long ts_refills = 0; unsigned long long ts_refilled = 0; unsigned long long ts_pref = 0;
       uint32_t ts_push[5] = {0, 0, 0, 0, 0}; uint32_t ts_root = 0, ts_root_pass = 0;   // root-pair steps, and those whose root box passes
       unsigned long long ts_usteps[2] = {0, 0}; unsigned long long ts_ulanes[2] = {0, 0};)   // COH: B / C steps on the scalar path
    TCK(unsigned long long tk_refill = 0, tk_vote = 0, tk_bmem = 0, tk_balu = 0, tk_c = 0, tk_a = 0; const unsigned long long tk_begin = TCK_NOW();)

    uint32_t pfa_off = 0;       // lane 0: offset returned by the pending frontier atomic (stage A)
    uint32_t pfa_seg = 0;
    bool pfa_valid = false;     // wave-uniform, like every *_valid / *_n below
    uint32_t pfb_pid = 0, pfb_n = 0;   // stage B: path ids of the chunk after next (queue load pending)
    bool pfb_valid = false;
    uint32_t pfc_pid = 0, pfc_n = 0;   // stage C: the next chunk's rays (ray loads pending)
    bool pfc_valid = false;
    float4 pfc_o, pfc_d;
    pfc_o.x = 0.f; pfc_o.y = 0.f; pfc_o.z = 0.f; pfc_o.w = 0.f;
    pfc_d = pfc_o;
    auto drained = [&]() -> bool { return segs_left == 0 && !pfa_valid && !pfb_valid && !pfc_valid; };
    auto pin_state = [&]() {   // see uni(): keeps the bookkeeping in scalar registers
        seg = uni(seg); segs_left = uni(segs_left); ring_tail = uni(ring_tail); ring_head = uni(ring_head);
        pfa_seg = uni(pfa_seg); pfa_valid = uni(pfa_valid); pfb_n = uni(pfb_n); pfb_valid = uni(pfb_valid);
        pfc_n = uni(pfc_n); pfc_valid = uni(pfc_valid);
    };
    auto pump_consume = [&]() {
        // stage C -> ring: conservative per-primitive prefilter of the 64 rays that arrived, all lanes busy
        if (LIST) {
            // the candidates were collected by k_candidates: the ring carries the path id and its chunk word
            if (pfc_valid) {
                if ((uint32_t)lane < pfc_n) {
                    const uint32_t slot = (ring_tail + (uint32_t)lane) & (AGPT_RING - 1);
                    ring_pid[slot] = pfc_pid;
                    ring_mask[slot] = (unsigned long long)__float_as_uint(pfc_o.x);
                }
                ring_tail += pfc_n;
                pfc_valid = false;
                TS(ts_pref++;)
            }
        } else if (pfc_valid) {
            if ((uint32_t)lane < pfc_n) {
                const uint32_t npid = pfc_pid;
                float4 o = pfc_o;
                const float4 d = pfc_d;
                const TraceRay nr = make_trace_ray(V3(o.x, o.y, o.z), V3(d.x, d.y, d.z), coords_ok);
                unsigned long long skip_bit = 0;
                // (The decoding of a MIS query is written out three times -- here, at the hand-over below and in k_candidates -- and so
                // is the analytic loop further down, here and in k_candidates.  As functions of agpt_trace.h (results by reference, by
                // value in a struct, the test of one primitive alone) each form compiled these kernels to other code: other register
                // numbers and instruction order at best.)
                if (MIS) {   // MIS rays carry the sampled light's sphere (primitive index, ~0u = infinite light) in o.w; tmax = inf
                    const uint32_t shape = __float_as_uint(o.w);
                    o.w = AGPT_FLT_MAX;
                    if (shape != 0xFFFFFFFFu) {
                        v3 lc;
                        float lr2, ts;
                        light_sphere((int)shape, lc, lr2);
                        if (sphere_test_c(lc, lr2, nr, o.w, ts)) o.w = ts;
                        skip_bit = 1ull << shape;
                    }
                }
                const SlabRay sr = make_slab_ray(nr);
                // The records come through SCALAR loads (wave-uniform index, constant address space: scene arrays are
                // read-only for the whole launch, and only loads from that address space are selected as s_load without a
                // no-clobber proof), so the box coordinates are SGPR operands of the FMAs and the loads of several records
                // are in flight at once; reading the LDS copy made every iteration wait for its own two ds_reads.
                unsigned long long m = 0;
                typedef const float __attribute__((address_space(4))) ConstF;
                typedef const DevPrim __attribute__((address_space(4))) ConstPrim;
                ConstF* pf = (ConstF*)sc.prefilter;
                const int j0 = sc.pf_begin[0], j1 = sc.pf_begin[1];
#pragma unroll 4
                for (int j = j0; j < j1; ++j) {   // non-empty meshes: conservative slab test of the root box
                    ConstF* q = pf + 8 * j;   // (bmin.xyz, bit index), (bmax.xyz, -)
                    const bool h = conservative_slab(sr, q[0], q[1], q[2], q[4], q[5], q[6], o.w);
                    m |= (unsigned long long)(h ? 1u : 0u) << __float_as_uint(q[3]);
                }
                ConstPrim* pr = (ConstPrim*)sc.prims;
                for (unsigned long long am = sc.analytic_masks[0]; am; am &= am - 1) {   // spheres, planes: exact
                    const int k = __ffsll((long long)am) - 1;
                    ConstPrim& P = pr[k];
                    float root;
                    const bool sphere = P.type == AGPT_PRIM_SPHERE;
                    if (analytic_test(sphere ? 1.f : 3.f, V3(P.cx, P.cy, P.cz), sphere ? P.r2 : P.r, P.r2, nr, o.w, root)) m |= 1ull << k;
                }
                const uint32_t slot = (ring_tail + (uint32_t)lane) & (AGPT_RING - 1);
                ring_pid[slot] = npid;
                ring_mask[slot] = (nr.fast ? m : all_prims) & ~skip_bit;
            }
            ring_tail += pfc_n;
            pfc_valid = false;
            TS(ts_pref++;)
        }
        pin_state();
    };
    // Loads are issued for all 64 lanes (indices clamped to valid entries): exec-mask branches around them would make
    // the compiler's s_waitcnt placement conservative (vmcnt(0) at every merge).
    auto pump_issue = [&]() {
        // (1) everything that READS a value loaded earlier comes first ...
        const uint32_t last = count ? count - 1u : 0u;
        const bool adv_b = pfb_valid, adv_a = pfa_valid;
        uint32_t b_pid = pfb_pid, offv = pfa_off;
        const uint32_t b_n = pfb_n;
        // one unconditional touch of every register a pending load may still target: the waits for them land HERE on every
        // path (free in the steady state: those loads were issued a whole top-up ago), not behind the new loads below;
        // it also keeps the readfirstlane of the atomic's result from being hoisted up to the atomic
        asm volatile("" : "+v"(b_pid), "+v"(offv) : "v"(pfc_o.x), "v"(pfc_d.x));
        bool in_range = false;
        uint32_t base = 0, n_new = 0;
        if (adv_a) {   // the frontier atomic has returned: where is that chunk (or is the segment drained)?
            const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)offv);
            const uint32_t seg_begin = pfa_seg * seg_len;
            const uint32_t seg_end = seg_begin + seg_len < count ? seg_begin + seg_len : count;
            in_range = seg_begin < seg_end && off < seg_end - seg_begin;
            base = in_range ? seg_begin + off : 0u;
            n_new = in_range ? (seg_end - base < 64u ? seg_end - base : 64u) : 0u;
            if (!in_range && segs_left > 0) {
                --segs_left;
                seg = (seg + 1u) & (AGPT_FRONTIERS - 1u);
                // PEEK (launches over small batches, e.g. a rank's share of a split film): segments that other waves have drained
                // meanwhile are skipped after ONE look at all the frontiers (lane k reads frontier k, past the L1) instead of one
                // failing atomic each.  At the end of a launch every wave of the grid walks through all eight segments -- 5,120 x 8
                // same-line atomics at ~11 ns, ~56 us during which the launch only drains: 2.4 % of a rank's step at an 8-way
                // split of the 1080p film, 3.4 % at a 4-way one.  A frontier only grows: a stale value costs an atomic, never a
                // ray.  Not in the instantiation for full-size batches: the code costs the hot loop two registers and 1 ms per
                // 1080p/64spp step, more than the drain it saves there.
                if (PEEK && segs_left > 0) {
                    uint32_t head = 0;
                    if (lane < (int)AGPT_FRONTIERS) head = __hip_atomic_load(work_head + lane * AGPT_QSTRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const uint32_t fb = (uint32_t)lane * seg_len;
                    const bool live = lane < (int)AGPT_FRONTIERS && fb < count && head < (count - fb < seg_len ? count - fb : seg_len);
                    const uint32_t live_mask = (uint32_t)__ballot(live);
                    while (segs_left > 0 && !((live_mask >> seg) & 1u)) {
                        --segs_left;
                        seg = (seg + 1u) & (AGPT_FRONTIERS - 1u);
                    }
                }
            }
        }
        // (2) ... then the new loads, back to back, with no use of a loaded value in between: a merge of branches with
        // different numbers of outstanding loads makes the compiler wait with vmcnt(0), i.e. for the loads just issued
        if (adv_b) {   // B -> C: fetch the rays of the path ids that have arrived
            pfc_pid = b_pid;
            pfc_n = b_n;
            if (LIST) {
                pfc_o.x = __uint_as_float(cand_chunks[b_pid]);
            } else {
                pfc_o = ray_o[b_pid];
                pfc_d = ray_d[b_pid];
            }
            pfc_valid = true;
        }
        pfb_valid = false;
        if (adv_a) {   // A -> B: fetch that chunk's path ids
            uint32_t idx = base + (uint32_t)lane;
            idx = idx < last ? idx : last;
            pfb_pid = queue ? queue[idx] : idx;
            pfb_n = n_new;
            pfb_valid = in_range;
        }
        pfa_valid = false;
        if (segs_left > 0) {   // A: reserve the next 64 queue entries of the current segment
            if (lane == 0) pfa_off = atomicAdd(work_head + seg * AGPT_QSTRIDE, 64u);
            pfa_seg = seg;
            pfa_valid = true;
        }
        pin_state();
    };

    for (;;) {
        TCK(const unsigned long long tk_r0 = TCK_NOW();)
        pin_state();
        any_slow = uni(any_slow);
        // ---- parked lanes: emitter pass-through ----------------------------------------------------------------
        // integrator.h:152-161's re-cast of a ray that has hit a primitive without a material, made here, on the spot, in
        // k_shade's arithmetic, where the next vertex would do nothing else: the path is spared an iteration of five launches for
        // it, and the render the trail of near-empty iterations such paths used to leave (4 ms of a 1080p/64spp step).  The new
        // ray is a Scene::Intersect call of its own (counted), walks every primitive of the list, and k_shade finds it in
        // ext_o / ext_d.  A re-cast that would need the true-division slab test is left to k_shade: the hit is written after all.
        // (Out here, not in the retire branch of the vote loop, where the same code cost the loop four registers and 1 ms.)
        if constexpr (MODE == 0 && !LIST) {
            if (__ballot(cur == CUR_RECAST) != 0 && cur == CUR_RECAST) {
                const v3 p = r.O + rayt * r.D;
                const v3 nO = p + AGPT_EPSILON * r.D;
                const v3 nD = normalize(r.D);
                const TraceRay nr = make_trace_ray(nO, nD, coords_ok);
                if (nr.fast) {
                    const float kind = ray_d[pid].w;
                    if (kind == 2.f) {
                        // a camera ray (d.w = 2): the vertex first adds the emitter's radiance (integrator.h:139-147, bounces == 0;
                        // nothing of an earlier vertex is pending on it), then re-casts
                        const int al = sc.prims[hid & 0x7FFFFFFFu].arealight;
                        const v3 Le = al >= 0 ? V3(sc.lights[al].L[0], sc.lights[al].L[1], sc.lights[al].L[2]) : V3s(0.f);
                        const float4 b4 = path_beta4[pid];
                        float4 l4 = path_L4[pid];
                        const v3 L = V3(l4.x, l4.y, l4.z) + V3(b4.x, b4.y, b4.z) * Le;
                        l4.x = L.x; l4.y = L.y; l4.z = L.z;
                        path_L4[pid] = l4;
                    }
                    float4 no4, nd4;
                    no4.x = nO.x; no4.y = nO.y; no4.z = nO.z; no4.w = AGPT_FLT_MAX;
                    nd4.x = nD.x; nd4.y = nD.y; nd4.z = nD.z; nd4.w = kind;
                    ray_o[pid] = no4;
                    ray_d[pid] = nd4;
                    atomicAdd(&counters->closest_rays, 1ull);
                    r = nr;
                    rayt = AGPT_FLT_MAX;
                    hid = AGPT_HIT_MISS;
                    hb1 = 0.f;
                    hb2 = 0.f;
                    sp = 0;
                    mask = all_prims;
                    cur = pick_next(mask);
                } else {
                    store_hit(hits, pid, rayt, hid, hb1, hb2);
                    cur = CUR_IDLE;
                }
            }
        }
        // ---- refill ---------------------------------------------------------------------------------------
        unsigned long long act = __ballot(cur != CUR_IDLE);
        const int n_active0 = __popcll(act);
        if (n_active0 <= 64 - refill && !(drained() && ring_head == ring_tail)) {
            const uint32_t n_idle = (uint32_t)(64 - n_active0);
            // top the ring up: one pump_consume() per 64 rays in the steady state; a cold pipeline is pumped synchronously
            if (ring_tail - ring_head < n_idle && pfc_valid) pump_consume();
            while (ring_tail - ring_head < n_idle && !drained()) {
                pump_issue();
                pump_consume();
            }
            // hand ring entries to idle lanes (same wave wrote them: a wave barrier orders the LDS writes and reads)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t avail = ring_tail - ring_head;
            const uint32_t take = n_idle < avail ? n_idle : avail;
            if (cur == CUR_IDLE) {
                const uint32_t rank = (uint32_t)__popcll(~act & lt_mask);
                if (rank < take) {
                    const uint32_t slot = (ring_head + rank) & (AGPT_RING - 1);
                    pid = ring_pid[slot];
                    mask = ring_mask[slot];
                    if (LIST) {   // the ring word says which chunks hold candidates: start on the first of them
                        cvisit = (uint32_t)mask;
                        cchunk = 0;
                        mask = 0;
                        mmask = 0;
                        if (cvisit) enter_chunk((uint32_t)__ffs((int)cvisit) - 1u);
                    }
                    float4 o = ray_o[pid], d = ray_d[pid];
                    r = make_trace_ray(V3(o.x, o.y, o.z), V3(d.x, d.y, d.z), coords_ok);
                    rayt = o.w;
                    if (MIS) {   // (pump_consume's decoding once more, see there)
                        mis_area = false;
                        mis_skip = -1;
                        mis_reach = true;
                        const uint32_t shape = __float_as_uint(o.w);   // the sampled light's sphere, ~0u = infinite light
                        rayt = AGPT_FLT_MAX;
                        if (shape != 0xFFFFFFFFu) {
                            v3 lc;
                            float lr2, ts;
                            light_sphere((int)shape, lc, lr2);
                            mis_area = true;
                            mis_skip = (int)shape;
                            mis_reach = sphere_test_c(lc, lr2, r, rayt, ts);
                            if (mis_reach) rayt = ts;
                        }
                    }
                    hid = AGPT_HIT_MISS;
                    hb1 = 0.f;
                    hb2 = 0.f;
                    sp = 0;
                    cur = pick_next(mask);
                }
            }
            ring_head += take;
            TS(ts_refills++; ts_refilled += take;)
            if (!pfc_valid && !drained()) pump_issue();   // refill the emptied stage: nothing below waits for these loads
            act = __ballot(cur != CUR_IDLE);
            any_slow = __ballot(cur != CUR_IDLE && !r.fast) != 0;
        }
        TCK(tk_refill += TCK_NOW() - tk_r0;)
        if (act == 0) break;

        // ---- traversal round: vote scheduling -------------------------------------------------------------------
        // Each lane is in one of three states: A = at a sphere / plane of its candidate list or at the list's end, B = at
        // an interior node (or a mesh's root pair), C = at a leaf.  Every step the wave executes the body most lanes are
        // waiting for; a lane's own sequence of operations is the reference's, only the interleaving between lanes
        // changes.  (A while-while loop makes every lane wait for the longest descent in the wave: 37 % active lanes.)
        for (;;) {
            TCK(const unsigned long long tk_v0 = TCK_NOW();)
            // (the counts as 32-bit words in scalar registers, see uni_word(): as the 64-bit popcounts they were, the majority tests
            // below ran as 64-bit compares on the vector unit)
            const uint32_t nA = uni_word((uint32_t)__popcll(__ballot(LIST ? cur - CUR_FETCH < 2u : cur == CUR_PICK))),
                           nB = uni_word((uint32_t)__popcll(__ballot(cur < CUR_B_END))), nC = uni_word((uint32_t)__popcll(__ballot((int32_t)cur < 0)));
            const uint32_t n_active = nA + nB + nC, n_refill = (uint32_t)(64 - refill);   // (refill is 1..64)
            if (n_active == 0 || (n_active <= n_refill && !(drained() && ring_head == ring_tail))) break;
            // (nothing left to refill with: lanes parked for a re-cast would wait for the last active lane of the wave)
            if (MODE == 0 && !LIST && n_active <= n_refill && __ballot(cur == CUR_RECAST) != 0) break;
            TCK(const unsigned long long tk_v1 = TCK_NOW(); tk_vote += tk_v1 - tk_v0;)
            TS(ts_act += (unsigned long long)n_active; if (!(nB >= nA && nB >= nC) && !(nC >= nA)) { ts_steps[0]++; ts_lanes[0] += nA; })
            // The three bodies stand one after the other, each behind a flag of its own that the compiler cannot relate to the other two
            // (exactly one is set).  As an if / else-if chain the bodies were laid out as alternatives that meet again behind
            // the last one: the state a body writes (cur, sp, mask; rayt and the hit record in C) and the state the next
            // alternative reads were then live side by side, in two sets of registers, and every round copied one into the other
            // at the entry of its body and back at the loop's end.  In sequence each body updates the one set in place.
            // (The flags in integer arithmetic -- counts of at most 64: a difference's sign bit is "less than" -- which stays on the scalar unit;
            // a flag made from a comparison's result goes through a lane mask and a vector select.)
            const uint32_t nAC = nA > nC ? nA : nC;
            const uint32_t do_b = uni_word(1u ^ ((nB - nAC) >> 31));                 // nB >= nA && nB >= nC
            const uint32_t do_c = uni_word((1u ^ do_b) & (1u ^ ((nC - nA) >> 31)));   // else nC >= nA
            const uint32_t do_a = uni_word(1u ^ (do_b | do_c));
            if (do_b) {
                asm volatile("");   // (keeps the flag a scalar branch of its own: folded into the lanes' own test it costs a v_cmp in every round)
                TS(ts_steps[1]++; ts_lanes[1] += nB;)
                if constexpr (COH) {
                    // the step below, once per record source: `np` is the pair record, in SGPRs on the scalar path
                    auto interior = [&](const NodePair& np) {
                        float dl, dr;
                        bool hl, hr;
                        const uint32_t encl = __float_as_uint(np.n3.x), encr = __float_as_uint(np.n3.y);
                        pair_boxes_fast(np, r, rayt, hl, hr, dl, dr);
                        if (any_slow) {
                            if (!r.fast) pair_boxes_exact(np, r, rayt, hl, hr, dl, dr);
                        }
                        TS(if (cur >= rootpair_base) { ts_root++; ts_root_pass += hl ? 1u : 0u; })
                        hr = hr && cur < rootpair_base;
                        if (hl && hr) {
                            const bool swap = dr < dl;
                            stack_push(sp, swap ? encl : encr);
                            sp++;
                            TS(ts_push[0]++; ts_push[1] += sp > 4; ts_push[2] += sp > 6; ts_push[3] += sp > 8; ts_push[4] += sp > 12;)
                            cur = swap ? encr : encl;
                        } else if (hl) {
                            cur = encl;
                        } else if (hr) {
                            cur = encr;
                        } else if (sp == 0) {
                            cur = pick_next(mask);
                        } else {
                            sp--;
                            cur = stack_at(sp);
                        }
                    };
                    const bool in_b = cur < CUR_B_END;
                    const uint32_t u = (uint32_t)__builtin_amdgcn_readlane((int)cur, __ffsll((long long)__ballot(in_b)) - 1);
                    if (__ballot(in_b && cur != u) == 0) {
                        // every voting lane stands at pair u: one 64-byte scalar fetch for the wave (the constant address space, as
                        // for the prefilter records in pump_consume)
                        TS(ts_usteps[0]++; ts_ulanes[0] += nB;)
                        typedef const float __attribute__((address_space(4))) ConstF;
                        ConstF* q = (ConstF*)sc.nodes + 8 * (size_t)u;
                        NodePair np;
                        np.n0.x = q[0]; np.n0.y = q[1]; np.n0.z = q[2]; np.n0.w = q[3];
                        np.n1.x = q[4]; np.n1.y = q[5]; np.n1.z = q[6]; np.n1.w = q[7];
                        np.n2.x = q[8]; np.n2.y = q[9]; np.n2.z = q[10]; np.n2.w = q[11];
                        np.n3.x = q[12]; np.n3.y = q[13]; np.n3.z = q[14]; np.n3.w = q[15];
                        // (one batch of loads and one wait: left to itself the compiler fetches the child encodings by a second load
                        // where they are first used, behind the box arithmetic)
                        asm volatile("" : "+s"(np.n0.x), "+s"(np.n0.y), "+s"(np.n0.z), "+s"(np.n0.w), "+s"(np.n1.x), "+s"(np.n1.y), "+s"(np.n1.z),
                                     "+s"(np.n1.w), "+s"(np.n2.x), "+s"(np.n2.y), "+s"(np.n2.z), "+s"(np.n2.w), "+s"(np.n3.x), "+s"(np.n3.y));
                        if (in_b) interior(np);
                    } else if (in_b) {
                        __builtin_amdgcn_s_setprio(1);
                        const NodePair np = load_pair(sc, cur);
                        asm volatile("" ::: "memory");
                        __builtin_amdgcn_s_setprio(0);
                        interior(np);
                    }
                } else if (cur < CUR_B_END) {
                    // the wave is about to wait for these loads whatever happens: let its issue win the arbitration against
                    // waves in the middle of their arithmetic (-1.5 ms per C3 step on the closest-hit and MIS launches; the
                    // short any-hit steps lose 0.3 ms with it)
                    if (MODE != 1) __builtin_amdgcn_s_setprio(1);
                    const NodePair np = load_pair(sc, cur);
                    if (MODE != 1) {
                        asm volatile("" ::: "memory");
                        __builtin_amdgcn_s_setprio(0);
                    }
                    TCK(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); tk_bmem += TCK_NOW() - tk_v1;)
                    float dl, dr;
                    bool hl, hr;
                    const uint32_t encl = __float_as_uint(np.n3.x), encr = __float_as_uint(np.n3.y);
                    pair_boxes_fast(np, r, rayt, hl, hr, dl, dr);
                    if (any_slow) {  // scalar branch: rays outside the Markstein divide's domain, agpt_trace.h (true divisions)
                        if (!r.fast) pair_boxes_exact(np, r, rayt, hl, hr, dl, dr);
                    }
                    if (COUNT) {   // the first record of a mesh is its root test, whichever record the lane entered at
                        if (at_entry) c_root++; else c_int++;
                        at_entry = false;
                    }
                    TS(if (cur >= rootpair_base) { ts_root++; ts_root_pass += hl ? 1u : 0u; })
                    hr = hr && cur < rootpair_base;   // a root pair has no right child
                    if (hl && hr) {
                        bool swap = ANY ? false : (dr < dl);
                        stack_push(sp, swap ? encl : encr);
                        sp++;
                        TS(ts_push[0]++; ts_push[1] += sp > 4; ts_push[2] += sp > 6; ts_push[3] += sp > 8; ts_push[4] += sp > 12;)
                        cur = swap ? encr : encl;
                    } else if (hl) {
                        cur = encl;
                    } else if (hr) {
                        cur = encr;
                    // (Pop the stack or pick_next: written out again at the end of the leaf step below, the second copy.  As one
                    // lambda -- [&] on sp / cur / mask, by reference or by value -- it changed every k_trace_fast instantiation.)
                    } else if (sp == 0) {
                        cur = pick_next(mask);
                    } else {
                        sp--;
                        cur = stack_at(sp);
                    }
                }
                TCK(asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); tk_balu += TCK_NOW() - tk_v1;)
                if (LIST) continue;   // (the long-list instantiations keep the layout as alternatives: in sequence they need up to three registers more)
            }
            if (do_c) {
                asm volatile("");
                TS(ts_steps[2]++; ts_lanes[2] += nC;)
                const bool in_c = (int32_t)cur < 0;
                bool same_leaf = false;
                uint32_t u = 0;
                if constexpr (COH) {
                    u = (uint32_t)__builtin_amdgcn_readlane((int)cur, __ffsll((long long)__ballot(in_c)) - 1);
                    same_leaf = __ballot(in_c && cur != u) == 0;
                }
                if (COH && same_leaf) {
                    // every voting lane stands at leaf u: its range and its triangle records come through scalar loads
                    TS(ts_usteps[1]++; ts_ulanes[1] += nC;)
                    typedef const float __attribute__((address_space(4))) ConstF;
                    typedef const uint32_t __attribute__((address_space(4))) ConstU;
                    uint32_t first, cnt;   // (leaf_range on the wave's value)
                    if ((u & AGPT_ENC_BIGLEAF) == AGPT_ENC_BIGLEAF) {
                        ConstU* bl = (ConstU*)sc.bigleaves + 2 * (size_t)(u & 0x0FFFFFFFu);
                        first = bl[0];
                        cnt = bl[1];
                    } else {
                        first = u & 0x0FFFFFFFu;
                        cnt = ((u >> 28) & 7u) + 1u;
                    }
                    if (in_c) {
                        for (uint32_t i = 0; i < cnt; ++i) {
                            ConstF* tp = (ConstF*)sc.tri_verts + 12 * (size_t)(first + i);
                            const v3 q0 = V3(tp[0], tp[1], tp[2]), q1 = V3(tp[4], tp[5], tp[6]), q2 = V3(tp[8], tp[9], tp[10]);
                            const uint32_t q_id = __float_as_uint(tp[3]), q_flags = __float_as_uint(tp[7]);
                            float t, b1, b2;
                            if (tri_test(q0, q1, q2, r, rayt, t, b1, b2)) {
                                if (!(q_flags & AGPT_TRI_FLAG_REJECT)) {
                                    rayt = t;
                                    hid = q_id;
                                    hb1 = b1;
                                    hb2 = b2;
                                }
                            }
                        }
                        if (sp == 0) {
                            cur = pick_next(mask);
                        } else {
                            sp--;
                            cur = stack_at(sp);
                        }
                    }
                } else if ((int32_t)cur < 0) {
                    uint32_t first, cnt;
                    leaf_range(sc, cur, first, cnt);
                    bool done = false;
                    for (uint32_t i = 0; i < cnt; ++i) {
                        const float4* tp = sc.tri_verts + 3 * (size_t)(first + i);
                        const float4 a = tp[0], b = tp[1], c = tp[2];
                        const v3 q0 = V3(a.x, a.y, a.z), q1 = V3(b.x, b.y, b.z), q2 = V3(c.x, c.y, c.z);
                        const uint32_t q_id = __float_as_uint(a.w), q_flags = __float_as_uint(b.w);
                        float t, b1, b2;
                        if (COUNT) c_tri++;
                        if (tri_test(q0, q1, q2, r, rayt, t, b1, b2)) {
                            if (MIS) {
                                if (!(q_flags & AGPT_TRI_FLAG_REJECT)) {
                                    done = true;
                                    break;
                                }
                            } else if (ANY) {
                                done = true;
                                break;
                            } else if (!(q_flags & AGPT_TRI_FLAG_REJECT)) {
                                rayt = t;
                                hid = q_id;
                                hb1 = b1;
                                hb2 = b2;
                            }
                        }
                    }
                    if (ANY && done) {
                        occluded[pid] = MIS ? 0u : 1u;   // MODE 2 writes "ok" (1 = add the BSDF-leg contribution)
                        cur = CUR_IDLE;
                    } else if (sp == 0) {   // (the interior step's pop or pick_next, the other copy, see there)
                        cur = pick_next(mask);
                    } else {
                        sp--;
                        cur = stack_at(sp);
                    }
                }
                TCK(asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); tk_c += TCK_NOW() - tk_v1;)
                if (LIST) continue;
            }
            if (!do_a) continue;
            asm volatile("");
            if (LIST && cur == CUR_FETCH) {
                // the next chunk that holds candidates of this ray (one dependent load; list steps are rare)
                enter_chunk((uint32_t)__ffs((int)cvisit) - 1u);
                cur = pick_next(mask);
                TCK(asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); tk_a += TCK_NOW() - tk_v1;)
            } else if (cur == CUR_PICK) {
                // end of the primitive list (retire), or the sphere / plane that is next in list order
                if (mask == 0) {
                    bool recast = false;
                    if (MIS) {
                        occluded[pid] = mis_reach ? 1u : 0u;
                    } else if (ANY) {
                        occluded[pid] = 0u;
                    } else {
                        // A closest hit on a primitive without a material (an emitter's sphere), on a ray whose next vertex would
                        // do nothing but re-cast it (d.w = 1, set by k_shade): the lane is parked for the re-cast at the top of the
                        // outer loop instead of retiring.
                        if (!LIST && recast_on && hid != AGPT_HIT_MISS && (hid & AGPT_HIT_SPHERE))
                            recast = s_prim[2 * (hid & 0x7FFFFFFFu) + 1].z != 0.f && ray_d[pid].w != 0.f;
                        if (!recast) store_hit(hits, pid, rayt, hid, hb1, hb2);
                    }
                    cur = recast ? CUR_RECAST : CUR_IDLE;
                } else {
                    const int k = (LIST ? 64 * (int)cchunk : 0) + __ffsll((long long)mask) - 1;   // list index
                    mask &= mask - 1;
                    float4 pa, pb2;
                    // (The long-list instantiation forms the fields it needs of the record staged at the kernel's top, the other copy:
                    // one function for both, by reference or by value, compiled the short-list instantiations to other code.)
                    if (!PRIM_LDS) {
                        const DevPrim& P = sc.prims[k];
                        const bool sphere = P.type == AGPT_PRIM_SPHERE;
                        pa.x = P.cx; pa.y = P.cy; pa.z = P.cz; pa.w = sphere ? 1.f : (P.type == AGPT_PRIM_PLANE ? 3.f : 2.f);
                        pb2.x = sphere ? P.r2 : P.r; pb2.y = sphere ? 0.f : P.r2; pb2.z = 0.f; pb2.w = 0.f;
                    } else {
                        pa = s_prim[2 * k];
                        pb2 = s_prim[2 * k + 1];
                    }
                    if (pa.w == 1.f || pa.w == 3.f) {
                        float root;
                        if (analytic_test(pa.w, V3(pa.x, pa.y, pa.z), pb2.x, pb2.y, r, rayt, root)) {
                            if (MIS) {
                                // a sphere listed before the light's sphere only wins a strict comparison (see above)
                                const bool tie_loses = pa.w == 1.f && mis_area && mis_reach && k < mis_skip && root == rayt;
                                if (!tie_loses) {
                                    occluded[pid] = 0u;
                                    cur = CUR_IDLE;
                                }
                            } else if (ANY) {
                                occluded[pid] = 1u;
                                cur = CUR_IDLE;
                            } else {
                                rayt = root;
                                hid = AGPT_HIT_SPHERE | (uint32_t)k;
                                hb1 = 0.f;
                                hb2 = 0.f;
                            }
                        }
                    }
                    if (cur == CUR_PICK) cur = pick_next(mask);   // (meshes never get here: pick_next routes them to B)
                }
                TCK(asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); tk_a += TCK_NOW() - tk_v1;)
            }
        }
    }
    // (stats build: the coherent launch keeps its own set of slots, mode "3")
    TS(constexpr int TS_BASE = COH ? AGPT_DBG_COH : 16 * MODE;)
    TS(if (lane == 0) {
        unsigned long long* d = counters->dbg + TS_BASE;
        if (COH) for (int k = 0; k < 2; ++k) { atomicAdd(d + 16 + k, ts_usteps[k]); atomicAdd(d + 18 + k, ts_ulanes[k]); }
        for (int k = 0; k < 3; ++k) { atomicAdd(d + k, ts_steps[k]); atomicAdd(d + 3 + k, ts_lanes[k]); }
        atomicAdd(d + 6, ts_act); atomicAdd(d + 7, ts_refills); atomicAdd(d + 8, ts_refilled); atomicAdd(d + 9, ts_pref);
    })
#if defined(AGPT_TRACE_STATS) && !defined(AGPT_TRACE_CLOCK)
    {   // stack-depth histogram of the pushes (per lane; slots 10..14 are the phase clocks' in the clock build)
        unsigned long long* d = counters->dbg + TS_BASE;
        for (int k = 0; k < 5; ++k) {
            uint32_t v = ts_push[k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
            if (lane == 0) atomicAdd(d + 10 + k, (unsigned long long)v);
        }
        // root-pair steps (slot 15) and the passing ones (AGPT_DBG_ROOT_PASS): what entering at the child pair saves, counted with AGPT_ROOT_STEP=1
        for (int off = 32; off > 0; off >>= 1) { ts_root += __shfl_down(ts_root, off); ts_root_pass += __shfl_down(ts_root_pass, off); }
        if (lane == 0) {
            atomicAdd(d + 15, (unsigned long long)ts_root);
            atomicAdd(counters->dbg + AGPT_DBG_ROOT_PASS + (COH ? 3 : MODE), (unsigned long long)ts_root_pass);
        }
    }
#endif
    TS(if (lane == 0) {
        unsigned long long* d = counters->dbg + TS_BASE;
        TCK(atomicAdd(d + 10, tk_refill); atomicAdd(d + 11, tk_vote); atomicAdd(d + 12, tk_bmem); atomicAdd(d + 13, tk_balu);
            atomicAdd(d + 14, tk_c); atomicAdd(d + 15, tk_a); atomicAdd(counters->dbg + 48 + (COH ? 3 : MODE), TCK_NOW() - tk_begin);)
    })
    if (COUNT) {   // (k_trace's flush, the other copy, see there; here in the order interior, roots, tris)
        for (int off = 32; off > 0; off >>= 1) {
            c_int += __shfl_down(c_int, off);
            c_root += __shfl_down(c_root, off);
            c_tri += __shfl_down(c_tri, off);
        }
        if (lane == 0) {
            atomicAdd(&counters->interior, (unsigned long long)c_int);
            atomicAdd(&counters->roots, (unsigned long long)c_root);
            atomicAdd(&counters->tris, (unsigned long long)c_tri);
        }
    }
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (MODE == 1)
            atomicAdd(&counters->anyhit_rays, (unsigned long long)count);
        else
            atomicAdd(&counters->closest_rays, (unsigned long long)count);   // MIS queries are Scene::Intersect calls
    }
}

// ---------------------------------------------------------------------------------------------------------
// Top-level structure over Scene::primitives (scene.h:5-19) for lists longer than 64 entries: one thread per ray walks the
// tree over the meshes' root boxes (agpt_scene.h: depth-first order with skip links, so the walk needs no stack -- hit ->
// next node, miss -> past the subtree) with the conservative slab test of the short-list prefilter, tests the spheres and
// planes exactly, and leaves the ray's candidates as one 64-bit word per chunk of 64 primitives (cand_mask[chunk * stride +
// path]) plus the set of non-empty chunks (cand_chunks[path]).  The candidates are a superset of the primitives the
// reference's list walk can hit at the ray's initial t; k_trace_fast<LIST> visits them in list order and re-runs the exact
// root-box test where the reference runs it.  No LDS besides the per-thread words and few registers: the dependent loads of
// the walk are hidden by occupancy, which the traversal kernel (5 waves per SIMD) could not do (a per-lane tree walk inside
// its prefilter measured 15 % slower than the per-primitive loop).
static_assert(AGPT_MAX_CHUNKS <= 32, "k_trace_fast<LIST> and k_candidates keep the chunks still to visit in one 32-bit word per ray");
#define AGPT_CAND_LIST 24   // mesh candidates a thread of k_candidates collects before it gives up and marks every primitive
template <int MODE>
__global__ void __launch_bounds__(AGPT_BLOCK)
k_candidates(DevScene sc, const uint32_t* __restrict__ queue, const uint32_t* __restrict__ count_ptr, uint32_t count_imm,
             const float4* __restrict__ ray_o, const float4* __restrict__ ray_d, unsigned long long* __restrict__ cand_mask,
             uint32_t* __restrict__ cand_chunks, uint32_t cand_stride) {
    constexpr bool MIS = MODE == 2;
    // the meshes the walk finds, as list indices, one column per thread (12 KiB per block: the register count, not LDS,
    // bounds the occupancy); a ray with more than AGPT_CAND_LIST of them gets every primitive as candidate -- any superset
    // of the true candidates is valid, the traversal re-tests each root box exactly
    __shared__ uint16_t s_list[AGPT_CAND_LIST][AGPT_BLOCK];
    const uint32_t count = count_ptr ? *count_ptr : count_imm;
    const int n_chunks = (sc.n_prims + 63) / 64;
    const int tid = threadIdx.x;
    const bool coords_ok = sc.mdiv_coords_ok != 0;
    for (uint32_t i = blockIdx.x * AGPT_BLOCK + tid; i < count; i += gridDim.x * AGPT_BLOCK) {
        const uint32_t pid = queue ? queue[i] : i;
        float4 o = ray_o[pid];
        const float4 d = ray_d[pid];
        const TraceRay nr = make_trace_ray(V3(o.x, o.y, o.z), V3(d.x, d.y, d.z), coords_ok);
        uint32_t skip = 0xFFFFFFFFu;
        if (MIS) {   // k_trace_fast's decoding (pump_consume; why it is a copy is said there): the sampled light's sphere in o.w, tmax = inf
            const uint32_t shape = __float_as_uint(o.w);
            o.w = AGPT_FLT_MAX;
            if (shape != 0xFFFFFFFFu) {
                const DevPrim& L = sc.prims[shape];
                float ts;
                if (sphere_test_c(V3(L.cx, L.cy, L.cz), L.r2, nr, o.w, ts)) o.w = ts;
                skip = shape;   // never a blocker itself
            }
        }
        int n_found = 0;
        bool all = !nr.fast;   // outside the Markstein divide's domain (agpt_trace.h): the conservative form does not hold
        if (!all) {
            const SlabRay sr = make_slab_ray(nr);
            uint32_t k = 0;
            const uint32_t k_end = (uint32_t)sc.n_toplevel;
            while (k < k_end) {
                const uint4 nd = sc.toplevel[k];   // six halves (box rounded outward) + skip | leaf << 16
                auto h2f = [](uint32_t bits16) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16); };
                const float lox = h2f(nd.x & 0xFFFFu), loy = h2f(nd.x >> 16), loz = h2f(nd.y & 0xFFFFu);
                const float hix = h2f(nd.y >> 16), hiy = h2f(nd.z & 0xFFFFu), hiz = h2f(nd.z >> 16);
                const bool h = conservative_slab(sr, lox, loy, loz, hix, hiy, hiz, o.w);
                const uint32_t prim = nd.w >> 16;
                if (h && prim != 0xFFFFu) {
                    if (n_found < AGPT_CAND_LIST) s_list[n_found][tid] = (uint16_t)prim;
                    n_found++;
                }
                k = h ? k + 1u : (nd.w & 0xFFFFu);
            }
            all = n_found > AGPT_CAND_LIST;
        }
        uint32_t chunks = 0;
        for (int c = 0; c < n_chunks; ++c) {
            unsigned long long m;
            if (all) {
                const int n_here = sc.n_prims - 64 * c < 64 ? sc.n_prims - 64 * c : 64;
                m = n_here >= 64 ? ~0ull : ((1ull << n_here) - 1ull);
            } else {
                m = 0;
                for (int j = 0; j < n_found; ++j) {
                    const uint32_t prim = s_list[j][tid];
                    if ((int)(prim >> 6) == c) m |= 1ull << (prim & 63u);
                }
                for (unsigned long long am = sc.analytic_masks[c]; am; am &= am - 1) {   // spheres, planes: exact -- pump_consume's loop (k_trace_fast; a copy, see there)
                    const int b = __ffsll((long long)am) - 1;
                    const DevPrim& P = sc.prims[64 * c + b];
                    float root;
                    const bool sphere = P.type == AGPT_PRIM_SPHERE;
                    if (analytic_test(sphere ? 1.f : 3.f, V3(P.cx, P.cy, P.cz), sphere ? P.r2 : P.r, P.r2, nr, o.w, root)) m |= 1ull << b;
                }
            }
            if (MIS && (int)(skip >> 6) == c) m &= ~(1ull << (skip & 63u));
            cand_mask[(size_t)c * cand_stride + pid] = m;
            chunks |= (m ? 1u : 0u) << c;
        }
        cand_chunks[pid] = chunks;
    }
}
