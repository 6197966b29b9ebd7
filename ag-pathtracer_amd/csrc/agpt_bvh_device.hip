// agpt_bvh_device.hip -- build_bvh (agpt_host_scene.cpp) on the GPU, byte for byte.  The box, the SAH decision, a triangle's box and
// centroid and the union of a child pair are SHARED with the host builder (agpt_bvh_arith.h); what differs is how the work is spread.
//
// Work tiers (thresholds in include/agpt.h):
//   big nodes   (n > AGPT_BVH_DEVICE_LANE_MAX)  level by level; every node is cut into chunks of AGPT_BVH_DEVICE_CHUNK
//                                               primitives, one 64-lane block per chunk, so the top of the tree uses the
//                                               whole GPU.  Per level: bounds, split axis, binning, SAH decision (one lane
//                                               per node), rank-based partition.
//   lane nodes  (n <= AGPT_BVH_DEVICE_LANE_MAX) one lane runs the host algorithm on the whole subtree.
// A last pass sums subtree sizes, hands out the pre-order pair slots (SubTree/embed's rule) and unions interior bounds.
//
// Exactness.  tminf/tmaxf folds keep the later of equal operands, so a fold's result is "the extreme value, taken from the
// last position holding it" (this only matters for +0.0 vs -0.0).  Every fold here reduces 64-bit keys
// (order-preserving value bits with -0 == +0, position) with integer min/max -- commutative and exact in any order, also
// as atomics -- and reads the winning position's value back.  The initial +-kBoxEmpty of Box() is position 0.
// Partition: std::partition (libstdc++, bidirectional) swaps the i-th non-matching primitive from the left with the i-th
// matching one from the right; with m matching primitives that is "rank the non-matching ones of [start, start+m) from
// the left, the matching ones of [start+m, end) from the right, swap equal ranks".
#include "agpt_bvh_device.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "agpt_bvh_arith.h"
#include "agpt_host_scene.hpp"

namespace agpt {
int fail(int code, const std::string& msg);   // agpt_api.hip: the message of agpt_last_error
}

namespace {

using namespace agpt;  // agpt_bvh_arith.h

typedef unsigned long long u64;

constexpr int kLaneMax = AGPT_BVH_DEVICE_LANE_MAX;
constexpr int kChunk = AGPT_BVH_DEVICE_CHUNK;
constexpr int kWave = 64;
static_assert(kLaneMax >= 2, "big nodes must not reach the n <= 2 rule");
static_assert(kChunk % kWave == 0, "");

// ---- per-triangle data: A = (lo.xyz, c.x), B = (hi.xyz, c.y), C = c.z -------------------------------------------------
struct Tris {
    const float4* A;
    const float4* B;
    const float* C;
    __device__ float comp(int t, int q) const {  // q: 0-2 lo, 3-5 hi, 6-8 centroid
        switch (q) {
            case 0: return A[t].x;
            case 1: return A[t].y;
            case 2: return A[t].z;
            case 3: return B[t].x;
            case 4: return B[t].y;
            case 5: return B[t].z;
            case 6: return A[t].w;
            case 7: return B[t].w;
            default: return C[t];
        }
    }
    __device__ float cent(int t, int axis) const { return comp(t, 6 + axis); }
    __device__ Box box(int t) const {
        const float4 a = A[t], b = B[t];
        Box r;
        r.lo[0] = a.x, r.lo[1] = a.y, r.lo[2] = a.z;
        r.hi[0] = b.x, r.hi[1] = b.y, r.hi[2] = b.z;
        return r;
    }
};

// ---- fold keys -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ord_bits(float v) {  // monotone in v, -0 and +0 equal
    uint32_t b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// pos1 = array position + 1 (0 = the fold's initial value); min: smallest value, then latest position; max: largest, latest
__device__ __forceinline__ u64 kmin(float v, uint32_t pos1) { return ((u64)ord_bits(v) << 32) | (u64)(0xFFFFFFFFu - pos1); }
__device__ __forceinline__ u64 kmax(float v, uint32_t pos1) { return ((u64)ord_bits(v) << 32) | (u64)pos1; }
__device__ __forceinline__ u64 umin64(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
    const int lo = __shfl_xor((int)(uint32_t)v, m, kWave);
    const int hi = __shfl_xor((int)(uint32_t)(v >> 32), m, kWave);
    return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}

// ---- records ---------------------------------------------------------------------------------------------------------
enum { REC_OPEN = 0, REC_INTERIOR = 1, REC_LEAF = 2, REC_LANE = 3 };
struct Rec {             // one per node the level passes create (big nodes and lane subtrees)
    int start, n, depth, kind;
    int left;            // interior: record of the left child, the right one is left + 1
    int total;           // nodes in the subtree
    int slot, base;      // output slot, first pair slot of the subtree's children (pre-order)
    float lo[3], hi[3];  // the node's bounds as written to the output
};
struct Lvl {             // a big node of the current level
    int rec, blk_first, nblk, act;  // act: 1 = binned and split this level
    int axis, split, m, k;          // split bucket, primitives on the left, swaps of the partition
    Box bounds, cb;
};
struct Ctr {
    int blocks, next_cnt;  // reset per level (adjacent: one memset)
    int records, lane_cnt, max_depth, overflow, nonfinite;
    uint32_t ext[6];       // ord_bits of min lo.xyz, max hi.xyz over all triangles
};
struct Bufs {
    Tris tr;
    int* perm;
    uint8_t* bucket;
    int *posL, *posR;
    int4* stk;
    agpt_bvh_node *scr, *out;
    Rec* recs;
    int* lane_ids;
    Lvl* lv;
    u64 *keys, *binkeys;
    int* bincnt;
    int *blk_node;
    int2 *blk_cnt, *blk_off;
    Ctr* ctr;
    int n, rec_cap, lvl_cap, blk_cap, max_prims;
};

// the initial keys of a fold (Box()'s values at position 0) and the value a folded key stands for
__device__ __forceinline__ u64 kmin0() { return kmin(kBoxEmpty, 0); }
__device__ __forceinline__ u64 kmax0() { return kmax(-kBoxEmpty, 0); }
__device__ __forceinline__ float key_value(const Bufs& B, u64 k, bool is_min, int q) {
    const uint32_t lo = (uint32_t)k;
    const uint32_t pos1 = is_min ? 0xFFFFFFFFu - lo : lo;
    return pos1 == 0 ? (is_min ? kBoxEmpty : -kBoxEmpty) : B.tr.comp(B.perm[pos1 - 1], q);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------
__global__ void k_prep(Bufs B, const float* __restrict__ V, const int32_t* __restrict__ I) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0, 0, 0};
    if (t < B.n) {
        v3 p[3];
        for (int k = 0; k < 3; k++) {
            const int v = I[(size_t)9 * t + 3 * k];
            p[k] = V3(V[(size_t)3 * v], V[(size_t)3 * v + 1], V[(size_t)3 * v + 2]);
            bad |= !__builtin_isfinite(p[k].x) || !__builtin_isfinite(p[k].y) || !__builtin_isfinite(p[k].z);
        }
        float c[3];
        const Box b = tri_box(p[0], p[1], p[2], c);
        for (int a = 0; a < 3; a++) {
            bad |= !__builtin_isfinite(c[a]);
            mn[a] = ord_bits(b.lo[a]);
            mx[a] = ord_bits(b.hi[a]);
        }
        float4* A = const_cast<float4*>(B.tr.A);
        float4* Bb = const_cast<float4*>(B.tr.B);
        A[t] = make_float4(b.lo[0], b.lo[1], b.lo[2], c[0]);
        Bb[t] = make_float4(b.hi[0], b.hi[1], b.hi[2], c[1]);
        const_cast<float*>(B.tr.C)[t] = c[2];
        B.perm[t] = t;
    }
    for (int m = 1; m < kWave; m <<= 1)
        for (int a = 0; a < 3; a++) {
            mn[a] = min(mn[a], (uint32_t)__shfl_xor((int)mn[a], m, kWave));
            mx[a] = max(mx[a], (uint32_t)__shfl_xor((int)mx[a], m, kWave));
        }
    if (__ballot(bad) != 0 && (threadIdx.x & (kWave - 1)) == 0) atomicOr(&B.ctr->nonfinite, 1);
    if ((threadIdx.x & (kWave - 1)) == 0)
        for (int a = 0; a < 3; a++) {
            atomicMin(&B.ctr->ext[a], mn[a]);
            atomicMax(&B.ctr->ext[3 + a], mx[a]);
        }
}

__global__ void k_init_root(Bufs B) {
    Rec& r = B.recs[0];
    r.start = 0;
    r.n = B.n;
    r.depth = 0;
    r.kind = B.n > kLaneMax ? REC_OPEN : REC_LANE;
    r.left = -1;
    r.total = 0;
    r.slot = 0;
    r.base = 2;
    B.ctr->records = 1;
    B.ctr->lane_cnt = B.n > kLaneMax ? 0 : 1;
    B.lane_ids[0] = 0;
}

// one lane per big node of the level: blocks, key and bin initial values
__global__ void k_level_setup(Bufs B, const int* __restrict__ ids, int cnt) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt) return;
    Lvl& L = B.lv[j];
    L.rec = ids[j];
    const int n = B.recs[L.rec].n;
    const int nb = (n + kChunk - 1) / kChunk;
    const int first = atomicAdd(&B.ctr->blocks, nb);
    L.blk_first = first;
    L.nblk = nb;
    L.act = 0;
    if (first + nb > B.blk_cap) {
        atomicOr(&B.ctr->overflow, 1);
        return;
    }
    for (int b = 0; b < nb; b++) B.blk_node[first + b] = j;
    const u64 imin = kmin0(), imax = kmax0();
    for (int a = 0; a < 3; a++) {
        B.keys[(size_t)j * 12 + a] = imin;
        B.keys[(size_t)j * 12 + 3 + a] = imax;
        B.keys[(size_t)j * 12 + 6 + a] = imin;
        B.keys[(size_t)j * 12 + 9 + a] = imax;
    }
    for (int b = 0; b < kBuckets; b++) {
        B.bincnt[(size_t)j * kBuckets + b] = 0;
        for (int a = 0; a < 3; a++) {
            B.binkeys[((size_t)j * kBuckets + b) * 6 + a] = imin;
            B.binkeys[((size_t)j * kBuckets + b) * 6 + 3 + a] = imax;
        }
    }
}

// block -> (level node, primitive range); false for the blocks past the level's count
__device__ __forceinline__ bool block_range(const Bufs& B, int& j, int& lo, int& hi, int& chunk) {
    const int b = blockIdx.x;
    if (b >= min(B.ctr->blocks, B.blk_cap) || B.ctr->overflow) return false;
    j = B.blk_node[b];
    const Lvl& L = B.lv[j];
    const Rec& r = B.recs[L.rec];
    chunk = b - L.blk_first;
    lo = r.start + chunk * kChunk;
    hi = min(r.start + r.n, lo + kChunk);
    return true;
}

// node bounds and centroid bounds
__global__ void __launch_bounds__(kWave) k_bounds(Bufs B) {
    int j, lo, hi, chunk;
    if (!block_range(B, j, lo, hi, chunk)) return;
    const int lane = threadIdx.x;
    u64 k[12];
    for (int a = 0; a < 3; a++) {
        k[a] = k[6 + a] = kmin0();
        k[3 + a] = k[9 + a] = kmax0();
    }
    for (int i = lo + lane; i < hi; i += kWave) {
        const int t = B.perm[i];
        const float4 A = B.tr.A[t], Bv = B.tr.B[t];
        const float cz = B.tr.C[t];
        const uint32_t p1 = (uint32_t)i + 1;
        k[0] = umin64(k[0], kmin(A.x, p1));
        k[1] = umin64(k[1], kmin(A.y, p1));
        k[2] = umin64(k[2], kmin(A.z, p1));
        k[3] = umax64(k[3], kmax(Bv.x, p1));
        k[4] = umax64(k[4], kmax(Bv.y, p1));
        k[5] = umax64(k[5], kmax(Bv.z, p1));
        k[6] = umin64(k[6], kmin(A.w, p1));
        k[7] = umin64(k[7], kmin(Bv.w, p1));
        k[8] = umin64(k[8], kmin(cz, p1));
        k[9] = umax64(k[9], kmax(A.w, p1));
        k[10] = umax64(k[10], kmax(Bv.w, p1));
        k[11] = umax64(k[11], kmax(cz, p1));
    }
    for (int m = 1; m < kWave; m <<= 1)
        for (int q = 0; q < 12; q++) {
            const u64 o = shfl_xor64(k[q], m);
            k[q] = (q % 6) < 3 ? umin64(k[q], o) : umax64(k[q], o);
        }
    u64* dst = B.keys + (size_t)j * 12;
    for (int q = 0; q < 12; q++)
        if (lane == q) {
            if ((q % 6) < 3) atomicMin(dst + q, k[q]);
            else atomicMax(dst + q, k[q]);
        }
}

__device__ void leaf_rec(Bufs& B, Rec& r) {
    r.kind = REC_LEAF;
    r.total = 1;
    atomicMax(&B.ctr->max_depth, r.depth);
}

// one lane per big node: bounds, axis, the equal-centroid leaf
__global__ void k_split_axis(Bufs B, int cnt) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt || B.ctr->overflow) return;
    Lvl& L = B.lv[j];
    Rec& r = B.recs[L.rec];
    const u64* k = B.keys + (size_t)j * 12;
    Box bounds, cb;
    for (int a = 0; a < 3; a++) {
        bounds.lo[a] = key_value(B, k[a], true, a);
        bounds.hi[a] = key_value(B, k[3 + a], false, 3 + a);
        cb.lo[a] = key_value(B, k[6 + a], true, 6 + a);
        cb.hi[a] = key_value(B, k[9 + a], false, 6 + a);
        r.lo[a] = bounds.lo[a];
        r.hi[a] = bounds.hi[a];
    }
    L.bounds = bounds;
    L.cb = cb;
    const int axis = cb.longest_axis();
    L.axis = axis;
    if (cb.lo[axis] == cb.hi[axis]) {
        leaf_rec(B, r);
        return;
    }
    L.act = 1;
}

// bucket of every primitive; per-bucket counts and boxes
__global__ void __launch_bounds__(kWave) k_bins(Bufs B) {
    int j, lo, hi, chunk;
    if (!block_range(B, j, lo, hi, chunk)) return;
    const Lvl& L = B.lv[j];
    if (!L.act) return;
    __shared__ u64 sk[kBuckets * 6];
    __shared__ int sc[kBuckets];
    const int lane = threadIdx.x;
    for (int q = lane; q < kBuckets * 6; q += kWave) sk[q] = (q % 6) < 3 ? kmin0() : kmax0();
    if (lane < kBuckets) sc[lane] = 0;
    __syncthreads();
    const Box cb = L.cb;
    const int axis = L.axis;
    for (int i = lo + lane; i < hi; i += kWave) {
        const int t = B.perm[i];
        const float4 A = B.tr.A[t], Bv = B.tr.B[t];
        const float c = axis == 0 ? A.w : (axis == 1 ? Bv.w : B.tr.C[t]);
        const int b = bucket_of(cb, c, axis);
        B.bucket[i] = (uint8_t)b;
        const uint32_t p1 = (uint32_t)i + 1;
        atomicAdd(&sc[b], 1);
        atomicMin(&sk[b * 6 + 0], kmin(A.x, p1));
        atomicMin(&sk[b * 6 + 1], kmin(A.y, p1));
        atomicMin(&sk[b * 6 + 2], kmin(A.z, p1));
        atomicMax(&sk[b * 6 + 3], kmax(Bv.x, p1));
        atomicMax(&sk[b * 6 + 4], kmax(Bv.y, p1));
        atomicMax(&sk[b * 6 + 5], kmax(Bv.z, p1));
    }
    __syncthreads();
    if (lane < kBuckets && sc[lane] > 0) {
        const size_t o = (size_t)j * kBuckets + lane;
        atomicAdd(&B.bincnt[o], sc[lane]);
        for (int q = 0; q < 3; q++) {
            atomicMin(&B.binkeys[o * 6 + q], sk[lane * 6 + q]);
            atomicMax(&B.binkeys[o * 6 + 3 + q], sk[lane * 6 + 3 + q]);
        }
    }
}

// one lane per binned node: SAH split or leaf; children records
__global__ void k_split_sah(Bufs B, int cnt, int* __restrict__ next_ids) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cnt || B.ctr->overflow) return;
    Lvl& L = B.lv[j];
    if (!L.act) return;
    Rec& r = B.recs[L.rec];
    Box bb[kBuckets];
    int count[kBuckets];
#pragma unroll
    for (int b = 0; b < kBuckets; b++) {
        const size_t o = (size_t)j * kBuckets + b;
        count[b] = B.bincnt[o];
        if (count[b] > 0)
            for (int a = 0; a < 3; a++) {
                bb[b].lo[a] = key_value(B, B.binkeys[o * 6 + a], true, a);
                bb[b].hi[a] = key_value(B, B.binkeys[o * 6 + 3 + a], false, 3 + a);
            }
    }
    float min_cost;
    const int split = sah_pick(bb, count, L.bounds, &min_cost);
    if (!sah_splits(r.n, B.max_prims, min_cost)) {
        L.act = 0;
        leaf_rec(B, r);
        return;
    }
    int m = 0;
#pragma unroll
    for (int b = 0; b < kBuckets; b++)
        if (b <= split) m += count[b];
    L.split = split;
    L.m = m;
    const int c = atomicAdd(&B.ctr->records, 2);
    if (c + 2 > B.rec_cap) {
        atomicOr(&B.ctr->overflow, 1);
        return;
    }
    r.kind = REC_INTERIOR;
    r.left = c;
    for (int s = 0; s < 2; s++) {
        Rec& ch = B.recs[c + s];
        ch.start = s == 0 ? r.start : r.start + m;
        ch.n = s == 0 ? m : r.n - m;
        ch.depth = r.depth + 1;
        ch.left = -1;
        ch.total = 0;
        if (ch.n > kLaneMax) {
            ch.kind = REC_OPEN;
            const int q = atomicAdd(&B.ctr->next_cnt, 1);
            if (q >= B.lvl_cap) atomicOr(&B.ctr->overflow, 1);
            else next_ids[q] = c + s;
        } else {
            ch.kind = REC_LANE;
            const int q = atomicAdd(&B.ctr->lane_cnt, 1);
            if (q >= B.n) atomicOr(&B.ctr->overflow, 1);
            else B.lane_ids[q] = c + s;
        }
    }
}

__device__ __forceinline__ bool goes_left(const Bufs& B, const Lvl& L, int i) { return B.bucket[i] <= L.split; }

// per block: primitives to swap on each side
__global__ void __launch_bounds__(kWave) k_part_count(Bufs B) {
    int j, lo, hi, chunk;
    if (!block_range(B, j, lo, hi, chunk)) return;
    const Lvl& L = B.lv[j];
    if (!L.act) return;
    const int mid = B.recs[L.rec].start + L.m;
    int cl = 0, cr = 0;
    for (int base = lo; base < hi; base += kWave) {
        const int i = base + threadIdx.x;
        const bool in = i < hi;
        const bool left = in && goes_left(B, L, i);
        cl += __popcll(__ballot(in && i < mid && !left));
        cr += __popcll(__ballot(in && i >= mid && left));
    }
    if (threadIdx.x == 0) B.blk_cnt[blockIdx.x] = make_int2(cl, cr);
}

// one wave per binned node: block offsets of the left ranks (prefix) and right ranks (suffix)
__global__ void __launch_bounds__(kWave) k_part_scan(Bufs B, int cnt) {
    const int j = blockIdx.x;
    if (j >= cnt || B.ctr->overflow) return;
    Lvl& L = B.lv[j];
    if (!L.act) return;
    const int lane = threadIdx.x;
    int totL = 0, totR = 0;
    for (int b = lane; b < L.nblk; b += kWave) {
        const int2 v = B.blk_cnt[L.blk_first + b];
        totL += v.x;
        totR += v.y;
    }
    for (int m = 1; m < kWave; m <<= 1) {
        totL += __shfl_xor(totL, m, kWave);
        totR += __shfl_xor(totR, m, kWave);
    }
    int runL = 0, runR = 0;
    for (int base = 0; base < L.nblk; base += kWave) {
        const int b = base + lane;
        const int2 v = b < L.nblk ? B.blk_cnt[L.blk_first + b] : make_int2(0, 0);
        int x = v.x, y = v.y;
        for (int d = 1; d < kWave; d <<= 1) {
            const int px = __shfl_up(x, d, kWave), py = __shfl_up(y, d, kWave);
            if (lane >= d) {
                x += px;
                y += py;
            }
        }
        if (b < L.nblk) B.blk_off[L.blk_first + b] = make_int2(runL + x - v.x, totR - (runR + y));
        runL += __shfl(x, kWave - 1, kWave);
        runR += __shfl(y, kWave - 1, kWave);
    }
    if (lane == 0) L.k = totL;
}

// rank every primitive that moves; posL / posR[start + rank] = its position
__global__ void __launch_bounds__(kWave) k_part_rank(Bufs B) {
    int j, lo, hi, chunk;
    if (!block_range(B, j, lo, hi, chunk)) return;
    const Lvl& L = B.lv[j];
    if (!L.act) return;
    const int start = B.recs[L.rec].start;
    const int mid = start + L.m;
    const int2 off = B.blk_off[blockIdx.x];
    const int cntR = B.blk_cnt[blockIdx.x].y;
    const int lane = threadIdx.x;
    const u64 below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int runL = 0, runR = 0;
    for (int base = lo; base < hi; base += kWave) {
        const int i = base + lane;
        const bool in = i < hi;
        const bool left = in && goes_left(B, L, i);
        const bool fl = in && i < mid && !left, fr = in && i >= mid && left;
        const u64 ml = __ballot(fl), mr = __ballot(fr);
        if (fl) B.posL[start + off.x + runL + __popcll(ml & below)] = i;
        if (fr) B.posR[start + off.y + cntR - (runR + __popcll(mr & below) + 1)] = i;
        runL += __popcll(ml);
        runR += __popcll(mr);
    }
}

__global__ void __launch_bounds__(kWave) k_part_swap(Bufs B) {
    int j, lo, hi, chunk;
    if (!block_range(B, j, lo, hi, chunk)) return;
    const Lvl& L = B.lv[j];
    if (!L.act) return;
    const int start = B.recs[L.rec].start;
    const int end = min(L.k, (chunk + 1) * kChunk);
    for (int r = chunk * kChunk + threadIdx.x; r < end; r += kWave) {
        const int a = B.posL[start + r], b = B.posR[start + r];
        const int t = B.perm[a];
        B.perm[a] = B.perm[b];
        B.perm[b] = t;
    }
}

// ---- lane tier: Builder::build / choose_split of agpt_host_scene.cpp on one lane, over the shared arithmetic ---------
struct LaneBins {
    float (*bb)[kWave];  // [kBuckets * 6][kWave]
    int (*cnt)[kWave];   // [kBuckets][kWave]
};

__device__ int lane_choose(const Bufs& B, int start, int end, Box& bounds, LaneBins sh, int lane) {
    bounds = Box();
    for (int i = start; i < end; i++) bounds.grow(B.tr.box(B.perm[i]));
    const int n = end - start;
    if (n == 1) return -1;
    Box cb;
    for (int i = start; i < end; i++) {
        const int t = B.perm[i];
        cb.grow(B.tr.cent(t, 0), B.tr.cent(t, 1), B.tr.cent(t, 2));
    }
    const int axis = cb.longest_axis();
    if (cb.lo[axis] == cb.hi[axis]) return -1;
    const int mid = (start + end) / 2;
    if (n <= 2) {  // std::nth_element on two elements: insertion sort
        const int t0 = B.perm[start], t1 = B.perm[start + 1];
        if (B.tr.cent(t1, axis) < B.tr.cent(t0, axis)) {
            B.perm[start] = t1;
            B.perm[start + 1] = t0;
        }
        return mid;
    }
    for (int b = 0; b < kBuckets; b++) {
        sh.cnt[b][lane] = 0;
        for (int a = 0; a < 3; a++) {
            sh.bb[b * 6 + a][lane] = kBoxEmpty;
            sh.bb[b * 6 + 3 + a][lane] = -kBoxEmpty;
        }
    }
    for (int i = start; i < end; i++) {
        const int t = B.perm[i];
        const int b = bucket_of(cb, B.tr.cent(t, axis), axis);
        sh.cnt[b][lane]++;
        const Box pb = B.tr.box(t);
        for (int a = 0; a < 3; a++) {
            sh.bb[b * 6 + a][lane] = tminf(sh.bb[b * 6 + a][lane], pb.lo[a]);
            sh.bb[b * 6 + 3 + a][lane] = tmaxf(sh.bb[b * 6 + 3 + a][lane], pb.hi[a]);
        }
    }
    Box bb[kBuckets];
    int count[kBuckets];
#pragma unroll
    for (int b = 0; b < kBuckets; b++) {
        count[b] = sh.cnt[b][lane];
        for (int a = 0; a < 3; a++) {
            bb[b].lo[a] = sh.bb[b * 6 + a][lane];
            bb[b].hi[a] = sh.bb[b * 6 + 3 + a][lane];
        }
    }
    float min_cost;
    const int split = sah_pick(bb, count, bounds, &min_cost);
    if (sah_splits(n, B.max_prims, min_cost)) {
        // std::partition (libstdc++, bidirectional iterators)
        int first = start, last = end;
        auto pred = [&](int i) { return bucket_of(cb, B.tr.cent(B.perm[i], axis), axis) <= split; };
        while (true) {
            while (true) {
                if (first == last) return first;
                if (pred(first)) ++first;
                else break;
            }
            --last;
            while (true) {
                if (first == last) return first;
                if (!pred(last)) --last;
                else break;
            }
            const int t = B.perm[first];
            B.perm[first] = B.perm[last];
            B.perm[last] = t;
            ++first;
        }
    }
    return -1;
}

// one lane per lane record: the subtree in the sequential builder's own layout (root 0, slot 1 unused, pairs from 2) at
// scr[2 * start ...], its explicit stack at stk[start ...] (at most n frames)
__global__ void __launch_bounds__(kWave) k_lane(Bufs B, int cnt) {
    __shared__ float sbb[kBuckets * 6][kWave];
    __shared__ int scnt[kBuckets][kWave];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= cnt) return;
    const int lane = threadIdx.x;
    LaneBins sh{sbb, scnt};
    Rec& r = B.recs[B.lane_ids[idx]];
    agpt_bvh_node* nd = B.scr + (size_t)2 * r.start;
    int4* stk = B.stk + r.start;
    int sp = 0;
    stk[sp++] = make_int4(r.start, r.start + r.n, 0, r.depth);
    int next_pair = 2, total = 0, maxd = 0;
    while (sp > 0) {
        const int4 f = stk[--sp];
        total++;
        Box bounds;
        const int mid = lane_choose(B, f.x, f.y, bounds, sh, lane);
        agpt_bvh_node& o = nd[f.z];
        if (mid < 0) {
            for (int a = 0; a < 3; a++) {
                o.bmin[a] = bounds.lo[a];
                o.bmax[a] = bounds.hi[a];
            }
            o.first = f.x;
            o.count = f.y - f.x;
            maxd = max(maxd, f.w);
            continue;
        }
        const int first = next_pair;
        next_pair += 2;
        o.first = first;
        o.count = 0;
        stk[sp++] = make_int4(mid, f.y, first + 1, f.w + 1);
        stk[sp++] = make_int4(f.x, mid, first, f.w + 1);
    }
    // children sit at higher slots than their parent: one backward sweep unions interior bounds bottom-up
    for (int s = total; s >= 0; s--) {
        if (s == 1 || nd[s].count != 0) continue;
        agpt_bvh_node& o = nd[s];
        const agpt_bvh_node &c0 = nd[o.first], &c1 = nd[o.first + 1];
        pair_union(c0.bmin, c0.bmax, c1.bmin, c1.bmax, o.bmin, o.bmax);
    }
    r.total = total;
    for (int a = 0; a < 3; a++) {
        r.lo[a] = nd[0].bmin[a];
        r.hi[a] = nd[0].bmax[a];
    }
    atomicMax(&B.ctr->max_depth, maxd);
}

// ---- numbering -------------------------------------------------------------------------------------------------------
__global__ void k_up(Bufs B, int rb, int re) {
    const int i = rb + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= re) return;
    Rec& r = B.recs[i];
    if (r.kind != REC_INTERIOR) return;
    const Rec &L = B.recs[r.left], &R = B.recs[r.left + 1];
    r.total = 1 + L.total + R.total;
    pair_union(L.lo, L.hi, R.lo, R.hi, r.lo, r.hi);
}

__global__ void k_down(Bufs B, int rb, int re) {
    const int i = rb + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= re) return;
    const Rec& r = B.recs[i];
    agpt_bvh_node o;
    for (int a = 0; a < 3; a++) {
        o.bmin[a] = r.lo[a];
        o.bmax[a] = r.hi[a];
    }
    if (r.kind == REC_INTERIOR) {
        o.first = r.base;
        o.count = 0;
        B.out[r.slot] = o;
        Rec &L = B.recs[r.left], &R = B.recs[r.left + 1];
        L.slot = r.base;
        L.base = r.base + 2;
        R.slot = r.base + 1;
        R.base = r.base + 2 + (L.total - 1);
    } else if (r.kind == REC_LEAF) {
        o.first = r.start;
        o.count = r.n;
        B.out[r.slot] = o;
    } else {  // lane subtree: embed (agpt_host_scene.cpp, build_subtree)
        const agpt_bvh_node* nd = B.scr + (size_t)2 * r.start;
        for (int s = 0; s <= r.total; s++) {
            if (s == 1) continue;
            agpt_bvh_node x = nd[s];
            if (x.count == 0) x.first = r.base + (x.first - 2);
            B.out[s == 0 ? r.slot : r.base + (s - 2)] = x;
        }
    }
}

__global__ void k_prim_index(Bufs B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B.n) B.posL[i] = 3 * B.perm[i];
}

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

float ord_decode(uint32_t u) {
    const uint32_t b = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

struct Arena {
    char* base = nullptr;
    size_t used = 0;
    template <class T>
    T* take(size_t count) {
        T* p = (T*)(base + used);
        used += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

int host_fallback(const float* vertices, int n_vertices, const int32_t* indices, int n_tris, int max_prims,
                  agpt_bvh_node* nodes_out, int32_t* prim_index_out, int* total_nodes, int* max_depth) {
    agpt::HostMesh m;
    m.vertices.resize(n_vertices);
    for (int i = 0; i < n_vertices; i++) m.vertices[i] = V3(vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]);
    m.indices.assign(indices, indices + (size_t)9 * n_tris);
    agpt::build_bvh(m, max_prims);
    if (nodes_out) std::memcpy(nodes_out, m.nodes.data(), m.nodes.size() * sizeof(agpt_bvh_node));
    if (prim_index_out) std::memcpy(prim_index_out, m.prim_index.data(), m.prim_index.size() * sizeof(int32_t));
    *total_nodes = m.total_nodes;
    *max_depth = m.max_depth;
    return AGPT_OK;
}

}  // namespace

namespace agpt {

#define BVH_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            err = fail(AGPT_ERR_DEVICE, std::string("agpt_bvh_build_device: ") + #expr + ": " +       \
                                                    hipGetErrorString(e_));                                   \
            goto done;                                                                                        \
        }                                                                                                     \
    } while (0)

int build_bvh_device(hipStream_t stream, const float* vertices, int n_vertices, const int32_t* indices, int n_tris,
                     int max_prims_in_node, agpt_bvh_node* nodes_out, int32_t* prim_index_out, int* total_nodes,
                     int* max_depth, int* on_device) {
    const int n = n_tris;
    const int lvl_cap = n / (kLaneMax + 1) + 1;
    const int blk_cap = n / kChunk + 1 + lvl_cap;
    const int rec_cap = 2 * n + 1;
    int err = AGPT_OK;
    bool fallback = false;
    Ctr* hc = nullptr;
    Bufs B{};
    Arena ar;
    int* ids[2];
    float* dV;
    int32_t* dI;
    std::vector<int> ranges;
    int cnt = 0, cur = 0;
    Ctr h{};
    {
        // sizes first, one allocation
        Arena probe;
        probe.take<float>((size_t)3 * n_vertices);
        probe.take<int32_t>((size_t)9 * n);
        probe.take<float4>(n);
        probe.take<float4>(n);
        probe.take<float>(n);
        probe.take<int>(n);
        probe.take<uint8_t>(n);
        probe.take<int>(n);
        probe.take<int>(n);
        probe.take<int4>(n);
        probe.take<agpt_bvh_node>((size_t)2 * n);
        probe.take<agpt_bvh_node>((size_t)2 * n + 2);
        probe.take<Rec>(rec_cap);
        probe.take<int>(n);
        probe.take<int>(lvl_cap);
        probe.take<int>(lvl_cap);
        probe.take<Lvl>(lvl_cap);
        probe.take<u64>((size_t)lvl_cap * 12);
        probe.take<u64>((size_t)lvl_cap * kBuckets * 6);
        probe.take<int>((size_t)lvl_cap * kBuckets);
        probe.take<int>(blk_cap);
        probe.take<int2>(blk_cap);
        probe.take<int2>(blk_cap);
        probe.take<Ctr>(1);
        const hipError_t e = hipMalloc((void**)&ar.base, probe.used);
        if (e != hipSuccess) {
            ar.base = nullptr;
            return fail(AGPT_ERR_NOMEM, std::string("agpt_bvh_build_device: hipMalloc: ") + hipGetErrorString(e));
        }
    }
    dV = ar.take<float>((size_t)3 * n_vertices);
    dI = ar.take<int32_t>((size_t)9 * n);
    B.tr.A = ar.take<float4>(n);
    B.tr.B = ar.take<float4>(n);
    B.tr.C = ar.take<float>(n);
    B.perm = ar.take<int>(n);
    B.bucket = ar.take<uint8_t>(n);
    B.posL = ar.take<int>(n);
    B.posR = ar.take<int>(n);
    B.stk = ar.take<int4>(n);
    B.scr = ar.take<agpt_bvh_node>((size_t)2 * n);
    B.out = ar.take<agpt_bvh_node>((size_t)2 * n + 2);
    B.recs = ar.take<Rec>(rec_cap);
    B.lane_ids = ar.take<int>(n);
    ids[0] = ar.take<int>(lvl_cap);
    ids[1] = ar.take<int>(lvl_cap);
    B.lv = ar.take<Lvl>(lvl_cap);
    B.keys = ar.take<u64>((size_t)lvl_cap * 12);
    B.binkeys = ar.take<u64>((size_t)lvl_cap * kBuckets * 6);
    B.bincnt = ar.take<int>((size_t)lvl_cap * kBuckets);
    B.blk_node = ar.take<int>(blk_cap);
    B.blk_cnt = ar.take<int2>(blk_cap);
    B.blk_off = ar.take<int2>(blk_cap);
    B.ctr = ar.take<Ctr>(1);
    B.n = n;
    B.rec_cap = rec_cap;
    B.lvl_cap = lvl_cap;
    B.blk_cap = blk_cap;
    B.max_prims = max_prims_in_node;

    BVH_TRY(hipHostMalloc((void**)&hc, sizeof(Ctr), hipHostMallocDefault));
    h.ext[0] = h.ext[1] = h.ext[2] = 0xFFFFFFFFu;
    BVH_TRY(hipMemcpyAsync(B.ctr, &h, sizeof(Ctr), hipMemcpyHostToDevice, stream));
    BVH_TRY(hipMemcpyAsync(dV, vertices, sizeof(float) * 3 * (size_t)n_vertices, hipMemcpyHostToDevice, stream));
    BVH_TRY(hipMemcpyAsync(dI, indices, sizeof(int32_t) * 9 * (size_t)n, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_prep, dim3(cdiv(n, 256)), dim3(256), 0, stream, B, dV, dI);
    hipLaunchKernelGGL(k_init_root, dim3(1), dim3(1), 0, stream, B);
    BVH_TRY(hipGetLastError());
    BVH_TRY(hipMemcpyAsync(hc, B.ctr, sizeof(Ctr), hipMemcpyDeviceToHost, stream));
    BVH_TRY(hipStreamSynchronize(stream));
    if (hc->nonfinite) {
        fallback = true;
        goto done;
    }
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(ord_decode(hc->ext[3 + a]) - ord_decode(hc->ext[a]))) {
            fallback = true;
            goto done;
        }

    ranges.push_back(0);
    ranges.push_back(1);
    cnt = n > kLaneMax ? 1 : 0;
    if (cnt) BVH_TRY(hipMemcpyAsync(ids[0], &cur, sizeof(int), hipMemcpyHostToDevice, stream));  // record 0
    while (cnt > 0) {
        int* cur_ids = ids[cur];
        int* nxt_ids = ids[cur ^ 1];
        const dim3 lanes(cdiv(cnt, kWave)), wave(kWave), grid(n / kChunk + 1 + cnt);
        BVH_TRY(hipMemsetAsync(B.ctr, 0, 2 * sizeof(int), stream));  // blocks, next_cnt
        hipLaunchKernelGGL(k_level_setup, lanes, wave, 0, stream, B, cur_ids, cnt);
        hipLaunchKernelGGL(k_bounds, grid, wave, 0, stream, B);
        hipLaunchKernelGGL(k_split_axis, lanes, wave, 0, stream, B, cnt);
        hipLaunchKernelGGL(k_bins, grid, wave, 0, stream, B);
        hipLaunchKernelGGL(k_split_sah, lanes, wave, 0, stream, B, cnt, nxt_ids);
        hipLaunchKernelGGL(k_part_count, grid, wave, 0, stream, B);
        hipLaunchKernelGGL(k_part_scan, dim3(cnt), wave, 0, stream, B, cnt);
        hipLaunchKernelGGL(k_part_rank, grid, wave, 0, stream, B);
        hipLaunchKernelGGL(k_part_swap, grid, wave, 0, stream, B);
        BVH_TRY(hipGetLastError());
        BVH_TRY(hipMemcpyAsync(hc, B.ctr, sizeof(Ctr), hipMemcpyDeviceToHost, stream));
        BVH_TRY(hipStreamSynchronize(stream));
        if (hc->overflow) {
            err = fail(AGPT_ERR_LIMIT, "agpt_bvh_build_device: scratch capacity exceeded");
            goto done;
        }
        ranges.push_back(hc->records);
        cnt = hc->next_cnt;
        cur ^= 1;
    }
    BVH_TRY(hipMemcpyAsync(hc, B.ctr, sizeof(Ctr), hipMemcpyDeviceToHost, stream));
    BVH_TRY(hipStreamSynchronize(stream));
    if (hc->lane_cnt > 0) hipLaunchKernelGGL(k_lane, dim3(cdiv(hc->lane_cnt, kWave)), dim3(kWave), 0, stream, B, hc->lane_cnt);
    for (size_t L = ranges.size() - 1; L-- > 0;)
        if (ranges[L + 1] > ranges[L])
            hipLaunchKernelGGL(k_up, dim3(cdiv(ranges[L + 1] - ranges[L], kWave)), dim3(kWave), 0, stream, B, ranges[L], ranges[L + 1]);
    for (size_t L = 0; L + 1 < ranges.size(); L++)
        if (ranges[L + 1] > ranges[L])
            hipLaunchKernelGGL(k_down, dim3(cdiv(ranges[L + 1] - ranges[L], kWave)), dim3(kWave), 0, stream, B, ranges[L], ranges[L + 1]);
    hipLaunchKernelGGL(k_prim_index, dim3(cdiv(n, 256)), dim3(256), 0, stream, B);
    BVH_TRY(hipGetLastError());
    BVH_TRY(hipMemsetAsync(B.out + 1, 0, sizeof(agpt_bvh_node), stream));
    {
        int total = 0;
        BVH_TRY(hipMemcpyAsync(&total, &B.recs[0].total, sizeof(int), hipMemcpyDeviceToHost, stream));
        BVH_TRY(hipMemcpyAsync(hc, B.ctr, sizeof(Ctr), hipMemcpyDeviceToHost, stream));
        BVH_TRY(hipStreamSynchronize(stream));
        if (total < 1 || total > 2 * n - 1) {
            err = fail(AGPT_ERR_DEVICE, "agpt_bvh_build_device: inconsistent node count " + std::to_string(total));
            goto done;
        }
        if (nodes_out)
            BVH_TRY(hipMemcpyAsync(nodes_out, B.out, sizeof(agpt_bvh_node) * ((size_t)total + 1), hipMemcpyDeviceToHost, stream));
        if (prim_index_out) BVH_TRY(hipMemcpyAsync(prim_index_out, B.posL, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
        BVH_TRY(hipStreamSynchronize(stream));
        *total_nodes = total;
        *max_depth = hc->max_depth;
        *on_device = 1;
    }
done:
    if (hc) (void)hipHostFree(hc);
    if (ar.base) {
        (void)hipStreamSynchronize(stream);
        (void)hipFree(ar.base);
    }
    if (err == AGPT_OK && fallback) {
        *on_device = 0;
        return host_fallback(vertices, n_vertices, indices, n, max_prims_in_node, nodes_out, prim_index_out, total_nodes, max_depth);
    }
    return err;
}

}  // namespace agpt
