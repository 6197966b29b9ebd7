// agpt_bvh_arith.h -- the arithmetic of the mesh BVH, ONE definition for the host builder and refit (agpt_host_scene.cpp), the device
// builder (agpt_bvh_device.hip) and the device refit (agpt_update.hip): the box with its tie rule, the binned-SAH decision, a
// triangle's box and centroid, the union an interior node stores.  Every unit compiles it with -ffp-contract=off, so host and device
// round the same operations in the same order and produce the same bits.
#pragma once

#include "agpt_math.h"

namespace agpt {

// Bounds (bvhtrimesh.h:96-124).  An empty box is (+kBoxEmpty, -kBoxEmpty); tminf / tmaxf keep the LATER of equal operands, which
// decides between +0 and -0.
constexpr float kBoxEmpty = 1e34f;

struct Box {
    float lo[3], hi[3];
    AGPT_HD Box() {
        for (int a = 0; a < 3; a++) {
            lo[a] = kBoxEmpty;
            hi[a] = -kBoxEmpty;
        }
    }
    AGPT_HD void grow(const Box& b) {
        for (int a = 0; a < 3; a++) {
            lo[a] = tminf(lo[a], b.lo[a]);
            hi[a] = tmaxf(hi[a], b.hi[a]);
        }
    }
    AGPT_HD void grow(float x, float y, float z) {
        lo[0] = tminf(lo[0], x);
        lo[1] = tminf(lo[1], y);
        lo[2] = tminf(lo[2], z);
        hi[0] = tmaxf(hi[0], x);
        hi[1] = tmaxf(hi[1], y);
        hi[2] = tmaxf(hi[2], z);
    }
    AGPT_HD void grow(v3 p) { grow(p.x, p.y, p.z); }
    AGPT_HD float extent(int a) const { return hi[a] - lo[a]; }
    AGPT_HD int longest_axis() const {
        int a = 0;
        if (extent(1) > extent(0)) a = 1;
        if (extent(2) > extent(a)) a = 2;
        return a;
    }
    AGPT_HD float area() const {
        float dx = extent(0), dy = extent(1), dz = extent(2);
        return 2 * (dx * dy + dx * dz + dy * dz);
    }
    AGPT_HD float offset(float p, int a) const {
        float o = p - lo[a];
        if (hi[a] > lo[a]) o /= hi[a] - lo[a];
        return o;
    }
};

// Primitive (bvhtrimesh.h:132-145): the box of the three vertices; c = its centre.
AGPT_HD Box tri_box(v3 v0, v3 v1, v3 v2, float c[3] = nullptr) {
    Box b;
    b.grow(v0);
    b.grow(v1);
    b.grow(v2);
    if (c)
        for (int a = 0; a < 3; a++) c[a] = (b.lo[a] + b.hi[a]) * 0.5f;
    return b;
}

// Bounds::Union of a child pair (bvhtrimesh.h:113-118): what an interior node stores, (left, right) in this order.
AGPT_HD void pair_union(const float llo[3], const float lhi[3], const float rlo[3], const float rhi[3], float lo[3], float hi[3]) {
    for (int a = 0; a < 3; a++) {
        lo[a] = tminf(llo[a], rlo[a]);
        hi[a] = tmaxf(lhi[a], rhi[a]);
    }
}

// ---- BuildRecursive's split decision (bvhtrimesh.h:240-305) ----------------------------------------------------------------
constexpr int kBuckets = 12;

// bucket of a centroid coordinate c inside the centroid bounds cb
AGPT_HD int bucket_of(const Box& cb, float c, int axis) {
    int b = (int)(kBuckets * cb.offset(c, axis));
    if (b == kBuckets) b = kBuckets - 1;
    return b;
}

// the 11 costs of splitting behind bucket i, in the reference's operation order; the first minimum wins
AGPT_HD int sah_pick(const Box* bb, const int* count, const Box& bounds, float* min_cost_out) {
    float cost[kBuckets - 1];
#pragma unroll
    for (int i = 0; i < kBuckets - 1; i++) {
        Box b0, b1;
        int c0 = 0, c1 = 0;
#pragma unroll
        for (int j = 0; j <= i; j++) {
            b0.grow(bb[j]);
            c0 += count[j];
        }
#pragma unroll
        for (int j = i + 1; j < kBuckets; j++) {
            b1.grow(bb[j]);
            c1 += count[j];
        }
        cost[i] = 1 + (c0 * b0.area() + c1 * b1.area()) / bounds.area();
    }
    float min_cost = cost[0];
    int split = 0;
#pragma unroll
    for (int i = 1; i < kBuckets - 1; i++)
        if (cost[i] < min_cost) {
            min_cost = cost[i];
            split = i;
        }
    *min_cost_out = min_cost;
    return split;
}

// a node of n primitives splits at sah_pick's bucket unless it may be a leaf and the leaf is no dearer
AGPT_HD bool sah_splits(int n, int max_prims, float min_cost) { return n > max_prims || min_cost < (float)n; }

}  // namespace agpt
