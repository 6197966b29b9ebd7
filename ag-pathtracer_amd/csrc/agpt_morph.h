// agpt_morph.h -- morph targets (blend shapes): a mesh's rest arrays plus a weighted sum of per-target deltas.  ONE source for
// agpt_morph_arrays (host, agpt_obj.cpp) and k_morph_mesh (agpt_update.hip, agpt_scene_morph_mesh): both units compile with
// -ffp-contract=off, every operation is fp32 and rounds on its own, so the two produce the same bits.
//
//   a mesh has T targets (1 .. kMorphMaxTargets); target t has one position delta per vertex, dP[t][i], and optionally one normal delta
//   per NORMAL, dN[t][j] (a mesh may have other counts of normals than vertices); target-major, packed xyz: [t][item][3].
//   position   acc = rest[i]; the targets in order t = 0 .. T-1; a target whose weight is exactly 0 (either sign) is skipped; every
//              other one adds acc[c] = acc[c] + w[t] * dP[t][i][c] per component -- the product rounds, then the sum.  Weights are
//              used as given: any finite value, neither normalised nor reordered.
//   normal     the same walk with dN; a mesh whose targets carry no normal deltas keeps its rest normals.  Not renormalised.
// All weights zero therefore gives the rest arrays bit for bit.  The skip is by WEIGHT, not by delta: a target of weight 1 whose delta
// is all zero turns a rest coordinate of -0.0 into +0.0 (-0.0 + 1 * 0.0).
//
// Both sides walk the list of ACTIVE targets (t, w), in target order with the zero weights dropped (morph_active_list): the cost of an
// item is proportional to the targets in use, not to the targets bound.
// With a skin the order is glTF's, morph then skin: the morphed position / normal is what skin_blend of agpt_skin.h receives as `rest`
// (so a vertex without a used slot keeps its MORPHED position).
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "agpt_transform.h"

namespace agpt {

constexpr int kMorphMaxTargets = 4096;

struct MorphActive {   // one target in use: 8 bytes, what a frame uploads per active target
    int32_t target;
    float weight;
};

// one vertex or one normal: `item` of `n_items`, its deltas at deltas[(target * n_items + item) * 3]
AGPT_HD void morph_blend(const MorphActive* active, int n_active, const float* deltas, size_t n_items, size_t item, const float rest[3],
                         float out[3]) {
    float acc[3] = {rest[0], rest[1], rest[2]};
    for (int k = 0; k < n_active; k++) {
        const float w = active[k].weight;
        const float* d = deltas + ((size_t)active[k].target * n_items + item) * 3;
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + w * d[c];
    }
    out[0] = acc[0];
    out[1] = acc[1];
    out[2] = acc[2];
}

// ---- host side: the targets, their checks and the active list ----

// A mesh's targets (agpt_scene_set_mesh_morph_targets): n_targets == 0 is "none".  normal_deltas is empty when the targets carry none
// or the mesh has no normals.
struct MorphTargets {
    int n_targets = 0;
    std::vector<float> position_deltas, normal_deltas;
};

// The checks agpt_morph_arrays and the scene calls share; each returns the message of the refusal, or "" when all is well.
inline std::string morph_check_count(int n_targets) {
    if (n_targets < 1 || n_targets > kMorphMaxTargets)
        return "n_targets is " + std::to_string(n_targets) + ", outside 1 .. " + std::to_string(kMorphMaxTargets);
    return "";
}
inline std::string morph_check_weights(const float* weights, int n_targets) {
    for (int t = 0; t < n_targets; t++)
        if (!std::isfinite(weights[t])) return "non-finite weight (target " + std::to_string(t) + ")";
    return "";
}
inline std::string morph_check_deltas(const char* what, const char* item, int n_targets, size_t n_items, const float* deltas) {
    const size_t per_target = n_items * 3, total = (size_t)n_targets * per_target;
    for (size_t i = 0; i < total; i++)
        if (!std::isfinite(deltas[i]))
            return std::string("non-finite ") + what + " delta (target " + std::to_string(i / per_target) + ", " + item + " " +
                   std::to_string(i % per_target / 3) + ")";
    return "";
}

// the targets of a frame that are in use, in target order
inline std::vector<MorphActive> morph_active_list(const float* weights, int n_targets) {
    std::vector<MorphActive> active;
    for (int t = 0; t < n_targets; t++)
        if (!(weights[t] == 0)) active.push_back(MorphActive{t, weights[t]});
    return active;
}

}  // namespace agpt
