// Passes over the emitted op list (internal to runtime/): everything lower_network does after the last layer was emitted.
#pragma once
#include <string>

#include "../options.h"
#include "plan.h"

namespace trtx {

// What the passes read besides the plan itself.
struct PassInputs {
    bool int8;                               // Network::int8 (kINT8 builder flag)
    const std::vector<float>& tensor_scale;  // Network::tensor_scale: calibrated scale per network tensor
    int max_aux_streams;                     // Network::max_aux_streams
    int dt;                                  // dtype of NHWC tensors
    const Options& opt;                      // the switches of this lowering
};

// top owner of a tensor and, for NHWC, the accumulated channel offset
inline int owner_of(const Plan& plan, int p, int* off = nullptr) {
    int o = 0;
    while (plan.tensors[p].parent >= 0) {
        o += plan.tensors[p].coff;
        p = plan.tensors[p].parent;
    }
    if (off) *off = o;
    return p;
}
inline bool is_binding_tensor(const Plan& plan, int p) {
    for (int b : plan.binding_ptensor)
        if (b == p) return true;
    return false;
}

// View geometry, folded upsamples, int8 tensors, storages, kernel choice, plugin workspaces, pool chains, grouped convolutions,
// dependencies, lanes and the arena.  Returns false with *err set.
bool finalize_plan(Plan& plan, const PassInputs& e, std::string* err);

}  // namespace trtx
